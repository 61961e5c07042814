"""Kernel outputs must not depend on what the memory they are handed held before.

Every case runs its kernel call once as the product does, then once inside tests/poison.poisoned_empty for each pattern (nan, 3e38, 0.75)
with the frhip buffer caches dropped, so that every output, partial-sum buffer, K-split workspace and caller-provided buffer the kernel's
contract says it overwrites starts out holding the pattern.  The poisoned outputs must be bit-identical to the unpoisoned ones and finite,
and the unpoisoned ones must match a float64 reference of the same operation at the tolerances of tests/test_kernels_gpu.py.  Caller-zeroed
accumulators (conv_wgrad's dw, gemm_tn's out, bn_backward's dgamma / dbeta) stay zeroed: that is their contract.

Shapes: the convolutions the ResNet50 bench step (cfg 2: bf16, B = 512) launches, recorded from one step, plus ragged ones -- M not a
multiple of 256, channel counts not multiples of 128, 7 x 7 maps with several images per tile."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from poison import PATTERNS, PATTERN_IDS, assert_poison_applies, poisoned_empty, reset_frhip_caches
from ref64 import ref_conv, ref_dgrad, ref_wgrad

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def _ops():
    from frhip import ops
    return ops


def _lib():
    from frhip._abi import lib
    return lib()


def tol(dtype, scale=1.0):
    return (dict(rtol=2e-4, atol=2e-5 * scale) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2 * scale))


def rnd(seed, shape, std=1.0, device="cuda"):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(shape, generator=g, device=device) * std


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def poisoned_parity(call, dtypes=(torch.float32, torch.bfloat16)):
    """call() -> tuple of output tensors (None entries ignored).  Runs it clean, then under every poison pattern; asserts the outputs are
    finite and bit-identical across the runs.  Returns the clean outputs."""
    reset_frhip_caches()
    clean = [t.clone() if t is not None else None for t in call()]
    torch.cuda.synchronize()
    for i, t in enumerate(clean):
        if t is not None and t.is_floating_point():
            assert bool(torch.isfinite(t).all()), "output %d of the clean run is not finite" % i
    try:
        for pattern, pid in zip(PATTERNS, PATTERN_IDS):
            with poisoned_empty(pattern):
                reset_frhip_caches()
                for dt in dtypes:
                    assert_poison_applies(pattern, dt)
                got = call()
                torch.cuda.synchronize()
            for i, (a, b) in enumerate(zip(clean, got)):
                if a is None:
                    continue
                assert a.shape == b.shape and a.dtype == b.dtype
                if not torch.equal(_bits(a), _bits(b)):
                    d = (a.double() - b.double()).abs()
                    bad = torch.nonzero(~torch.eq(_bits(a), _bits(b)).reshape(-1)).flatten()
                    raise AssertionError("poison %s: output %d differs from the clean run in %d of %d elements (first flat index %d, "
                                         "max |diff| %s)" % (pid, i, bad.numel(), a.numel(), int(bad[0]),
                                                             float(d.nan_to_num(float("inf")).max())))
    finally:
        reset_frhip_caches()                # no poisoned workspace survives into the next test
    return clean


def close(got, ref, dtype, scale=None):
    ref = ref.double()
    scale = float(ref.abs().max()) if scale is None else scale
    np.testing.assert_allclose(got.double().cpu().numpy(), ref.cpu().numpy(), **tol(dtype, scale))


def stats_match_stored(part, y):
    """the BatchNorm partial sums (every row of the buffer) are those of the STORED tensor"""
    k = y.shape[-1]
    yy = y.double().reshape(-1, k)
    s = part.double().sum(0)
    for j, want in enumerate((yy.sum(0), (yy * yy).sum(0))):
        slack = 1e-5 * float((yy.abs() if j == 0 else yy * yy).sum(0).max()) + 1e-2
        np.testing.assert_allclose(s[j].cpu().numpy(), want.cpu().numpy(), rtol=1e-3, atol=slack)


def q(t, dtype):
    return t.to(dtype)


# ----------------------------------------------------------------------------------------------- shapes
# (n, h, w, c, k, r, stride, pad): every distinct convolution of the ResNet50 bench step (cfg 2, B = 512; basic blocks 3-4-14-4 on a
# 56 x 56 stem output), as recorded from one step by wrapping frhip.ops.conv_fwd / conv_fwd_bnrelu / conv_dgrad / conv_wgrad*.
CFG2_CONVS = [
    (512, 56, 56, 64, 64, 3, 1, 1),        # layer1 conv1 / conv2
    (512, 56, 56, 64, 128, 3, 1, 1),       # layer2.0 conv1
    (512, 56, 56, 128, 128, 3, 2, 1),      # layer2.0 conv2 (stride 2: parity-class data gradient)
    (512, 56, 56, 64, 128, 1, 2, 0),       # layer2.0 shortcut
    (512, 28, 28, 128, 128, 3, 1, 1),      # layer2 body
    (512, 28, 28, 128, 256, 3, 1, 1),      # layer3.0 conv1
    (512, 28, 28, 256, 256, 3, 2, 1),      # layer3.0 conv2
    (512, 28, 28, 128, 256, 1, 2, 0),      # layer3.0 shortcut
    (512, 14, 14, 256, 256, 3, 1, 1),      # layer3 body (rows14 / chained weight gradient)
    (512, 14, 14, 256, 512, 3, 1, 1),      # layer4.0 conv1
    (512, 14, 14, 512, 512, 3, 2, 1),      # layer4.0 conv2
    (512, 14, 14, 256, 512, 1, 2, 0),      # layer4.0 shortcut
    (512, 7, 7, 512, 512, 3, 1, 1),        # layer4 body
]
RAGGED_CONVS = [
    (3, 7, 7, 64, 128, 3, 1, 1),           # M = 147
    (9, 7, 7, 512, 512, 3, 1, 1),          # 441 pixels, 5+ images per 256-row tile
    (5, 9, 9, 64, 64, 3, 2, 1),            # odd map, stride 2
    (2, 10, 6, 64, 192, 3, 2, 1),          # K = 192, non-square, stride 2
    (7, 14, 14, 64, 192, 3, 1, 1),         # K not a multiple of 128, M = 1372
    (3, 28, 28, 64, 320, 3, 1, 1),         # K = 320
    (4, 13, 13, 128, 128, 1, 2, 0),        # 1x1 stride 2 on an odd map
]


def _conv_case_inputs(case, dtype):
    n, h, w, c, k, r, stride, pad = case
    x = rnd(1, (n, h, w, c)).to(dtype)
    wt = (rnd(2, (k, r, r, c)) * (1.0 / (r * r * c) ** 0.5)).to(dtype)
    return x, wt


def _dtypes_for(case):
    return [torch.bfloat16] if case[0] >= 64 else DTYPES


CONV_PARAMS = [(d, c) for c in CFG2_CONVS + RAGGED_CONVS for d in _dtypes_for(c)]
CONV_IDS = ["%s-%s" % ("bf16" if d == torch.bfloat16 else "fp32", "x".join(map(str, c))) for d, c in CONV_PARAMS]


@pytest.mark.parametrize("dtype,case", CONV_PARAMS, ids=CONV_IDS)
def test_conv_fwd_on_poisoned_memory(dtype, case):
    ops = _ops()
    n, h, w, c, k, r, stride, pad = case
    x, wt = _conv_case_inputs(case, dtype)
    y, part = poisoned_parity(lambda: ops.conv_fwd(x, wt, stride, pad))
    ho, wo = ops.conv_out_hw(h, w, r, r, stride, pad)
    assert part.shape[0] == _lib().frhip_conv_stat_rows(ops.dt_of(x), n * ho * wo, k, h, w, c, r, r, stride, pad)
    close(y, ref_conv(x, wt, stride, pad), dtype)
    stats_match_stored(part, y)


@pytest.mark.parametrize("dtype,case", CONV_PARAMS, ids=CONV_IDS)
def test_conv_dgrad_on_poisoned_memory(dtype, case):
    """plain, with a residual (compact stride-2 residual where the product uses one) and with the fused BN-backward reduction"""
    ops = _ops()
    n, h, w, c, k, r, stride, pad = case
    x, wt = _conv_case_inputs(case, dtype)
    ho, wo = ops.conv_out_hw(h, w, r, r, stride, pad)
    dy = rnd(3, (n, ho, wo, k)).to(dtype)
    wpack = ops.pack_wt(wt.float(), dtype)
    ref = ref_dgrad(dy, wt, (n, h, w, c), stride, pad)
    dx, = poisoned_parity(lambda: (ops.conv_dgrad(dy, wpack, (n, h, w, c), r, r, stride, pad),))
    close(dx, ref, dtype)
    y_bn = rnd(5, (n, h, w, c)).to(dtype)
    rows = n * h * w
    st = ops.bn_finalize(ops.colstats(y_bn.view(rows, c)), rows, (1 + 0.1 * rnd(6, (c,))), 0.1 * rnd(7, (c,)), None, None)
    if stride == 1 and r == 3:
        res2 = rnd(4, (n, (h + 1) // 2, (w + 1) // 2, c)).to(dtype)
        dx2, part = poisoned_parity(lambda: ops.conv_dgrad(dy, wpack, (n, h, w, c), r, r, stride, pad, residual=res2,
                                                           bnred=(y_bn, st, True), residual_stride=2))
        want = ref.clone()
        want[:, ::2, ::2, :] += res2.double()
        close(dx2, want, dtype)
    else:
        res = rnd(4, (n, h, w, c)).to(dtype)
        dx2, part = poisoned_parity(lambda: ops.conv_dgrad(dy, wpack, (n, h, w, c), r, r, stride, pad, residual=res,
                                                           bnred=(y_bn, st, True)))
        close(dx2, ref + res.double(), dtype)
    assert part.shape[0] == _lib().frhip_dgrad_stat_rows(ops.dt_of(dy), n, h, w, c, k, r, r, stride, pad)
    # the partial sums are the BN-backward sums over (dx as stored, y_bn) through the ReLU mask: sum d, sum d * xhat
    d = dx2.double().reshape(rows, c)
    yb = y_bn.double().reshape(rows, c)
    mask = (yb * st.scale.double() + st.shift.double()) > 0
    d = d * mask
    xhat = (yb - st.mean.double()) * st.invstd.double()
    s = part.double().sum(0)
    for j, want in enumerate((d.sum(0), (d * xhat).sum(0))):
        slack = 2e-4 * float((d.abs() * (1 if j == 0 else xhat.abs())).sum(0).max()) + 1e-3
        np.testing.assert_allclose(s[j].cpu().numpy(), want.cpu().numpy(), rtol=2e-3, atol=slack)


def _wgrad_ws(dy, x, dw, r, s, stride, pad, splits, ws, bnrelu=None):
    """frhip_conv_wgrad[_bnrelu] with an explicit workspace (a smaller one reaches tn_slab_splits' cap)"""
    ops = _ops()
    n, h, wd, c = x.shape
    k = dy.shape[3]
    P = ops._p
    if bnrelu is None:
        ops.check(_lib().frhip_conv_wgrad(ops.dt_of(x), P(dy), P(x), P(dw), n, h, wd, c, k, r, s, stride, pad, splits, P(ws),
                                          ws.numel() * 4, ops._s()), "frhip_conv_wgrad")
    else:
        ops.check(_lib().frhip_conv_wgrad_bnrelu(ops.dt_of(x), P(dy), P(x), P(bnrelu.scale), P(bnrelu.shift), P(dw), n, h, wd, c, k,
                                                 r, s, stride, pad, splits, P(ws), ws.numel() * 4, ops._s()), "frhip_conv_wgrad_bnrelu")
    return dw


WGRAD_PARAMS = [(d, c) for c in CFG2_CONVS + RAGGED_CONVS for d in _dtypes_for(c)]


@pytest.mark.parametrize("dtype,case", WGRAD_PARAMS, ids=CONV_IDS)
def test_conv_wgrad_on_poisoned_memory(dtype, case):
    """splits 0 (heuristic), 1 and 3; a request that ksteps_per_split rounding cuts down; a count capped by a small workspace"""
    ops = _ops()
    n, h, w, c, k, r, stride, pad = case
    x, _ = _conv_case_inputs(case, dtype)
    ho, wo = ops.conv_out_hw(h, w, r, r, stride, pad)
    dy = (rnd(3, (n, ho, wo, k)) * 0.1).to(dtype)
    ref = ref_wgrad(dy, x, r, r, stride, pad)
    scale = float(ref.abs().max())
    ksteps = (n * ho * wo + 63) // 64
    # rounding: the smallest request s with ceil(ksteps / ceil(ksteps / s)) < s
    rounded = next((sp for sp in range(2, min(ksteps, 64) + 1) if (ksteps + (ksteps + sp - 1) // sp - 1) // ((ksteps + sp - 1) // sp) < sp),
                   None)
    slab = k * r * r * c
    variants = [("splits=0", 0, None), ("splits=1", 1, None), ("splits=3", 3, None)]
    if rounded is not None:
        variants.append(("splits=%d (rounded down)" % rounded, rounded, None))
    variants.append(("splits=8, workspace of 2.5 slabs", 8, (5 * slab) // 2 // 4 * 4))
    for name, splits, ws_elems in variants:
        def call():
            dw = torch.zeros((k, r, r, c), dtype=torch.float32, device="cuda")          # caller-zeroed accumulator
            ws = ops.workspace(x.device) if ws_elems is None else torch.empty(ws_elems, dtype=torch.float32, device="cuda")
            return (_wgrad_ws(dy, x, dw, r, r, stride, pad, splits, ws),)
        dw, = poisoned_parity(call)
        np.testing.assert_allclose(dw.double().cpu().numpy(), ref.cpu().numpy(), rtol=2e-3 if dtype == torch.bfloat16 else 2e-4,
                                   atol=1e-3 * scale, err_msg=name)


BNRELU_CASES = [(512, 56, 56, 64, 64), (512, 28, 28, 128, 128), (512, 14, 14, 256, 256), (512, 7, 7, 512, 512), (9, 7, 7, 64, 64),
                (3, 14, 14, 128, 64), (5, 13, 13, 64, 128)]


@pytest.mark.parametrize("case", BNRELU_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_bnrelu_forward_and_weight_gradient_on_poisoned_memory(case):
    """conv_fwd_bnrelu with act_out (a caller buffer the kernel overwrites), conv_wgrad_bnrelu, and conv_fwd_affine (eval-mode BN folded)"""
    ops = _ops()
    n, h, w, c, k = case
    dtype = torch.bfloat16
    x = (rnd(11, (n, h, w, c)) * 2 + 0.3).to(dtype)
    wt = (rnd(12, (k, 3, 3, c)) * (1.0 / (9 * c) ** 0.5)).to(dtype)
    rows = n * h * w
    st = ops.bn_finalize(ops.colstats(x.view(rows, c)), rows, 1 + 0.1 * rnd(13, (c,)), 0.1 * rnd(14, (c,)), None, None)
    if not ops.conv_bnrelu_fusable(x, wt, 1, 1):
        pytest.skip("not a fusable shape")      # never taken for the listed shapes (asserted below through the count of runs)

    def fwd():
        act = torch.empty_like(x)
        y, part = ops.conv_fwd_bnrelu(x, st, wt, 1, 1, act_out=act)
        return y, part, act
    y, part, act = poisoned_parity(fwd)
    a_ref = torch.relu(x.double() * st.scale.double() + st.shift.double())
    close(act, a_ref, dtype)
    close(y, ref_conv(act, wt, 1, 1), dtype)
    stats_match_stored(part, y)
    dy = (rnd(15, (n, h, w, k)) * 0.1).to(dtype)
    ref = ref_wgrad(dy, act, 3, 3, 1, 1)
    for splits in (0, 1, 3):
        dw, = poisoned_parity(lambda: (ops.conv_wgrad_bnrelu(dy, x, st, torch.zeros((k, 3, 3, c), device="cuda"), 3, 3, 1, 1, splits),))
        np.testing.assert_allclose(dw.double().cpu().numpy(), ref.cpu().numpy(), rtol=2e-3, atol=1e-3 * float(ref.abs().max()))
    # eval-mode BatchNorm folded into the store epilogue, with a residual
    aff = ops.bn_eval_affine(1 + 0.1 * rnd(16, (k,)), 0.1 * rnd(17, (k,)), 0.1 * rnd(18, (k,)), 1 + 0.1 * rnd(19, (k,)).abs())
    res = rnd(20, (n, h, w, k)).to(dtype)
    ya, = poisoned_parity(lambda: (ops.conv_fwd_affine(x, wt, aff, 1, 1, relu=True, residual=res),))
    want = torch.relu(ref_conv(x, wt, 1, 1) * aff.scale.double() + aff.shift.double() + res.double())
    close(ya, want, dtype)


@pytest.mark.parametrize("case", [(512, 256, 256), (37, 128, 192), (8, 256, 256), (3, 128, 64)], ids=lambda c: "x".join(map(str, c)))
def test_rows14_and_chained_weight_gradients_on_poisoned_memory(case):
    """the 14 x 14 rows kernel (through conv_wgrad), and a chain of three links + conv_wgrad_chain_finish on poisoned slab buffers"""
    ops = _ops()
    n, c, k = case
    x = rnd(21, (n, 14, 14, c)).bfloat16()
    dy = (rnd(22, (n, 14, 14, k)) * 0.1).bfloat16()
    ref = ref_wgrad(dy, x, 3, 3, 1, 1)
    tolw = dict(rtol=2e-3, atol=1e-3 * float(ref.abs().max()))
    dw, = poisoned_parity(lambda: (ops.conv_wgrad(dy, x, torch.zeros((k, 3, 3, c), device="cuda"), 3, 3, 1, 1),))
    np.testing.assert_allclose(dw.double().cpu().numpy(), ref.cpu().numpy(), **tolw)
    if not ops.conv_wgrad_chain_ok(dy, x, 3, 3, 1, 1):
        return
    x2 = rnd(23, (n, 14, 14, c)).bfloat16()
    dy2 = (rnd(24, (n, 14, 14, k)) * 0.1).bfloat16()
    ref2 = ref_wgrad(dy2, x2, 3, 3, 1, 1)

    def chain():
        bufs = ops.chain_slabs(x.device)
        dws = [torch.zeros((k, 3, 3, c), device="cuda") for _ in range(3)]
        link = None
        for i, (dd, xx) in enumerate(((dy, x), (dy2, x2), (dy, x))):
            link = ops.conv_wgrad_chain(dd, xx, dws[i], bufs[i & 1], link)
        ops.conv_wgrad_chain_finish(link)
        return dws
    d0, d1, d2 = poisoned_parity(chain)
    for got, want in ((d0, ref), (d1, ref2), (d2, ref)):
        np.testing.assert_allclose(got.double().cpu().numpy(), want.cpu().numpy(), **tolw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(96, 200, 208, 64), (512, 512, 512, 25088), (3000, 128, 128, 256), (70, 24, 24, 32),
                                   (4096, 1525, 1528, 512)], ids=lambda s: "x".join(map(str, s)))
def test_gemm_tn_and_overwrite_on_poisoned_memory(dtype, shape):
    """out += P^T Q (caller-zeroed out) and out = P^T Q into a buffer that need not be initialised; (512, 512, 512, 25088) is the fc
    weight gradient of the bench step, (4096, 1525, ...) the cfg-3 head shard"""
    ops = _ops()
    m, kc, ldp, c = shape
    p = rnd(31, (m, ldp)).to(dtype)
    qq = rnd(32, (m, c)).to(dtype)
    ref = p[:, :kc].double().t() @ qq.double()
    t = dict(rtol=2e-4, atol=2e-4 * float(ref.abs().max()))
    for splits in (0, 3):
        out, = poisoned_parity(lambda: (ops.gemm_tn(p, qq, torch.zeros((kc, c), device="cuda"), kc=kc, splits=splits),))
        np.testing.assert_allclose(out.double().cpu().numpy(), ref.cpu().numpy(), **t)
    out, = poisoned_parity(lambda: (ops.gemm_tn(p, qq, torch.empty((kc, c), device="cuda"), kc=kc, overwrite=True),))
    np.testing.assert_allclose(out.double().cpu().numpy(), ref.cpu().numpy(), **t)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mnk", [(512, 512, 25088), (16, 512, 1024), (200, 64, 128), (300, 72, 64)], ids=lambda s: "x".join(map(str, s)))
def test_gemm_nt_splitk_on_poisoned_memory(dtype, mnk):
    """out = a b^T + bias with per-split slabs in the workspace; (512, 512, 25088) is the fc of the bench step"""
    ops = _ops()
    m, n, k = mnk
    a, b = rnd(41, (m, k)).to(dtype), (rnd(42, (n, k)) * k ** -0.5).to(dtype)
    bias = rnd(43, (n,))
    out, = poisoned_parity(lambda: (ops.gemm_nt_splitk(a, b, bias, splits=16),))
    ref = a.double() @ b.double().t() + bias.double()
    np.testing.assert_allclose(out.double().cpu().numpy(), ref.cpu().numpy(), rtol=2e-4, atol=2e-4 * float(ref.abs().max()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mnk", [(600, 256, 64), (5000, 512, 128), (300, 72, 64), (3136, 384, 128), (1000, 200, 192)],
                         ids=lambda s: "x".join(map(str, s)))
def test_linear_forward_and_gelu_gradient_on_poisoned_memory(dtype, mnk):
    ops = _ops()
    m, n, k = mnk
    a, w = rnd(51, (m, k)).to(dtype), (rnd(52, (n, k)) * k ** -0.5).to(dtype)
    bias = 0.1 * rnd(53, (n,))
    out, act, part = poisoned_parity(lambda: ops.linear_fwd(a, w, bias, want_act=True, want_stats=True))
    pre = a.double() @ w.double().t() + bias.double()
    close(out, pre, dtype)
    close(act, F.gelu(out.double()), dtype)
    stats_match_stored(part, out)
    dy = rnd(54, (m, k)).to(dtype)
    wt = (rnd(55, (n, k)) * k ** -0.5).to(dtype)
    into = torch.zeros(n, device="cuda")

    def dgrad():
        dx, cs = ops.linear_dgrad_gelu(dy, wt, out, want_colsum=True)
        into.zero_()
        _, cs2 = ops.linear_dgrad_gelu(dy, wt, out, want_colsum=True, colsum_into=into)
        return dx, cs, cs2.clone()
    dx, cs, cs2 = poisoned_parity(dgrad)
    x64 = out.double()
    gelu_d = 0.5 * (1 + torch.erf(x64 / 2 ** 0.5)) + x64 * torch.exp(-0.5 * x64 * x64) / (2 * np.pi) ** 0.5
    close(dx, (dy.double() @ wt.double().t()) * gelu_d, dtype)
    want = dx.double().sum(0)
    slack = 1e-5 * float(dx.double().abs().sum(0).max()) + 1e-3
    np.testing.assert_allclose(cs.double().cpu().numpy(), want.cpu().numpy(), rtol=1e-3, atol=slack)
    np.testing.assert_allclose(cs2.double().cpu().numpy(), want.cpu().numpy(), rtol=1e-3, atol=slack)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rc", [(300, 64), (4 * 7 * 7, 512), (2000, 128), (512 * 49, 512), (512, 512), (70, 32)],
                         ids=lambda s: "x".join(map(str, s)))
def test_batchnorm_passes_on_poisoned_memory(dtype, rc):
    """colstats -> bn_finalize (running statistics) -> bn_apply; bn_backward without a part, with one, with a per-sample scale;
    sum_partials through colsum_accumulate"""
    ops = _ops()
    rows, c = rc
    y = (rnd(61, (rows, c)) * 2 + 0.5).to(dtype)
    dout = rnd(62, (rows, c)).to(dtype)
    gamma, beta = 1 + 0.1 * rnd(63, (c,)), 0.1 * rnd(64, (c,))
    rm0, rv0 = 0.1 * rnd(65, (c,)), 1 + 0.1 * rnd(66, (c,)).abs()

    def fwd():
        rm, rv = rm0.clone(), rv0.clone()
        st = ops.bn_finalize(ops.colstats(y), rows, gamma, beta, rm, rv)
        out = ops.bn_apply(y, st, relu=True)
        acc = torch.zeros(c, device="cuda")
        ops.colsum_accumulate(y, acc)
        return out, rm, rv, st.mean.clone(), st.invstd.clone(), acc
    out, rm, rv, mean, invstd, acc = poisoned_parity(fwd)
    y64 = y.double()
    mu, var = y64.mean(0), y64.var(0, unbiased=False)
    np.testing.assert_allclose(mean.double().cpu().numpy(), mu.cpu().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(invstd.double().cpu().numpy(), (1 / (var + 1e-5).sqrt()).cpu().numpy(), rtol=1e-4)
    np.testing.assert_allclose(rm.double().cpu().numpy(), (0.9 * rm0.double() + 0.1 * mu).cpu().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(rv.double().cpu().numpy(), (0.9 * rv0.double() + 0.1 * var * rows / (rows - 1)).cpu().numpy(),
                               rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(acc.double().cpu().numpy(), y64.sum(0).cpu().numpy(), rtol=1e-4, atol=1e-4 * rows)
    xhat = (y64 - mu) / (var + 1e-5).sqrt()
    close(out, torch.relu(xhat * gamma.double() + beta.double()), dtype, 4.0)
    st = ops.bn_finalize(ops.colstats(y), rows, gamma, beta, None, None)

    def bwd_ref(d):
        db = d.sum(0)
        dg = (d * xhat).sum(0)
        return (gamma.double() / (var + 1e-5).sqrt()) * (d - db / rows - xhat * dg / rows), dg, db

    for relu in (False, True):
        def bwd():
            dg, db = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
            return ops.bn_backward(dout, y, st, gamma, dg, db, relu_mask=relu), dg, db
        dy, dg, db = poisoned_parity(bwd)
        d = dout.double() * ((xhat * gamma.double() + beta.double()) > 0) if relu else dout.double()
        want, wdg, wdb = bwd_ref(d)
        close(dy, want, dtype)
        np.testing.assert_allclose(dg.double().cpu().numpy(), wdg.cpu().numpy(), rtol=2e-3, atol=2e-2 if dtype == torch.bfloat16 else 2e-3)
        np.testing.assert_allclose(db.double().cpu().numpy(), wdb.cpu().numpy(), rtol=2e-3, atol=2e-2 if dtype == torch.bfloat16 else 2e-3)
    if rows % 4 == 0:
        keep = 0.75
        rs = torch.tensor([0.0, 1 / keep, 1 / keep, 0.0], device="cuda").repeat(1)
        rows_per = rows // 4

        def bwd_rs():
            dg, db = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
            return ops.bn_backward(dout, y, st, gamma, dg, db, rowscale=rs, rows_per=rows_per), dg, db
        dy, dg, db = poisoned_parity(bwd_rs)
        scale = rs.double().repeat_interleave(rows_per)[:, None]
        want, wdg, wdb = bwd_ref(dout.double() * scale)
        close(dy, want, dtype)
        np.testing.assert_allclose(db.double().cpu().numpy(), wdb.cpu().numpy(), rtol=2e-3, atol=2e-2 if dtype == torch.bfloat16 else 2e-3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 12, 10), (3, 23, 57), (16, 112, 112)], ids=lambda s: "x".join(map(str, s)))
def test_recompute_stem_on_poisoned_memory(dtype, shape):
    """stem_stats -> stem_fwd (pool + arg-max) -> stem_gram (blocks + the extra row) -> stem_bwd (partials, slabs, both weight-gradient
    forms), and the im2col stem's kp padding columns"""
    ops = _ops()
    b, h, w = shape
    x = rnd(71, (b, 3, h, w)).clamp(-1, 1)
    w27 = rnd(72, (64, 27), 0.2)
    gamma, beta = 1 + 0.1 * rnd(73, (64,)), 0.1 * rnd(74, (64,))
    wp = ops.pack_stem(w27, dtype, kp=32)

    def fwd():
        part = ops.stem_stats(x, wp)
        st = ops.bn_finalize(part, b * h * w, gamma, beta, None, None)
        pooled, arg = ops.stem_fwd(x, wp, st)
        gram = ops.stem_gram(x, dtype)
        return part, pooled, arg, gram, st.mean.clone(), st.invstd.clone(), st.scale.clone(), st.shift.clone()
    part, pooled, arg, gram, mean, invstd, scale, shift = poisoned_parity(fwd)
    xq = x.to(dtype).double().cpu()
    wq = w27.to(dtype).double().cpu().view(64, 3, 3, 3).permute(0, 3, 1, 2)    # [K][R][S][C] -> [K][C][R][S]
    y0 = F.conv2d(xq, wq, None, 1, 1)
    s = part.double().sum(0)
    np.testing.assert_allclose(s[0].cpu().numpy(), y0.sum((0, 2, 3)).cpu().numpy(), rtol=1e-3, atol=1e-3 * float(y0.abs().sum((0, 2, 3)).max()) * 1e-2 + 1e-2)
    c4 = lambda v: v.double().cpu()[None, :, None, None]      # noqa: E731
    a0 = torch.relu((y0 - c4(mean)) * c4(invstd) * c4(gamma) + c4(beta))
    p0 = F.max_pool2d(a0, 3, 2, 1).permute(0, 2, 3, 1)
    close(pooled, p0, dtype, 3.0)
    st = ops.bn_finalize(part, b * h * w, gamma, beta, None, None)
    dpool = rnd(75, tuple(pooled.shape)).to(dtype)
    for use_gram in (False, True):
        def bwd():
            dg, db, dw = torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda"), torch.zeros((64, 27), device="cuda")
            ops.stem_bwd(x, wp, dpool, arg, st, gamma, dg, db, dw, gram=gram if use_gram else None, pooled=pooled if use_gram else None)
            return dg, db, dw
        poisoned_parity(bwd)
    col = poisoned_parity(lambda: (ops.stem_im2col(x, dtype),))[0]
    kp = col.shape[1]
    assert not col[:, 27:].float().any(), "the kp padding columns of the im2col stem must be written as zeros"
    want = F.unfold(x.to(dtype).double(), 3, padding=1).transpose(1, 2).reshape(b * h * w, 3, 9).transpose(1, 2).reshape(-1, 27)
    close(col[:, :27], want, dtype)
    assert kp in (32, 64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(512, 122000, 512), (24, 1003, 128), (130, 200, 512), (4096, 1525, 512)], ids=lambda s: "x".join(map(str, s)))
def test_head_kernels_on_poisoned_memory(dtype, shape):
    """l2norm_rows, head_fwd (pm / ps group buffers), head_bwd_dt (dT / dTt pad columns), head_dw or its gemm_tn fallback, l2norm_bwd"""
    ops = _ops()
    from oracle import head_ref
    n, classes, d = shape
    emb = rnd(81, (n, d))
    w = rnd(82, (classes, d)) * 0.05
    lab = torch.randint(0, classes, (n,), generator=torch.Generator().manual_seed(83)).to(torch.int32).cuda()
    lab[2] = -1
    s, m = 30.0, 0.35
    from nets.PartialFC import HipHeadKernels
    hk = HipHeadKernels(dtype)

    def run():
        eh, en = hk.normalize(emb)
        wh, wn = hk.normalize(w)
        zt, rmax, rsum = hk.forward_stats(eh, wh, lab, s, m)
        qv = hk.target_prob(zt, lab, rmax, rsum)
        loss = hk.loss(qv)
        dt, dtt = ops.head_bwd_dt(eh, wh, lab, s, m, rmax, rsum, 1.0 / n, transposed=True)
        d_e, d_w = hk.backward(eh, en, wh, wn, lab, s, m, rmax, rsum, n, None)
        return loss, eh, en, zt, rmax, rsum, dt, dtt, d_e, d_w
    loss, eh, en, zt, rmax, rsum, dt, dtt, d_e, d_w = poisoned_parity(run)
    ldt = dt.shape[1]
    assert not dt[:, classes:].float().any() and not dtt[:, n:].float().any(), "pad columns of dT / dTt must be written as zeros"
    assert torch.equal(dtt[:, :n].t(), dt[:, :classes])
    if n * classes > 50_000_000:
        return                                  # the oracle comparison at this size lives in test_head_gpu.py
    ll = lab.long().cpu()
    e64, w64 = emb.double().cpu(), w.double().cpu()
    ehr, enr = head_ref.l2_normalize(e64)
    whr, wnr = head_ref.l2_normalize(w64)
    raw = ehr @ whr.t()
    z, slope = head_ref.arcface_logits(raw.clamp(-1, 1), ll, s, m)
    loss_ref, grads = head_ref.dist_cross_entropy([z], [ll])
    dcos = grads[0] * s * slope * ((raw >= -1) & (raw <= 1))
    d_e_ref = head_ref.l2_normalize_bwd(dcos @ whr, ehr, enr)
    d_w_ref = head_ref.l2_normalize_bwd(dcos.t() @ ehr, whr, wnr)
    rt = 1e-3 if dtype == torch.float32 else 3e-2
    np.testing.assert_allclose(float(loss), float(loss_ref), rtol=rt)
    np.testing.assert_allclose(d_e.double().cpu().numpy(), d_e_ref.numpy(), rtol=rt, atol=rt * float(d_e_ref.abs().max()))
    np.testing.assert_allclose(d_w.double().cpu().numpy(), d_w_ref.numpy(), rtol=rt, atol=rt * float(d_w_ref.abs().max()))
    assert ldt >= classes


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [(2, 14, 14, 128, 4, 0), (3, 7, 7, 256, 8, 0), (1, 28, 28, 64, 2, 3), (4, 12, 12, 128, 4, 3)],
                         ids=lambda s: "x".join(map(str, s)))
def test_window_attention_on_poisoned_memory(dtype, case):
    """winattn_fwd / winattn_bwd (plain, with the fused column sums, with the q / v bias gradients added into accumulators) on poisoned
    outputs and a poisoned workspace.  d(bias), d(scale) and the column sums are sums over windows: each workgroup stores its partial sums
    to the workspace and one pass adds them in a fixed order, so they too are bit-identical from run to run (fp32 atomics, as before,
    made them differ in the last bits).  (4, 12, 12, ...) has 6 x 6 windows: n = 36 < 49 partial-sum rows per head."""
    ops = _ops()
    b, h, w, c, heads, shift = case
    ws = 6 if h % 7 else 7
    rows = b * h * w
    qkv = rnd(91, (rows, 3 * c)).to(dtype)
    dout = rnd(92, (rows, c)).to(dtype)
    bias = 0.1 * rnd(93, (heads, ws * ws, ws * ws))
    scale = 1 + 0.1 * rnd(94, (heads,)).abs()
    out, = poisoned_parity(lambda: (ops.winattn_fwd(qkv, bias, scale, b, h, w, heads, ws, shift),))
    plain = poisoned_parity(lambda: ops.winattn_bwd(qkv, dout, bias, scale, b, h, w, heads, ws, shift))
    assert bool(torch.isfinite(out.float()).all())
    if dtype != torch.bfloat16:
        return                                        # the column-sum forms are bf16 (MFMA kernels) only
    dqkv, dbias, dscale, colsum = poisoned_parity(lambda: ops.winattn_bwd(qkv, dout, bias, scale, b, h, w, heads, ws, shift,
                                                                          want_colsum=True))
    assert torch.equal(dqkv, plain[0]) and torch.equal(dbias, plain[1]) and torch.equal(dscale, plain[2])

    def qv():
        gq, gv = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
        r = ops.winattn_bwd(qkv, dout, bias, scale, b, h, w, heads, ws, shift, want_colsum=True, qv_grads=(gq, gv))
        return r[0], r[1], r[2], gq, gv
    _, _, _, gq, gv = poisoned_parity(qv)
    assert torch.equal(gq, colsum[:c]) and torch.equal(gv, colsum[2 * c:])
    want = dqkv.double().sum(0)
    np.testing.assert_allclose(colsum.double().cpu().numpy(), want.cpu().numpy(), rtol=1e-3,
                               atol=1e-5 * float(dqkv.double().abs().sum(0).max()) + 1e-3)


@pytest.mark.parametrize("case", [(4, 14, 14, 128, 128, 3, 1, 1), (3, 7, 7, 256, 512, 3, 1, 1), (2, 28, 28, 128, 256, 1, 2, 0),
                                  (512, 7, 7, 512, 512, 3, 1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_fp8_conv_and_linear_partials_on_poisoned_memory(case):
    ops = _ops()
    n, h, w, c, k, r, stride, pad = case
    x = rnd(101, (n, h, w, c)).clamp(-4, 4)
    wt = rnd(102, (k, r, r, c)) * (1.0 / (r * r * c) ** 0.5)
    w8, wscale = ops.quant_fp8_weights(wt)
    x8 = ops.quant_fp8(x.bfloat16())
    y, part = poisoned_parity(lambda: ops.conv_fwd_fp8(x8, w8, wscale, stride, pad))
    stats_match_stored(part, y)
    m = n * h * w
    a8 = x8.view(m, c)
    lw8, lscale = ops.quant_fp8_weights(wt.reshape(k, -1)[:, :c].contiguous())
    bias = 0.1 * rnd(103, (k,))
    out, lpart = poisoned_parity(lambda: ops.linear_fwd_fp8(a8, lw8, lscale, bias, want_stats=True))
    stats_match_stored(lpart, out)
