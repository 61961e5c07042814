"""CurricularFace (hard negatives re-weighted by a running mean of the target cosines) on the MI355X against the float64 restatement in
tests/curricular_double.py: the threshold kernel, exact routing of every non-target element through the explicit-logit kernels and the
fused head (both dtypes, one and three centres), the degenerate route that must be plain ArcFace, the fused head in fp32 mode at world
sizes 1 and 2 (real ranks on gloo, every rank on cuda:0), the bf16 head, three sub-centres, the stand-alone module and two optimisation
steps through Model with conf.margin_loss = CurricularFace.

Condition, not a tolerance: no branch may be decided by rounding.  The head inputs (curricular_double.case) keep every non-target cosine
>= 2e-4 from its row's threshold and >= 1e-3 from +-1, every target >= 1e-3 from theta; curricular_double.assert_case asserts it on the
double, and that rows whose negatives are all hard, rows with none and mixed rows occur.  2e-4 is enough: the fp32 dot error is
d 2^-24 = 3.1e-5 at d = 512 and the threshold's sensitivity to the target cosine is below 1.9 for targets <= 0.9 at m = 0.5."""
import ctypes
import math
import os
import sys
import tempfile
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import head_ref, recipe, resnet_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
S, M, ALPHA = 64.0, 0.5, 0.01
SENS = 1.9                                # |d thr / d target cosine| = cos m + c sin m / sqrt(1 - c^2): 1.87 at c = 0.9, m = 0.5


def _sens(tcos):
    """the largest sensitivity of a threshold to its target cosine over the owned rows of the double's tcos (an eighth added: the
    cosine the device holds is off by the dot error itself)"""
    c = tcos[tcos > -2.0].double().clamp(-1.0, 1.0)
    return float((math.cos(M) + c * math.sin(M) / torch.sqrt(1.0 - c * c)).abs().max()) * 1.125


@pytest.fixture(scope="module")
def pg():
    if not dist.is_initialized():
        d = tempfile.mkdtemp()
        dist.init_process_group("gloo", init_method="file://" + os.path.join(d, "pg"), rank=0, world_size=1)
    yield
    if dist.is_initialized():
        dist.destroy_process_group()


def _ulps(a, b):
    """largest distance in fp32 steps between two float32 tensors of equal sign"""
    return int((a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs().max())


def _f32(x):
    return torch.tensor([float(x)], dtype=torch.float64).float()


# ------------------------------------------------------------------------------------------------ 1. the threshold kernel
def _rows_input(n, ws, seed):
    g = torch.Generator().manual_seed(seed)
    values = torch.rand(n, generator=g) * 1.8 - 0.9
    owner = torch.randint(0, ws, (n,), generator=g)
    tcos = torch.full((ws, n), -2.0)
    tcos[owner, torch.arange(n)] = values
    if n == 1:
        tcos[:, 0], tcos[0, 0] = -2.0, 1.0
    elif n == 2:
        tcos[:, 0], tcos[ws - 1, 0] = -2.0, -1.0
        tcos[:, 1], tcos[0, 1] = -2.0, float("nan")                     # a NaN and nothing else: nobody owns the row
    else:
        tcos[:, 3] = -2.0                                               # nobody owns it
        tcos[:, 5], tcos[0, 5] = -2.0, float("nan")
        tcos[:, 7], tcos[ws - 1, 7] = -2.0, 1.0
        tcos[:, 8], tcos[0, 8] = -2.0, -1.0
        tcos[:, 9], tcos[0, 9], tcos[ws - 1, 9] = -2.0, float("nan"), 0.5          # ws = 2: a NaN beside the owner's value
        tcos[:, 11], tcos[0, 11] = -2.0, 1.0 + 2.0 ** -20                # a dot product that rounded past 1: clamped
    return tcos


@pytest.mark.parametrize("update", [True, False])
@pytest.mark.parametrize("ws", [1, 2])
@pytest.mark.parametrize("n", [1, 2, 130])
def test_curricular_rows_kernel_vs_float64(n, ws, update):
    """thr within 2^-23 of the double rounded to fp32, unowned rows exactly 2.0f, t within one fp32 ulp of the double's (untouched without
    update); three successive calls give the three-fold EMA"""
    from curricular_double import merged, thresholds, update_t
    from frhip import ops
    tcos = _rows_input(n, ws, 13 * n + ws)
    owned = merged(tcos)[1]
    want = thresholds(tcos, M).float()
    t = torch.full((1,), 0.4, device="cuda")
    dev = tcos.cuda()
    ema = float(t)
    for call in range(3):
        before = t.cpu().clone()
        thr = ops.curricular_rows(dev, M, ALPHA, t, update).cpu()
        assert thr.dtype == torch.float32 and thr.shape == (n,)
        assert float((thr - want).abs().max()) <= 2.0 ** -23
        assert bool((thr[~owned] == 2.0).all()) and bool((thr[owned] <= 1.0).all())
        if not update:
            assert torch.equal(t.cpu(), before)
            continue
        step = _f32(update_t(tcos, before, ALPHA))
        ema = float(update_t(tcos, ema, ALPHA))
        print("n=%d ws=%d call %d: t %.9g (double from the device's previous t %.9g, pure double %.9g)" % (n, ws, call, float(t), float(step), ema))
        assert _ulps(t.cpu(), step) <= 1
        assert _ulps(t.cpu(), _f32(ema)) <= call + 1                     # one rounding to fp32 per call
    if update:
        assert float(t) != pytest.approx(0.4, abs=1e-6)


# ------------------------------------------------------------------------------------------------ 2. exact routing
def _exact_case(K, seed):
    """operands that are multiples of 1/8 with few non-zeros: every cosine an exact multiple of 1/64 in [-1, 1] in both dtypes"""
    n, classes, d = 130, 257, 64
    g = torch.Generator().manual_seed(seed)
    e = torch.zeros((n, d), dtype=torch.float64)
    for i in range(n):
        cols = torch.randperm(d, generator=g)[:4]
        e[i, cols] = (torch.randint(1, 5, (4,), generator=g) * (2 * torch.randint(0, 2, (4,), generator=g) - 1)).double() / 8
    w = torch.randint(-4, 5, (K * classes, d), generator=g).double() / 8
    labels = torch.randint(0, classes, (n,), generator=g)
    labels[6:12] = torch.tensor([0, 63, 64, 127, 128, 256])
    labels[1] = labels[0]
    labels[2] = -1
    planes = (e @ w.t()).view(n, K, classes)
    from subcenter_double import pool
    raw, win, _ = pool(planes)
    assert float(raw.abs().max()) <= 1.0 and torch.equal(raw * 64, (raw * 64).round())
    thr = torch.randint(-32, 33, (n,), generator=g).double() / 64
    odd = torch.arange(n) % 2 == 1
    thr[odd] = (2 * torch.randint(-32, 32, (n,), generator=g).double()[odd] + 1) / 128
    own = torch.nonzero(labels >= 0).flatten()
    onehot = torch.zeros(raw.shape, dtype=torch.bool)
    onehot[own, labels[own]] = True
    assert float(raw[onehot].abs().max()) < 1.0                                    # a target at +-1 has no finite slope
    ties = (raw == thr[:, None]) & ~onehot
    assert int(ties.sum()) >= 100 and int(ties[2].sum()) >= 1                      # exact ties, in the label -1 row as well
    return e, w, labels, raw, win, thr, onehot


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_exact_routing_of_every_negative(dtype, K):
    """s = 64, t = 0.25, thresholds that are multiples of 1/64 (exact ties: not hard) or odd multiples of 1/128 (strictly between values):
    every non-target logit is exact in fp32, so the explicit-logit kernels' non-target outputs and the head's part_max (groups without the
    row's target) and the label -1 row's rowmax must EQUAL the double's.  Row sums, target logits and dT: the fp32-mode criterion of
    tests/test_subcenter_gpu.py (rtol 1e-3, atol 1e-3 of the largest reference element); a bf16 dT adds its storage rounding, 2^-9."""
    from curricular_double import logits
    from frhip import ops
    from nets.ArcFace import CurrRows
    e, w, labels, raw, win, thr, onehot = _exact_case(K, 500 + K)
    n, classes = raw.shape
    d = e.shape[1]
    tt = 0.25
    z, slope = logits(raw, labels, thr, tt, S, M)
    assert torch.equal(z[~onehot].float().double(), z[~onehot])                    # exact in fp32
    t_dev = torch.full((1,), tt, device="cuda")
    rows = CurrRows(S, M, thr.float().cuda(), t_dev)
    # -- the explicit-logit pair on the pooled cosines
    cos32 = raw.float().cuda()
    out = ops.margin_fwd_curr(cos32, labels.cuda(), rows).cpu()
    gin = ops.margin_bwd_curr(torch.ones_like(cos32), cos32, labels.cuda(), rows).cpu()
    assert torch.equal(out[~onehot].double(), z[~onehot]) and torch.equal(gin[~onehot].double(), slope[~onehot])
    np.testing.assert_allclose(out[onehot].numpy(), z[onehot].numpy(), rtol=1e-6, atol=1e-5)
    np.testing.assert_allclose(gin[onehot].numpy(), slope[onehot].numpy(), rtol=1e-5, atol=1e-5)
    # -- the fused head at the C ABI
    lib, p = ops.lib(), ops._p
    eh, wh, lab = e.to(dtype).cuda(), w.to(dtype).cuda(), labels.to(torch.int32).cuda()
    groups = lib.frhip_head_groups(classes)
    pm = torch.full((groups, n), float("nan"), device="cuda")
    ps = torch.full((groups, n), float("nan"), device="cuda")
    zt, rmax, rsum = (torch.full((n,), float("nan"), device="cuda") for _ in range(3))
    tsub = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    desc = ops._margin_curr_desc(rows, n)
    head = (ops.dt_of(eh), p(eh), p(wh), p(lab), n, classes, d)
    if K == 1:
        ops.check(lib.frhip_head_fwd_curr(*head, ctypes.byref(desc), p(pm), p(ps), p(zt), p(rmax), p(rsum), ops._s()), "frhip_head_fwd_curr")
    else:
        ops.check(lib.frhip_head_fwd_sub_curr(*head, K, ctypes.byref(desc), p(pm), p(ps), p(zt), p(tsub), p(rmax), p(rsum), ops._s()),
                  "frhip_head_fwd_sub_curr")
    want_pm = torch.full((groups, n), float("-inf"), dtype=torch.float64)
    clean = torch.ones((groups, n), dtype=torch.bool)
    for gq in range(groups):
        lo, hi = 64 * gq, min(64 * gq + 64, classes)
        if lo < hi:
            want_pm[gq] = z[:, lo:hi].max(dim=1).values
            clean[gq] = ~onehot[:, lo:hi].any(dim=1)
    pm, zt, rmax, rsum = pm.cpu(), zt.cpu(), rmax.cpu(), rsum.cpu()
    assert int(clean.sum()) >= (groups - 1) * n and bool(clean[:, 2].all())
    assert torch.equal(pm[clean].double(), want_pm[clean])
    want_max = z.max(dim=1).values
    assert float(rmax[2]) == float(want_max[2]) and int(labels[2]) == -1
    want_sum = torch.exp(z - want_max[:, None]).sum(dim=1)
    own = torch.nonzero(labels >= 0).flatten()
    want_zt = torch.zeros(n, dtype=torch.float64)
    want_zt[own] = z[own, labels[own]]
    for name, got, want in (("part_max", pm[:groups - 1], want_pm[:groups - 1]), ("ztarget", zt[own], want_zt[own]), ("rowmax", rmax, want_max),
                            ("rowsum", rsum, want_sum)):
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-3, atol=1e-3 * float(want.abs().max()), err_msg=name)
    if K > 1:
        want_tsub = torch.full((n,), -1, dtype=torch.int32)
        want_tsub[own] = win[own, labels[own]].to(torch.int32)
        assert torch.equal(tsub.cpu(), want_tsub)
    dt, dtt = ops.head_bwd_dt(eh, wh, lab, S, M, rmax.cuda(), rsum.cuda(), 1.0 / n, transposed=True, margin=rows, subcenters=K)
    dt, dtt = dt.cpu().float().view(n, K, -1), dtt.cpu().float()
    prob = torch.exp(z - want_max[:, None]) / want_sum[:, None]
    dcos = (prob - onehot.double()) / n * slope
    rtol = 1e-3 + (2.0 ** -9 if dtype == torch.bfloat16 else 0.0)
    assert not dt[:, :, classes:].any() and not dtt[:, n:].any()
    for k in range(K):
        want = torch.where(win == k, dcos, torch.zeros_like(dcos))
        np.testing.assert_allclose(dt[:, k, :classes].numpy(), want.numpy(), rtol=rtol, atol=1e-3 * float(dcos.abs().max()), err_msg="dT plane %d" % k)
        assert torch.equal(dtt[k * classes:(k + 1) * classes, :n].t(), dt[:, k, :classes])


# ------------------------------------------------------------------------------------------------ 3. the degenerate route
def test_thresholds_of_two_reproduce_plain_arcface():
    """thr = +2 everywhere: nothing is hard, and the kernels must give what the plain ArcFace entry points give (fp32 mode)"""
    from frhip import ops
    from nets.ArcFace import CurrRows
    n, classes, d = 130, 257, 64
    g = torch.Generator().manual_seed(77)
    emb, weight = torch.randn((n, d), generator=g), torch.randn((classes, d), generator=g)
    labels = torch.randint(0, classes, (n,), generator=g)
    labels[6:12] = torch.tensor([0, 63, 64, 127, 128, 256])
    labels[5], labels[9] = -1, labels[8]
    eh, wh = ops.l2norm_rows(emb.cuda(), torch.float32)[0], ops.l2norm_rows(weight.cuda(), torch.float32)[0]
    lab = labels.to(torch.int32).cuda()
    rows = CurrRows(S, M, torch.full((n,), 2.0, device="cuda"), torch.full((1,), 0.4, device="cuda"))
    plain = ops.head_fwd(eh, wh, lab, S, M)
    curr = ops.head_fwd(eh, wh, lab, S, M, margin=rows)
    for name, a, b in zip(("ztarget", "rowmax", "rowsum"), curr, plain):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-6, err_msg=name)
    dt_plain = ops.head_bwd_dt(eh, wh, lab, S, M, plain[1], plain[2], 1.0 / n)
    dt_curr = ops.head_bwd_dt(eh, wh, lab, S, M, plain[1], plain[2], 1.0 / n, margin=rows)
    np.testing.assert_allclose(dt_curr.cpu().numpy(), dt_plain.cpu().numpy(), rtol=1e-5)


# ------------------------------------------------------------------------------------------------ shared head inputs
_CASES = {}


def _case(n, classes, d, dtype=torch.float32):
    """seeded inputs, built once per shape and shared (never modified: every user clones)"""
    from curricular_double import case
    key = (n, classes, d, dtype)
    if key not in _CASES:
        _CASES[key] = case(n, classes, d, 9300 + n + classes, M, dtype)
        print("case %s: at most %d nudges per row" % (key[:3], _CASES[key][3]))
    return _CASES[key][:3]


# ------------------------------------------------------------------------------------------------ 4. the fused head, fp32 mode
def _recording_kernels(P, dtype):
    class Recording(P.HipHeadKernels):
        """the HIP kernels, remembering the thresholds the head was handed"""
        seen = None

        def forward_stats(self, ehat, what, labels_i32, s, m, margin=None, subcenters=1):
            self.seen = margin.thr.cpu()
            return super().forward_stats(ehat, what, labels_i32, s, m, margin=margin, subcenters=subcenters)

    return Recording(dtype)


def _run_head(P, rank, ws, shape, rate, t0):
    """one rank of `ws`: its rows of the shared batch of shape[0] rows through PartialFC(margin_loss = CurricularFace) on the HIP kernels"""
    from nets.ArcFace import CurricularFace
    n, classes, d = shape
    b = n // ws
    dev = torch.device("cuda", 0)
    emb, weight, labels = _case(n, classes, d)
    conf = types.SimpleNamespace(emd_size=d, sample_rate=rate, mixed_precision=False, loss_s=S, loss_m=M, frhip_dtype="fp32")
    kern = _recording_kernels(P, torch.float32)
    pfc = P.PartialFC(conf, classes, margin_loss=CurricularFace, kernels=kern).to(dev)
    assert pfc.margin_softmax.t.is_cuda
    start, num = head_ref.shard_range(classes, ws, rank)
    with torch.no_grad():
        (pfc.weight if rate < 1 else pfc.weight_activated.data).copy_(weight[start:start + num].to(dev))
        pfc.margin_softmax.t.fill_(t0)
    dummy = torch.nn.Parameter(torch.zeros(1, device=dev))
    opt = torch.optim.SGD([{"params": [dummy]}, {"params": pfc.parameters()}], lr=0.1, momentum=0.9)
    mine = slice(rank * b, (rank + 1) * b)
    e = emb[mine].clone().to(dev).requires_grad_(True)
    torch.manual_seed(1000 + rank)                          # the sampling permutation comes from the CPU generator
    loss = pfc(e, labels[mine].clone().to(dev), opt)
    loss.backward()
    idx = pfc.weight_index if rate < 1 else torch.arange(pfc.num_local)
    return dict(loss=float(loss.detach()), d_emb=e.grad.cpu().numpy(), d_w=pfc.weight_activated.grad.cpu().numpy(),
                index=idx.cpu().numpy(), thr=kern.seen.numpy(), t=pfc.margin_softmax.t.cpu().numpy())


def _head_worker(rank, ws, path, ret, shape):
    """one rank, both sample rates and both starting values of t in one process group; results travel through files"""
    for p in (ROOT, os.path.join(ROOT, "face-recognition-pytorch_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import nets.PartialFC as P
    torch.set_num_threads(1)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="file://" + path, rank=rank, world_size=ws)
    for rate in (1.0, 0.3):
        for t0 in (0.0, 0.4):
            np.savez(os.path.join(ret, "r%.1f_t%.1f_rank%d.npz" % (rate, t0, rank)), **_run_head(P, rank, ws, shape, rate, t0))
    dist.destroy_process_group()


def _check_head(outs, ws, shape, rate, t0):
    """every rank against ONE evaluation of the double on the whole batch and the class rows the ranks activated; criteria of
    tests/test_adaface_gpu.py _check_head (loss rtol 1e-4; gradients rtol 1e-3, atol 1e-5 of the largest reference element).  t after the
    step: the double's, to the rounding of the buffer plus alpha x the fp32 dot error of the target cosines; the thresholds the head was
    handed: the double's, to SENS x that dot error plus their own rounding; both equal across ranks bit for bit."""
    from curricular_double import assert_case, cosines, head_reference, update_t
    n, classes, d = shape
    b = n // ws
    emb, weight, labels = _case(n, classes, d)
    tcos, thr, hard = assert_case(cosines(emb, weight), labels, M)
    assert float(tcos.max()) <= 0.9 + 1e-6 and _sens(tcos) / 1.125 <= SENS
    t1 = _f32(update_t(tcos, t0, ALPHA))
    rows, pos, offset = [], torch.full_like(labels, -1), 0
    for r in range(ws):
        start, num = head_ref.shard_range(classes, ws, r)
        index = torch.from_numpy(outs[r]["index"]).long()
        own = (labels >= start) & (labels < start + num)
        assert bool(torch.isin(labels[own] - start, index).all()), "a positive class was not activated"
        pos[own] = torch.searchsorted(index, labels[own] - start) + offset
        rows.append(index + start)
        offset += index.numel()
    if rate < 1:
        assert int(torch.unique(labels[labels >= 0]).numel()) < offset < classes      # negatives were drawn, class rows were dropped
    rows = torch.cat(rows)
    assert bool(hard[:, rows].any()) and not bool(hard[:, rows].all())
    ref = head_reference(emb, weight[rows], pos, S, M, thr, float(t1))
    dot_err = d * 2.0 ** -24
    offset = 0
    for r in range(ws):
        o = outs[r]
        k = o["index"].shape[0]
        refs = (("d_emb", ws * ref["d_emb"][r * b:(r + 1) * b].numpy()), ("d_w", ref["d_w"][offset:offset + k].numpy()))
        offset += k
        print("ws %d rank %d rate %.1f t0 %.1f %s: loss %.8g (double %.8g), t %.9g (double %.9g), max |thr - double| %.3g" % (
            ws, r, rate, t0, shape, float(o["loss"]), float(ref["loss"]), float(o["t"][0]), float(t1), float(np.abs(o["thr"] - thr.numpy()).max())),
            "".join("  max |%s - double| %.3g of %.3g" % (key, float(np.abs(o[key] - w_).max()), float(np.abs(w_).max())) for key, w_ in refs))
        assert abs(float(o["t"][0]) - float(t1)) <= ALPHA * dot_err + 2.0 ** -23 * abs(float(t1))
        assert float(np.abs(o["thr"] - thr.numpy()).max()) <= _sens(tcos) * dot_err + 2.0 ** -23
        assert np.array_equal(o["t"], outs[0]["t"]) and np.array_equal(o["thr"], outs[0]["thr"])          # equal across ranks, bit for bit
        np.testing.assert_allclose(float(o["loss"]), float(ref["loss"]), rtol=1e-4, err_msg="rank %d loss" % r)
        for key, w_ in refs:
            np.testing.assert_allclose(o[key], w_, rtol=1e-3, atol=1e-3 * float(np.abs(w_).max()) * 1e-2, err_msg="rank %d %s" % (r, key))


HEAD_SHAPES = [(130, 257, 512), (8, 40, 512)]       # two row tiles and three 128-class tiles with ragged ends; one tile


@pytest.mark.parametrize("t0", [0.0, 0.4])
@pytest.mark.parametrize("rate", [1.0, 0.3])
@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_fused_head_fp32_vs_float64(pg, shape, rate, t0):
    import nets.PartialFC as P
    _check_head([_run_head(P, 0, 1, shape, rate, t0)], 1, shape, rate, t0)


@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_fused_head_fp32_two_ranks_vs_float64(shape):
    """half the batch on each of two ranks: the target cosines are all-gathered, every rank derives the whole batch's thresholds and the
    same t; a row whose class the other shard owns has no exempt column and uses the threshold its owner produced"""
    ws = 2
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_head_worker, args=(ws, os.path.join(td, "pg"), td, shape), nprocs=ws, join=True)
        for rate in (1.0, 0.3):
            for t0 in (0.0, 0.4):
                outs = [dict(np.load(os.path.join(td, "r%.1f_t%.1f_rank%d.npz" % (rate, t0, r)))) for r in range(ws)]
                _check_head(outs, ws, shape, rate, t0)


# ------------------------------------------------------------------------------------------------ 5. bf16
def test_bf16_head_vs_float64():
    """(130, 257, 512) in bf16 through the kernels PartialFC calls; criteria of tests/test_adaface_gpu.py test_bf16_head_vs_float64 (loss
    rtol 3e-2; gradients rtol 0.1, atol 5 % of the largest reference element).  The double works on the SAME bf16-rounded normalised
    operands (read back from the device), and the band condition is asserted on their cosines."""
    import nets.PartialFC as P
    from curricular_double import CurricularHeadKernels, assert_case, thresholds, update_t
    from frhip import ops
    from nets.ArcFace import CurricularFace, CurrRows
    n, classes, d = 130, 257, 512
    t0 = 0.4
    emb, weight, labels = _case(n, classes, d, torch.bfloat16)
    kern = P.HipHeadKernels(torch.bfloat16)
    assert ops.lib().frhip_head_dw_ok(0, n, classes, d) == 1
    e_c, w_c, l_c = emb.cuda(), weight.cuda(), labels.to(torch.int32).cuda()
    ehat, enorm = kern.normalize(e_c)
    what, wnorm = kern.normalize(w_c)
    eh64, wh64 = ehat.cpu().double(), what.cpu().double()
    tcos64, thr64, hard = assert_case(eh64 @ wh64.t(), labels, M)
    t1 = _f32(update_t(tcos64, t0, ALPHA))
    double = CurricularHeadKernels()
    lab32 = labels.to(torch.int32)
    mg64 = CurrRows(S, M, thr64, t1)
    zt, rmax, rsum = double.forward_stats(eh64, wh64, lab32, S, M, margin=mg64)
    loss_ref = float(double.loss(double.target_prob(zt, lab32, rmax, rsum)))
    d_e_ref, d_w_ref = double.backward(eh64, enorm.cpu().double(), wh64, wnorm.cpu().double(), lab32, S, M, rmax, rsum, n,
                                       torch.ones(1, dtype=torch.float64), margin=mg64)
    mod = CurricularFace(S, M).cuda()
    with torch.no_grad():
        mod.t.fill_(t0)
    tcos = kern.head_target_cos(ehat, what, l_c)
    np.testing.assert_allclose(tcos.cpu().double().numpy(), tcos64.numpy(), rtol=0, atol=d * 2.0 ** -24)
    cr = mod.row_thresholds(tcos, kern)
    assert isinstance(cr, CurrRows) and cr.s == S and cr.t is mod.t
    assert abs(float(mod.t) - float(t1)) <= ALPHA * d * 2.0 ** -24 + 2.0 ** -23 * abs(float(t1))
    assert float((cr.thr.cpu().double() - thr64).abs().max()) <= _sens(tcos64) * d * 2.0 ** -24 + 2.0 ** -23
    zt, rmax, rsum = kern.forward_stats(ehat, what, l_c, S, M, margin=cr)
    loss = float(kern.loss(kern.target_prob(zt, l_c, rmax, rsum)))
    d_e, d_w = kern.backward(ehat, enorm, what, wnorm, l_c, S, M, rmax, rsum, n, torch.ones(1, device="cuda"), margin=cr)
    d_e, d_w = d_e.cpu(), d_w.cpu()
    print("bf16 CurricularFace: loss %.6g (double %.6g); max |dE - double| %.3g of %.3g; max |dW - double| %.3g of %.3g" % (
        loss, loss_ref, float((d_e.double() - d_e_ref).abs().max()), float(d_e_ref.abs().max()),
        float((d_w.double() - d_w_ref).abs().max()), float(d_w_ref.abs().max())))
    np.testing.assert_allclose(loss, loss_ref, rtol=3e-2)
    np.testing.assert_allclose(d_e.numpy(), d_e_ref.numpy(), rtol=0.1, atol=0.05 * float(d_e_ref.abs().max()))
    np.testing.assert_allclose(d_w.numpy(), d_w_ref.numpy(), rtol=0.1, atol=0.05 * float(d_w_ref.abs().max()))


# ------------------------------------------------------------------------------------------------ 6. three sub-centres
def test_fused_head_fp32_three_subcenters(pg):
    """conf.subcenters = 3: the cosine that is compared with the threshold and scaled is the pooled one (the maximum over the class's
    centres), the target cosine behind the threshold as well; tsub is subcenter_double's winner map, as for every other margin.
    Criteria of the fp32-mode head above."""
    import nets.PartialFC as P
    from curricular_double import BAND, head_reference, thresholds, update_t
    from nets.ArcFace import CurricularFace
    from subcenter_double import assert_case, case
    n, classes, d, K = 37, 150, 64, 3
    t0 = 0.4
    for seed in range(4500, 4520):                          # the first seed whose pooled cosines keep the band around the thresholds
        emb, weight, labels, res = case(n, classes, d, K, seed)
        own = torch.nonzero(labels >= 0).flatten()
        tcos = torch.full((n,), -2.0, dtype=torch.float64)
        tcos[own] = res["raw"][own, labels[own]]
        thr = thresholds(tcos, M)
        gap = (res["raw"] - thr[:, None]).abs()
        gap[own, labels[own]] = 1.0
        if float(gap.min()) >= BAND:
            break
    assert float(gap.min()) >= BAND
    assert_case(emb, weight, labels, K, res)
    theta = math.cos(math.pi - M)
    assert float((tcos[own] - theta).abs().min()) >= 1e-3
    hard = (res["raw"] > thr[:, None])
    hard[own, labels[own]] = False
    assert bool(hard.any()) and not bool(hard[own].all()) and not bool(hard[labels < 0].any())
    t1 = _f32(update_t(tcos, t0, ALPHA))
    ref = head_reference(emb, weight, labels, S, M, thr, float(t1), K=K)
    assert torch.equal(ref["win"], res["win"])
    dev = torch.device("cuda", 0)
    conf = types.SimpleNamespace(emd_size=d, sample_rate=1.0, mixed_precision=False, loss_s=S, loss_m=M, frhip_dtype="fp32", subcenters=K)
    kern = _recording_kernels(P, torch.float32)
    pfc = P.PartialFC(conf, classes, margin_loss=CurricularFace, kernels=kern).to(dev)
    with torch.no_grad():
        pfc.weight_activated.data.copy_(weight.to(dev))
        pfc.margin_softmax.t.fill_(t0)
    e = emb.clone().to(dev).requires_grad_(True)
    loss = pfc(e, labels.clone().to(dev), None)
    loss.backward()
    print("K = 3: loss %.8g (double %.8g), t %.9g (double %.9g), max |thr - double| %.3g" % (
        float(loss.detach()), float(ref["loss"]), float(pfc.margin_softmax.t), float(t1), float((kern.seen.double() - thr).abs().max())))
    tsub = torch.full((n,), -1, dtype=torch.int64)
    tsub[own] = ref["win"][own, labels[own]]
    assert torch.equal(pfc.last_target_sub.cpu().long(), tsub)
    assert float((kern.seen.double() - thr).abs().max()) <= _sens(tcos) * d * 2.0 ** -24 + 2.0 ** -23
    assert abs(float(pfc.margin_softmax.t) - float(t1)) <= ALPHA * d * 2.0 ** -24 + 2.0 ** -23 * abs(float(t1))
    np.testing.assert_allclose(float(loss.detach()), float(ref["loss"]), rtol=1e-4)
    for name, a, b_ in (("d_emb", e.grad.cpu().numpy(), ref["d_emb"].numpy()), ("d_w", pfc.weight_activated.grad.cpu().numpy(), ref["d_w"].numpy())):
        np.testing.assert_allclose(a, b_, rtol=1e-3, atol=1e-3 * float(np.abs(b_).max()) * 1e-2, err_msg=name)


# ------------------------------------------------------------------------------------------------ 7. the module, and through Model
def test_curricular_module_forward_backward_and_eval_vs_float64():
    """CurricularFace.forward(logits, labels) on explicit cosines (frhip_curricular_rows, then frhip_margin_fwd_curr / _bwd_curr): output and
    input gradient at the tolerances of tests/test_elastic_gpu.py's module test; the thresholds come from the fp32 cosines the module is
    given, and so do the double's.  Eval mode: the same with the t that stands, which does not move."""
    from curricular_double import assert_case, cosines, logits, update_t
    from nets.ArcFace import CurricularFace
    n, classes, d = 37, 150, 64
    emb, weight, labels = _case(n, classes, d)
    cos32 = cosines(emb, weight).float()                                      # the module's input
    tcos, thr, _ = assert_case(cos32.double(), labels, M)
    t0 = 0.4
    t1 = _f32(update_t(tcos, t0, ALPHA))
    upstream = torch.randn((n, classes), generator=torch.Generator().manual_seed(5))
    mod = CurricularFace(S, M).cuda()
    with torch.no_grad():
        mod.t.fill_(t0)
    for training in (True, False):
        mod.train(training)
        ref_in = cos32.double().requires_grad_(True)
        ref_out, _ = logits(ref_in, labels, thr, float(t1), S, M)
        ref_out.backward(upstream.double())
        leaf = cos32.cuda().requires_grad_(True)
        out = mod(leaf, labels.cuda())
        out.backward(upstream.cuda())
        assert torch.equal(leaf.detach().cpu(), cos32) and out.data_ptr() != leaf.data_ptr()         # not in place
        assert _ulps(mod.t.cpu(), t1) <= 1                                    # advanced once in training mode, untouched in eval mode
        print("module training=%s: max |out - double| %.3g, max |grad - double| %.3g" % (
            training, float((out.detach().cpu().double() - ref_out.detach()).abs().max()), float((leaf.grad.cpu().double() - ref_in.grad).abs().max())))
        np.testing.assert_allclose(out.detach().cpu().numpy(), ref_out.detach().numpy(), rtol=1e-6, atol=1e-5)
        np.testing.assert_allclose(leaf.grad.cpu().numpy(), ref_in.grad.numpy(), rtol=1e-5, atol=1e-5)
        t1 = mod.t.cpu().clone() if training else t1


def test_two_sgd_steps_through_model_conf_margin_loss_curricularface(pg):
    """conf.margin_loss = CurricularFace is all a user sets.  Two optimisation steps: finite losses, weights that move, t advanced at each
    step (from 0: alpha x the batch's mean target cosine), and losses that differ from plain ArcFace's on the same run (every negative of a
    fresh head is hard: its target cosines are near 0)"""
    from model.FR_PartialFC import Model
    from nets.ArcFace import ArcFace, CurricularFace
    classes, b = 256, 8
    torch.cuda.set_device(0)
    spec = resnet_ref.resnet_spec(resnet_ref.BLOCKS["ResNet18"])
    losses, ts = {}, []
    for name, factory in (("curricular", CurricularFace), ("arcface", ArcFace)):
        conf = types.SimpleNamespace(network="ResNet18", emd_size=512, img_size=112, local_rank=0, world_size=1, sample_rate=1.0,
                                     mixed_precision=False, loss_s=S, loss_m=M, n_classes=classes, optimizer="SGD", lr=0.1, wd=5e-4,
                                     mom=0.9, loss="PartialFC", lr_scheduler=None, frhip_dtype="fp32", ckpt_path=None, margin_loss=factory)
        model = Model(conf, None, "train")
        head = model.loss
        assert isinstance(head.margin_softmax, factory)
        sd = recipe.fill_state(spec, 777)
        for key, _, kd in spec:
            if kd in ("bn_w", "bn_rv"):
                sd[key].fill_(1.0)
            elif kd in ("bn_b", "bn_rm"):
                sd[key].zero_()
        model.encoder.load_state_dict(sd, strict=True)
        with torch.no_grad():
            head.weight_activated.data.copy_(recipe.normal(778, (classes, 512), 0.01).cuda())
        got = []
        for st in range(2):
            w_before = head.weight_activated.detach().cpu().clone()
            img, ids = recipe.images(779 + 10 * st, b), recipe.labels(780 + 10 * st, b, classes)
            got.append(float(model.training_step((img, ids.clone()))["loss"]))
            assert not torch.equal(head.weight_activated.detach().cpu(), w_before)
            if name == "curricular":
                assert head.margin_softmax.t.is_cuda
                ts.append(float(head.margin_softmax.t))
        assert all(math.isfinite(v) for v in got)
        losses[name] = got
    print("losses with CurricularFace: %s (t %s), with ArcFace: %s" % (losses["curricular"], ts, losses["arcface"]))
    assert ts[0] != 0.0 and ts[1] != ts[0] and abs(ts[0]) <= ALPHA and abs(ts[1]) <= 2 * ALPHA
    assert losses["curricular"][0] != losses["arcface"][0] and losses["curricular"][1] != losses["arcface"][1]
