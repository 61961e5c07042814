"""ElasticFace (random per-row margins, ranked for the "+" variants) on the MI355X against the float64 restatement in
tests/elastic_double.py: the draw kernel, the target-cosine pre-pass and the ranking kernel (both exact), the stand-alone module, the
fused head in fp32 mode at world sizes 1 and 2 (real ranks on gloo, every rank on cuda:0), the bf16 head, three sub-centres, and two
optimisation steps through Model with conf.margin_loss = partial(ElasticFace, plus=True).

The head inputs (elastic_double.case) hold targets in columns 0, 63, 64, 127, 128 and the last class, a duplicate label, a label -1 row,
a target pushed past pi - eps and a raw cosine above 1 - eps; every other target keeps 1e-3 from each boundary for margins within five
sigma of m, and two distinct target cosines are at least 1e-4 apart, far above the fp32 dot error: no rank and no branch is decided by
rounding (elastic_double.assert_case asserts all of it on the double)."""
import functools
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
S, EPS, SEED = 64.0, 1e-3, 77
VARIANTS = {"arc": (0.5, 0.05, "arc", False), "cos": (0.35, 0.05, "cos", False), "arc_plus": (0.5, 0.0175, "arc", True)}
STEP0 = 5 + 2 ** 32                      # where the tests start the counter: both words of it reach the generator


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


def _step(value=STEP0):
    return torch.full((1,), value, dtype=torch.int64, device="cuda")


# ------------------------------------------------------------------------------------------------ 1. the draw kernel
@pytest.mark.parametrize("update", [True, False])
@pytest.mark.parametrize("kind", ["arc", "cos"])
@pytest.mark.parametrize("n", [1, 37, 1000, 4097])
def test_elastic_margins_kernel_vs_float64(n, kind, update):
    """at most 1 fp32 ulp from the double: device and host float64 log / cos may differ in the last bit before the rounding to fp32"""
    from elastic_double import draws
    from frhip import ops
    m, std = (0.5, 0.05) if kind == "arc" else (0.35, 0.05)
    want = draws(n, m, std, SEED, STEP0, update)
    step = _step()
    m_ang, m_add = ops.elastic_margins(n, kind, m, std, SEED, step, update)
    got, other = (m_ang, m_add) if kind == "arc" else (m_add, m_ang)
    print("n=%d %s update=%s: %d ulp from the double" % (n, kind, update, _ulps(got.cpu(), want)))
    assert int(step) == STEP0 + int(update)                                   # exactly + 1, or untouched
    assert not other.any() and got.dtype == torch.float32 and got.shape == (n,)
    assert _ulps(got.cpu(), want) <= 1
    if not update:
        assert torch.equal(got.cpu(), torch.full((n,), float(np.float32(m))))
        return
    # a draw depends on (seed, step, row) alone: the bare draws agree with the margins bit for bit, and so does a shorter batch
    bare = ops.elastic_draws(n, m, std, SEED, _step(), True)
    assert torch.equal(bare, got)
    if n >= 37:
        assert torch.equal(ops.elastic_draws(37, m, std, SEED, _step(), True), got[:37])
        assert not torch.equal(ops.elastic_draws(37, m, std, SEED, _step(STEP0 + 1), True), got[:37])
        assert not torch.equal(ops.elastic_draws(37, m, std, SEED + 2 ** 32, _step(), True), got[:37])


# ------------------------------------------------------------------------------------------------ 2. the target cosine, exact
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("d", [64, 512])
def test_head_target_cos_is_exact(d, dtype, K):
    """operands are multiples of 1/8 in [-1, 1]: exact in bf16, and every partial sum of their products (multiples of 1/64, below 512) is
    exact in fp32 in any order -- the kernel must EQUAL float64"""
    from frhip import ops
    n, classes = 11, 130
    g = torch.Generator().manual_seed(d + 7 * K)
    e = torch.randint(-8, 9, (n, d), generator=g).double() / 8
    w = torch.randint(-8, 9, (K * classes, d), generator=g).double() / 8
    e[5], w[64], w[(K - 1) * classes + 64] = 1.0, 1.0, 1.0                   # the largest sum there is: d, in the last plane as well
    labels = torch.randint(0, classes, (n,), generator=g)
    labels[:6] = torch.tensor([0, 63, -1, classes - 1, -1, 64])
    want = torch.full((n,), -2.0, dtype=torch.float64)
    own = torch.nonzero(labels >= 0).flatten()
    want[own] = (e @ w.t()).view(n, K, classes).max(dim=1).values[own, labels[own]]
    assert float(want.max()) == d
    got = ops.head_target_cos(e.to(dtype).cuda(), w.to(dtype).cuda(), labels.to(torch.int32).cuda(), subcenters=K)
    assert got.dtype == torch.float32 and torch.equal(got.cpu().double(), want)
    assert got[2].item() == -2.0 and got[4].item() == -2.0


# ------------------------------------------------------------------------------------------------ 3. the ranking, exact
@pytest.mark.parametrize("n,ws", [(n, ws) for n in (1, 2, 37, 256, 257, 4097) for ws in (1, 3)] + [(65536, 1)])
def test_elastic_assign_is_exact(n, ws):
    """duplicated cosines, rows no rank owns, duplicated draws: bitwise the stable-sort double, and a permutation of the draws; 65 536 is
    the largest batch the entry point serves"""
    from elastic_double import assign, draws, margins_of
    from frhip import ops
    g =torch.Generator().manual_seed(31 * n + ws)
    values = torch.randint(-40, 41, (n,), generator=g).float() / 64          # a pool of 81 cosines: duplicates from n = 37 on
    owner = torch.randint(0, ws + 1, (n,), generator=g)                       # == ws: nobody owns the row
    if n >= 37:
        owner[n // 2], owner[n - 1] = ws, ws
    tcos = torch.full((ws, n), -2.0)
    for r in range(ws):
        tcos[r, owner == r] = values[owner == r]
    draw = draws(n, 0.5, 0.05, SEED, n)
    if n > 1:
        draw[n - 1] = draw[0]
    kind = "arc" if n % 2 else "cos"
    want = margins_of(assign(tcos, draw), kind)
    m_ang, m_add = ops.elastic_assign(tcos.cuda(), draw.cuda(), kind)
    assert torch.equal(m_ang.cpu(), want[0]) and torch.equal(m_add.cpu(), want[1])
    got = m_ang if kind == "arc" else m_add
    assert torch.equal(got.cpu().sort().values, draw.sort().values)
    again = ops.elastic_assign(tcos.cuda(), draw.cuda(), kind)
    assert torch.equal(again[0], m_ang) and torch.equal(again[1], m_add)


# ------------------------------------------------------------------------------------------------ shared head inputs
_CASES = {}


def _case(n, classes, d, specials=True):
    """seeded inputs, built once per shape and shared (never modified: every user clones)"""
    from elastic_double import case
    key = (n, classes, d, specials)
    if key not in _CASES:
        _CASES[key] = case(n, classes, d, 9100 + n + classes, specials)
    return _CASES[key]


def _want_margins(variant, emb, weight, labels, step=STEP0, specials=True):
    """the double's margins of one training step on the whole batch -> (m_ang, m_add) float32"""
    from elastic_double import assert_case, row_margins
    m, std, kind, plus = VARIANTS[variant]
    tcos = assert_case(emb, weight, labels, m, std, kind, specials=specials)
    m_ang, m_add = row_margins(labels.numel(), m, std, kind, plus, SEED, step, tcos)
    assert float(((m_ang if kind == "arc" else m_add) - m).abs().max()) < 5 * std       # inside the band assert_case vouches for
    return m_ang, m_add


def _module(variant):
    from nets.ArcFace import ElasticFace
    m, std, kind, plus = VARIANTS[variant]
    return functools.partial(ElasticFace, std=std, kind=kind, plus=plus, seed=SEED), m


# ------------------------------------------------------------------------------------------------ 4. the stand-alone module
@pytest.mark.parametrize("variant", ["arc", "cos", "arc_plus"])
def test_elastic_module_forward_backward_vs_float64(variant):
    """ElasticFace.forward(logits, labels) on explicit cosines (frhip_elastic_margins or _draws + _assign, then frhip_margin_fwd_rows /
    _bwd_rows): output and input gradient; tolerances of tests/test_adaface_gpu.py test_adaface_module_forward_backward_vs_float64.  With
    plus the module ranks the fp32 cosines it is given, and so does the double."""
    from adaface_double import logits
    from elastic_double import assign, cosines, draws, margins_of
    n, classes, d = 37, 150, 64
    emb, weight, labels = _case(n, classes, d)
    m, std, kind, plus = VARIANTS[variant]
    m_ang, m_add = _want_margins(variant, emb, weight, labels)
    cos32 = cosines(emb, weight).float()                                      # the module's input
    if plus:
        own = labels >= 0
        tcos = torch.where(own, cos32.gather(1, labels.clamp(min=0)[:, None]).flatten(), torch.full((n,), -2.0))
        m_ang, m_add = margins_of(assign(tcos, draws(n, m, std, SEED, STEP0)), kind)
    upstream = torch.randn((n, classes), generator=torch.Generator().manual_seed(5))
    ref_in = cos32.double().requires_grad_(True)
    ref_out = logits(ref_in, labels, S, m_ang, m_add, EPS)
    ref_out.backward(upstream.double())
    factory, _ = _module(variant)
    mod = factory(S, m).cuda()
    with torch.no_grad():
        mod.step.fill_(STEP0)
    leaf = cos32.cuda().requires_grad_(True)
    out = mod(leaf, labels.cuda())
    out.backward(upstream.cuda())
    assert torch.equal(leaf.detach().cpu(), cos32) and int(mod.step) == STEP0 + 1          # not in place; one step
    print("module %s: max |out - double| %.3g, max |grad - double| %.3g" % (
        variant, float((out.detach().cpu().double() - ref_out.detach()).abs().max()), float((leaf.grad.cpu().double() - ref_in.grad).abs().max())))
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref_out.detach().numpy(), rtol=1e-6, atol=1e-5)
    np.testing.assert_allclose(leaf.grad.cpu().numpy(), ref_in.grad.numpy(), rtol=1e-5, atol=1e-5)
    mod.eval()                                                                # eval: the margin is m, the counter stands still
    ev = mod(cos32.cuda(), labels.cuda())
    g_m = torch.full((n,), float(np.float32(m)))
    ref_ev = logits(cos32.double(), labels, S, *margins_of(g_m, kind), EPS)
    np.testing.assert_allclose(ev.cpu().numpy(), ref_ev.numpy(), rtol=1e-6, atol=1e-5)
    assert int(mod.step) == STEP0 + 1


# ------------------------------------------------------------------------------------------------ 5. the fused head, fp32 mode
def _recording_kernels(P, dtype):
    class Recording(P.HipHeadKernels):
        """the HIP kernels, remembering the margins the head was handed"""
        seen = None

        def forward_stats(self, ehat, what, labels_i32, s, m, margin=None, subcenters=1):
            self.seen = torch.stack([margin.m_ang, margin.m_add]).cpu()
            return super().forward_stats(ehat, what, labels_i32, s, m, margin=margin, subcenters=subcenters)

    return Recording(dtype)


def _run_head(P, rank, ws, b, shape, rate, variant):
    """one rank of `ws`, `b` rows each: PartialFC(margin_loss = ElasticFace) on the HIP kernels"""
    _, classes, d = shape
    dev = torch.device("cuda", 0)
    emb, weight, labels = _case(ws * b, classes, d)
    factory, m = _module(variant)
    conf = types.SimpleNamespace(emd_size=d, sample_rate=rate, mixed_precision=False, loss_s=S, loss_m=m, frhip_dtype="fp32")
    kern = _recording_kernels(P, torch.float32)
    pfc = P.PartialFC(conf, classes, margin_loss=factory, kernels=kern).to(dev)
    assert pfc.margin_softmax.step.is_cuda
    start, num = head_ref.shard_range(classes, ws, rank)
    with torch.no_grad():
        (pfc.weight if rate < 1 else pfc.weight_activated.data).copy_(weight[start:start + num].to(dev))
        pfc.margin_softmax.step.fill_(STEP0)
    dummy = torch.nn.Parameter(torch.zeros(1, device=dev))
    opt = torch.optim.SGD([{"params": [dummy]}, {"params": pfc.parameters()}], lr=0.1, momentum=0.9)
    mine = slice(rank * b, (rank + 1) * b)
    e = emb[mine].clone().to(dev).requires_grad_(True)
    torch.manual_seed(1000 + rank)                          # the sampling permutation comes from the CPU generator
    loss = pfc(e, labels[mine].clone().to(dev), opt)
    loss.backward()
    idx = pfc.weight_index if rate < 1 else torch.arange(pfc.num_local)
    return dict(loss=float(loss.detach()), d_emb=e.grad.cpu().numpy(), d_w=pfc.weight_activated.grad.cpu().numpy(),
                index=idx.cpu().numpy(), margins=kern.seen.numpy(), step=int(pfc.margin_softmax.step))


def _head_worker(rank, ws, path, ret, b, shape, rate):
    """one rank, both variants in one process group; results travel through files (see tests/test_head_dist_gpu.py)"""
    for p in (ROOT, os.path.join(ROOT, "face-recognition-pytorch_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import nets.PartialFC as P
    torch.set_num_threads(1)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="file://" + path, rank=rank, world_size=ws)
    for variant in ("arc", "arc_plus"):
        np.savez(os.path.join(ret, "%s_rank%d.npz" % (variant, rank)), **_run_head(P, rank, ws, b, shape, rate, variant))
    dist.destroy_process_group()


def _check_head(outs, ws, b, shape, rate, variant):
    """every rank against ONE evaluation of the double on the whole batch and the class rows the ranks activated; criteria of
    tests/test_adaface_gpu.py _check_head (loss rtol 1e-4; gradients rtol 1e-3, atol 1e-5 of the largest reference element)"""
    from adaface_double import head_reference
    _, classes, d = shape
    emb, weight, labels = _case(ws * b, classes, d)
    m_ang, m_add = _want_margins(variant, emb, weight, labels)
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
    loss, d_emb, d_w = head_reference(emb, weight[rows], pos, S, m_ang, m_add, EPS)
    want = torch.stack([m_ang, m_add])
    offset = 0
    for r in range(ws):
        o = outs[r]
        k = o["index"].shape[0]
        refs = (("d_emb", ws * d_emb[r * b:(r + 1) * b].numpy()), ("d_w", d_w[offset:offset + k].numpy()))
        offset += k
        got = torch.from_numpy(o["margins"])
        print("%s ws %d rank %d rate %.1f %s: loss %.8g (double %.8g), margins %d ulp from the double" % (
            variant, ws, r, rate, shape, float(o["loss"]), float(loss), _ulps(got, want)), "".join(
            "  max |%s - double| %.3g of %.3g" % (key, float(np.abs(o[key] - ref).max()), float(np.abs(ref).max())) for key, ref in refs))
        assert int(o["step"]) == STEP0 + 1
        assert _ulps(got, want) <= 1                                              # the draw kernel's criterion; the ranks are exact
        assert np.array_equal(o["margins"], outs[0]["margins"])                   # equal across ranks, bit for bit
        np.testing.assert_allclose(float(o["loss"]), float(loss), rtol=1e-4, err_msg="rank %d loss" % r)
        for key, ref in refs:
            np.testing.assert_allclose(o[key], ref, rtol=1e-3, atol=1e-3 * float(np.abs(ref).max()) * 1e-2, err_msg="rank %d %s" % (r, key))


HEAD_SHAPES = [(37, 150, 64), (130, 257, 64)]      # ragged 16-row fragments; one and three 128-class tiles; a 64-group tail


@pytest.mark.parametrize("variant", ["arc", "arc_plus"])
@pytest.mark.parametrize("rate", [1.0, 0.3])
@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_fused_head_fp32_vs_float64(pg, shape, rate, variant):
    import nets.PartialFC as P
    _check_head([_run_head(P, 0, 1, shape[0], shape, rate, variant)], 1, shape[0], shape, rate, variant)


@pytest.mark.parametrize("rate", [1.0, 0.3])
def test_fused_head_fp32_two_ranks_vs_float64_and_one_rank(pg, rate):
    """37 rows on each of two ranks, Arc and Arc+: every rank draws the whole batch's margins itself (Arc+: from the all-gathered target
    cosines), and they are the margins ONE rank derives for the same 74 rows, bit for bit"""
    import nets.PartialFC as P
    ws, b, shape = 2, 37, (37, 150, 64)
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_head_worker, args=(ws, os.path.join(td, "pg"), td, b, shape, rate), nprocs=ws, join=True)
        outs = {v: [dict(np.load(os.path.join(td, "%s_rank%d.npz" % (v, r)))) for r in range(ws)] for v in ("arc", "arc_plus")}
    for variant in ("arc", "arc_plus"):
        _check_head(outs[variant], ws, b, shape, rate, variant)
        one = _run_head(P, 0, 1, ws * b, shape, rate, variant)
        _check_head([one], 1, ws * b, shape, rate, variant)
        assert np.array_equal(one["margins"], outs[variant][0]["margins"])        # the same margins at both world sizes


# ------------------------------------------------------------------------------------------------ 6. bf16, Arc+
def test_bf16_head_arc_plus_vs_float64():
    """(130, 257, 512) in bf16 through the kernels PartialFC calls; criteria of tests/test_adaface_gpu.py test_bf16_head_vs_float64 (loss
    rtol 3e-2; gradients rtol 0.1, atol 5 % of the largest reference element).  The double ranks the cosines of the SAME bf16-rounded
    operands (they keep the 1e-4 gap, asserted), so the margins are the double's; no target is near a boundary (specials off)."""
    import nets.PartialFC as P
    from adaface_double import head_reference
    from elastic_double import assert_case, assert_gaps, row_margins, target_cos
    from frhip import ops
    from nets.ArcFace import RowMargins
    n, classes, d = 130, 257, 512
    m, std, kind, plus = VARIANTS["arc_plus"]
    emb, weight, labels = _case(n, classes, d, specials=False)
    assert_case(emb, weight, labels, m, std, kind, specials=False)
    kern = P.HipHeadKernels(torch.bfloat16)
    assert ops.lib().frhip_head_dw_ok(0, n, classes, d) == 1
    e_c, w_c, l_c = emb.cuda(), weight.cuda(), labels.to(torch.int32).cuda()
    ehat, enorm = kern.normalize(e_c)
    what, wnorm = kern.normalize(w_c)
    tcos64 = target_cos(ehat.cpu(), what.cpu(), labels)
    assert_gaps(tcos64)
    m_ang, m_add = row_margins(n, m, std, kind, plus, SEED, STEP0, tcos64)
    loss_ref, d_e_ref, d_w_ref = head_reference(emb, weight, labels, S, m_ang, m_add, EPS)
    factory, _ = _module("arc_plus")
    mod = factory(S, m).cuda()
    with torch.no_grad():
        mod.step.fill_(STEP0)
    tcos = kern.head_target_cos(ehat, what, l_c)
    np.testing.assert_allclose(tcos.cpu().double().numpy(), tcos64.numpy(), rtol=0, atol=d * 2.0 ** -24)
    rm = mod.row_margins(kern, tcos)
    assert isinstance(rm, RowMargins) and rm.s == S and int(mod.step) == STEP0 + 1
    assert _ulps(rm.m_ang.cpu(), m_ang) <= 1 and not rm.m_add.any()
    zt, rmax, rsum = kern.forward_stats(ehat, what, l_c, S, m, margin=rm)
    loss = float(kern.loss(kern.target_prob(zt, l_c, rmax, rsum)))
    d_e, d_w = kern.backward(ehat, enorm, what, wnorm, l_c, S, m, rmax, rsum, n, torch.ones(1, device="cuda"), margin=rm)
    d_e, d_w = d_e.cpu(), d_w.cpu()
    print("bf16 Arc+: loss %.6g (double %.6g); max |dE - double| %.3g of %.3g; max |dW - double| %.3g of %.3g" % (
        loss, float(loss_ref), float((d_e.double() - d_e_ref).abs().max()), float(d_e_ref.abs().max()),
        float((d_w.double() - d_w_ref).abs().max()), float(d_w_ref.abs().max())))
    np.testing.assert_allclose(loss, float(loss_ref), rtol=3e-2)
    np.testing.assert_allclose(d_e.numpy(), d_e_ref.numpy(), rtol=0.1, atol=0.05 * float(d_e_ref.abs().max()))
    np.testing.assert_allclose(d_w.numpy(), d_w_ref.numpy(), rtol=0.1, atol=0.05 * float(d_w_ref.abs().max()))


# ------------------------------------------------------------------------------------------------ 7. three sub-centres, Arc+
def test_fused_head_fp32_three_subcenters_arc_plus(pg):
    """conf.subcenters = 3 with plus=True: the target cosine that is ranked is the maximum over the class's three centres.  Reference:
    subcenter_double.pooled_head with the double's margins; criteria of the fp32-mode head above."""
    import nets.PartialFC as P
    from elastic_double import MIN_GAP, assert_gaps, row_margins
    from nets.ArcFace import RowMargins
    from subcenter_double import assert_case, case
    n, classes, d, K = 37, 150, 64, 3
    m, std, kind, plus = VARIANTS["arc_plus"]
    for seed in range(4300, 4320):                          # the first seed whose pooled target cosines keep the ranking gap
        emb, weight, labels, res = case(n, classes, d, K, seed)
        own = torch.nonzero(labels >= 0).flatten()
        tcos = torch.full((n,), -2.0, dtype=torch.float64)
        tcos[own] = res["raw"][own, labels[own]]
        gaps = tcos.sort().values.diff()
        if float(gaps[gaps > 0].min()) >= MIN_GAP:
            break
    assert_case(emb, weight, labels, K, res)
    assert_gaps(tcos)
    u = tcos[own].acos()
    assert float((u + m - 5 * std).min()) > EPS + 1e-3 and float((u + m + 5 * std).max()) < math.pi - EPS - 1e-3
    m_ang, m_add = row_margins(n, m, std, kind, plus, SEED, STEP0, tcos)
    from subcenter_double import pooled_head
    ref = pooled_head(emb, weight, labels, K, S, m, margin=RowMargins(S, EPS, m_ang, m_add))
    dev = torch.device("cuda", 0)
    factory, _ = _module("arc_plus")
    conf = types.SimpleNamespace(emd_size=d, sample_rate=1.0, mixed_precision=False, loss_s=S, loss_m=m, frhip_dtype="fp32", subcenters=K)
    kern = _recording_kernels(P, torch.float32)
    pfc = P.PartialFC(conf, classes, margin_loss=factory, kernels=kern).to(dev)
    with torch.no_grad():
        pfc.weight_activated.data.copy_(weight.to(dev))
        pfc.margin_softmax.step.fill_(STEP0)
    e = emb.clone().to(dev).requires_grad_(True)
    loss = pfc(e, labels.clone().to(dev), None)
    loss.backward()
    got = kern.seen
    print("K = 3 Arc+: loss %.8g (double %.8g), margins %d ulp from the double" % (float(loss.detach()), float(ref["loss"]),
                                                                                  _ulps(got, torch.stack([m_ang, m_add]))))
    assert _ulps(got, torch.stack([m_ang, m_add])) <= 1 and int(pfc.margin_softmax.step) == STEP0 + 1
    tsub = torch.full((n,), -1, dtype=torch.int64)
    tsub[own] = ref["win"][own, labels[own]]
    assert torch.equal(pfc.last_target_sub.cpu().long(), tsub)
    np.testing.assert_allclose(float(loss.detach()), float(ref["loss"]), rtol=1e-4)
    for name, a, b in (("d_emb", e.grad.cpu().numpy(), ref["d_emb"].numpy()), ("d_w", pfc.weight_activated.grad.cpu().numpy(), ref["d_w"].numpy())):
        np.testing.assert_allclose(a, b, rtol=1e-3, atol=1e-3 * float(np.abs(b).max()) * 1e-2, err_msg=name)


# ------------------------------------------------------------------------------------------------ 8. through Model
def test_two_sgd_steps_through_model_conf_margin_loss_elasticface_plus(pg):
    """conf.margin_loss = functools.partial(ElasticFace, plus=True) is all a user sets.  Two optimisation steps: finite losses, the counter
    at 2, and losses that differ from those of the same run with std = 0 (every margin m)"""
    from model.FR_PartialFC import Model
    from nets.ArcFace import ElasticFace
    classes, b = 256, 8
    torch.cuda.set_device(0)
    spec = resnet_ref.resnet_spec(resnet_ref.BLOCKS["ResNet18"])
    losses = {}
    for std in (0.05, 0.0):
        conf = types.SimpleNamespace(network="ResNet18", emd_size=512, img_size=112, local_rank=0, world_size=1, sample_rate=1.0,
                                     mixed_precision=False, loss_s=S, loss_m=0.5, n_classes=classes, optimizer="SGD", lr=0.1, wd=5e-4,
                                     mom=0.9, loss="PartialFC", lr_scheduler=None, frhip_dtype="fp32", ckpt_path=None,
                                     margin_loss=functools.partial(ElasticFace, std=std, plus=True))
        model = Model(conf, None, "train")
        head = model.loss
        assert isinstance(head.margin_softmax, ElasticFace) and head.margin_softmax.plus and head.margin_softmax.step.is_cuda
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
        assert all(math.isfinite(v) for v in got) and int(head.margin_softmax.step) == 2
        losses[std] = got
    print("losses with std 0.05: %s, with std 0: %s" % (losses[0.05], losses[0.0]))
    assert losses[0.05][0] != losses[0.0][0] and losses[0.05][1] != losses[0.0][1]
