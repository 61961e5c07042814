"""UniFace (the sigmoid / binary cross-entropy head with one learnable threshold b) on the MI355X against the float64 restatement in
tests/uniface_double.py: the explicit-logit kernels (with the tiny-term case a log(1 + e) softplus fails), the fused head in fp32 mode at
world sizes 1 and 2 (real ranks on gloo, every rank on cuda:0), exact routing of dT in NaN-filled guarded buffers (both dtypes, one and
three centres), the bf16 head, three sub-centres, run-to-run identity, and two optimisation steps through Model with
conf.margin_loss = UniFace.

Condition, not a tolerance: no branch may be decided by rounding.  The inputs (uniface_double.case) keep every cosine >= 1e-3 from +-1
and, for kind "arc", every target >= 1e-3 from cos(pi - m); a label -1 row occurs; uniface_double.assert_case asserts it on the double.
1e-3 is enough: the fp32 dot error is d 2^-24 = 3.1e-5 at d = 512, and the bf16 head is held against the double on its own rounded
operands."""
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
S, M = 64.0, 0.4
M_NEG, W_POS, W_NEG = 0.1, 0.7, 1.3            # unequal weights and a margin on the negatives: every descriptor field is live


@pytest.fixture(scope="module")
def pg():
    if not dist.is_initialized():
        d = tempfile.mkdtemp()
        dist.init_process_group("gloo", init_method="file://" + os.path.join(d, "pg"), rank=0, world_size=1)
    yield
    if dist.is_initialized():
        dist.destroy_process_group()


def _mg(kind, m_neg=M_NEG, w_pos=W_POS, w_neg=W_NEG, s=S, m=M):
    from uniface_double import KINDS
    return (KINDS[kind], s, m, m_neg, w_pos, w_neg)


def _bias_of(which, classes):
    """the two thresholds of the tests, as the fp32 parameter holds them"""
    return float(np.float32(0.0 if which == "zero" else math.log(10 * classes)))


def _factory(kind):
    def make(s, m):
        from nets.ArcFace import UniFace
        return UniFace(s, m, kind=kind, w_pos=W_POS, w_neg=W_NEG, m_neg=M_NEG)
    return make


# ------------------------------------------------------------------------------------------------ 1. the explicit-logit kernels
@pytest.mark.parametrize("kind", ["arc", "cos"])
@pytest.mark.parametrize("shape", [(1, 1), (5, 130)])
def test_explicit_kernels_vs_float64(shape, kind):
    """frhip_bce_fwd / _bwd on fp32 cosines against the double on the same fp32 values: per-row loss and rowdb rtol 1e-5, gin rtol 1e-5 with
    atol 1e-7 of the largest element; then reduce + merge give the mean over rows"""
    from frhip import ops
    from nets.ArcFace import BceMargin
    from uniface_double import assert_case, terms
    n, c = shape
    g = torch.Generator().manual_seed(31 * n + c)
    cos32 = (torch.rand((n, c), generator=g) * 1.9 - 0.95)
    labels = torch.randint(0, c, (n,), generator=g)
    if n > 2:
        labels[2], labels[3], labels[4] = -1, 0, c - 1
        cos32[3, 0], cos32[4, c - 1] = -0.97, 0.9              # ArcFace's lower branch and a confident target
    assert_case(cos32.double(), labels, _mg(kind)[0], M, need_unowned=n > 2)
    b = 1.75
    mg = _mg(kind)
    term, dcos, db, _ = terms(cos32.double(), labels, mg, b)
    margin = BceMargin(*mg, torch.full((1,), b, device="cuda"))
    dev, lab = cos32.cuda(), labels.cuda()
    rowloss, rowdb = ops.bce_fwd(dev, lab, margin)
    up = torch.full((1,), 3.0, device="cuda")
    gin = ops.bce_bwd(dev, lab, margin, 0.5, up).cpu()
    want = dcos * 1.5
    print("explicit %s %s: max rel row-loss err %.3g, rowdb %.3g; max |gin - double| %.3g of %.3g" % (
        shape, kind, float(((rowloss.cpu().double() - term.sum(1)) / term.sum(1)).abs().max()),
        float(((rowdb.cpu().double() - db.sum(1)) / db.sum(1)).abs().max()), float((gin.double() - want).abs().max()), float(want.abs().max())))
    np.testing.assert_allclose(rowloss.cpu().numpy(), term.sum(1).numpy(), rtol=1e-5)
    np.testing.assert_allclose(rowdb.cpu().numpy(), db.sum(1).numpy(), rtol=1e-5)
    np.testing.assert_allclose(gin.numpy(), want.numpy(), rtol=1e-5, atol=1e-7 * float(want.abs().max()))
    loss, dbias = ops.bce_merge(ops.bce_reduce(rowloss, rowdb), n)
    np.testing.assert_allclose(float(loss), float(term.sum() / n), rtol=1e-5)
    np.testing.assert_allclose(float(dbias), float(db.sum() / n), rtol=1e-5)


def test_explicit_kernels_keep_tiny_terms():
    """n = 2, c = 20 000, every cosine -0.5, b = 8, labels {0, -1}: every negative term is softplus(-40) = 4.2e-18, which logf(1 + e) rounds
    to 0; the second row's loss is 20 000 of them, 8.5e-14.  Row losses at rtol 1e-4."""
    from frhip import ops
    from nets.ArcFace import BceMargin
    from uniface_double import COS, terms
    n, c = 2, 20000
    cos32 = torch.full((n, c), -0.5)
    labels = torch.tensor([0, -1])
    mg = (COS, 64.0, 0.4, 0.0, 1.0, 1.0)
    term, _, db, a = terms(cos32.double(), labels, mg, 8.0)
    assert float(a[1, 0]) == -40.0 and float(term[1].sum()) == pytest.approx(20000 * math.exp(-40.0), rel=1e-6)
    assert np.log(np.float32(1.0) + np.exp(np.float32(-40.0))) == 0.0                      # what the naive form gives
    rowloss, rowdb = ops.bce_fwd(cos32.cuda(), labels.cuda(), BceMargin(*mg, torch.full((1,), 8.0, device="cuda")))
    print("tiny terms: row losses %s (double %s)" % (rowloss.cpu().tolist(), term.sum(1).tolist()))
    np.testing.assert_allclose(rowloss.cpu().numpy(), term.sum(1).numpy(), rtol=1e-4)
    np.testing.assert_allclose(rowdb.cpu().numpy(), db.sum(1).numpy(), rtol=1e-4)
    assert float(rowloss[1]) > 0.0


# ------------------------------------------------------------------------------------------------ 2. / 3. the fused head, fp32 mode
def _case(n, classes, d):
    from uniface_double import case
    return case(n, classes, d, 9400 + n + classes)


def _run_head(P, rank, ws, shape, rate, kind, which, dtype=torch.float32, K=1):
    """one rank of `ws`: its rows of the shared batch of shape[0] rows through PartialFC(margin_loss = UniFace) on the HIP kernels"""
    n, classes, d = shape
    b = n // ws
    dev = torch.device("cuda", 0)
    emb, weight, labels = _case(n, classes, d)
    conf = types.SimpleNamespace(emd_size=d, sample_rate=rate, mixed_precision=False, loss_s=S, loss_m=M, frhip_dtype="fp32")
    pfc = P.PartialFC(conf, classes, margin_loss=_factory(kind), kernels=P.HipHeadKernels(dtype)).to(dev)
    bias = pfc.margin_softmax.bias
    assert bias.is_cuda and float(bias.detach()) == _bias_of("log", classes)          # reset_bias(num_classes) at construction
    start, num = head_ref.shard_range(classes, ws, rank)
    with torch.no_grad():
        (pfc.weight if rate < 1 else pfc.weight_activated.data).copy_(weight[start:start + num].to(dev))
        bias.fill_(_bias_of(which, classes))
    dummy = torch.nn.Parameter(torch.zeros(1, device=dev))
    opt = torch.optim.SGD([{"params": [dummy]}, {"params": [bias]}, {"params": [pfc.weight_activated]}], lr=0.1, momentum=0.9)
    mine = slice(rank * b, (rank + 1) * b)
    e = emb[mine].clone().to(dev).requires_grad_(True)
    torch.manual_seed(1000 + rank)                          # the sampling permutation comes from the CPU generator
    loss = pfc(e, labels[mine].clone().to(dev), opt)
    loss.backward()
    idx = pfc.weight_index if rate < 1 else torch.arange(pfc.num_local)
    return dict(loss=loss.detach().cpu().numpy().reshape(1), d_emb=e.grad.cpu().numpy(), d_w=pfc.weight_activated.grad.cpu().numpy(),
                dbias=bias.grad.cpu().numpy(), index=idx.cpu().numpy())


HEAD_SHAPES = [(130, 257, 512), (8, 40, 512)]       # two row tiles and three 128-class tiles with ragged ends; one tile
HEAD_GRID = [(rate, kind, which) for rate in (1.0, 0.3) for kind in ("cos", "arc") for which in ("zero", "log")]


def _head_worker(rank, ws, path, ret, shape):
    """one rank, the whole grid in one process group; results travel through files"""
    for p in (ROOT, os.path.join(ROOT, "face-recognition-pytorch_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import nets.PartialFC as P
    torch.set_num_threads(1)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="file://" + path, rank=rank, world_size=ws)
    for rate, kind, which in HEAD_GRID:
        np.savez(os.path.join(ret, "r%.1f_%s_%s_rank%d.npz" % (rate, kind, which, rank)), **_run_head(P, rank, ws, shape, rate, kind, which))
    dist.destroy_process_group()


def _check_head(outs, ws, shape, rate, kind, which):
    """every rank against ONE evaluation of the double on the whole batch and the class rows the ranks activated; criteria of
    tests/test_adaface_gpu.py _check_head (loss rtol 1e-4; gradients rtol 1e-3, atol 1e-5 of the largest reference element); bias.grad
    rtol 1e-4; loss and bias.grad equal across ranks bit for bit"""
    from uniface_double import assert_case, cosines, head_reference
    n, classes, d = shape
    b = n // ws
    emb, weight, labels = _case(n, classes, d)
    mg = _mg(kind)
    assert_case(cosines(emb, weight), labels, mg[0], M)
    rows, pos, offset, unowned = [], torch.full_like(labels, -1), 0, []
    for r in range(ws):
        start, num = head_ref.shard_range(classes, ws, r)
        index = torch.from_numpy(outs[r]["index"]).long()
        own = (labels >= start) & (labels < start + num)
        unowned.append(int(((labels >= 0) & ~own).sum()))
        assert bool(torch.isin(labels[own] - start, index).all()), "a positive class was not activated"
        pos[own] = torch.searchsorted(index, labels[own] - start) + offset
        rows.append(index + start)
        offset += index.numel()
    if ws > 1:
        assert min(unowned) >= 1                            # rows whose class the other shard owns: no target column on this one
    if rate < 1:
        assert int(torch.unique(labels[labels >= 0]).numel()) < offset < classes      # negatives were drawn, class rows were dropped
    rows = torch.cat(rows)
    ref = head_reference(emb, weight[rows], pos, mg, _bias_of(which, classes))
    offset = 0
    for r in range(ws):
        o = outs[r]
        k = o["index"].shape[0]
        refs = (("d_emb", ws * ref["d_emb"][r * b:(r + 1) * b].numpy()), ("d_w", ref["d_w"][offset:offset + k].numpy()))
        offset += k
        print("ws %d rank %d rate %.1f %s b=%s %s: loss %.8g (double %.8g), dbias %.8g (double %.8g)" % (
            ws, r, rate, kind, which, shape, float(o["loss"][0]), float(ref["loss"]), float(o["dbias"][0]), float(ref["dbias"])),
            "".join("  max |%s - double| %.3g of %.3g" % (key, float(np.abs(o[key] - w_).max()), float(np.abs(w_).max())) for key, w_ in refs))
        assert np.array_equal(o["loss"], outs[0]["loss"]) and np.array_equal(o["dbias"], outs[0]["dbias"])      # equal across ranks, bit for bit
        np.testing.assert_allclose(float(o["loss"][0]), float(ref["loss"]), rtol=1e-4, err_msg="rank %d loss" % r)
        np.testing.assert_allclose(float(o["dbias"][0]), float(ref["dbias"]), rtol=1e-4, err_msg="rank %d bias.grad" % r)
        for key, w_ in refs:
            np.testing.assert_allclose(o[key], w_, rtol=1e-3, atol=1e-5 * float(np.abs(w_).max()), err_msg="rank %d %s" % (r, key))


@pytest.mark.parametrize("which", ["zero", "log"])
@pytest.mark.parametrize("kind", ["cos", "arc"])
@pytest.mark.parametrize("rate", [1.0, 0.3])
@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_fused_head_fp32_vs_float64(pg, shape, rate, kind, which):
    """a missing mask of the padded classes shifts the loss of the 257-class shape by 24 % at b = 0 and 0.14 % at b = log(10 C)"""
    import nets.PartialFC as P
    _check_head([_run_head(P, 0, 1, shape, rate, kind, which)], 1, shape, rate, kind, which)


@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_fused_head_fp32_two_ranks_vs_float64(shape):
    """half the batch on each of two ranks: the only statistics exchange is the all-gather of the two-float pairs; every rank ends with
    the same loss and the same bias gradient, bit for bit"""
    ws = 2
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_head_worker, args=(ws, os.path.join(td, "pg"), td, shape), nprocs=ws, join=True)
        for rate, kind, which in HEAD_GRID:
            outs = [dict(np.load(os.path.join(td, "r%.1f_%s_%s_rank%d.npz" % (rate, kind, which, r)))) for r in range(ws)]
            _check_head(outs, ws, shape, rate, kind, which)


# ------------------------------------------------------------------------------------------------ 4. exact routing
S_EX, M_EX, B_EX = 8.0, 0.3, 0.5            # cos(pi - 0.3) = -0.95534 lies 2.2e-3 from the nearest multiple of 1/64
GUARD = 1024                                   # elements of NaN in front of and behind every buffer the kernels write


def _exact_case(K, seed):
    """operands that are multiples of 1/8 with few non-zeros: every cosine an exact multiple of 1/64 in [-1, 1] in both dtypes"""
    from subcenter_double import pool
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
    raw, win, _ = pool((e @ w.t()).view(n, K, classes))
    assert float(raw.abs().max()) <= 1.0 and torch.equal(raw * 64, (raw * 64).round())
    own = torch.nonzero(labels >= 0).flatten()
    assert float(raw[own, labels[own]].abs().max()) < 1.0                          # a target at +-1 has no finite slope
    return e, w, labels, raw, win


def _guarded(numel, dtype):
    """-> (the whole NaN-filled allocation, its interior view of `numel` elements, 16-byte aligned)"""
    flat = torch.full((numel + 2 * GUARD,), float("nan"), dtype=dtype, device="cuda")
    return flat, flat[GUARD:GUARD + numel]


def _guards_intact(flat, numel):
    return bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[GUARD + numel:]).all())


@pytest.mark.parametrize("which", ["w_neg=0", "w_pos=0"])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_exact_routing_in_guarded_buffers(dtype, K, which):
    """The C ABI on exact cosines, every output inside a NaN-filled allocation with NaN guards on both sides.
    w_neg = 0: dT and dTt hold exactly ONE non-zero per owned row, in the label's column (of the winning plane), none in the label -1 row.
    w_pos = 0: the mirror image -- the target's own rule is switched off (an exact 0 in the label's column) and every other column of every
    row, the label -1 row included, carries the negative rule's non-zero in the winning plane.
    Both: exact zeros fill the pitch padding of dT (columns past the classes) and of dTt (columns past the rows), dTt is dT transposed
    bit for bit, nothing is written outside the buffers, and the values match the double (rtol 1e-3; a bf16 dT adds the unit roundoff of
    its 8-bit significand, 2^-8).
    The forward's partials are all written (no NaN survives) and fold to the double's row sums."""
    from frhip import ops
    from uniface_double import terms
    e, w, labels, raw, win = _exact_case(K, 600 + K)
    n, classes = raw.shape
    d = e.shape[1]
    kind = "arc" if K == 3 else "cos"
    mg = _mg(kind, m_neg=0.125, w_pos=0.0 if which == "w_pos=0" else 0.75, w_neg=0.0 if which == "w_neg=0" else 1.5, s=S_EX, m=M_EX)
    term, dcos, db, a = terms(raw, labels, mg, B_EX)
    tgt = raw[labels >= 0, labels[labels >= 0]]
    assert float((tgt - math.cos(math.pi - M_EX)).abs().min()) >= 1e-3              # exact cosines: no branch is decided by rounding
    lib, p = ops.lib(), ops._p
    eh, wh, lab = e.to(dtype).cuda(), w.to(dtype).cuda(), labels.to(torch.int32).cuda()
    bias = torch.full((1,), B_EX, device="cuda")
    desc = ops._MarginBceDesc(int(mg[0]), *[float(v) for v in mg[1:]], bias.data_ptr())
    head = (ops.dt_of(eh), p(eh), p(wh), p(lab), n, classes, d)
    # -- forward
    groups = lib.frhip_head_groups(classes)
    f_pl, pl = _guarded(groups * n, torch.float32)
    f_pd, pd = _guarded(groups * n, torch.float32)
    f_row, row = _guarded(3 * n, torch.float32)
    zt, rowloss, rowdb = row[:n], row[n:2 * n], row[2 * n:]
    tsub = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    if K == 1:
        ops.check(lib.frhip_head_fwd_bce(*head, ctypes.byref(desc), p(pl), p(pd), p(zt), p(rowloss), p(rowdb), ops._s()), "frhip_head_fwd_bce")
    else:
        ops.check(lib.frhip_head_fwd_sub_bce(*head, K, ctypes.byref(desc), p(pl), p(pd), p(zt), p(tsub), p(rowloss), p(rowdb), ops._s()),
                  "frhip_head_fwd_sub_bce")
    assert _guards_intact(f_pl, groups * n) and _guards_intact(f_pd, groups * n) and _guards_intact(f_row, 3 * n)
    assert not bool(torch.isnan(pl).any()) and not bool(torch.isnan(pd).any())
    own = torch.nonzero(labels >= 0).flatten()
    assert bool(torch.isnan(zt.cpu()[labels < 0]).all())                            # no target: untouched
    np.testing.assert_allclose(zt.cpu()[own].numpy(), a[own, labels[own]].numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(rowloss.cpu().numpy(), term.sum(1).numpy(), rtol=1e-5)
    np.testing.assert_allclose(rowdb.cpu().numpy(), db.sum(1).numpy(), rtol=1e-5, atol=1e-6)
    # the last 64-class group holds ONE live class (256): its partial is that class's term alone, the 63 padded columns add exactly 0
    np.testing.assert_allclose(pl.view(groups, n)[4].cpu().numpy(), term[:, 256].numpy(), rtol=1e-5)
    assert not bool(pl.view(groups, n)[5].any()) and not bool(pd.view(groups, n)[5].any())
    if K > 1:
        want_tsub = torch.full((n,), -1, dtype=torch.int32)
        want_tsub[own] = win[own, labels[own]].to(torch.int32)
        assert torch.equal(tsub.cpu(), want_tsub)
    # -- recompute
    epv = ops.epv(dtype)
    ldp, ldtt = (classes + epv - 1) // epv * epv, (n + epv - 1) // epv * epv
    assert ldp > classes and ldtt > n                                               # both paddings exist
    f_dt, dt = _guarded(n * K * ldp, dtype)
    f_dtt, dtt = _guarded(K * classes * ldtt, dtype)
    if K == 1:
        ops.check(lib.frhip_head_bwd_dt_bce(*head, ctypes.byref(desc), 1.0 / n, None, p(dt), ldp, p(dtt), ldtt, ops._s()), "frhip_head_bwd_dt_bce")
    else:
        ops.check(lib.frhip_head_bwd_dt_sub_bce(*head, K, ctypes.byref(desc), 1.0 / n, None, p(dt), K * ldp, ldp, p(dtt), ldtt, ops._s()),
                  "frhip_head_bwd_dt_sub_bce")
    assert _guards_intact(f_dt, n * K * ldp) and _guards_intact(f_dtt, K * classes * ldtt)
    dt, dtt = dt.view(n, K, ldp).cpu(), dtt.view(K * classes, ldtt).cpu()
    assert not bool(torch.isnan(dt.float()).any()) and not bool(torch.isnan(dtt.float()).any())
    assert int(torch.count_nonzero(dt[:, :, classes:])) == 0 and int(torch.count_nonzero(dtt[:, n:])) == 0
    for k in range(K):
        assert torch.equal(dtt[k * classes:(k + 1) * classes, :n].t(), dt[:, k, :classes])
    onehot = torch.zeros(raw.shape, dtype=torch.bool)
    onehot[own, labels[own]] = True
    live = onehot if which == "w_neg=0" else ~onehot
    nz = dt[:, :, :classes] != 0
    for k in range(K):
        assert torch.equal(nz[:, k], live & (win == k)), "plane %d" % k
    if which == "w_neg=0":
        assert torch.equal(torch.count_nonzero(dt.view(n, -1), dim=1), (labels >= 0).long()) and int(torch.count_nonzero(dt[2])) == 0
        assert int(torch.count_nonzero(dtt)) == own.numel()
    else:
        assert int(torch.count_nonzero(dt[own, :, :][:, :, :classes].sum(1)[torch.arange(own.numel()), labels[own]])) == 0
        assert int(torch.count_nonzero(dt[2])) == classes
    rtol = 1e-3 + (2.0 ** -8 if dtype == torch.bfloat16 else 0.0)       # bf16 keeps 8 significant bits: unit roundoff 2^-8
    for k in range(K):
        want = torch.where(win == k, dcos / n, torch.zeros_like(dcos))
        np.testing.assert_allclose(dt[:, k, :classes].float().numpy(), want.numpy(), rtol=rtol, atol=0, err_msg="dT plane %d" % k)


# ------------------------------------------------------------------------------------------------ 5. bf16
def test_bf16_head_vs_float64():
    """(130, 257, 512) in bf16 through the kernels PartialFC calls; criteria of tests/test_adaface_gpu.py test_bf16_head_vs_float64 (loss
    rtol 3e-2; gradients rtol 0.1, atol 5 % of the largest reference element; the bias gradient as the loss).  The double works on the
    SAME bf16-rounded normalised operands (read back from the device), and the condition is asserted on their cosines."""
    import nets.PartialFC as P
    from frhip import ops
    from nets.ArcFace import BceMargin
    from uniface_double import UniHeadKernels, assert_case
    n, classes, d = 130, 257, 512
    emb, weight, labels = _case(n, classes, d)
    kern = P.HipHeadKernels(torch.bfloat16)
    assert ops.lib().frhip_head_dw_ok(0, n, classes, d) == 1
    e_c, w_c, l_c = emb.cuda(), weight.cuda(), labels.to(torch.int32).cuda()
    ehat, enorm = kern.normalize(e_c)
    what, wnorm = kern.normalize(w_c)
    eh64, wh64 = ehat.cpu().double(), what.cpu().double()
    for kind in ("arc", "cos"):
        mg = _mg(kind)
        assert_case(eh64 @ wh64.t(), labels, mg[0], M)
        b = _bias_of("log", classes)
        double, lab32 = UniHeadKernels(), labels.to(torch.int32)
        m64 = BceMargin(*mg, torch.tensor([b], dtype=torch.float64))
        _, rl, rd = double.forward_stats(eh64, wh64, lab32, S, M, margin=m64)
        loss_ref, db_ref = double.bce_merge(double.bce_reduce(rl, rd), n)
        d_e_ref, d_w_ref = double.backward(eh64, enorm.cpu().double(), wh64, wnorm.cpu().double(), lab32, S, M, None, None, n,
                                           torch.ones(1, dtype=torch.float64), margin=m64)
        mdev = BceMargin(*mg, torch.full((1,), b, device="cuda"))
        _, rl, rd = kern.forward_stats(ehat, what, l_c, S, M, margin=mdev)
        loss, db = kern.bce_merge(kern.bce_reduce(rl, rd), n)
        d_e, d_w = kern.backward(ehat, enorm, what, wnorm, l_c, S, M, None, None, n, torch.ones(1, device="cuda"), margin=mdev)
        d_e, d_w = d_e.cpu(), d_w.cpu()
        print("bf16 UniFace %s: loss %.6g (double %.6g), dbias %.6g (double %.6g); max |dE - double| %.3g of %.3g; max |dW - double| %.3g of %.3g" % (
            kind, float(loss), float(loss_ref), float(db), float(db_ref), float((d_e.double() - d_e_ref).abs().max()),
            float(d_e_ref.abs().max()), float((d_w.double() - d_w_ref).abs().max()), float(d_w_ref.abs().max())))
        np.testing.assert_allclose(float(loss), float(loss_ref), rtol=3e-2)
        np.testing.assert_allclose(float(db), float(db_ref), rtol=3e-2)
        np.testing.assert_allclose(d_e.numpy(), d_e_ref.numpy(), rtol=0.1, atol=0.05 * float(d_e_ref.abs().max()))
        np.testing.assert_allclose(d_w.numpy(), d_w_ref.numpy(), rtol=0.1, atol=0.05 * float(d_w_ref.abs().max()))


# ------------------------------------------------------------------------------------------------ 6. three sub-centres
def test_fused_head_fp32_three_subcenters(pg):
    """conf.subcenters = 3: the pooled cosine (the maximum over the class's centres) enters the rule, the gradient reaches the winning
    plane only (the double's d_w through subcenter_double.pool has exact zeros elsewhere), tsub is subcenter_double's winner map, as for
    every other margin.  Criteria of the fp32-mode head above."""
    import nets.PartialFC as P
    from subcenter_double import assert_case as assert_sub_case, case
    from uniface_double import assert_case, head_reference
    n, classes, d, K = 37, 150, 64, 3
    emb, weight, labels, res = case(n, classes, d, K, 4500)
    assert_sub_case(emb, weight, labels, K, res)
    mg = _mg("arc")
    assert_case(res["raw"], labels, mg[0], M)
    b = _bias_of("log", classes)
    ref = head_reference(emb, weight, labels, mg, b, K=K)
    assert torch.equal(ref["win"], res["win"])
    dev = torch.device("cuda", 0)
    conf = types.SimpleNamespace(emd_size=d, sample_rate=1.0, mixed_precision=False, loss_s=S, loss_m=M, frhip_dtype="fp32", subcenters=K)
    pfc = P.PartialFC(conf, classes, margin_loss=_factory("arc"), kernels=P.HipHeadKernels(torch.float32)).to(dev)
    with torch.no_grad():
        pfc.weight_activated.data.copy_(weight.to(dev))
    assert float(pfc.margin_softmax.bias.detach()) == b
    e = emb.clone().to(dev).requires_grad_(True)
    loss = pfc(e, labels.clone().to(dev), None)
    loss.backward()
    own = torch.nonzero(labels >= 0).flatten()
    tsub = torch.full((n,), -1, dtype=torch.int64)
    tsub[own] = ref["win"][own, labels[own]]
    assert torch.equal(pfc.last_target_sub.cpu().long(), tsub)
    d_w = pfc.weight_activated.grad.cpu()
    print("K = 3: loss %.8g (double %.8g), dbias %.8g (double %.8g)" % (
        float(loss.detach()), float(ref["loss"]), float(pfc.margin_softmax.bias.grad), float(ref["dbias"])))
    # a centre that won no (row, class) pair gets no gradient at all
    never = torch.stack([(ref["win"] == k).sum(0) == 0 for k in range(K)]).reshape(-1)
    assert int(never.sum()) >= 1 and not bool(d_w[never].any()) and not bool(ref["d_w"][never].any())
    np.testing.assert_allclose(float(loss.detach()), float(ref["loss"]), rtol=1e-4)
    np.testing.assert_allclose(float(pfc.margin_softmax.bias.grad), float(ref["dbias"]), rtol=1e-4)
    for name, a_, b_ in (("d_emb", e.grad.cpu().numpy(), ref["d_emb"].numpy()), ("d_w", d_w.numpy(), ref["d_w"].numpy())):
        np.testing.assert_allclose(a_, b_, rtol=1e-3, atol=1e-5 * float(np.abs(b_).max()), err_msg=name)


# ------------------------------------------------------------------------------------------------ 7. run-to-run identity
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_run_to_run_identity(pg, dtype):
    """the same inputs twice: loss, dT, d_w and bias.grad are equal bit for bit (every fold has an order fixed by the shape)"""
    import nets.PartialFC as P
    from frhip import ops
    from nets.ArcFace import BceMargin
    shape = (130, 257, 512)
    runs = [_run_head(P, 0, 1, shape, 1.0, "arc", "log", dtype=dtype) for _ in range(2)]
    for key in ("loss", "d_w", "dbias"):
        assert np.array_equal(runs[0][key], runs[1][key]), key
    emb, weight, labels = _case(*shape)
    kern = P.HipHeadKernels(dtype)
    ehat, what = kern.normalize(emb.cuda())[0], kern.normalize(weight.cuda())[0]
    margin = BceMargin(*_mg("arc"), torch.full((1,), _bias_of("log", shape[1]), device="cuda"))
    dts = [ops.head_bwd_dt(ehat, what, labels.to(torch.int32).cuda(), S, M, None, None, 1.0 / shape[0], transposed=True, margin=margin) for _ in range(2)]
    assert torch.equal(dts[0][0], dts[1][0]) and torch.equal(dts[0][1], dts[1][1])
    assert not bool(torch.isnan(dts[0][0].float()).any())


# ------------------------------------------------------------------------------------------------ 8. through Model
def test_two_sgd_steps_through_model_conf_margin_loss_uniface(pg):
    """conf.margin_loss = UniFace is all a user sets.  Two optimisation steps: finite losses; three optimizer groups with the class centres
    last, updated early (step_group_early on the last group, accepted) at every step; the threshold moves, and after the first step it is
    the double's SGD update b0 - lr dbias (first step: the momentum buffer is the gradient; no weight decay on the group) at rtol 1e-4,
    dbias evaluated in float64 on the normalised operands the head kernels saw; a checkpoint saved after step 1 reloads into the same
    threshold."""
    import nets.PartialFC as P
    from model.FR_PartialFC import Model
    from nets.ArcFace import UniFace
    from uniface_double import terms
    classes, b, lr = 256, 8, 0.1
    torch.cuda.set_device(0)
    spec = resnet_ref.resnet_spec(resnet_ref.BLOCKS["ResNet18"])
    conf = types.SimpleNamespace(network="ResNet18", emd_size=512, img_size=112, local_rank=0, world_size=1, sample_rate=1.0,
                                 mixed_precision=False, loss_s=S, loss_m=M, n_classes=classes, optimizer="SGD", lr=lr, wd=5e-4,
                                 mom=0.9, loss="PartialFC", lr_scheduler=None, frhip_dtype="fp32", ckpt_path=None, margin_loss=UniFace)
    model = Model(conf, None, "train")
    head = model.loss
    assert isinstance(head.margin_softmax, UniFace)
    groups = model.opt.param_groups
    assert len(groups) == 3 and groups[1]["params"][0] is head.margin_softmax.bias and groups[1]["weight_decay"] == 0.0
    assert len(groups[2]["params"]) == 1 and groups[2]["params"][0] is head.weight_activated

    seen = {}
    kern = head.kernels
    fwd = kern.forward_stats

    def recording(ehat, what, labels_i32, s, m, margin=None, subcenters=1):
        seen.update(ehat=ehat.cpu().double(), what=what.cpu().double(), labels=labels_i32.cpu().long(), bias=float(margin.bias))
        return fwd(ehat, what, labels_i32, s, m, margin=margin, subcenters=subcenters)

    kern.forward_stats = recording
    early = []
    step_early = model.opt.step_group_early

    def counting(gi, stream):
        ok = step_early(gi, stream)
        early.append((gi, ok))
        return ok

    model.opt.step_group_early = counting
    sd = recipe.fill_state(spec, 777)
    for key, _, kd in spec:
        if kd in ("bn_w", "bn_rv"):
            sd[key].fill_(1.0)
        elif kd in ("bn_b", "bn_rm"):
            sd[key].zero_()
    model.encoder.load_state_dict(sd, strict=True)
    with torch.no_grad():
        head.weight_activated.data.copy_(recipe.normal(778, (classes, 512), 0.01).cuda())
    bias = head.margin_softmax.bias
    b0 = float(bias.detach())
    assert b0 == _bias_of("log", classes)
    losses, biases, saved = [], [], None
    for st in range(2):
        w_before = head.weight_activated.detach().cpu().clone()
        img, ids = recipe.images(779 + 10 * st, b), recipe.labels(780 + 10 * st, b, classes)
        losses.append(float(model.training_step((img, ids.clone()))["loss"]))
        torch.cuda.synchronize()
        assert not torch.equal(head.weight_activated.detach().cpu(), w_before)
        assert early == [(2, True)] * (st + 1), early                # the class-centre group, every step
        biases.append(float(bias.detach()))
        if st == 0:
            _, _, db, _ = terms(seen["ehat"] @ seen["what"].t(), seen["labels"], _mg("cos", 0.0, 1.0, 1.0), seen["bias"])
            want = b0 - lr * float(db.sum() / b)
            print("threshold after step 1: %.8g (double's SGD update %.8g, from %.8g)" % (biases[0], want, b0))
            assert seen["bias"] == b0
            np.testing.assert_allclose(biases[0], want, rtol=1e-4)
            saved = {k: v.detach().clone() for k, v in head.state_dict().items()}
    print("losses with UniFace: %s, thresholds %s" % (losses, biases))
    assert all(math.isfinite(v) for v in losses) and biases[0] != b0 and biases[1] != biases[0]
    assert float(saved["margin_softmax.bias"]) == biases[0]
    fresh = P.PartialFC(conf, classes, margin_loss=UniFace).to(torch.device("cuda", 0))
    assert float(fresh.margin_softmax.bias.detach()) == b0
    fresh.load_state_dict(saved)
    assert float(fresh.margin_softmax.bias.detach()) == biases[0] and fresh.margin_softmax.bias.is_cuda
