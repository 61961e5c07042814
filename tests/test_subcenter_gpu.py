"""Sub-centre head (K centres per class, sub-center ArcFace) on the MI355X against the float64 restatement in tests/subcenter_double.py:
the kernels behind ops.head_fwd / ops.head_bwd_dt(subcenters=K), the head module at world sizes 1 and 2 (real ranks on gloo, every rank
on cuda:0), the bf16 head with frhip_head_dw on the path, the same calls on poisoned memory, two optimisation steps through Model with
conf.subcenters = 3, and run-to-run identity.

The fp32-mode inputs (subcenter_double.case) hold one class whose first planes are bitwise copies of each other -- the exact tie, which
must go to plane 0 -- and keep the double's top-two gap at every other (row, class) at 1e-5 or more: 2.6 times the worst-case fp32 error
of a 64-term dot product of unit vectors, so no winner is decided by rounding (subcenter_double.assert_case asserts it on the double).
n = 37 is no multiple of the 16-row fragment; 150 classes are two 128-column tiles, the second partial, and a multiple of neither
16-byte vector width (4 fp32, 8 bf16)."""
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
S, M = 30.0, 0.35
N, CLASSES, D = 37, 150, 64


@pytest.fixture(scope="module")
def pg():
    if not dist.is_initialized():
        d = tempfile.mkdtemp()
        dist.init_process_group("gloo", init_method="file://" + os.path.join(d, "pg"), rank=0, world_size=1)
    yield
    if dist.is_initialized():
        dist.destroy_process_group()


def _margin(kind, n):
    """-> (margin for the kernels or None, the same for the double)"""
    from nets.ArcFace import Margin, RowMargins
    if kind == "arcface":
        return None, None
    if kind == "cosface_filt":
        mg = Margin(1, False, S, M, 0.2)
        return mg, mg
    g = torch.Generator().manual_seed(17)
    k = torch.linspace(-1.0, 1.0, n)[torch.randperm(n, generator=g)]            # AdaFace: m_ang = -m k, m_add = m + m k
    m_ang, m_add = -0.4 * k, 0.4 + 0.4 * k
    return RowMargins(S, 1e-3, m_ang.cuda(), m_add.cuda()), RowMargins(S, 1e-3, m_ang.double(), m_add.double())


def _kmax():
    from frhip import ops
    return ops.head_sub_max()


def _kernel_case(K, kind):
    from subcenter_double import assert_case, case, pooled_head
    emb, weight, labels, res = case(N, CLASSES, D, K, 4100 + K)
    assert_case(emb, weight, labels, K, res)
    mg, mg64 = _margin(kind, N)
    ref = pooled_head(emb, weight, labels, K, S, M, margin=mg64)
    assert torch.equal(ref["win"], res["win"])
    if kind == "cosface_filt":          # elements are filtered, and none sits where fp32 rounding decides it
        own = torch.nonzero(labels >= 0).flatten()
        off = ref["raw"].clone()
        off[own, labels[own]] = -1.0
        assert int((off > 0.2).sum()) >= 20 and float((off - 0.2).abs().min()) > 1e-5
    return emb, weight, labels, mg, ref


def _kernel_calls(emb, weight, labels, mg, K):
    from frhip import ops
    eh, en = ops.l2norm_rows(emb.cuda(), torch.float32)
    wh, wn = ops.l2norm_rows(weight.cuda(), torch.float32)
    lab = labels.to(torch.int32).cuda()
    zt, rmax, rsum, tsub = ops.head_fwd(eh, wh, lab, S, M, margin=mg, subcenters=K)
    dt, dtt = ops.head_bwd_dt(eh, wh, lab, S, M, rmax, rsum, 1.0 / emb.shape[0], transposed=True, margin=mg, subcenters=K)
    return zt, rmax, rsum, tsub, dt, dtt


def _check_kernel_outputs(outs, labels, ref, K):
    """`ref`: the double's result.  fp32-mode criterion of tests/test_head_gpu.py: rtol 1e-3, atol 1e-3 of the largest reference element"""
    zt, rmax, rsum, tsub, dt, dtt = [t.cpu() for t in outs]
    n, classes = ref["win"].shape
    own = torch.nonzero(labels >= 0).flatten()
    z = ref["z"]
    want_zt = torch.zeros(n, dtype=torch.float64)
    want_zt[own] = z[own, labels[own]]
    want_max = z.max(dim=1).values
    want_sum = torch.exp(z - want_max[:, None]).sum(dim=1)
    # d loss / d pooled cosine from the double's gradient of the normalised centres is not needed: the chain rule through the winner map
    # is the statement itself -- dT[m][k][c] = (win == k) * d[m][c] with d = (softmax - onehot) / n * dz/dcos
    p = torch.exp(z - want_max[:, None]) / want_sum[:, None]
    onehot = torch.zeros_like(p)
    onehot[own, labels[own]] = 1.0
    raw = ref["raw"].clone().requires_grad_(True)
    from subcenter_double import logits
    (logits(raw, labels, S, M, ref["margin"]) * ((p - onehot) / n)).sum().backward()
    d = raw.grad
    print("K=%d: max |zt - double| %.3g, |rowmax - double| %.3g, rel rowsum %.3g" % (
        K, float((zt.double() - want_zt).abs().max()), float((rmax.double() - want_max).abs().max()),
        float(((rsum.double() - want_sum) / want_sum).abs().max())))
    for name, got, want in (("ztarget", zt, want_zt), ("rowmax", rmax, want_max), ("rowsum", rsum, want_sum)):
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-3, atol=1e-3 * float(want.abs().max()), err_msg=name)
    from subcenter_double import ROWS, TIE_CLASS
    want_tsub = torch.full((n,), -1, dtype=torch.int32)
    want_tsub[own] = ref["win"][own, labels[own]].to(torch.int32)
    assert tsub.dtype == torch.int32 and torch.equal(tsub, want_tsub)
    assert int(tsub[ROWS["tie"]]) == 0 and int(labels[ROWS["tie"]]) == TIE_CLASS and int(tsub[ROWS["no_target"]]) == -1
    e = 4
    ldp, ldtt = (classes + e - 1) // e * e, (n + e - 1) // e * e
    assert dt.shape == (n, K, ldp) and dtt.shape == (K * classes, ldtt)
    assert not dt[:, :, classes:].any() and not dtt[:, n:].any(), "pad columns of dT / dTt must be written as zeros"
    for k in range(K):
        plane = dt[:, k, :classes]
        won = ref["win"] == k
        assert torch.equal(plane != 0, won & (d != 0)), "plane %d: the zero pattern of dT is not the double's winner map" % k
        want = torch.where(won, d, torch.zeros_like(d))
        np.testing.assert_allclose(plane.numpy(), want.numpy(), rtol=1e-3, atol=1e-3 * float(d.abs().max()), err_msg="dT plane %d" % k)
        assert torch.equal(dtt[k * classes:(k + 1) * classes, :n].t(), plane), "dTt is not the transpose of dT bit for bit"
    assert float(d.abs().min()) > 0 or ref["margin"] is not None        # ArcFace: every (row, class) carries a gradient to route


KERNEL_CASES = [(2, "arcface"), (3, "arcface"), ("max", "arcface"), (2, "cosface_filt"), (2, "rows")]


@pytest.mark.parametrize("K,kind", KERNEL_CASES)
def test_kernels_fp32_vs_float64(K, kind):
    K = _kmax() if K == "max" else K
    assert K >= 2
    emb, weight, labels, mg, ref = _kernel_case(K, kind)
    ref["margin"] = _margin(kind, N)[1]
    _check_kernel_outputs(_kernel_calls(emb, weight, labels, mg, K), labels, ref, K)


@pytest.mark.parametrize("K,kind", KERNEL_CASES)
def test_kernels_on_poisoned_memory(K, kind):
    """the same calls with every torch.empty (outputs, partial-sum groups, workspace) holding NaN, 3e38, 0.75: bit-identical to the
    clean run, so every element of dT, dTt, tsub and the statistics is written or a defined zero; and still the double's"""
    from test_poisoned_kernels_gpu import poisoned_parity
    K = _kmax() if K == "max" else K
    emb, weight, labels, mg, ref = _kernel_case(K, kind)
    ref["margin"] = _margin(kind, N)[1]
    outs = poisoned_parity(lambda: _kernel_calls(emb, weight, labels, mg, K))
    _check_kernel_outputs(outs, labels, ref, K)


@pytest.mark.parametrize("kind", ["arcface", "cosface_filt", "rows"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_one_centre_is_bit_identical_through_both_kernels(dtype, kind):
    """head_kernel (ops.head_fwd / ops.head_bwd_dt) and head_sub_kernel with K = 1 (the _sub entry points called directly: ops sends one
    centre per class to head_kernel) inline one epilogue and one tile store on the same accumulators, so every output agrees bit for bit;
    tsub is 0 where the label is owned and -1 elsewhere.  Random unit rows, one label -1, one duplicate label."""
    import ctypes
    from frhip import ops
    g = torch.Generator().manual_seed(4400)
    emb, weight = torch.randn((N, D), generator=g), torch.randn((CLASSES, D), generator=g)
    labels = torch.randint(0, CLASSES, (N,), generator=g)
    labels[5], labels[9] = -1, labels[8]
    mg = _margin(kind, N)[0]
    eh, wh = ops.l2norm_rows(emb.cuda(), dtype)[0], ops.l2norm_rows(weight.cuda(), dtype)[0]
    lab = labels.to(torch.int32).cuda()
    zt, rmax, rsum = ops.head_fwd(eh, wh, lab, S, M, margin=mg)
    dt, dtt = ops.head_bwd_dt(eh, wh, lab, S, M, rmax, rsum, 1.0 / N, transposed=True, margin=mg)

    lib, p = ops.lib(), ops._p
    if kind == "rows":
        desc, fwd, bwd = ops._margin_rows_desc(mg, N), "frhip_head_fwd_sub_rows", "frhip_head_bwd_dt_sub_rows"
    else:
        desc = ops._margin_desc((ops.MARGIN_ARCFACE, 0, S, M, 0.0) if mg is None else mg)
        fwd, bwd = "frhip_head_fwd_sub", "frhip_head_bwd_dt_sub"
    part = torch.empty((2, lib.frhip_head_groups(CLASSES), N), dtype=torch.float32, device="cuda")
    zt1, rmax1, rsum1 = torch.zeros(N, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    tsub = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    dt1, dtt1 = torch.empty_like(dt), torch.empty_like(dtt)
    head = (ops.dt_of(eh), p(eh), p(wh), p(lab), N, CLASSES, D, 1, ctypes.byref(desc))
    ops.check(getattr(lib, fwd)(*head, p(part[0]), p(part[1]), p(zt1), p(tsub), p(rmax1), p(rsum1), ops._s()), fwd)
    ldt = dt.shape[1]
    ops.check(getattr(lib, bwd)(*head, p(rmax1), p(rsum1), 1.0 / N, None, p(dt1), ldt, ldt, p(dtt1), dtt.shape[1], ops._s()), bwd)
    for name, a, b in (("ztarget", zt, zt1), ("rowmax", rmax, rmax1), ("rowsum", rsum, rsum1), ("dT", dt, dt1), ("dTt", dtt, dtt1)):
        assert torch.equal(a, b), "%s: head_kernel and head_sub_kernel (K = 1) differ" % name
    assert bool(dt.any()) and bool(torch.isfinite(rsum).all())
    assert torch.equal(tsub.cpu(), torch.where(labels >= 0, 0, -1).to(torch.int32))


# ------------------------------------------------------------------------------------------------ 2. the module, fp32 mode
K3 = 3


def _shard_table(weight, K, classes, start, num):
    return weight.view(K, classes, -1)[:, start:start + num].reshape(K * num, -1).clone()


def _run_head(P, rank, ws, rate, dtype="fp32", seed=4300):
    from subcenter_double import case
    dev = torch.device("cuda", 0)
    emb, weight, labels, _ = case(ws * N, CLASSES, D, K3, seed)
    conf = types.SimpleNamespace(emd_size=D, sample_rate=rate, mixed_precision=False, loss_s=S, loss_m=M, frhip_dtype=dtype, subcenters=K3)
    pfc = P.PartialFC(conf, CLASSES).to(dev)
    assert type(pfc.kernels).__name__ == "HipHeadKernels" and pfc.subcenters == K3
    start, num = head_ref.shard_range(CLASSES, ws, rank)
    with torch.no_grad():
        (pfc.weight if rate < 1 else pfc.weight_activated.data).copy_(_shard_table(weight, K3, CLASSES, start, num).to(dev))
    dummy = torch.nn.Parameter(torch.zeros(1, device=dev))
    opt = torch.optim.SGD([{"params": [dummy]}, {"params": pfc.parameters()}], lr=0.1, momentum=0.9)
    mine = slice(rank * N, (rank + 1) * N)
    e = emb[mine].clone().to(dev).requires_grad_(True)
    torch.manual_seed(1000 + rank)                          # the sampling permutation comes from the CPU generator
    loss = pfc(e, labels[mine].clone().to(dev), opt)
    loss.backward()
    idx = pfc.weight_index if rate < 1 else torch.arange(pfc.num_local)
    return dict(loss=float(loss.detach()), d_emb=e.grad.cpu().numpy(), d_w=pfc.weight_activated.grad.cpu().numpy(),
                index=idx.cpu().numpy(), tsub=pfc.last_target_sub.cpu().numpy())


def _head_worker(rank, ws, path, ret, rate):
    for p in (ROOT, os.path.join(ROOT, "face-recognition-pytorch_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import nets.PartialFC as P
    torch.set_num_threads(1)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="file://" + path, rank=rank, world_size=ws)
    np.savez(os.path.join(ret, "rank%d.npz" % rank), **_run_head(P, rank, ws, rate))
    dist.destroy_process_group()


def _check_head(outs, ws, rate, seed=4300):
    """every rank against ONE evaluation of the double on the whole batch and the class rows the ranks activated; the criterion of
    tests/test_adaface_gpu.py's fp32-mode head (loss rtol 1e-4; gradients rtol 1e-3, atol 1e-5 of the largest reference element)"""
    from subcenter_double import case, pooled_head
    emb, weight, labels, _ = case(ws * N, CLASSES, D, K3, seed)
    shards = [head_ref.shard_range(CLASSES, ws, r) for r in range(ws)]
    index = [torch.from_numpy(outs[r]["index"]).long() for r in range(ws)]
    pos, offset = torch.full_like(labels, -1), 0
    for r, (start, num) in enumerate(shards):
        own = (labels >= start) & (labels < start + num)
        assert bool(torch.isin(labels[own] - start, index[r]).all()), "a positive class was not activated"
        pos[own] = torch.searchsorted(index[r], labels[own] - start) + offset
        offset += index[r].numel()
    if rate < 1:
        assert int(torch.unique(labels[labels >= 0]).numel()) < offset < CLASSES      # negatives were drawn, class rows were dropped
    planes = weight.view(K3, CLASSES, D)
    act = torch.cat([torch.cat([planes[k, index[r] + shards[r][0]] for r in range(ws)]) for k in range(K3)])
    ref = pooled_head(emb, act, pos, K3, S, M)
    gap = ref["gap"].clone()
    gap[:, pos[3]] = float("inf")
    assert float(gap.min()) >= 1e-5                                                    # also among the activated rows
    d_w = ref["d_w"].view(K3, offset, D)
    offset = 0
    for r, (start, num) in enumerate(shards):
        o, cnt = outs[r], index[r].numel()
        want_w = d_w[:, offset:offset + cnt].reshape(K3 * cnt, D).numpy()
        offset += cnt
        refs = (("d_emb", ws * ref["d_emb"][r * N:(r + 1) * N].numpy()), ("d_w", want_w))
        print("ws %d rank %d rate %.1f: loss %.8g (double %.8g)" % (ws, r, rate, float(o["loss"]), float(ref["loss"])), "".join(
            "  max |%s - double| %.3g of %.3g" % (key, float(np.abs(o[key] - w_).max()), float(np.abs(w_).max())) for key, w_ in refs))
        own = torch.nonzero((labels >= start) & (labels < start + num)).flatten()
        tsub = torch.full((ws * N,), -1, dtype=torch.int64)
        tsub[own] = ref["win"][own, pos[own]]
        assert np.array_equal(o["tsub"], tsub.numpy())
        np.testing.assert_allclose(float(o["loss"]), float(ref["loss"]), rtol=1e-4, err_msg="rank %d loss" % r)
        for key, w_ in refs:
            np.testing.assert_allclose(o[key], w_, rtol=1e-3, atol=1e-3 * float(np.abs(w_).max()) * 1e-2, err_msg="rank %d %s" % (r, key))
        # the centres that never won on this rank got an exact zero row
        never = np.abs(want_w).max(axis=1) == 0
        assert not o["d_w"][never].any()


@pytest.mark.parametrize("rate", [1.0, 0.3])
def test_module_fp32_vs_float64(pg, rate):
    import nets.PartialFC as P
    _check_head([_run_head(P, 0, 1, rate)], 1, rate)


@pytest.mark.parametrize("rate", [1.0, 0.3])
def test_module_fp32_two_ranks_vs_float64(rate):
    ws = 2
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_head_worker, args=(ws, os.path.join(td, "pg"), td, rate), nprocs=ws, join=True)
        outs = [dict(np.load(os.path.join(td, "rank%d.npz" % r))) for r in range(ws)]
    _check_head(outs, ws, rate)


# ------------------------------------------------------------------------------------------------ 3. bf16, frhip_head_dw on the path
def _bf16_case():
    """(130, 300, 512), K = 3: every row's target class has ONE centre built as the row's direction plus noise (cosine ~0.55: the clear
    winner, yet a target probability around one half, so that the targets and not the label -1 row set the size of the gradients), in a
    plane that rotates with the row; everything else is random (cosines of a few hundredths)."""
    n, classes, d = 130, 300, 512
    g = torch.Generator().manual_seed(n + classes + d)
    emb = torch.randn((n, d), generator=g)
    emb = emb / emb.norm(dim=1, keepdim=True) * (0.5 + 4.0 * torch.rand(n, generator=g))[:, None]
    weight = torch.randn((K3, classes, d), generator=g) * 0.05
    labels = torch.randperm(classes, generator=g)[:n].clone()                # distinct targets ...
    for i, c in enumerate((0, 63, 64, 127, 128, classes - 1)):
        hit = torch.nonzero(labels == c).flatten()
        if hit.numel():
            labels[hit] = int(labels[3 + i])
        labels[3 + i] = c
    labels[1] = labels[0]                                                    # ... but one duplicate: rows 0 and 1 pull on two centres of one class
    labels[2] = -1
    for i in range(n):
        if labels[i] >= 0:
            e = emb[i] / emb[i].norm()
            weight[i % K3, labels[i]] = (e + torch.randn(d, generator=g) * (1.5 / math.sqrt(d))) * 0.3
    return emb, weight.reshape(K3 * classes, d), labels


def _flip_bounds(emb, weight, ref, close, entry):
    """the largest element of dE / dW that one flipped winner among the `close` (row, class) pairs can move; entry [n, C] = s p / n"""
    e64, w64 = emb.double(), weight.double()
    en, wn = e64.norm(dim=1), w64.norm(dim=1)
    eh, wh = e64 / en[:, None], w64 / wn[:, None]
    n, k, c = ref["planes"].shape
    top = ref["planes"].argsort(dim=1, descending=True)[:, :2]              # [n, 2, C]: best and runner-up plane
    moved_e = moved_w = 0.0
    for m_, c_ in torch.nonzero(close).tolist():
        a, b = int(top[m_, 0, c_]) * c + c_, int(top[m_, 1, c_]) * c + c_
        moved_e = max(moved_e, float(entry[m_, c_] * (wh[a] - wh[b]).abs().max() / en[m_]))
        moved_w = max(moved_w, float(entry[m_, c_] * eh[m_].abs().max() / min(wn[a], wn[b])))
    return moved_e, moved_w


def test_bf16_head_vs_float64():
    """criterion of tests/test_adaface_gpu.py's bf16 head (loss rtol 3e-2; gradients rtol 0.1, atol 5 % of the largest reference element),
    no element excluded.  Every target's top-two gap is >= 0.02 on the double, far above bf16 rounding of unit vectors (2^-9 per
    element, ~1e-3 on a 512-term cosine): a winner can flip only on a non-target, where the gradient entry that moves to another centre
    is at most the element's softmax probability / n -- asserted below to be far inside the absolute tolerance."""
    import nets.PartialFC as P
    from frhip import ops
    from subcenter_double import pooled_head
    emb, weight, labels = _bf16_case()
    n, d = emb.shape
    classes = weight.shape[0] // K3
    ref = pooled_head(emb, weight, labels, K3, S, M)
    own = torch.nonzero(labels >= 0).flatten()
    tgap = ref["gap"][own, labels[own]]
    assert float(tgap.min()) >= 0.02
    twin = ref["win"][own, labels[own]]
    assert all(int((twin == k).sum()) >= 10 for k in range(K3))
    # non-targets whose winner bf16 could flip (gap < 0.02): the entry that would move, s x p / n, against the tolerance on d(cosine)
    z = ref["z"]
    p = torch.softmax(z, dim=1)
    p[own, labels[own]] = 0.0
    close = ref["gap"] < 0.02
    assert int(close.sum()) > 0
    print("bf16: %d of %d non-target winners within 0.02 of the runner-up, their largest softmax probability %.3g" % (
        int(close.sum()), close.numel(), float(p[close].max())))
    # the entry s p / n of d(cosine), moved from the best centre a to the runner-up b, changes element j of d(normalised embedding) by
    # s p / n x |what_a - what_b|[j] and one of d(normalised centre a, b) by s p / n x |ehat|[j] (before the normalisations' projections)
    moved_e, moved_w = _flip_bounds(emb, weight, ref, close, p * S / n)
    print("bf16: a flipped non-target moves at most %.3g of dE (atol %.3g) and %.3g of dW (atol %.3g)" % (
        moved_e, 0.05 * float(ref["d_emb"].abs().max()), moved_w, 0.05 * float(ref["d_w"].abs().max())))
    assert moved_e < 0.05 * float(ref["d_emb"].abs().max()) and moved_w < 0.05 * float(ref["d_w"].abs().max())

    kern = P.HipHeadKernels(torch.bfloat16)
    assert ops.lib().frhip_head_dw_ok(0, n, classes, d) == 1
    e_c, w_c, l_c = emb.cuda(), weight.cuda(), labels.to(torch.int32).cuda()
    ehat, enorm = kern.normalize(e_c)
    what, wnorm = kern.normalize(w_c)
    zt, rmax, rsum, tsub = kern.forward_stats(ehat, what, l_c, S, M, subcenters=K3)
    assert torch.equal(tsub.cpu()[own].long(), twin) and int(tsub[2]) == -1
    loss = float(kern.loss(kern.target_prob(zt, l_c, rmax, rsum)))
    d_e, d_w = kern.backward(ehat, enorm, what, wnorm, l_c, S, M, rmax, rsum, n, torch.ones(1, device="cuda"), subcenters=K3)
    d_e, d_w = d_e.cpu(), d_w.cpu()
    d_e_ref, d_w_ref = ref["d_emb"], ref["d_w"]
    print("bf16: loss %.6g (double %.6g); max |dE - double| %.3g of %.3g; max |dW - double| %.3g of %.3g" % (
        loss, float(ref["loss"]), float((d_e.double() - d_e_ref).abs().max()), float(d_e_ref.abs().max()),
        float((d_w.double() - d_w_ref).abs().max()), float(d_w_ref.abs().max())))
    assert d_w.shape == (K3 * classes, d)
    np.testing.assert_allclose(loss, float(ref["loss"]), rtol=3e-2)
    np.testing.assert_allclose(d_e.numpy(), d_e_ref.numpy(), rtol=0.1, atol=0.05 * float(d_e_ref.abs().max()))
    np.testing.assert_allclose(d_w.numpy(), d_w_ref.numpy(), rtol=0.1, atol=0.05 * float(d_w_ref.abs().max()))


# ------------------------------------------------------------------------------------------------ 5. through Model
@pytest.mark.parametrize("optimizer,rate", [("SGD", 1.0), ("AdamW", 0.3)])
def test_two_steps_through_model_with_three_centres(pg, optimizer, rate):
    """conf.subcenters = 3 is all a user sets.  Each step's loss is the double's on the embeddings the encoder produced (forward hook;
    fp32-mode head criterion, rtol 1e-4) and the class table as it stood; both parameter groups move; a centre that won no (row, class)
    of the step has an exactly zero gradient row, so it moves by the weight decay alone (SGD, first step: w - lr wd w)."""
    from model.FR_PartialFC import Model
    from subcenter_double import pooled_head
    classes, b, lr, wd = 256, 8, 0.1 if optimizer == "SGD" else 5e-4, 5e-4
    torch.cuda.set_device(0)
    conf = types.SimpleNamespace(network="ResNet18", emd_size=512, img_size=112, local_rank=0, world_size=1, sample_rate=rate,
                                 mixed_precision=False, loss_s=S, loss_m=M, n_classes=classes, optimizer=optimizer, lr=lr, wd=wd, mom=0.9,
                                 eps=1e-8, betas=(0.9, 0.999), loss="PartialFC", lr_scheduler=None, frhip_dtype="fp32", ckpt_path=None,
                                 subcenters=K3, subcenter_track=True)
    torch.manual_seed(31)
    model = Model(conf, None, "train")
    head = model.loss
    assert head.subcenters == K3 and head.sub_hits.is_cuda
    spec = resnet_ref.resnet_spec(resnet_ref.BLOCKS["ResNet18"])
    sd = recipe.fill_state(spec, 777)
    for key, _, kd in spec:
        if kd in ("bn_w", "bn_rv"):
            sd[key].fill_(1.0)
        elif kd in ("bn_b", "bn_rm"):
            sd[key].zero_()
    model.encoder.load_state_dict(sd, strict=True)
    table0 = recipe.normal(778, (K3 * classes, 512), 0.01)
    with torch.no_grad():
        (head.weight if rate < 1 else head.weight_activated.data).copy_(table0.cuda())
    seen = []
    hook = model.encoder.register_forward_hook(lambda mod, args, out: seen.append(out.detach().float().cpu()))
    probe = "layer1.0.conv1.weight"
    hits = torch.zeros((K3, classes), dtype=torch.int64)
    for st in range(2):
        if rate < 1:                        # the full table as the step will find it: the previous step's rows are still to be scattered
            full = head.weight.detach().cpu().clone()
            if st > 0:
                full[head._plane_rows(head.weight_index).cpu()] = head.weight_activated.detach().cpu()
        else:
            full = head.weight_activated.detach().cpu().clone()
        enc_before = model.encoder.state_dict()[probe].float().cpu().clone()
        img, ids = recipe.images(779 + 10 * st, b), recipe.labels(780 + 10 * st, b, classes)
        out = model.training_step((img, ids.clone()))
        emb = seen[st]
        assert emb.shape == (b, 512)
        index = head.weight_index.cpu() if rate < 1 else torch.arange(classes)
        rows = torch.cat([index + k * classes for k in range(K3)])
        lab = ids.reshape(-1).long()
        assert bool(torch.isin(lab, index).all())
        ref = pooled_head(emb, full[rows], torch.searchsorted(index, lab), K3, S, M)
        print("%s rate %.1f step %d: loss %.8g (double %.8g)" % (optimizer, rate, st, float(out["loss"]), float(ref["loss"])))
        np.testing.assert_allclose(float(out["loss"]), float(ref["loss"]), rtol=1e-4)
        after = head.weight_activated.detach().cpu()
        assert after.shape == (K3 * index.numel(), 512)
        assert not torch.equal(after, full[rows])
        assert not torch.equal(model.encoder.state_dict()[probe].float().cpu(), enc_before)
        safe = (ref["gap"] >= 1e-5).all(dim=0)                                           # classes whose winners fp32 cannot flip
        tsub = head.last_target_sub.cpu().long()
        if bool(safe[torch.searchsorted(index, lab)].all()):
            assert torch.equal(tsub, ref["win"][torch.arange(b), torch.searchsorted(index, lab)])
        for m_ in range(b):
            hits[tsub[m_], lab[m_]] += 1
        if optimizer == "SGD" and st == 0:
            won = torch.stack([(ref["win"] == k).any(dim=0) for k in range(K3)])          # [K, classes]
            idle = (~won) & safe[None, :]
            assert int(idle.sum()) > 0 and int(won.sum()) > 0
            before, now = full.view(K3, classes, 512), after.view(K3, classes, 512)
            decayed = before - lr * (wd * before)
            np.testing.assert_allclose(now[idle].numpy(), decayed[idle].numpy(), rtol=1e-6, atol=1e-9)
            assert float((now - decayed).abs().amax(dim=2)[won & safe[None, :]].min()) > 0
    hook.remove()
    assert torch.equal(head.sub_hits.cpu(), hits) and int(hits.sum()) == 2 * b
    sd_head = head.state_dict()
    assert sd_head["weight"].shape == (K3 * classes, 512) and torch.equal(sd_head["sub_hits"].cpu(), hits)
    assert head.collapse_subcenters().shape == (classes, 512)


# ------------------------------------------------------------------------------------------------ 6. run to run
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_two_identical_steps_are_byte_identical(pg, dtype):
    import nets.PartialFC as P
    a, b = _run_head(P, 0, 1, 1.0, dtype), _run_head(P, 0, 1, 1.0, dtype)
    assert a["loss"] == b["loss"] and np.isfinite(a["loss"])
    for key in ("d_emb", "d_w", "tsub"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert np.abs(a["d_w"]).max() > 0
