"""MagFace (magnitude-aware margins, a gradient through the norms) on the MI355X against the float64 restatement in
tests/magface_double.py: the margin kernel, the normalise-backward with the norm gradient folded in, the norm-gradient kernel, the fused
head in fp32 mode at world sizes 1 and 2 (real ranks on gloo, every rank on cuda:0), sub-centres, the bf16 head with frhip_head_dw on
the path, and optimisation steps through Model with conf.margin_loss = MagFace.

The fp32-mode inputs (magface_double.branch_case) make the double itself take every branch of the definition -- norms below l_a, above
u_a and inside, a target pushed past pi - eps, one whose raw cosine is above 1 - eps, a duplicate label, a label -1 row, targets in
columns 0, 63, 64, 127, 128 and the last class -- and keep every other target at least 1e-2 rad inside the clip of the angle and every
norm 0.5 away from both ends of the window, so that no branch is decided by rounding (magface_double.assert_branches asserts all of it
on the double).  Every comparison prints its measured maximum error; no element is excluded anywhere."""
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
S, L_M, U_M, L_A, U_A, LAMBDA_G, EPS = 64.0, 0.45, 0.8, 10.0, 110.0, 35.0, 1e-3


@pytest.fixture(scope="module")
def pg():
    if not dist.is_initialized():
        d = tempfile.mkdtemp()
        dist.init_process_group("gloo", init_method="file://" + os.path.join(d, "pg"), rank=0, world_size=1)
    yield
    if dist.is_initialized():
        dist.destroy_process_group()


def _close(name, got, ref, rtol, atol_of_max):
    """assert_allclose with atol = atol_of_max x the largest reference element, printing the measured maximum error first"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    top = float(np.abs(ref).max())
    print("  max |%s - double| %.3g of %.3g" % (name, float(np.abs(got - ref).max()), top))
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol_of_max * top, err_msg=name)


# ------------------------------------------------------------------------------------------------ 1. the margin kernel
@pytest.mark.parametrize("n", [1, 2, 37, 1000, 4097])
def test_magface_margins_kernel_vs_float64(n):
    """m_ang and reg: rtol 1e-6, the criterion of the AdaFace margin kernel (tests/test_adaface_gpu.py); m_add exactly 0"""
    from frhip import ops
    from magface_double import margins
    g = torch.Generator().manual_seed(11 * n)
    norms = torch.exp(torch.randn(n, generator=g) * 1.2 + 3.3)            # median 27, tails past both ends of [10, 110]
    if n >= 2:
        norms[0], norms[-1] = 1e-4, 500.0
    want_ang, _, want_reg = margins(norms)
    if n >= 37:
        assert int((norms < L_A).sum()) and int((norms > U_A).sum()) and int(((norms > L_A) & (norms < U_A)).sum())
    m_ang, m_add, reg = ops.magface_margins(norms.cuda(), L_A, U_A, L_M, U_M)
    print("n=%d: reg %.9g (double %.9g), max rel m_ang %.3g" % (
        n, float(reg), float(want_reg), float(((m_ang.cpu().double() - want_ang).abs() / want_ang).max())))
    np.testing.assert_allclose(m_ang.cpu().numpy(), want_ang.numpy(), rtol=1e-6)
    np.testing.assert_allclose(float(reg), float(want_reg), rtol=1e-6)
    assert m_add.shape == (n,) and int((m_add != 0).sum()) == 0


# ------------------------------------------------------------------------------------------------ 2. normalise-backward + norm gradient
@pytest.mark.parametrize("rows,d,dtype", [(1, 64, torch.float32), (3, 64, torch.float32), (5, 64, torch.float32), (130, 64, torch.float32),
                                          (5, 512, torch.bfloat16), (130, 512, torch.bfloat16)])
def test_l2norm_bwd_norm_vs_float64(rows, d, dtype):
    """dx = ((g - xhat <g, xhat>) / |x| + dnorm xhat) out_scale on the operands the kernel is given; maximum error <= 2e-5 of the largest
    reference element, the criterion of tests/test_kernels_gpu.py for the normalise-backward"""
    from frhip import ops
    g = torch.Generator().manual_seed(rows * 1000 + d)
    x = (torch.randn((rows, d), generator=g) * torch.linspace(0.5, 40.0, rows)[:, None]).cuda()
    dxhat = torch.randn((rows, d), generator=g).cuda()
    dnorm = (torch.randn(rows, generator=g) * 0.3).cuda()
    xhat, norms = ops.l2norm_rows(x, dtype)
    h, g64 = xhat.double(), dxhat.double()
    tangent = (g64 - h * (g64 * h).sum(1, keepdim=True)) / norms.double()[:, None]
    for scale in (1.0, 2.0):
        got = ops.l2norm_bwd_norm(dxhat, xhat, norms, dnorm, out_scale=scale)
        want = (tangent + dnorm.double()[:, None] * h) * scale
        err = float((got.double() - want).abs().max())
        print("rows %d d %d %s x%g: max error %.3g of %.3g" % (rows, d, dtype, scale, err, float(want.abs().max())))
        assert err <= 2e-5 * float(want.abs().max())
    plain = ops.l2norm_bwd(dxhat, xhat, norms, out_scale=2.0)
    got = ops.l2norm_bwd_norm(dxhat, xhat, norms, torch.zeros_like(dnorm), out_scale=2.0)
    print("dnorm = 0 against frhip_l2norm_bwd: max difference %.3g, bit-equal: %s" % (float((got - plain).abs().max()), torch.equal(got, plain)))
    assert float((got - plain).abs().max()) <= 2e-5 * float(plain.abs().max())
    assert float((got.double() - tangent * 2.0).abs().max()) <= 2e-5 * float(tangent.abs().max() * 2.0)


# ------------------------------------------------------------------------------------------------ shared fp32-mode inputs
_CASES = {}


def _case(n, classes, d):
    """seeded inputs and the double's evaluation of them, built once per shape and shared (never modified: every user clones)"""
    from magface_double import assert_branches, branch_case
    key = (n, classes, d)
    if key not in _CASES:
        emb, weight, labels = branch_case(n, classes, d, 9100 + n + classes)
        assert_branches(emb, weight, labels)
        _CASES[key] = (emb, weight, labels)
    return _CASES[key]


_REFS = {}


def _reference(n, classes, d):
    from magface_double import head_reference
    key = (n, classes, d)
    if key not in _REFS:
        _REFS[key] = head_reference(*_case(n, classes, d))
    return _REFS[key]


# ------------------------------------------------------------------------------------------------ 3. the norm-gradient kernel
def test_magface_norm_grad_kernel_vs_float64():
    """frhip_magface_norm_grad at world size 1, fed the statistics of frhip_head_fwd_rows in fp32 mode, against the double's d loss / d norm
    (autograd through the clamp of the norms, acos, the clip of the angle and the cross-entropy): rtol 1e-3, atol 1e-5 of the largest
    reference element, the fp32-mode head gradient criterion of tests/test_adaface_gpu.py; exactly 0 where the clamp of the norm binds."""
    import nets.PartialFC as P
    from magface_double import SPECIAL_ROWS
    from nets.ArcFace import MagFace, margin_of
    n, classes, d = 37, 150, 64
    emb, weight, labels = _case(n, classes, d)
    _, _, _, d_norm = _reference(n, classes, d)
    kern = P.HipHeadKernels(torch.float32)
    mod = MagFace()
    mg = margin_of(mod)
    norms = emb.norm(dim=1).cuda()
    lab = labels.to(torch.int32).cuda()
    ehat, _ = kern.normalize(emb.cuda())
    what, _ = kern.normalize(weight.cuda())
    rm, _ = mod.row_margins(norms, kern)
    zt, rmax, rsum = kern.forward_stats(ehat, what, lab, S, L_M, margin=rm)
    packed = kern.pack_stats(zt, lab, rmax, rsum).unsqueeze(0)
    outside = (norms.cpu() < L_A) | (norms.cpu() > U_A)
    assert int(outside.sum()) >= 4 and bool((d_norm[outside] == 0).all()) and bool((d_norm[~outside] != 0).all())
    over = SPECIAL_ROWS["over_pi"]                       # the cross-entropy term is clipped away, the regulariser's is what remains
    np.testing.assert_allclose(float(d_norm[over]), LAMBDA_G / n * (1 / U_A ** 2 - 1 / float(emb[over].double().norm()) ** 2), rtol=1e-12)
    for upstream, scale in ((None, 1.0), (0.37, 2.0)):
        up = None if upstream is None else torch.full((1,), upstream, device="cuda")
        got = kern.magface_norm_grad(norms, packed, rmax, rsum, mg, 1.0 / n, up, out_scale=scale).cpu()
        want = d_norm * (1.0 if upstream is None else float(np.float32(upstream))) * scale
        print("upstream %s, out_scale %g:" % (upstream, scale))
        _close("d_norm", got.numpy(), want.numpy(), 1e-3, 1e-5)
        assert bool((got[outside] == 0).all())


def test_magface_module_forward_backward_vs_float64():
    """MagFace.forward(logits, labels, norms) on explicit cosines (frhip_magface_margins + frhip_margin_fwd_rows / _bwd_rows): output and
    input gradient; tolerances of tests/test_adaface_gpu.py test_adaface_module_forward_backward_vs_float64"""
    from adaface_double import logits
    from magface_double import margins
    from nets.ArcFace import MagFace
    n, classes, d = 37, 150, 64
    emb, weight, labels = _case(n, classes, d)
    norms = emb.norm(dim=1)
    e, w = emb.double(), weight.double()
    cos32 = ((e / e.norm(dim=1, keepdim=True)) @ (w / w.norm(dim=1, keepdim=True)).t()).float()      # the module's input
    upstream = torch.randn((n, classes), generator=torch.Generator().manual_seed(5))
    m_ang, m_add, _ = margins(norms)
    ref_in = cos32.double().requires_grad_(True)
    ref_out = logits(ref_in, labels, S, m_ang, m_add, EPS)
    ref_out.backward(upstream.double())
    leaf = cos32.cuda().requires_grad_(True)
    out = MagFace()(leaf, labels.cuda(), norms.cuda())
    out.backward(upstream.cuda())
    assert torch.equal(leaf.detach().cpu(), cos32)                          # not in place
    print("module: max |out - double| %.3g, max |grad - double| %.3g" % (
        float((out.detach().cpu().double() - ref_out.detach()).abs().max()), float((leaf.grad.cpu().double() - ref_in.grad).abs().max())))
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref_out.detach().numpy(), rtol=1e-6, atol=1e-5)
    np.testing.assert_allclose(leaf.grad.cpu().numpy(), ref_in.grad.numpy(), rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------ 4. the fused head, fp32 mode
def _head_worker(rank, ws, path, ret, shape, rate):
    """one rank: PartialFC(margin_loss = MagFace) on the HIP kernels, its rows of the shared batch; results travel through files
    (see tests/test_head_dist_gpu.py)"""
    for p in (ROOT, os.path.join(ROOT, "face-recognition-pytorch_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import nets.PartialFC as P
    torch.set_num_threads(1)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="file://" + path, rank=rank, world_size=ws)
    out = _run_head(P, rank, ws, shape, rate)
    np.savez(os.path.join(ret, "rank%d.npz" % rank), **out)
    dist.destroy_process_group()


def _run_head(P, rank, ws, shape, rate):
    from nets.ArcFace import MagFace
    b, classes, d = shape
    dev = torch.device("cuda", 0)
    emb, weight, labels = _case(ws * b, classes, d)
    conf = types.SimpleNamespace(emd_size=d, sample_rate=rate, mixed_precision=False, loss_s=S, loss_m=L_M, frhip_dtype="fp32")
    pfc = P.PartialFC(conf, classes, margin_loss=MagFace).to(dev)
    assert type(pfc.kernels).__name__ == "HipHeadKernels"
    start, num = head_ref.shard_range(classes, ws, rank)
    with torch.no_grad():
        (pfc.weight if rate < 1 else pfc.weight_activated.data).copy_(weight[start:start + num].to(dev))
    dummy = torch.nn.Parameter(torch.zeros(1, device=dev))
    opt = torch.optim.SGD([{"params": [dummy]}, {"params": pfc.parameters()}], lr=0.1, momentum=0.9)
    mine = slice(rank * b, (rank + 1) * b)
    e = emb[mine].clone().to(dev).requires_grad_(True)
    norms = emb[mine].norm(dim=1).to(dev).requires_grad_(True)          # a leaf of its own: its .grad is the head's norm gradient
    torch.manual_seed(1000 + rank)                          # the sampling permutation comes from the CPU generator
    loss = pfc(e, labels[mine].clone().to(dev), opt, norms=norms)
    loss.backward()
    idx = pfc.weight_index if rate < 1 else torch.arange(pfc.num_local)
    return dict(loss=loss.detach().cpu().numpy(), d_emb=e.grad.cpu().numpy(), d_norm=norms.grad.cpu().numpy(),
                d_w=pfc.weight_activated.grad.cpu().numpy(), index=idx.cpu().numpy())


def _check_head(outs, ws, shape, rate):
    """every rank against ONE evaluation of the double on the whole batch and the class rows the ranks activated; criteria of
    tests/test_adaface_gpu.py _check_head (loss rtol 1e-4; gradients rtol 1e-3, atol 1e-5 of the largest reference element)"""
    from magface_double import head_reference
    b, classes, d = shape
    emb, weight, labels = _case(ws * b, classes, d)
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
    loss, d_emb, d_w, d_norm = head_reference(emb, weight[rows], pos) if rate < 1 else _reference(ws * b, classes, d)
    assert float(d_norm.abs().max()) > 0
    offset = 0
    for r in range(ws):
        o = outs[r]
        k = o["index"].shape[0]
        print("ws %d rank %d rate %.1f %s: loss %.8g (double %.8g)" % (ws, r, rate, shape, float(o["loss"]), float(loss)))
        assert np.array_equal(o["loss"], outs[0]["loss"])                             # equal across ranks, bit for bit
        np.testing.assert_allclose(float(o["loss"]), float(loss), rtol=1e-4, err_msg="rank %d loss" % r)
        _close("d_emb", o["d_emb"], ws * d_emb[r * b:(r + 1) * b].numpy(), 1e-3, 1e-5)
        _close("d_w", o["d_w"], d_w[offset:offset + k].numpy(), 1e-3, 1e-5)
        _close("d_norm", o["d_norm"], ws * d_norm[r * b:(r + 1) * b].numpy(), 1e-3, 1e-5)
        offset += k


HEAD_SHAPES = [(37, 150, 64), (130, 257, 64)]      # ragged 16-row fragments; one and three 128-class tiles; a 64-group tail


@pytest.mark.parametrize("rate", [1.0, 0.3])
@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_fused_head_fp32_vs_float64(pg, shape, rate):
    import nets.PartialFC as P
    _check_head([_run_head(P, 0, 1, shape, rate)], 1, shape, rate)


@pytest.mark.parametrize("rate", [1.0, 0.3])
@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_fused_head_fp32_two_ranks_vs_float64(shape, rate):
    """`shape[0]` rows per rank: the norms of both ranks are gathered in rank order, both derive the same margins and the same loss, and
    each keeps its slice of the norm gradient (x world size)"""
    ws = 2
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_head_worker, args=(ws, os.path.join(td, "pg"), td, shape, rate), nprocs=ws, join=True)
        outs = [dict(np.load(os.path.join(td, "rank%d.npz" % r))) for r in range(ws)]
    _check_head(outs, ws, shape, rate)


# ------------------------------------------------------------------------------------------------ 5. sub-centres
def _sub_head(k):
    """adaface_double.head_loss with K centres per class: weight [K x classes, d] plane-major, a class's cosine the maximum over them"""
    import adaface_double as A

    def head(emb, weight, labels, s, m_ang, m_add, eps):
        labels = labels.reshape(-1).long()
        eh = emb / emb.norm(dim=1, keepdim=True).clamp_min(head_ref.NORM_EPS)
        wh = weight / weight.norm(dim=1, keepdim=True).clamp_min(head_ref.NORM_EPS)
        cos = (eh @ wh.t()).view(emb.shape[0], k, -1).max(dim=1).values
        z = A.logits(cos, labels, s, m_ang, m_add, eps)
        lse = torch.logsumexp(z, dim=1)
        zt = z.gather(1, labels.clamp(min=0)[:, None]).flatten()
        per_row = torch.where(labels >= 0, lse - zt, lse - lse.detach() + A.NO_TARGET)
        value = per_row.detach().clamp(max=A.NO_TARGET)
        return (per_row + (value - per_row.detach())).mean()
    return head


def test_fused_head_with_two_subcentres_vs_float64(pg):
    """conf.subcenters = 2 through the _sub_rows kernels at (37, 150, 64), world size 1, fp32 mode: float64 autograd with the maximum over
    the centres; criteria of the fused-head test above.  Plane 0 is the shared case's table; plane 1 is random except for the class whose
    target must stay past pi - eps (a centre at cosine -0.9999 of that embedding: it wins, and u is still past the clip)."""
    import nets.PartialFC as P
    from magface_double import SPECIAL_ROWS, head_reference, margins
    from nets.ArcFace import MagFace
    import adaface_double as A
    b, classes, d, k = 37, 150, 64, 2
    emb, weight, labels = _case(b, classes, d)
    g = torch.Generator().manual_seed(77)
    second = torch.randn((classes, d), generator=g, dtype=torch.float64) * 0.05
    e = emb[SPECIAL_ROWS["over_pi"]].double()
    e = e / e.norm()
    r = torch.randn(d, generator=g, dtype=torch.float64)
    perp = r - (r @ e) * e
    second[10] = (-0.9999 * e + math.sqrt(1 - 0.9999 ** 2) * perp / perp.norm()) * 0.3
    table = torch.cat([weight.double(), second]).float()
    # on the double: no (row, class) whose two centres are closer than 1e-6 in cosine (ten times the rounding of an fp32 cosine at
    # d = 64: the kernels then pick the same winner), the special rows keep their branches, every other target is 1e-2 inside the clip
    e64, w64 = emb.double(), table.double()
    planes = ((e64 / e64.norm(dim=1, keepdim=True)) @ (w64 / w64.norm(dim=1, keepdim=True)).t()).view(b, k, classes)
    assert float((planes[:, 0] - planes[:, 1]).abs().min()) > 1e-6
    raw = planes.max(dim=1).values
    m_ang, _, _ = margins(e64.norm(dim=1))
    u = A.target_angle(raw, labels, m_ang, EPS)
    own = torch.nonzero(labels >= 0).flatten()
    assert u[SPECIAL_ROWS["over_pi"]] > math.pi - EPS and raw[SPECIAL_ROWS["clamp_hi"], 12] > 1 - EPS
    others = torch.tensor([i for i in own.tolist() if i != SPECIAL_ROWS["over_pi"]])
    assert float((u[others] - EPS).min()) >= 1e-2 and float((math.pi - EPS - u[others]).min()) >= 1e-2
    loss_ref, d_emb, d_w, d_norm = head_reference(emb, table, labels, head=_sub_head(k))
    assert float(d_w[:classes].abs().max()) > 0 and float(d_w[classes:].abs().max()) > 0      # both planes won somewhere

    dev = torch.device("cuda", 0)
    conf = types.SimpleNamespace(emd_size=d, sample_rate=1.0, mixed_precision=False, loss_s=S, loss_m=L_M, frhip_dtype="fp32", subcenters=k)
    pfc = P.PartialFC(conf, classes, margin_loss=MagFace).to(dev)
    with torch.no_grad():
        pfc.weight_activated.data.copy_(table.to(dev))
    x = emb.clone().to(dev).requires_grad_(True)
    norms = emb.norm(dim=1).to(dev).requires_grad_(True)
    loss = pfc(x, labels.clone().to(dev), None, norms=norms)
    loss.backward()
    print("sub-centres: loss %.8g (double %.8g)" % (float(loss.detach()), float(loss_ref)))
    np.testing.assert_allclose(float(loss.detach()), float(loss_ref), rtol=1e-4)
    _close("d_emb", x.grad.cpu().numpy(), d_emb.numpy(), 1e-3, 1e-5)
    _close("d_w", pfc.weight_activated.grad.cpu().numpy(), d_w.numpy(), 1e-3, 1e-5)
    _close("d_norm", norms.grad.cpu().numpy(), d_norm.numpy(), 1e-3, 1e-5)


# ------------------------------------------------------------------------------------------------ 6. bf16, frhip_head_dw on the path
def test_bf16_head_vs_float64():
    """(130, 257, 512) in bf16 through the kernels PartialFC calls; criteria of tests/test_adaface_gpu.py test_bf16_head_vs_float64 (loss
    rtol 3e-2; gradients, the norms' included, rtol 0.1, atol 5 % of the largest reference element), no element excluded.  Every target
    has |t| <= 0.9 and u at least 0.05 inside its clip bounds: bf16 cosines decide no branch."""
    import nets.PartialFC as P
    from frhip import ops
    from magface_double import head_reference, target_angle
    from nets.ArcFace import MagFace, RowMargins, margin_of
    n, classes, d = 130, 257, 512
    g = torch.Generator().manual_seed(n + classes + d + 1)
    emb = torch.randn((n, d), generator=g)
    emb = emb / emb.norm(dim=1, keepdim=True) * torch.linspace(4.0, 140.0, n)[torch.randperm(n, generator=g)][:, None]
    weight = torch.randn((classes, d), generator=g) * 0.05
    labels = torch.randint(0, classes, (n,), generator=g)
    labels[1] = labels[0]
    labels[2] = -1
    for i, c in enumerate((0, 63, 64, 127, 128, classes - 1)):
        labels[3 + i] = c
    for i in range(9, 20):                                                  # correlated targets, t from -0.5 to 0.8
        t = -0.5 + 0.13 * (i - 9)
        r = torch.randn(d, generator=g)
        e = emb[i] / emb[i].norm()
        perp = r - (r @ e) * e
        labels[i] = 200 + i
        weight[200 + i] = t * e + math.sqrt(1 - t * t) * perp / perp.norm()
    norms = emb.norm(dim=1)
    assert float((norms - L_A).abs().min()) > 0.1 and float((norms - U_A).abs().min()) > 0.1
    assert int((norms < L_A).sum()) and int((norms > U_A).sum()) and int(((norms > L_A) & (norms < U_A)).sum())
    u, raw, _ = target_angle(emb, weight, labels)
    own = torch.nonzero(labels >= 0).flatten()
    assert float(raw[own, labels[own]].abs().max()) <= 0.9 and float(raw[own, labels[own]].abs().max()) > 0.7
    assert float(u[own].min()) >= EPS + 0.05 and float(u[own].max()) <= math.pi - EPS - 0.05
    loss_ref, d_e_ref, d_w_ref, d_n_ref = head_reference(emb, weight, labels)

    kern = P.HipHeadKernels(torch.bfloat16)
    assert ops.lib().frhip_head_dw_ok(0, n, classes, d) == 1
    mod = MagFace()
    mg = margin_of(mod)
    rm, reg = mod.row_margins(norms.cuda(), kern)
    assert isinstance(rm, RowMargins) and rm.s == mg.s
    e_c, w_c, l_c = emb.cuda(), weight.cuda(), labels.to(torch.int32).cuda()
    ehat, enorm = kern.normalize(e_c)
    what, wnorm = kern.normalize(w_c)
    zt, rmax, rsum = kern.forward_stats(ehat, what, l_c, S, L_M, margin=rm)
    loss = float(kern.loss(kern.target_prob(zt, l_c, rmax, rsum))) + mg.lambda_g * float(reg)
    one = torch.ones(1, device="cuda")
    d_e, d_w = kern.backward(ehat, enorm, what, wnorm, l_c, S, L_M, rmax, rsum, n, one, margin=rm)
    d_n = kern.magface_norm_grad(norms.cuda(), kern.pack_stats(zt, l_c, rmax, rsum).unsqueeze(0), rmax, rsum, mg, 1.0 / n, one)
    print("bf16: loss %.6g (double %.6g)" % (loss, float(loss_ref)))
    np.testing.assert_allclose(loss, float(loss_ref), rtol=3e-2)
    _close("d_emb", d_e.cpu().numpy(), d_e_ref.numpy(), 0.1, 0.05)
    _close("d_w", d_w.cpu().numpy(), d_w_ref.numpy(), 0.1, 0.05)
    _close("d_norm", d_n.cpu().numpy(), d_n_ref.numpy(), 0.1, 0.05)


# ------------------------------------------------------------------------------------------------ 7. through Model
def test_sgd_steps_through_model_conf_margin_loss_magface(pg):
    """conf.margin_loss = MagFace is all a user sets: differentiable norms travel from the normalise node to the head and their gradient
    back into it.  Step 0's loss is the double's on the embeddings the encoder produced (forward hook; fp32-mode head criterion, rtol
    1e-4); both parameter groups move in both steps.  Then one more forward / backward with lambda_g = 0 and a window [l_a, u_a] above
    every norm: the norm path is silent there, and the gradient that reaches the encoder's output is bit for bit the one of the same
    pass with the norm path not taken at all (norms_need_grad off: detached norms, the plain normalise-backward)."""
    from frhip.optim import run_deferred_side
    from magface_double import head_reference
    from model.FR_PartialFC import Model, normalize_with_norms
    from nets.ArcFace import MagFace
    classes, b = 256, 8
    torch.cuda.set_device(0)
    conf = types.SimpleNamespace(network="ResNet18", emd_size=512, img_size=112, local_rank=0, world_size=1, sample_rate=1.0,
                                 mixed_precision=False, loss_s=S, loss_m=L_M, n_classes=classes, optimizer="SGD", lr=0.1, wd=5e-4, mom=0.9,
                                 loss="PartialFC", lr_scheduler=None, frhip_dtype="fp32", ckpt_path=None, margin_loss=MagFace)
    model = Model(conf, None, "train")
    head = model.loss
    assert isinstance(head.margin_softmax, MagFace)
    spec = resnet_ref.resnet_spec(resnet_ref.BLOCKS["ResNet18"])
    sd = recipe.fill_state(spec, 777)
    for key, _, kd in spec:
        if kd in ("bn_w", "bn_rv"):
            sd[key].fill_(1.0)
        elif kd in ("bn_b", "bn_rm"):
            sd[key].zero_()
    model.encoder.load_state_dict(sd, strict=True)
    with torch.no_grad():
        head.weight_activated.data.copy_(recipe.normal(778, (classes, 512), 0.01).cuda())
    seen = []
    hook = model.encoder.register_forward_hook(lambda mod, args, out: seen.append(out.detach().float().cpu()))
    probe = "layer1.0.conv1.weight"
    for st in range(2):
        w_before = head.weight_activated.detach().cpu().clone()
        enc_before = model.encoder.state_dict()[probe].float().cpu().clone()
        img, ids = recipe.images(779 + 10 * st, b), recipe.labels(780 + 10 * st, b, classes)
        out = model.training_step((img, ids.clone()))
        emb = seen[st]
        assert emb.shape == (b, 512)
        nrm = emb.norm(dim=1)
        print("step %d: loss %.8g; norms %.4g .. %.4g, %d of %d inside (%g, %g)" % (
            st, float(out["loss"]), float(nrm.min()), float(nrm.max()), int(((nrm > L_A) & (nrm < U_A)).sum()), b, L_A, U_A))
        if st == 0:
            loss_ref, _, _, _ = head_reference(emb, w_before, ids.reshape(-1))
            print("step 0: double's loss %.8g" % float(loss_ref))
            np.testing.assert_allclose(float(out["loss"]), float(loss_ref), rtol=1e-4)
        assert not torch.equal(head.weight_activated.detach().cpu(), w_before)
        assert not torch.equal(model.encoder.state_dict()[probe].float().cpu(), enc_before)
    hook.remove()
    assert len(seen) == 2

    mod = head.margin_softmax
    mod.lambda_g, mod.l_a, mod.u_a = 0.0, 1e4, 2e4
    img, ids = recipe.images(799, b).cuda(), recipe.labels(800, b, classes).cuda()

    def encoder_output_gradient(norm_path):
        model.opt.zero_grad()
        out = model.forward(img)
        got = []
        out.register_hook(lambda g: got.append(g.detach().clone()))
        feat, norms = normalize_with_norms(out, norm_path)
        assert norms.requires_grad == norm_path and float(norms.detach().max()) < mod.l_a
        loss = head(feat, ids.clone(), model.opt, norms=norms)
        loss.backward()
        run_deferred_side()
        assert len(got) == 1
        return float(loss.detach()), got[0]

    loss_on, g_on = encoder_output_gradient(True)
    loss_off, g_off = encoder_output_gradient(False)
    print("silent norm path: loss %.8g / %.8g, max |difference| of the encoder-output gradient %.3g of %.3g" % (
        loss_on, loss_off, float((g_on - g_off).abs().max()), float(g_off.abs().max())))
    assert loss_on == loss_off and float(g_off.abs().max()) > 0
    assert torch.equal(g_on, g_off)
