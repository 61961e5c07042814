"""AdaFace (per-row adaptive margins) on the MI355X against the float64 restatement in tests/adaface_double.py: the margin kernel, the
stand-alone module, the fused head in fp32 mode at world sizes 1 and 2 (real ranks on gloo, every rank on cuda:0), the bf16 head with
frhip_head_dw on the path, and two optimisation steps through Model with conf.margin_loss = AdaFace.

The fp32-mode inputs (adaface_double.branch_case) make the double itself take every branch of the definition -- k at -1, at +1 and
inside, a target pushed past pi - eps, one pulled below eps, one whose raw cosine is above 1 - eps, a duplicate label, a label -1 row,
targets in columns 0, 63, 64, 127, 128 and the last class -- and keep every other target at least 1e-3 away from each boundary, so
that no branch is decided by rounding (adaface_double.assert_branches asserts all of it on the double).  The running buffers start
from (10, 2): the initial 20 / 100 never reach the clips of k."""
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
S, M, H, T_ALPHA, EPS = 64.0, 0.4, 0.333, 0.01, 1e-3


@pytest.fixture(scope="module")
def pg():
    if not dist.is_initialized():
        d = tempfile.mkdtemp()
        dist.init_process_group("gloo", init_method="file://" + os.path.join(d, "pg"), rank=0, world_size=1)
    yield
    if dist.is_initialized():
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------ 1. the margin kernel
@pytest.mark.parametrize("update", [True, False])
@pytest.mark.parametrize("n", [2, 37, 1000, 4097])
def test_adaface_margins_kernel_vs_float64(n, update):
    from adaface_double import BUFFERS, margins
    from frhip import ops
    g = torch.Generator().manual_seed(7 * n + int(update))
    norms = torch.exp(torch.randn(n, generator=g) * 1.2 + 2.2)            # median 9, a tail past both clips of k
    norms[0], norms[-1] = 1e-4, 150.0                                     # below and above the clip of the norms themselves
    mean = torch.full((1,), BUFFERS[0], device="cuda")
    std = torch.full((1,), BUFFERS[1], device="cuda")
    want = margins(norms, M, H, T_ALPHA, BUFFERS[0], BUFFERS[1], update, EPS)
    if n >= 37:
        k = want["k"]
        assert int((k == -1).sum()) and int((k == 1).sum()) and int(((k > -1) & (k < 1)).sum())
    m_ang, m_add = ops.adaface_margins(norms.cuda(), M, H, T_ALPHA, EPS, mean, std, update)
    print("n=%d update=%s: batch_mean %.9g (double %.9g), batch_std %.9g (double %.9g), max rel m_ang %.3g" % (
        n, update, float(mean), float(want["batch_mean"]), float(std), float(want["batch_std"]),
        float(((m_ang.cpu().double() - want["m_ang"]).abs() / want["m_ang"].abs().clamp_min(1e-300)).max())))
    if update:
        np.testing.assert_allclose(float(mean), float(want["batch_mean"]), rtol=1e-6)
        np.testing.assert_allclose(float(std), float(want["batch_std"]), rtol=1e-6)
    else:
        assert float(mean) == BUFFERS[0] and float(std) == BUFFERS[1]      # untouched
    np.testing.assert_allclose(m_ang.cpu().numpy(), want["m_ang"].numpy(), rtol=1e-6)
    np.testing.assert_allclose(m_add.cpu().numpy(), want["m_add"].numpy(), rtol=1e-6)


# ------------------------------------------------------------------------------------------------ 2. the stand-alone module
def test_adaface_module_forward_backward_vs_float64():
    """AdaFace.forward(logits, labels, norms) on explicit cosines (frhip_adaface_margins + frhip_margin_fwd_rows / _bwd_rows): output and
    input gradient; tolerances of tests/test_margins_gpu.py test_margin_module_forward_backward_vs_reference"""
    from adaface_double import BUFFERS, assert_branches, logits
    from nets.ArcFace import AdaFace
    n, classes, d = 37, 150, 64
    emb, weight, labels = _case(n, classes, d)
    norms = emb.norm(dim=1)
    mr = assert_branches(emb, weight, labels, norms, S, M, H, T_ALPHA)
    e, w = emb.double(), weight.double()
    cos32 = ((e / e.norm(dim=1, keepdim=True)) @ (w / w.norm(dim=1, keepdim=True)).t()).float()      # the module's input
    upstream = torch.randn((n, classes), generator=torch.Generator().manual_seed(5))
    ref_in = cos32.double().requires_grad_(True)
    ref_out = logits(ref_in, labels, S, mr["m_ang"], mr["m_add"], EPS)
    ref_out.backward(upstream.double())
    mod = AdaFace(S, M, H, T_ALPHA).cuda()
    with torch.no_grad():
        mod.batch_mean.fill_(BUFFERS[0])
        mod.batch_std.fill_(BUFFERS[1])
    leaf = cos32.cuda().requires_grad_(True)
    out = mod(leaf, labels.cuda(), norms.cuda())
    out.backward(upstream.cuda())
    assert torch.equal(leaf.detach().cpu(), cos32)                          # not in place
    np.testing.assert_allclose(float(mod.batch_mean), float(mr["batch_mean"]), rtol=1e-6)
    np.testing.assert_allclose(float(mod.batch_std), float(mr["batch_std"]), rtol=1e-6)
    print("module: max |out - double| %.3g, max |grad - double| %.3g" % (
        float((out.detach().cpu().double() - ref_out.detach()).abs().max()), float((leaf.grad.cpu().double() - ref_in.grad).abs().max())))
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref_out.detach().numpy(), rtol=1e-6, atol=1e-5)
    np.testing.assert_allclose(leaf.grad.cpu().numpy(), ref_in.grad.numpy(), rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------ 3. / 4. the fused head, fp32 mode
_CASES = {}


def _case(n, classes, d):
    """seeded inputs, built once per shape and shared (never modified: every user clones)"""
    from adaface_double import branch_case
    key = (n, classes, d)
    if key not in _CASES:
        _CASES[key] = branch_case(n, classes, d, 9000 + n + classes)
    return _CASES[key]


def _head_worker(rank, ws, path, ret, shape, rate):
    """one rank: PartialFC(margin_loss = AdaFace) on the HIP kernels, its rows of the shared batch; results travel through files
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
    from adaface_double import BUFFERS
    from nets.ArcFace import AdaFace
    b, classes, d = shape
    dev = torch.device("cuda", 0)
    emb, weight, labels = _case(ws * b, classes, d)
    norms = emb.norm(dim=1)
    conf = types.SimpleNamespace(emd_size=d, sample_rate=rate, mixed_precision=False, loss_s=S, loss_m=M, frhip_dtype="fp32")
    pfc = P.PartialFC(conf, classes, margin_loss=lambda s, m: AdaFace(s, m, H, T_ALPHA)).to(dev)
    assert type(pfc.kernels).__name__ == "HipHeadKernels"
    start, num = head_ref.shard_range(classes, ws, rank)
    with torch.no_grad():
        (pfc.weight if rate < 1 else pfc.weight_activated.data).copy_(weight[start:start + num].to(dev))
        pfc.margin_softmax.batch_mean.fill_(BUFFERS[0])
        pfc.margin_softmax.batch_std.fill_(BUFFERS[1])
    dummy = torch.nn.Parameter(torch.zeros(1, device=dev))
    opt = torch.optim.SGD([{"params": [dummy]}, {"params": pfc.parameters()}], lr=0.1, momentum=0.9)
    mine = slice(rank * b, (rank + 1) * b)
    e = emb[mine].clone().to(dev).requires_grad_(True)
    torch.manual_seed(1000 + rank)                          # the sampling permutation comes from the CPU generator
    loss = pfc(e, labels[mine].clone().to(dev), opt, norms=norms[mine].clone().to(dev))
    loss.backward()
    idx = pfc.weight_index if rate < 1 else torch.arange(pfc.num_local)
    return dict(loss=float(loss.detach()), d_emb=e.grad.cpu().numpy(), d_w=pfc.weight_activated.grad.cpu().numpy(),
                index=idx.cpu().numpy(), mean=pfc.margin_softmax.batch_mean.cpu().numpy(), std=pfc.margin_softmax.batch_std.cpu().numpy())


def _check_head(outs, ws, shape, rate):
    """every rank against ONE evaluation of the double on the whole batch and the class rows the ranks activated; criteria of
    tests/test_margins_gpu.py _run_fixture (loss rtol 1e-4; gradients rtol 1e-3, atol 1e-5 of the largest reference element)"""
    from adaface_double import assert_branches, head_reference
    b, classes, d = shape
    emb, weight, labels = _case(ws * b, classes, d)
    norms = emb.norm(dim=1)
    mr = assert_branches(emb, weight, labels, norms, S, M, H, T_ALPHA)
    # the activated class rows of all ranks in rank order, and every label as its position in that list
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
    loss, d_emb, d_w = head_reference(emb, weight[rows], pos, S, mr["m_ang"], mr["m_add"], EPS)
    offset = 0
    for r in range(ws):
        o = outs[r]
        k = o["index"].shape[0]
        refs = (("d_emb", ws * d_emb[r * b:(r + 1) * b].numpy()), ("d_w", d_w[offset:offset + k].numpy()))
        offset += k
        print("ws %d rank %d rate %.1f %s: loss %.8g (double %.8g)" % (ws, r, rate, shape, float(o["loss"]), float(loss)), "".join(
            "  max |%s - double| %.3g of %.3g" % (key, float(np.abs(o[key] - ref).max()), float(np.abs(ref).max())) for key, ref in refs))
        np.testing.assert_allclose(float(o["mean"]), float(mr["batch_mean"]), rtol=1e-6)
        np.testing.assert_allclose(float(o["std"]), float(mr["batch_std"]), rtol=1e-6)
        assert np.array_equal(o["mean"], outs[0]["mean"]) and np.array_equal(o["std"], outs[0]["std"])      # equal across ranks, bit for bit
        np.testing.assert_allclose(float(o["loss"]), float(loss), rtol=1e-4, err_msg="rank %d loss" % r)
        for key, ref in refs:
            np.testing.assert_allclose(o[key], ref, rtol=1e-3, atol=1e-3 * float(np.abs(ref).max()) * 1e-2, err_msg="rank %d %s" % (r, key))


HEAD_SHAPES = [(37, 150, 64), (130, 257, 64)]      # ragged 16-row fragments; one and three 128-class tiles; a 64-group tail


@pytest.mark.parametrize("rate", [1.0, 0.3])
@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_fused_head_fp32_vs_float64(pg, shape, rate):
    import nets.PartialFC as P
    _check_head([_run_head(P, 0, 1, shape, rate)], 1, shape, rate)


@pytest.mark.parametrize("rate", [1.0, 0.3])
@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_fused_head_fp32_two_ranks_vs_float64(shape, rate):
    """`shape[0]` rows per rank: the norms of both ranks are gathered in rank order and both derive the same margins and buffers"""
    ws = 2
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_head_worker, args=(ws, os.path.join(td, "pg"), td, shape, rate), nprocs=ws, join=True)
        outs = [dict(np.load(os.path.join(td, "rank%d.npz" % r))) for r in range(ws)]
    _check_head(outs, ws, shape, rate)


# ------------------------------------------------------------------------------------------------ 5. bf16, frhip_head_dw on the path
def test_bf16_head_vs_float64():
    """(130, 257, 512) in bf16 through the kernels PartialFC calls; criteria of tests/test_margins_gpu.py
    test_full_size_bf16_head_vs_fp32_torch_formulation (loss rtol 3e-2; gradients rtol 0.1, atol 5 % of the largest reference element),
    no element excluded.  Every target has |t| <= 0.9 and u at least 0.05 inside its clip bounds: bf16 cosines decide no branch."""
    import nets.PartialFC as P
    from adaface_double import BUFFERS, head_reference, margins, target_angle
    from frhip import ops
    from nets.ArcFace import AdaFace, RowMargins, margin_of
    n, classes, d = 130, 257, 512
    g = torch.Generator().manual_seed(n + classes + d)
    emb = torch.randn((n, d), generator=g)
    emb = emb / emb.norm(dim=1, keepdim=True) * torch.linspace(0.5, 25.0, n)[torch.randperm(n, generator=g)][:, None]
    weight = torch.randn((classes, d), generator=g) * 0.05
    labels = torch.randint(0, classes, (n,), generator=g)
    labels[1] = labels[0]
    labels[2] = -1
    for i, c in enumerate((0, 63, 64, 127, 128, classes - 1)):
        labels[3 + i] = c
    for i in range(9, 20):                                                  # correlated targets, |t| up to 0.8 on either side
        t = -0.8 + 0.16 * (i - 9)
        r = torch.randn(d, generator=g)
        e = emb[i] / emb[i].norm()
        perp = r - (r @ e) * e
        labels[i] = 200 + i
        weight[200 + i] = t * e + math.sqrt(1 - t * t) * perp / perp.norm()
    norms = emb.norm(dim=1)
    mr = margins(norms, M, H, T_ALPHA, BUFFERS[0], BUFFERS[1], True, EPS)
    e64, w64 = emb.double(), weight.double()
    raw = (e64 / e64.norm(dim=1, keepdim=True)) @ (w64 / w64.norm(dim=1, keepdim=True)).t()
    own = torch.nonzero(labels >= 0).flatten()
    u = target_angle(raw, labels, mr["m_ang"], EPS)[own]
    assert float(raw[own, labels[own]].abs().max()) <= 0.9 and float(raw[own, labels[own]].abs().max()) > 0.7
    assert float(u.min()) >= EPS + 0.05 and float(u.max()) <= math.pi - EPS - 0.05
    k = mr["k"]
    assert int((k == -1).sum()) and int((k == 1).sum()) and int(((k > -1) & (k < 1)).sum())
    loss_ref, d_e_ref, d_w_ref = head_reference(emb, weight, labels, S, mr["m_ang"], mr["m_add"], EPS)

    kern = P.HipHeadKernels(torch.bfloat16)
    assert ops.lib().frhip_head_dw_ok(0, n, classes, d) == 1
    mod = AdaFace(S, M, H, T_ALPHA).cuda()
    with torch.no_grad():
        mod.batch_mean.fill_(BUFFERS[0])
        mod.batch_std.fill_(BUFFERS[1])
    rm = mod.row_margins(norms.cuda(), kern)
    assert isinstance(rm, RowMargins) and rm.s == margin_of(mod).s
    e_c, w_c, l_c = emb.cuda(), weight.cuda(), labels.to(torch.int32).cuda()
    ehat, enorm = kern.normalize(e_c)
    what, wnorm = kern.normalize(w_c)
    zt, rmax, rsum = kern.forward_stats(ehat, what, l_c, S, M, margin=rm)
    loss = float(kern.loss(kern.target_prob(zt, l_c, rmax, rsum)))
    d_e, d_w = kern.backward(ehat, enorm, what, wnorm, l_c, S, M, rmax, rsum, n, torch.ones(1, device="cuda"), margin=rm)
    d_e, d_w = d_e.cpu(), d_w.cpu()
    print("bf16: loss %.6g (double %.6g); max |dE - double| %.3g of %.3g; max |dW - double| %.3g of %.3g" % (
        loss, float(loss_ref), float((d_e.double() - d_e_ref).abs().max()), float(d_e_ref.abs().max()),
        float((d_w.double() - d_w_ref).abs().max()), float(d_w_ref.abs().max())))
    np.testing.assert_allclose(loss, float(loss_ref), rtol=3e-2)
    np.testing.assert_allclose(d_e.numpy(), d_e_ref.numpy(), rtol=0.1, atol=0.05 * float(d_e_ref.abs().max()))
    np.testing.assert_allclose(d_w.numpy(), d_w_ref.numpy(), rtol=0.1, atol=0.05 * float(d_w_ref.abs().max()))


# ------------------------------------------------------------------------------------------------ 6. through Model
def test_two_sgd_steps_through_model_conf_margin_loss_adaface(pg):
    """conf.margin_loss = AdaFace is all a user sets: the norms travel from the normalise node to the head.  Step 1's loss is the double's
    on the embeddings the encoder produced (forward hook; fp32-mode head criterion, rtol 1e-4); after each step the running buffers are the
    double's update from those embeddings' norms (rtol 1e-6, the margin kernel's criterion); both parameter groups moved."""
    from adaface_double import head_reference, margins
    from model.FR_PartialFC import Model
    from nets.ArcFace import AdaFace
    classes, b = 256, 8
    torch.cuda.set_device(0)
    conf = types.SimpleNamespace(network="ResNet18", emd_size=512, img_size=112, local_rank=0, world_size=1, sample_rate=1.0,
                                 mixed_precision=False, loss_s=S, loss_m=M, n_classes=classes, optimizer="SGD", lr=0.1, wd=5e-4, mom=0.9,
                                 loss="PartialFC", lr_scheduler=None, frhip_dtype="fp32", ckpt_path=None, margin_loss=AdaFace)
    model = Model(conf, None, "train")
    head = model.loss
    assert isinstance(head.margin_softmax, AdaFace) and head.margin_softmax.batch_mean.is_cuda
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
    mean, std = 20.0, 100.0                                                 # the initial buffers
    for st in range(2):
        w_before = head.weight_activated.detach().cpu().clone()
        enc_before = model.encoder.state_dict()[probe].float().cpu().clone()
        img, ids = recipe.images(779 + 10 * st, b), recipe.labels(780 + 10 * st, b, classes)
        out = model.training_step((img, ids.clone()))
        emb = seen[st]
        assert emb.shape == (b, 512)
        mr = margins(emb.double().norm(dim=1), M, H, T_ALPHA, mean, std, True, EPS)
        got = (float(head.margin_softmax.batch_mean), float(head.margin_softmax.batch_std))
        print("step %d: loss %.8g, buffers %.9g %.9g (double %.9g %.9g)" % (st, float(out["loss"]), got[0], got[1],
                                                                           float(mr["batch_mean"]), float(mr["batch_std"])))
        np.testing.assert_allclose(got[0], float(mr["batch_mean"]), rtol=1e-6)
        np.testing.assert_allclose(got[1], float(mr["batch_std"]), rtol=1e-6)
        mean, std = got                                                     # the next step starts from the stored fp32 values
        if st == 0:
            loss_ref, _, _ = head_reference(emb, w_before, ids.reshape(-1), S, mr["m_ang"], mr["m_add"], EPS)
            print("step 0: double's loss %.8g" % float(loss_ref))
            np.testing.assert_allclose(float(out["loss"]), float(loss_ref), rtol=1e-4)
        assert not torch.equal(head.weight_activated.detach().cpu(), w_before)
        assert not torch.equal(model.encoder.state_dict()[probe].float().cpu(), enc_before)
    hook.remove()
    assert len(seen) == 2
