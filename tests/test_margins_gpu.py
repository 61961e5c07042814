"""Every margin module the reference's PartialFC can be built with, through the fused HIP head on the MI355X: CosFace, ArcFace
easy_margin, and CombinedMarginLoss with interclass filtering, against fixtures of the real reference (tools/make_golden_margins.py)
at world sizes 1 and 2 (real ranks on gloo, as tests/test_head_dist_gpu.py), through PartialFCAdamW and through Model with
conf.margin_loss; the stand-alone modules' kernels; and the full 512 x 122 000 x 512 bf16 head against an fp32 torch formulation."""
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

HEAD_FIXTURES = ["head_margin_cosface_ws1_rate10", "head_margin_cosface_ws1_rate03", "head_margin_cosface_ws2_rate03",
                 "head_margin_arc_filt_ws1_rate10", "head_margin_arc_filt_ws2_rate03", "head_margin_cos_filt_ws1_rate03",
                 "head_margin_arc_easy_ws1_rate10"]


def _worker(rank, ws, path, name, ret, adamw):
    for p in (ROOT, os.path.join(ROOT, "face-recognition-pytorch_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import nets.PartialFC as P
    from frhip import optim as fo
    from test_margins_cpu import margin_factory
    torch.set_num_threads(1)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")))
    dist.init_process_group("gloo", init_method="file://" + path, rank=rank, world_size=ws)
    C, B, D, rate, kind = int(g["C"]), int(g["B"]), int(g["D"]), float(g["rate"]), str(g["kind"])
    conf = types.SimpleNamespace(emd_size=D, sample_rate=rate, mixed_precision=False, loss_s=float(g["s"]), loss_m=float(g["m"]),
                                 frhip_dtype="fp32")
    cls = P.PartialFCAdamW if adamw else P.PartialFC
    pfc = cls(conf, C, margin_loss=margin_factory(kind, float(g["thr"]))).to(dev)
    assert type(pfc.kernels).__name__ == "HipHeadKernels"
    if kind == "arc_easy":
        pfc.margin_softmax.easy_margin = True           # after construction: read at call time, as the reference does
    with torch.no_grad():
        (pfc.weight if rate < 1 else pfc.weight_activated.data).copy_(recipe.normal(500 + rank, (pfc.num_local, D), 0.05).to(dev))
    dummy = torch.nn.Parameter(torch.zeros(1, device=dev))
    groups = [{"params": [dummy]}, {"params": pfc.parameters()}]
    opt = fo.AdamW(groups, lr=5e-4, weight_decay=5e-4) if adamw else torch.optim.SGD(groups, lr=0.1, momentum=0.9)
    emb = recipe.normal(100 + rank, (B, D)).to(dev).requires_grad_(True)
    lab = recipe.labels(200 + rank, B, C)
    lab[0] = 3
    lab[1] = 3
    torch.manual_seed(1000 + rank)
    loss = pfc(emb, lab.clone().to(dev), opt)
    loss.backward()
    idx = pfc.weight_index if rate < 1 else torch.arange(pfc.num_local)
    np.savez(os.path.join(ret, "rank%d.npz" % rank), loss=float(loss.detach()), d_emb=emb.grad.cpu().numpy(),
             d_w=pfc.weight_activated.grad.cpu().numpy(), index=idx.cpu().numpy())
    dist.destroy_process_group()


def _run_fixture(golden, name, adamw=False):
    g = golden(name)
    ws = int(g["ws"])
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_worker, args=(ws, os.path.join(td, "pg"), name, td, adamw), nprocs=ws, join=True)
        for r in range(ws):
            out = dict(np.load(os.path.join(td, "rank%d.npz" % r)))
            assert np.array_equal(out["index"], g["r%d_index" % r]), "rank %d: sampled rows differ" % r     # bit-exact
            np.testing.assert_allclose(float(out["loss"]), g["r%d_loss" % r], rtol=1e-4, err_msg="rank %d loss" % r)
            for key, ref in (("d_emb", g["r%d_d_emb" % r]), ("d_w", g["r%d_d_w_act" % r])):
                np.testing.assert_allclose(out[key], ref, rtol=1e-3, atol=1e-3 * float(np.abs(ref).max()) * 1e-2,
                                           err_msg="rank %d %s" % (r, key))


@pytest.mark.parametrize("name", HEAD_FIXTURES)
def test_partial_fc_margin_variants_vs_reference(golden, name):
    _run_fixture(golden, name)


def test_partial_fc_adamw_cosface_vs_reference(golden):
    _run_fixture(golden, "head_margin_cosface_ws1_rate03", adamw=True)


@pytest.mark.parametrize("kind", ["cosface", "arc_filt", "cos_filt", "arc_easy"])
def test_margin_module_forward_backward_vs_reference(golden, kind):
    """stand-alone module (frhip_margin_fwd_ex / _bwd_ex): reference output and input gradient, edge cosines included"""
    from test_margins_cpu import margin_factory
    g = golden("margin_" + kind)
    mod = margin_factory(kind, float(g["thr"]))(float(g["s"]), float(g["m"]))
    if kind == "arc_easy":
        mod.easy_margin = True
    leaf = torch.from_numpy(g["logits_in"]).cuda().requires_grad_(True)
    out = mod(leaf.clone(), torch.from_numpy(g["labels"]).cuda())
    out.backward(torch.from_numpy(g["upstream"]).cuda())
    np.testing.assert_allclose(out.detach().cpu().numpy(), g["logits_out"], rtol=1e-6, atol=1e-5)
    np.testing.assert_allclose(leaf.grad.cpu().numpy(), g["grad"], rtol=1e-5, atol=1e-5)
    if kind.endswith("filt"):
        assert int((leaf.grad == 0).sum()) >= int(g["n_filtered"])


@pytest.mark.parametrize("kind", ["cosface", "arc_filt"])
def test_full_size_bf16_head_vs_fp32_torch_formulation(kind):
    """512 x 122 000 x 512 in bf16 (frhip_head_dw serves d = 512) against explicit fp32 logits, the reference margin code restated in
    tests/margin_formula.py and cross-entropy; criteria of tests/test_head_gpu.py's cfg-2 size head test"""
    import nets.PartialFC as P
    from frhip import ops
    from margin_formula import margin_logits
    from nets.ArcFace import COSFACE, ARCFACE, Margin
    n, classes, d = 512, 122000, 512
    gen = torch.Generator().manual_seed(n + classes)
    emb = torch.randn((n, d), generator=gen)
    w = torch.randn((classes, d), generator=gen) * 0.05
    lab = torch.randint(0, classes, (n,), generator=gen)
    lab[1] = lab[0]
    lab[2] = -1
    w[lab[3]] = emb[3] * 0.9 + 0.1 * torch.randn(d, generator=gen)
    w[lab[4]] = -emb[4]
    s, m, thr = 30.0, 0.35, 0.05            # d = 512: cosine spread ~0.044, so ~13 % of the elements are filtered at 0.05
    mg = Margin(COSFACE, False, s, m, 0.0) if kind == "cosface" else Margin(ARCFACE, False, s, m, thr)
    eh, en = head_ref.l2_normalize(emb)
    wh, wn = head_ref.l2_normalize(w)
    raw = eh @ wh.t()
    z, slope = margin_logits(raw.clamp(-1, 1), lab, mg.kind, mg.easy, s, m, mg.filter_thr)
    if mg.filter_thr:
        assert float((slope == 0).float().mean()) >= 0.05
    logp = torch.log_softmax(z, dim=1)
    rows = torch.nonzero(lab >= 0).flatten()
    q = torch.zeros(n)
    q[rows] = logp[rows, lab[rows]].exp()
    loss_ref = -(q.clamp_min(1e-30).log().mean())
    dz = logp.exp()
    dz[rows, lab[rows]] -= 1.0
    dcos = dz / n * s * slope * ((raw >= -1) & (raw <= 1))
    d_e_ref = head_ref.l2_normalize_bwd(dcos @ wh, eh, en)
    d_w_ref = head_ref.l2_normalize_bwd(dcos.t() @ eh, wh, wn)
    del raw, z, slope, logp, dz, dcos
    kern = P.HipHeadKernels(torch.bfloat16)
    e_c, w_c, l_c = emb.cuda(), w.cuda(), lab.to(torch.int32).cuda()
    ehat, enorm = kern.normalize(e_c)
    what, wnorm = kern.normalize(w_c)
    zt, rmax, rsum = kern.forward_stats(ehat, what, l_c, s, m, margin=mg)
    loss = float(kern.loss(kern.target_prob(zt, l_c, rmax, rsum)))
    up = torch.ones(1, device="cuda")
    d_e, d_w = kern.backward(ehat, enorm, what, wnorm, l_c, s, m, rmax, rsum, n, up, margin=mg)
    d_e, d_w = d_e.cpu(), d_w.cpu()
    np.testing.assert_allclose(loss, loss_ref.item(), rtol=3e-2)
    np.testing.assert_allclose(d_e.numpy(), d_e_ref.numpy(), rtol=0.1, atol=0.05 * d_e_ref.abs().max().item())
    np.testing.assert_allclose(d_w.numpy(), d_w_ref.numpy(), rtol=0.1, atol=0.05 * d_w_ref.abs().max().item())


@pytest.fixture(scope="module")
def pg():
    if not dist.is_initialized():
        d = tempfile.mkdtemp()
        dist.init_process_group("gloo", init_method="file://" + os.path.join(d, "pg"), rank=0, world_size=1)
    yield
    if dist.is_initialized():
        dist.destroy_process_group()


def test_three_sgd_steps_cosface_through_model_conf_margin_loss(golden, pg):
    """Model with conf.margin_loss = CosFace against the reference's PartialFC(margin_loss=CosFace): tolerances of
    tests/test_train_step_gpu.py test_three_sgd_steps_on_fresh_batches_match_reference"""
    from model.FR_PartialFC import Model
    from nets.ArcFace import CosFace
    g = golden("train_step_resnet18_c256_fresh_cosface_rate03")
    rate, C, B, steps = float(g["rate"]), int(g["C"]), int(g["B"]), int(g["steps"])
    torch.cuda.set_device(0)
    conf = types.SimpleNamespace(network="ResNet18", emd_size=512, img_size=112, local_rank=0, world_size=1, sample_rate=rate,
                                 mixed_precision=False, loss_s=30.0, loss_m=0.35, n_classes=C, optimizer="SGD", lr=0.1, wd=5e-4, mom=0.9,
                                 loss="PartialFC", lr_scheduler=None, frhip_dtype="fp32", ckpt_path=None, margin_loss=CosFace)
    model = Model(conf, None, "train")
    assert isinstance(model.loss.margin_softmax, CosFace)
    spec = resnet_ref.resnet_spec(resnet_ref.BLOCKS["ResNet18"])
    sd = recipe.fill_state(spec, 777)
    for k, _, kd in spec:
        if kd in ("bn_w", "bn_rv"):
            sd[k].fill_(1.0)
        elif kd in ("bn_b", "bn_rm"):
            sd[k].zero_()
    model.encoder.load_state_dict(sd, strict=True)
    with torch.no_grad():
        model.loss.weight.copy_(recipe.normal(778, (C, 512), 0.01).cuda())
    for st in range(steps):
        img, ids = recipe.images(779 + 10 * st, B), recipe.labels(780 + 10 * st, B, C)
        torch.manual_seed(3000 + st)
        out = model.training_step((img, ids.clone()))
        np.testing.assert_allclose(float(out["loss"]), g["losses"][st], rtol=1e-3 if st == 0 else 2e-3)
        np.testing.assert_allclose(float(model.opt.last_grad_norm()), g["grad_norms"][st], rtol=5e-3)
        assert np.array_equal(model.loss.weight_index.cpu().numpy(), g["index_step%d" % st])
    model.loss.update()
    esd = model.encoder.state_dict()
    for k in [k[6:] for k in g if k.startswith("probe.") and k != "probe.head_weight"]:
        want = g["probe." + k]
        rms = want[1] / esd[k].numel() ** 0.5
        got = recipe.probe(esd[k].float().cpu())
        np.testing.assert_allclose(got[1], want[1], rtol=2e-3, err_msg=k)
        np.testing.assert_allclose(got[2:], want[2:], rtol=5e-3, atol=5e-2 * rms + 1e-7, err_msg=k)
    want = g["probe.head_weight"]
    wfin = model.loss.weight
    np.testing.assert_allclose(recipe.probe(wfin.cpu(), 4096)[1:], want[1:], rtol=5e-3, atol=5e-2 * want[1] / wfin.numel() ** 0.5)
