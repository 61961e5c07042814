"""Margin modules other than plain ArcFace (CosFace, ArcFace easy_margin, CombinedMarginLoss with interclass filtering) through the
drop-in PartialFC without a GPU: how each module resolves to the kernels' margin descriptor, and the product host logic on gloo with a
margin-aware kernel double against the fixtures the real reference produced (tools/make_golden_margins.py)."""
import os
import sys
import tempfile
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEAD_FIXTURES = ["head_margin_cosface_ws1_rate10", "head_margin_cosface_ws1_rate03", "head_margin_cosface_ws2_rate03",
                 "head_margin_arc_filt_ws1_rate10", "head_margin_arc_filt_ws2_rate03", "head_margin_cos_filt_ws1_rate03",
                 "head_margin_arc_easy_ws1_rate10"]


def margin_factory(kind, thr):
    """the factory the fixture's reference PartialFC was built with, on this package's modules"""
    from nets.ArcFace import ArcFace, CombinedMarginLoss, CosFace
    if kind == "cosface":
        return CosFace
    if kind == "arc_filt":
        return lambda s, m: CombinedMarginLoss(s, 1.0, m, 0.0, thr)
    if kind == "cos_filt":
        return lambda s, m: CombinedMarginLoss(s, 1.0, 0.0, m, thr)
    if kind == "arc_easy":
        return ArcFace
    raise ValueError(kind)


def test_margin_descriptor_of_every_module():
    from nets.ArcFace import ARCFACE, COSFACE, ArcFace, CombinedMarginLoss, CosFace, Margin, is_plain_arcface, margin_of
    assert margin_of(ArcFace(30.0, 0.35)) == Margin(ARCFACE, False, 30.0, 0.35, 0.0)
    assert is_plain_arcface(margin_of(ArcFace(30.0, 0.35)))
    assert margin_of(CosFace(64.0, 0.4)) == Margin(COSFACE, False, 64.0, 0.4, 0.0)
    assert margin_of(CombinedMarginLoss(64.0, 1.0, 0.5, 0.0)) == Margin(ARCFACE, False, 64.0, 0.5, 0.0)
    assert is_plain_arcface(margin_of(CombinedMarginLoss(64.0, 1.0, 0.5, 0.0)))
    assert margin_of(CombinedMarginLoss(64.0, 1.0, 0.5, 0.0, 0.2)) == Margin(ARCFACE, False, 64.0, 0.5, 0.2)
    assert margin_of(CombinedMarginLoss(64.0, 0.9, 0.3, 0.4, 0.2)) == Margin(COSFACE, False, 64.0, 0.4, 0.2)   # m1, m2 ignored
    assert margin_of(CombinedMarginLoss(64.0, 1.0, 0.5, 0.0, -1)).filter_thr == 0.0
    with pytest.raises(RuntimeError):
        margin_of(CombinedMarginLoss(64.0, 0.9, 0.5, 0.0))
    with pytest.raises(NotImplementedError, match="CosFace"):
        margin_of(torch.nn.Identity())
    a = ArcFace(30.0, 0.35)
    a.easy_margin = True                              # read at call time, as the reference's forward does
    assert margin_of(a).easy and not is_plain_arcface(margin_of(a))
    c = CombinedMarginLoss(64.0, 1.0, 0.5, 0.0)
    c.easy_margin = True
    assert margin_of(c).easy


class _RecordingKernels:
    """kernel double that only records how the host called the margin-dependent kernels"""

    def __init__(self):
        from head_double import OracleHeadKernels
        self.inner, self.calls = OracleHeadKernels(), []

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def forward_stats(self, *a, **k):
        self.calls.append(("forward_stats", k))
        return self.inner.forward_stats(*a)

    def backward(self, *a, **k):
        self.calls.append(("backward", {x: k[x] for x in k if x == "margin"}))
        return self.inner.backward(*a, **{x: k[x] for x in k if x != "margin"})


def test_plain_arcface_keeps_the_kernel_interface_and_others_pass_the_descriptor():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nets.PartialFC as P
    from nets.ArcFace import ArcFace, CombinedMarginLoss, CosFace
    with tempfile.TemporaryDirectory() as td:
        dist.init_process_group("gloo", init_method="file://" + os.path.join(td, "pg"), rank=0, world_size=1)
        try:
            conf = types.SimpleNamespace(emd_size=64, sample_rate=1.0, mixed_precision=False, loss_s=30.0, loss_m=0.35)
            for factory, want in ((ArcFace, None), (lambda s, m: CombinedMarginLoss(s, 1.0, m, 0.0), None), (CosFace, "cos")):
                kern = _RecordingKernels()
                pfc = P.PartialFC(conf, 50, margin_loss=factory, kernels=kern)
                pfc(torch.randn(4, 64, requires_grad=True), torch.tensor([1, 2, 3, 4]), None).backward()
                if want is None:
                    assert kern.calls == [("forward_stats", {}), ("backward", {})]
                else:
                    assert [c[0] for c in kern.calls] == ["forward_stats", "backward"]
                    assert all(c[1]["margin"].kind == 1 for c in kern.calls)
            kern = _RecordingKernels()
            pfc = P.PartialFC(conf, 50, kernels=kern)
            pfc.margin_softmax.easy_margin = True        # after construction, as a user of the reference would
            pfc(torch.randn(4, 64), torch.tensor([1, 2, 3, 4]), None)
            assert kern.calls[0][1]["margin"].easy
            with pytest.raises(NotImplementedError):
                P.PartialFC(conf, 50, margin_loss=lambda s, m: torch.nn.Identity(), kernels=kern)
        finally:
            dist.destroy_process_group()


def _worker(rank, ws, path, name, ret):
    for p in (ROOT, os.path.join(ROOT, "face-recognition-pytorch_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from head_double import OracleHeadKernels
    from margin_formula import margin_logits
    from oracle import head_ref, recipe
    import nets.PartialFC as P
    from test_margins_cpu import margin_factory

    class MarginKernels(OracleHeadKernels):
        """the oracle double with the margin descriptor: explicit logits from tests/margin_formula.py"""

        def _logits_m(self, ehat, what, labels, mg):
            raw = ehat @ what.t()
            z, slope = margin_logits(raw.clamp(-1.0, 1.0), labels, mg.kind, mg.easy, mg.s, mg.m, mg.filter_thr)
            return raw, z, slope

        def forward_stats(self, ehat, what, labels_i32, s, m, margin):
            _, z, _ = self._logits_m(ehat, what, labels_i32, margin)
            rmax = z.max(dim=1).values
            rsum = torch.exp(z - rmax[:, None]).sum(dim=1)
            zt = torch.zeros(z.shape[0])
            rows = torch.nonzero(labels_i32 >= 0).flatten()
            zt[rows] = z[rows, labels_i32[rows].long()]
            return zt, rmax, rsum

        def backward(self, ehat, enorm, what, wnorm, labels_i32, s, m, rmax, rsum, n_global, upstream, e_scale=1.0, on_de=None,
                     margin=None):
            raw, z, slope = self._logits_m(ehat, what, labels_i32, margin)
            dz = torch.exp(z - rmax[:, None]) / rsum[:, None]
            rows = torch.nonzero(labels_i32 >= 0).flatten()
            dz[rows, labels_i32[rows].long()] -= 1.0
            dz = dz / n_global * upstream
            dcos = dz * s * slope * ((raw >= -1.0) & (raw <= 1.0))
            d_e = head_ref.l2_normalize_bwd(dcos @ what, ehat, enorm[:, None]) * e_scale
            if on_de is not None:
                on_de(d_e)
            return d_e, head_ref.l2_normalize_bwd(dcos.t() @ ehat, what, wnorm[:, None])

    torch.set_num_threads(1)
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")))
    dist.init_process_group("gloo", init_method="file://" + path, rank=rank, world_size=ws)
    C, B, D, rate = int(g["C"]), int(g["B"]), int(g["D"]), float(g["rate"])
    conf = types.SimpleNamespace(emd_size=D, sample_rate=rate, mixed_precision=False, loss_s=float(g["s"]), loss_m=float(g["m"]))
    kind = str(g["kind"])
    pfc = P.PartialFC(conf, C, margin_loss=margin_factory(kind, float(g["thr"])), kernels=MarginKernels())
    if kind == "arc_easy":
        pfc.margin_softmax.easy_margin = True
    with torch.no_grad():
        (pfc.weight if rate < 1 else pfc.weight_activated.data).copy_(recipe.normal(500 + rank, (pfc.num_local, D), 0.05))
    dummy = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([{"params": [dummy]}, {"params": pfc.parameters()}], lr=0.1, momentum=0.9)
    emb = recipe.normal(100 + rank, (B, D)).requires_grad_(True)
    lab = recipe.labels(200 + rank, B, C)
    lab[0] = 3
    lab[1] = 3
    torch.manual_seed(1000 + rank)
    loss = pfc(emb, lab.clone(), opt)
    loss.backward()
    idx = pfc.weight_index if rate < 1 else torch.arange(pfc.num_local)
    np.savez(os.path.join(ret, "rank%d.npz" % rank), loss=float(loss), d_emb=emb.grad.numpy(), d_w=pfc.weight_activated.grad.numpy(),
             index=idx.numpy())
    dist.destroy_process_group()


@pytest.mark.parametrize("name", HEAD_FIXTURES)
def test_partial_fc_host_logic_with_margin_variants_vs_reference(golden, name):
    g = golden(name)
    ws = int(g["ws"])
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_worker, args=(ws, os.path.join(td, "pg"), name, td), nprocs=ws, join=True)
        for r in range(ws):
            out = dict(np.load(os.path.join(td, "rank%d.npz" % r)))
            assert np.array_equal(out["index"], g["r%d_index" % r])
            np.testing.assert_allclose(float(out["loss"]), g["r%d_loss" % r], rtol=1e-5)
            np.testing.assert_allclose(out["d_emb"], g["r%d_d_emb" % r], rtol=1e-4, atol=1e-7)
            np.testing.assert_allclose(out["d_w"], g["r%d_d_w_act" % r], rtol=1e-4, atol=1e-7)


def test_filtering_fixtures_filter_a_meaningful_fraction(golden):
    for name in HEAD_FIXTURES:
        g = golden(name)
        if str(g["kind"]).endswith("filt"):
            ws = int(g["ws"])
            frac = sum(int(g["r%d_n_filtered" % r]) for r in range(ws)) / sum(int(g["r%d_n_elements" % r]) for r in range(ws))
            assert frac >= 0.05, (name, frac)


@pytest.mark.parametrize("kind", ["cosface", "arc_filt", "cos_filt", "arc_easy"])
def test_margin_formula_matches_reference_module_fixture(golden, kind):
    """the torch restatement the GPU tests compare against reproduces the reference modules, edges included"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from margin_formula import margin_logits
    g = golden("margin_" + kind)
    t = torch.from_numpy(g["logits_in"])
    z, slope = margin_logits(t, torch.from_numpy(g["labels"]), 0 if kind.startswith("arc") else 1, kind == "arc_easy",
                             float(g["s"]), float(g["m"]), float(g["thr"]))
    np.testing.assert_allclose(z.numpy(), g["logits_out"], rtol=1e-6, atol=1e-5)
    np.testing.assert_allclose((g["upstream"] * float(g["s"]) * slope.numpy()), g["grad"], rtol=1e-5, atol=1e-5)
