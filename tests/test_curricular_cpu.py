"""CurricularFace (hard negatives re-weighted by a running mean of the target cosines) without a GPU: the float64 double of
tests/curricular_double.py against the published forward written out here, the module and descriptor surface, the C ABI's refusal of bad
arguments, and the distributed host logic on real gloo ranks with the double's kernels -- the same loss and the same t at world sizes 1
and 2, eval mode, checkpoints."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
S, M, ALPHA = 64.0, 0.5, 0.01
C, B, D = 150, 37, 64


# ------------------------------------------------------------------------------------------------ the double against the published forward
def _published_forward(cos, label, t, s, m, training=True):
    """CurricularFace.forward of the official implementation from the clamped cosines on, float64, written out: the mask against
    cos(theta_y + m) without a fallback, the EMA BEFORE t is used, the modulation of the masked elements, the scatter of the target.
    -> (output, the new t)"""
    cos_m, sin_m = math.cos(m), math.sin(m)
    threshold, mm = math.cos(math.pi - m), math.sin(math.pi - m) * m
    cos_theta = cos.clamp(-1, 1).clone()
    rows = torch.arange(cos.shape[0])
    target_logit = cos_theta[rows, label].view(-1, 1)
    sin_theta = torch.sqrt(1.0 - torch.pow(target_logit, 2))
    cos_theta_m = target_logit * cos_m - sin_theta * sin_m
    mask = cos_theta > cos_theta_m
    final_target_logit = torch.where(target_logit > threshold, cos_theta_m, target_logit - mm)
    hard_example = cos_theta[mask]
    if training:
        with torch.no_grad():
            t = target_logit.mean() * 0.01 + (1 - 0.01) * t
    cos_theta[mask] = hard_example * (t + hard_example)
    cos_theta.scatter_(1, label.view(-1, 1).long(), final_target_logit)
    return cos_theta * s, t


def _published_inputs():
    g = torch.Generator().manual_seed(41)
    n, classes = 23, 67
    cos = (torch.rand((n, classes), generator=g, dtype=torch.float64) * 1.2 - 0.6)
    label = torch.randint(0, classes, (n,), generator=g)
    label[1] = label[0]
    rows = torch.arange(n)
    cos[rows, label] = torch.linspace(-0.95, 0.93, n, dtype=torch.float64)     # targets on both sides of theta = cos(pi - m) = -0.8776
    return cos, label


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("t0", [0.0, 0.4])
def test_double_is_the_published_forward(t0, training):
    from curricular_double import hard_mask, logits, thresholds, update_t
    cos, label = _published_inputs()
    n = cos.shape[0]
    tcos = cos[torch.arange(n), label]
    assert float(tcos.min()) < math.cos(math.pi - M) < float(tcos.max())              # both target branches
    upstream = torch.randn(cos.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    a = cos.clone().requires_grad_(True)
    want, t_want = _published_forward(a, label, torch.tensor(t0, dtype=torch.float64), S, M, training)
    want.backward(upstream)
    thr = thresholds(tcos, M)
    t1 = update_t(tcos, t0, ALPHA) if training else torch.tensor(t0, dtype=torch.float64)
    hard = hard_mask(cos, label, thr)
    per_row = hard.sum(dim=1)
    assert int((per_row == cos.shape[1] - 1).sum()) and int((per_row == 0).sum()) and int(((per_row > 0) & (per_row < cos.shape[1] - 1)).sum())
    b = cos.clone().requires_grad_(True)
    got, slope = logits(b, label, thr, t1, S, M)
    got.backward(upstream)
    assert float(t1) == pytest.approx(float(t_want), rel=1e-15, abs=0) and (float(t1) != t0) == training
    np.testing.assert_allclose(got.detach().numpy(), want.detach().numpy(), rtol=1e-14, atol=1e-13)
    np.testing.assert_allclose(b.grad.numpy(), a.grad.numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose((slope * upstream).numpy(), a.grad.numpy(), rtol=1e-12, atol=1e-12)     # the kernels' slope formula


def test_double_thresholds_unowned_rows_and_clamp():
    from curricular_double import logits, merged, thresholds, update_t
    nan = float("nan")
    tcos = torch.tensor([[0.5, -2.0, -2.0, nan, 1.0, -2.0, 1.5], [-2.0, -1.0, -2.0, -2.0, -2.0, nan, -2.0]])
    c, owned = merged(tcos)
    assert c.tolist() == [0.5, -1.0, -1.0, -1.0, 1.0, -1.0, 1.0] and owned.tolist() == [True, True, False, False, True, False, True]
    thr = thresholds(tcos, M)
    assert thr[2] == 2.0 and thr[3] == 2.0 and thr[5] == 2.0
    assert float(thr[1]) == pytest.approx(-math.cos(M)) and float(thr[4]) == pytest.approx(math.cos(M)) and float(thr[6]) == float(thr[4])
    assert float(thr[0]) == pytest.approx(math.cos(math.acos(0.5) + M))
    assert float(update_t(tcos, 0.25, ALPHA)) == pytest.approx(ALPHA * (0.5 - 1.0 + 1.0 + 1.0) / 4 + (1 - ALPHA) * 0.25)
    assert float(update_t(torch.full((2, 3), -2.0), 0.25, ALPHA)) == 0.25              # nobody owns a row: unchanged
    # a tie is not hard; the clamp has gradient 0 and the clamped value is what is compared; a label -1 row has no exempt column
    cos = torch.tensor([[0.25, 0.5, 1.5, -1.5], [0.25, 0.5, 0.75, 0.0]], dtype=torch.float64, requires_grad=True)
    z, slope = logits(cos, torch.tensor([3, -1]), torch.tensor([0.25, 0.5]), 0.5, 2.0, M)
    assert z[0, :3].tolist() == [2 * 0.25, 2 * 0.5 * (0.5 + 0.5), 2 * 1.0 * (0.5 + 1.0)] and slope[0, :3].tolist() == [2.0, 2 * 1.5, 0.0]
    assert float(z[0, 3].detach()) == pytest.approx(2 * (-1.0 - math.sin(math.pi - M) * M)) and float(slope[0, 3]) == 0.0
    assert z[1].tolist() == [0.5, 1.0, 2 * 0.75 * 1.25, 0.0] and slope[1].tolist() == [2.0, 2.0, 2 * 2.0, 2.0]
    z.sum().backward()
    assert torch.equal(cos.grad, slope)


# ------------------------------------------------------------------------------------------------ descriptor, module, ABI
def test_margin_descriptor_and_module_surface():
    from nets.ArcFace import SUPPORTED, CurricularFace, CurricularMargin, CurrRows, is_plain_arcface, margin_of
    mod = CurricularFace(48.0, 0.35, alpha=0.05)
    assert margin_of(mod) == CurricularMargin(48.0, 0.35, 0.05)
    assert margin_of(CurricularFace()) == CurricularMargin(64.0, 0.5, 0.01)
    assert (mod.scale, mod.margin) == (48.0, 0.35) and not is_plain_arcface(margin_of(mod))
    assert "CurricularFace" in SUPPORTED and "ElasticFace" in SUPPORTED
    assert not getattr(mod, "needs_norms", False)
    assert set(dict(mod.named_buffers())) == {"t"} and mod.t.dtype == torch.float32 and mod.t.tolist() == [0.0]
    assert "t" in mod.state_dict()                       # checkpointed
    mod.alpha = 0.01                                     # read at call time, like the other modules
    assert margin_of(mod).alpha == 0.01
    assert CurrRows._fields == ("s", "m", "thr", "t")
    with pytest.raises(ValueError, match="alpha"):
        CurricularFace(alpha=1.5)
    with pytest.raises(ValueError, match="m must"):
        CurricularFace(m=4.0)
    # row_thresholds with a kernel double: t advances in training mode only, the record carries the module's own buffer
    from curricular_double import CurricularHeadKernels, thresholds
    tcos = torch.tensor([[0.5, -2.0, 0.25]])
    rows = mod.row_thresholds(tcos, CurricularHeadKernels())
    assert isinstance(rows, CurrRows) and rows.t is mod.t and (rows.s, rows.m) == (48.0, 0.35)
    assert torch.equal(rows.thr, thresholds(tcos, 0.35)) and float(mod.t) == pytest.approx(0.01 * 0.375, rel=1e-6)
    mod.eval()
    mod.row_thresholds(tcos, CurricularHeadKernels())
    assert float(mod.t) == pytest.approx(0.01 * 0.375, rel=1e-6)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    import __graft_entry__ as ge
    ge.build()
    from frhip import _abi, ops
    lib = _abi.lib()
    host = (ctypes.c_float * 8)()                        # never dereferenced: every call below must return before a launch
    p = ctypes.addressof(host)

    def refused(rc, name, *words):
        err = lib.frhip_last_error()
        assert rc == -1 and name in err and all(w in err for w in words), (rc, err)

    who = b"frhip_curricular_rows"
    refused(lib.frhip_curricular_rows(p, 1, 0, 0.5, 0.01, 1, p, p, None), who, b"n=0")
    refused(lib.frhip_curricular_rows(p, 0, 4, 0.5, 0.01, 1, p, p, None), who, b"world_size=0")
    refused(lib.frhip_curricular_rows(None, 1, 4, 0.5, 0.01, 1, p, p, None), who, b"non-null tcos")
    refused(lib.frhip_curricular_rows(p, 1, 4, 0.5, 0.01, 1, None, p, None), who, b"non-null t")
    refused(lib.frhip_curricular_rows(p, 1, 4, 0.5, 0.01, 1, p, None, None), who, b"non-null thr")
    for m in (-0.1, math.pi, 4.0, float("nan")):
        refused(lib.frhip_curricular_rows(p, 1, 4, m, 0.01, 1, p, p, None), who, b"margin m")
    for alpha in (-0.01, 1.01, float("nan")):
        refused(lib.frhip_curricular_rows(p, 1, 4, 0.5, alpha, 1, p, p, None), who, b"alpha")

    good = ops._MarginCurrDesc(64.0, 0.5, p, p)
    bad = [None, ops._MarginCurrDesc(64.0, 0.5, None, p), ops._MarginCurrDesc(64.0, 0.5, p, None), ops._MarginCurrDesc(64.0, -0.1, p, p),
           ops._MarginCurrDesc(64.0, 4.0, p, p), ops._MarginCurrDesc(64.0, float("nan"), p, p)]
    ref = lambda d: None if d is None else ctypes.byref(d)      # noqa: E731
    for desc in bad:
        refused(lib.frhip_head_fwd_curr(1, p, p, p, 4, 10, 64, ref(desc), p, p, p, p, p, None), b"frhip_head_fwd_curr", b"CurricularFace descriptor")
        refused(lib.frhip_head_bwd_dt_curr(1, p, p, p, 4, 10, 64, ref(desc), p, p, 0.25, None, p, 12, None, 0, None),
                b"frhip_head_bwd_dt_curr", b"CurricularFace descriptor")
        refused(lib.frhip_head_fwd_sub_curr(1, p, p, p, 4, 10, 64, 3, ref(desc), p, p, p, p, p, p, None), b"frhip_head_fwd_sub_curr",
                b"CurricularFace descriptor")
        refused(lib.frhip_head_bwd_dt_sub_curr(1, p, p, p, 4, 10, 64, 3, ref(desc), p, p, 0.25, None, p, 36, 12, None, 0, None),
                b"frhip_head_bwd_dt_sub_curr", b"CurricularFace descriptor")
        refused(lib.frhip_margin_fwd_curr(p, p, 4, 10, ref(desc), p, None), b"frhip_margin_fwd_curr", b"null pointer")
        refused(lib.frhip_margin_bwd_curr(p, p, p, 4, 10, ref(desc), p, None), b"frhip_margin_bwd_curr", b"null pointer")
    # a good descriptor does not rescue a bad shape, dtype, pitch or operand
    g = ctypes.byref(good)
    refused(lib.frhip_head_fwd_curr(2, p, p, p, 4, 10, 64, g, p, p, p, p, p, None), b"frhip_head_fwd_curr", b"bad dtype 2")
    refused(lib.frhip_head_fwd_curr(1, p, p, p, 4, 10, 48, g, p, p, p, p, p, None), b"frhip_head_fwd_curr", b"d=48")
    refused(lib.frhip_head_fwd_sub_curr(1, p, p, p, 4, 10, 64, 0, g, p, p, p, p, p, p, None), b"frhip_head_fwd_sub_curr", b"0 sub-centres")
    refused(lib.frhip_head_bwd_dt_curr(1, p, p, p, 4, 10, 64, g, p, p, 0.25, None, p, 10, None, 0, None), b"frhip_head_bwd_dt_curr", b"bad dT pitch 10")
    refused(lib.frhip_head_bwd_dt_sub_curr(1, p, p, p, 4, 10, 64, 3, g, p, p, 0.25, None, p, 24, 12, None, 0, None), b"frhip_head_bwd_dt_sub_curr",
            b"bad dT pitches")
    refused(lib.frhip_margin_fwd_curr(None, p, 4, 10, g, p, None), b"frhip_margin_fwd_curr", b"null pointer")
    refused(lib.frhip_margin_bwd_curr(p, p, p, 4, 10, g, None, None), b"frhip_margin_bwd_curr", b"null pointer")
    with pytest.raises(_abi.FrhipError):
        _abi.check(-1, "frhip_curricular_rows")
    from nets.ArcFace import CurrRows
    with pytest.raises(ValueError, match="curricular_rows: tcos must be a tensor on the GPU"):
        ops.curricular_rows(torch.zeros(1, 4), 0.5, 0.01, torch.zeros(1), True)
    with pytest.raises(ValueError, match="margin_fwd_curr: logits must be a tensor on the GPU"):
        ops.margin_fwd_curr(torch.zeros(4, 10), torch.zeros(4, dtype=torch.int64), CurrRows(64.0, 0.5, torch.zeros(4), torch.zeros(1)))


# ------------------------------------------------------------------------------------------------ PartialFC on gloo with the double
def _inputs():
    from curricular_double import case
    emb, weight, labels, _ = case(2 * B, C, D, 6200, M)
    return emb.double(), weight, labels


def _worker(rank, ws, path, ret, t0):
    for p in (ROOT, os.path.join(ROOT, "face-recognition-pytorch_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="file://" + path, rank=rank, world_size=ws)
    np.savez(os.path.join(ret, "rank%d.npz" % rank), **_run(rank, ws, t0))
    dist.destroy_process_group()


def _run(rank, ws, t0):
    """one rank's part of a two-step run: its rows of the shared batch (2 B rows in all, at either world size)"""
    import nets.PartialFC as P
    from curricular_double import CurricularHeadKernels
    from nets.ArcFace import CurricularFace
    from oracle import head_ref

    class Recording(CurricularHeadKernels):
        def __init__(self):
            self.thr, self.gathered, self.t_used = [], [], []

        def curricular_rows(self, tcos, mg, t, update):
            self.gathered.append(tcos.clone())
            thr = super().curricular_rows(tcos, mg, t, update)
            self.thr.append(thr.clone())
            self.t_used.append(float(t))
            return thr

    emb, weight, labels = _inputs()
    conf = types.SimpleNamespace(emd_size=D, sample_rate=1.0, mixed_precision=False, loss_s=S, loss_m=M)
    kern = Recording()
    pfc = P.PartialFC(conf, C, margin_loss=CurricularFace, kernels=kern)
    assert isinstance(pfc.margin_softmax, CurricularFace) and pfc.margin_softmax.alpha == ALPHA
    start, num = head_ref.shard_range(C, ws, rank)
    with torch.no_grad():
        pfc.weight_activated.data.copy_(weight[start:start + num])
        pfc.margin_softmax.t.fill_(t0)
    rows = 2 * B // ws
    mine = slice(rank * rows, (rank + 1) * rows)
    out = {}
    for st in range(2):
        e = emb[mine].clone().requires_grad_(True)
        loss = pfc(e, labels[mine].clone(), None)
        loss.backward()
        out["loss%d" % st], out["t%d" % st] = float(loss.detach()), pfc.margin_softmax.t.numpy().copy()
        if st == 0:
            out["d_emb"], out["d_w"] = e.grad.numpy(), pfc.weight_activated.grad.numpy().copy()
            pfc.weight_activated.grad = None
            sd = {k: v.clone() for k, v in pfc.state_dict().items()}                   # after step 0
    out["saved_t"] = sd["margin_softmax.t"].numpy()
    # a fresh head from the checkpoint carries t on; one from a checkpoint without it starts at 0 again
    for name, state in (("fresh", sd), ("bare", {"weight": sd["weight"]})):
        fresh = P.PartialFC(conf, C, margin_loss=CurricularFace, kernels=Recording())
        with torch.no_grad():
            fresh.margin_softmax.t.fill_(0.7)
        fresh.load_state_dict(state)
        out[name + "_t"] = fresh.margin_softmax.t.numpy().copy()
    # eval: t is only read, the thresholds are still derived
    pfc.eval()
    calls = len(kern.thr)
    out["eval_loss"] = float(pfc(emb[mine].clone(), labels[mine].clone(), None).detach())
    out["eval_t"], out["eval_calls"] = pfc.margin_softmax.t.numpy().copy(), len(kern.thr) - calls
    out["thr0"], out["gathered"] = kern.thr[0].numpy(), kern.gathered[0].numpy()
    out["t_used"] = np.array(kern.t_used)
    with pytest.raises(ValueError, match="does not take"):
        pfc(emb[mine].clone(), labels[mine].clone(), None, norms=torch.ones(rows))
    return out


def _one_process(t0):
    with tempfile.TemporaryDirectory() as td:
        dist.init_process_group("gloo", init_method="file://" + os.path.join(td, "pg"), rank=0, world_size=1)
        try:
            return _run(0, 1, t0)
        finally:
            dist.destroy_process_group()


@pytest.mark.parametrize("t0", [0.0, 0.4])
def test_same_loss_and_t_at_world_sizes_1_and_2(t0):
    from curricular_double import assert_case, cosines, head_reference, update_t
    from oracle import head_ref
    emb, weight, labels = _inputs()
    n = 2 * B
    tcos, thr, _ = assert_case(cosines(emb, weight), labels, M)
    t1 = np.float32(float(update_t(tcos, t0, ALPHA)))                                  # the buffer is fp32
    t2 = np.float32(float(update_t(tcos, t1, ALPHA)))
    assert t1 != np.float32(t0) and t2 != t1
    ref = head_reference(emb, weight, labels, S, M, thr, float(t1))
    one = _one_process(t0)
    ws = 2
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_worker, args=(ws, os.path.join(td, "pg"), td, t0), nprocs=ws, join=True)
        two = [dict(np.load(os.path.join(td, "rank%d.npz" % r))) for r in range(ws)]
    for r, o in [(0, one)] + list(enumerate(two)):
        world = 1 if o is one else ws
        assert np.array_equal(o["t0"], one["t0"]) and np.array_equal(o["t1"], one["t1"]), (world, r)      # the same t, bit for bit
        np.testing.assert_allclose([o["t0"][0], o["t1"][0]], [t1, t2], rtol=2e-7)         # and the double's, to the buffer's fp32 rounding
        np.testing.assert_allclose(o["thr0"], thr.numpy(), rtol=0, atol=1e-12)
        np.testing.assert_allclose(float(o["loss0"]), float(ref["loss"]), rtol=1e-12)
        np.testing.assert_allclose(float(o["loss0"]), float(one["loss0"]), rtol=1e-12)
        np.testing.assert_allclose(float(o["loss1"]), float(one["loss1"]), rtol=1e-12)
        assert float(o["loss1"]) != float(o["loss0"])                                  # t moved on, the hard negatives weigh more
        rows = n // world
        np.testing.assert_allclose(o["d_emb"], world * ref["d_emb"][r * rows:(r + 1) * rows].numpy(), rtol=1e-9, atol=1e-12)
        start, num = head_ref.shard_range(C, world, r)
        want = ref["d_w"][start:start + num].numpy()
        np.testing.assert_allclose(o["d_w"], want, rtol=1e-6, atol=1e-7 * np.abs(want).max())      # the parameter is fp32
        assert o["saved_t"][0] == o["t0"][0] and o["fresh_t"][0] == o["t0"][0] and o["bare_t"][0] == 0.0
        assert o["eval_t"][0] == o["t1"][0] and int(o["eval_calls"]) == 1              # eval: thresholds derived, t stands still
        assert o["t_used"].tolist() == [float(o["t0"][0]), float(o["t1"][0]), float(o["t1"][0])]
        g = o["gathered"]
        assert g.shape == (world, n)
        np.testing.assert_allclose(g.max(axis=0), tcos.numpy(), rtol=0, atol=1e-12)
        if world == ws:
            assert np.array_equal(g, two[0]["gathered"]) and int((g == -2.0).sum()) == n + 1     # one owner per row; the label -1 row none


def test_adamw_flavour_with_sampling_and_two_subcenters():
    """PartialFCAdamW, sample_rate 0.3, conf.subcenters = 2 on the double's kernels: the thresholds come from the pooled target cosines
    (targets are always among the sampled rows), the loss and the embedding gradient are the double's on the activated rows, and the
    sampled rows carry their Adam state into the optimizer"""
    import nets.PartialFC as P
    from curricular_double import CurricularHeadKernels, head_reference, thresholds, update_t
    from nets.ArcFace import CurricularFace
    from subcenter_double import case
    n, K = 2 * B, 2
    emb, weight, labels, res = case(n, C, D, K, 7300)
    own = torch.nonzero(labels >= 0).flatten()
    tcos = torch.full((n,), -2.0, dtype=torch.float64)
    tcos[own] = res["raw"][own, labels[own]]
    with tempfile.TemporaryDirectory() as td:
        dist.init_process_group("gloo", init_method="file://" + os.path.join(td, "pg"), rank=0, world_size=1)
        try:
            conf = types.SimpleNamespace(emd_size=D, sample_rate=0.3, mixed_precision=False, loss_s=S, loss_m=M, subcenters=K)
            pfc = P.PartialFCAdamW(conf, C, margin_loss=CurricularFace, kernels=CurricularHeadKernels())
            with torch.no_grad():
                pfc.weight.copy_(weight)
            dummy = torch.nn.Parameter(torch.zeros(1))
            opt = torch.optim.AdamW([{"params": [dummy]}, {"params": pfc.parameters()}], lr=1e-2)
            e = emb.double().requires_grad_(True)
            torch.manual_seed(5)
            loss = pfc(e, labels.clone(), opt)
            loss.backward()
            index = pfc.weight_index.clone()
            assert opt.param_groups[-1]["params"][0] is pfc.weight_activated and pfc.weight_activated.grad.shape == (K * index.numel(), D)
            assert opt.state[pfc.weight_activated]["exp_avg"] is pfc.weight_activated_exp_avg
            t_after = pfc.margin_softmax.t.clone()
            tsub = pfc.last_target_sub.clone()
        finally:
            dist.destroy_process_group()
    assert index.numel() == int(0.3 * C) and bool(torch.isin(labels[own], index).all())
    pos = torch.full_like(labels, -1)
    pos[own] = torch.searchsorted(index, labels[own])
    rows = torch.cat([index + k * C for k in range(K)])
    t1 = np.float32(float(update_t(tcos, 0.0, ALPHA)))
    ref = head_reference(emb, weight[rows], pos, S, M, thresholds(tcos, M), float(t1), K=K)
    assert float(t_after) == pytest.approx(float(t1), rel=2e-7)
    np.testing.assert_allclose(float(loss.detach()), float(ref["loss"]), rtol=1e-12)
    np.testing.assert_allclose(e.grad.numpy(), ref["d_emb"].numpy(), rtol=1e-9, atol=1e-12)
    want = torch.full((n,), -1, dtype=torch.int64)
    want[own] = res["win"][own, labels[own]]
    assert torch.equal(tsub.long(), want)
