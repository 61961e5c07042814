"""AdaFace (per-row adaptive margins) without a GPU: the descriptor, PartialFC's argument checks, the C ABI's refusal of bad arguments,
and the distributed host logic -- norms all-gathered in rank order, identical running statistics on every rank -- on two real gloo
ranks with the float64 kernel double of tests/adaface_double.py."""
import ctypes
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
S, M, H, T_ALPHA = 64.0, 0.4, 0.333, 0.01
C, B, D = 150, 37, 64


def test_margin_descriptor_of_adaface():
    from nets.ArcFace import AdaFace, AdaMargin, SUPPORTED, is_plain_arcface, margin_of
    mod = AdaFace(48.0, 0.3, h=0.25, t_alpha=0.05)
    assert margin_of(mod) == AdaMargin(48.0, 0.3, 0.25, 0.05, 1e-3)
    assert margin_of(AdaFace()) == AdaMargin(64.0, 0.4, 0.333, 0.01, 1e-3)
    assert not is_plain_arcface(margin_of(mod))
    assert mod.needs_norms is True and "AdaFace" in SUPPORTED and "CosFace" in SUPPORTED
    assert float(mod.batch_mean) == 20.0 and float(mod.batch_std) == 100.0
    assert set(dict(mod.named_buffers())) == {"batch_mean", "batch_std"}
    mod.m = 0.5                                          # read at call time, like the other modules
    assert margin_of(mod).m == 0.5


def test_partial_fc_builds_with_adaface_and_checks_norms():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nets.PartialFC as P
    from adaface_double import AdaHeadKernels
    from nets.ArcFace import AdaFace, ArcFace
    with tempfile.TemporaryDirectory() as td:
        dist.init_process_group("gloo", init_method="file://" + os.path.join(td, "pg"), rank=0, world_size=1)
        try:
            conf = types.SimpleNamespace(emd_size=D, sample_rate=1.0, mixed_precision=False, loss_s=S, loss_m=M)
            pfc = P.PartialFC(conf, 50, margin_loss=AdaFace, kernels=AdaHeadKernels())
            assert isinstance(pfc.margin_softmax, AdaFace) and pfc.margin_softmax.s == S and pfc.margin_softmax.m == M
            emb, lab = torch.randn(4, D, requires_grad=True), torch.tensor([1, 2, 3, 4])
            with pytest.raises(ValueError, match="norms"):
                pfc(emb, lab.clone(), None)
            with pytest.raises(ValueError, match="one value per local embedding"):
                pfc(emb, lab.clone(), None, norms=torch.ones(3))
            loss = pfc(emb, lab.clone(), None, norms=emb.detach().norm(dim=1))
            loss.backward()
            assert torch.isfinite(loss) and emb.grad is not None and pfc.weight_activated.grad is not None
            assert float(pfc.margin_softmax.batch_mean) != 20.0              # training mode: the statistics moved
            plain = P.PartialFC(conf, 50, margin_loss=ArcFace, kernels=AdaHeadKernels())
            with pytest.raises(ValueError, match="does not take"):
                plain(emb, lab.clone(), None, norms=torch.ones(4))
            # eval mode reads the buffers and leaves them alone
            before = (float(pfc.margin_softmax.batch_mean), float(pfc.margin_softmax.batch_std))
            pfc.eval()
            pfc(emb, lab.clone(), None, norms=emb.detach().norm(dim=1))
            assert (float(pfc.margin_softmax.batch_mean), float(pfc.margin_softmax.batch_std)) == before
            # a checkpoint without the statistics loads as the initial values; one with them restores them
            sd = {k: v.clone() for k, v in pfc.state_dict().items()}         # state_dict() hands out the live buffers
            assert float(sd["margin_softmax.batch_mean"]) == before[0] and float(sd["margin_softmax.batch_std"]) == before[1]
            pfc.load_state_dict({"weight": sd["weight"]})
            assert (float(pfc.margin_softmax.batch_mean), float(pfc.margin_softmax.batch_std)) == (20.0, 100.0)
            pfc.load_state_dict(sd)
            assert (float(pfc.margin_softmax.batch_mean), float(pfc.margin_softmax.batch_std)) == before
        finally:
            dist.destroy_process_group()


def test_adaface_margins_refuses_bad_arguments_before_any_launch():
    import __graft_entry__ as ge
    ge.build()
    from frhip import _abi
    lib = _abi.lib()
    host = (ctypes.c_float * 8)()                        # never dereferenced: every call below must return before a launch
    ptr = ctypes.addressof(host)
    rc = lib.frhip_adaface_margins(ptr, 1, M, H, T_ALPHA, 1e-3, 1, ptr, ptr, ptr, ptr, None)
    assert rc == -1 and b"frhip_adaface_margins" in lib.frhip_last_error() and b"n=1" in lib.frhip_last_error()
    for hole in range(5):
        args = [ptr] * 5
        args[hole] = None
        rc = lib.frhip_adaface_margins(args[0], 8, M, H, T_ALPHA, 1e-3, 1, args[1], args[2], args[3], args[4], None)
        assert rc == -1 and b"non-null" in lib.frhip_last_error(), hole
    with pytest.raises(_abi.FrhipError):
        _abi.check(rc, "frhip_adaface_margins")


# ------------------------------------------------------------------------------------------------ two real ranks on gloo
def _inputs():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from adaface_double import branch_case
    emb, weight, labels = branch_case(2 * B, C, D, 4100)
    return emb.double(), weight, labels, emb.norm(dim=1)


def _worker(rank, ws, path, ret):
    for p in (ROOT, os.path.join(ROOT, "face-recognition-pytorch_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import nets.PartialFC as P
    from adaface_double import BUFFERS, AdaHeadKernels
    from nets.ArcFace import AdaFace
    from oracle import head_ref

    class Recording(AdaHeadKernels):
        seen = []

        def adaface_margins(self, norms, *a):
            self.seen.append(norms.clone())
            return super().adaface_margins(norms, *a)

    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="file://" + path, rank=rank, world_size=ws)
    emb, weight, labels, norms = _inputs()
    conf = types.SimpleNamespace(emd_size=D, sample_rate=1.0, mixed_precision=False, loss_s=S, loss_m=M)
    kern = Recording()
    pfc = P.PartialFC(conf, C, margin_loss=lambda s, m: AdaFace(s, m, H, T_ALPHA), kernels=kern)
    start, num = head_ref.shard_range(C, ws, rank)
    with torch.no_grad():
        pfc.weight_activated.data.copy_(weight[start:start + num])
        pfc.margin_softmax.batch_mean.fill_(BUFFERS[0])
        pfc.margin_softmax.batch_std.fill_(BUFFERS[1])
    mine = slice(rank * B, (rank + 1) * B)
    e = emb[mine].clone().requires_grad_(True)
    loss = pfc(e, labels[mine].clone(), None, norms=norms[mine].clone())
    loss.backward()
    sd = pfc.state_dict()
    fresh = P.PartialFC(conf, C, margin_loss=AdaFace, kernels=kern)
    fresh.load_state_dict(sd)
    np.savez(os.path.join(ret, "rank%d.npz" % rank), loss=float(loss.detach()), d_emb=e.grad.numpy(), d_w=pfc.weight_activated.grad.numpy(),
             calls=len(kern.seen), gathered=kern.seen[0].numpy(), mean=pfc.margin_softmax.batch_mean.numpy(),
             std=pfc.margin_softmax.batch_std.numpy(), sd_mean=sd["margin_softmax.batch_mean"].numpy(),
             sd_std=sd["margin_softmax.batch_std"].numpy(), fresh_mean=fresh.margin_softmax.batch_mean.numpy(),
             fresh_std=fresh.margin_softmax.batch_std.numpy(), fresh_w=fresh.weight_activated.data.numpy())
    dist.destroy_process_group()


def test_two_gloo_ranks_gather_norms_in_rank_order_and_agree_with_one_process():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from adaface_double import BUFFERS, assert_branches, head_reference
    from oracle import head_ref
    ws = 2
    emb, weight, labels, norms = _inputs()
    mr = assert_branches(emb, weight, labels, norms, S, M, H, T_ALPHA)                # the ONE-process evaluation of the double
    loss, d_emb, d_w = head_reference(emb, weight, labels, S, mr["m_ang"], mr["m_add"])
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_worker, args=(ws, os.path.join(td, "pg"), td), nprocs=ws, join=True)
        out = [dict(np.load(os.path.join(td, "rank%d.npz" % r))) for r in range(ws)]
    for r in range(ws):
        o = out[r]
        assert int(o["calls"]) == 1                                                   # once per forward
        assert np.array_equal(o["gathered"], norms.numpy())                           # rank order, every rank
        # the buffers are fp32: the double's float64 update, rounded once
        assert o["mean"] == np.float32(float(mr["batch_mean"])) and o["std"] == np.float32(float(mr["batch_std"]))
        assert float(o["mean"][0]) != BUFFERS[0] and float(o["std"][0]) != BUFFERS[1]
        assert o["mean"] == out[0]["mean"] and o["std"] == out[0]["std"] and float(o["loss"]) == float(out[0]["loss"])
        np.testing.assert_allclose(float(o["loss"]), float(loss), rtol=1e-12)
        # the embedding gradient comes back x world_size (the reference's AllGatherFunc, nets/PartialFC.py:504-522)
        np.testing.assert_allclose(o["d_emb"], ws * d_emb[r * B:(r + 1) * B].numpy(), rtol=1e-9, atol=1e-12)
        start, num = head_ref.shard_range(C, ws, r)
        ref = d_w[start:start + num].numpy()
        np.testing.assert_allclose(o["d_w"], ref, rtol=1e-6, atol=1e-7 * np.abs(ref).max())      # the parameter is fp32
        assert np.array_equal(o["sd_mean"], o["mean"]) and np.array_equal(o["sd_std"], o["std"])
        assert np.array_equal(o["fresh_mean"], o["mean"]) and np.array_equal(o["fresh_std"], o["std"])
        assert np.array_equal(o["fresh_w"], weight[start:start + num].numpy())
