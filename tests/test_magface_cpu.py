"""MagFace (magnitude-aware margins, a gradient through the norms) without a GPU: the descriptor, the C ABI's refusal of bad arguments,
PartialFC's argument checks and the norm path on one gloo rank, and the distributed host logic -- norms all-gathered in rank order, the
same loss on every rank, every rank's slice of the norm gradient -- on two real gloo ranks, with the float64 kernel double of
tests/magface_double.py."""
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
C, B, D = 150, 37, 64


def test_margin_descriptor_of_magface():
    from nets.ArcFace import MagFace, MagMargin, SUPPORTED, is_plain_arcface, margin_of
    assert margin_of(MagFace()) == MagMargin(64.0, 0.45, 0.8, 10.0, 110.0, 35.0, 1e-3)
    mod = MagFace(48.0, 0.3, u_margin=0.7, l_a=5.0, u_a=90.0, lambda_g=20.0)
    assert margin_of(mod) == MagMargin(48.0, 0.3, 0.7, 5.0, 90.0, 20.0, 1e-3)
    assert not is_plain_arcface(margin_of(mod))
    assert mod.needs_norms is True and mod.norms_need_grad is True and mod.kind == "magface"
    assert (mod.scale, mod.margin) == (48.0, 0.3)
    assert "MagFace" in SUPPORTED and "AdaFace" in SUPPORTED and "CosFace" in SUPPORTED
    assert dict(mod.named_buffers()) == {} and list(mod.parameters()) == []
    mod.u_a, mod.lambda_g = 100.0, 0.0                   # read at call time, like the other modules
    assert margin_of(mod).u_a == 100.0 and margin_of(mod).lambda_g == 0.0


def test_magface_entry_points_refuse_bad_arguments_before_any_launch():
    import __graft_entry__ as ge
    ge.build()
    from frhip import _abi
    lib = _abi.lib()
    host = (ctypes.c_float * 8)()                        # never dereferenced: every call below must return before a launch
    ptr = ctypes.addressof(host)

    def margins(n=8, l_a=10.0, u_a=110.0, ptrs=(ptr,) * 4):
        return lib.frhip_magface_margins(ptrs[0], n, l_a, u_a, 0.45, 0.8, ptrs[1], ptrs[2], ptrs[3], None)

    def norm_grad(n=8, l_a=10.0, u_a=110.0, ptrs=(ptr,) * 5, upstream=ptr):
        return lib.frhip_magface_norm_grad(ptrs[0], ptrs[1], 1, n, ptrs[2], ptrs[3], 64.0, 1e-3, l_a, u_a, 0.45, 0.8, 35.0, 1.0 / 8,
                                           upstream, 1.0, ptrs[4], None)

    for name, fn, nptr in ((b"frhip_magface_margins", margins, 4), (b"frhip_magface_norm_grad", norm_grad, 5)):
        assert fn(n=0) == -1 and name in lib.frhip_last_error() and b"n=0" in lib.frhip_last_error()
        for hole in range(nptr):
            ptrs = [ptr] * nptr
            ptrs[hole] = None
            assert fn(ptrs=ptrs) == -1 and name in lib.frhip_last_error() and b"non-null" in lib.frhip_last_error(), (name, hole)
        for l_a, u_a in ((10.0, 10.0), (110.0, 10.0), (0.0, 110.0), (-1.0, 110.0)):
            assert fn(l_a=l_a, u_a=u_a) == -1 and name in lib.frhip_last_error() and b"l_a" in lib.frhip_last_error(), (name, l_a, u_a)
    with pytest.raises(_abi.FrhipError):
        _abi.check(-1, "frhip_magface_norm_grad")
    # the normalise-backward with the norm gradient: declared, exported, and behind the one dtype guard
    assert lib.frhip_l2norm_bwd_norm(2, None, None, None, None, None, 0, 0, 0.0, None) == -1
    assert lib.frhip_last_error() == b"frhip_l2norm_bwd_norm: bad dtype 2"
    assert lib.frhip_l2norm_bwd_norm(1, ptr, ptr, ptr, None, ptr, 4, 64, 1.0, None) == -1 and b"non-null" in lib.frhip_last_error()
    assert lib.frhip_abi_version() == 1


def test_ops_wrappers_check_their_arguments():
    from frhip import ops
    cpu = torch.ones(4)
    with pytest.raises(ValueError, match="magface_margins: norms must be a tensor on the GPU"):
        ops.magface_margins(cpu, 10.0, 110.0, 0.45, 0.8)
    with pytest.raises(ValueError, match="magface_norm_grad: norms must be a tensor on the GPU"):
        ops.magface_norm_grad(cpu, cpu, cpu, cpu, 64.0, 1e-3, 10.0, 110.0, 0.45, 0.8, 35.0, 0.25)
    with pytest.raises(ValueError, match="l2norm_bwd_norm: dxhat must be a tensor on the GPU"):
        ops.l2norm_bwd_norm(cpu, cpu, cpu, cpu)


def _paths():
    for p in (ROOT, os.path.join(ROOT, "face-recognition-pytorch_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)


def test_partial_fc_with_magface_on_one_rank_carries_the_norm_gradient():
    _paths()
    import nets.PartialFC as P
    from magface_double import LAMBDA_G, L_M, S, MagHeadKernels, assert_branches, branch_case, head_reference, margins
    from nets.ArcFace import ArcFace, MagFace
    emb32, weight, labels = branch_case(B, C, D, 5100)
    assert_branches(emb32, weight, labels)
    loss_ref, d_hat, d_w, d_norm = head_reference(emb32, weight, labels)
    e64 = emb32.double()
    full = d_hat + d_norm[:, None] * e64 / e64.norm(dim=1, keepdim=True)     # with respect to the un-normalised embeddings
    with tempfile.TemporaryDirectory() as td:
        own_pg = not dist.is_initialized()       # in the whole suite an earlier module may have left its one-rank group: use it, leave it
        if own_pg:
            dist.init_process_group("gloo", init_method="file://" + os.path.join(td, "pg"), rank=0, world_size=1)
        try:
            assert dist.get_world_size() == 1
            conf = types.SimpleNamespace(emd_size=D, sample_rate=1.0, mixed_precision=False, loss_s=S, loss_m=L_M)
            kern = MagHeadKernels()
            pfc = P.PartialFC(conf, C, margin_loss=MagFace, kernels=kern)
            assert isinstance(pfc.margin_softmax, MagFace) and pfc.margin_softmax.s == S and pfc.margin_softmax.m == L_M
            with torch.no_grad():
                pfc.weight_activated.data.copy_(weight)
            emb = e64.clone().requires_grad_(True)
            with pytest.raises(ValueError, match="norms"):
                pfc(emb, labels.clone(), None)
            with pytest.raises(ValueError, match="one value per local embedding"):
                pfc(emb, labels.clone(), None, norms=torch.ones(3))
            plain = P.PartialFC(conf, C, margin_loss=ArcFace, kernels=kern)
            with pytest.raises(ValueError, match="does not take"):
                plain(emb, labels.clone(), None, norms=torch.ones(B))
            # differentiable norms: the loss is the double's, emb.grad carries the tangential part AND the norm path
            loss = pfc(emb, labels.clone(), None, norms=emb.norm(dim=1))
            loss.backward()
            loss = loss.detach()
            np.testing.assert_allclose(float(loss), float(loss_ref), rtol=1e-12)
            np.testing.assert_allclose(emb.grad.numpy(), full.numpy(), rtol=1e-9, atol=1e-12)
            ref_w = d_w.numpy()
            np.testing.assert_allclose(pfc.weight_activated.grad.numpy(), ref_w, rtol=1e-6, atol=1e-7 * np.abs(ref_w).max())
            # detached norms: the same value (the regulariser is in it), the tangential gradient alone
            pfc.weight_activated.grad = None
            emb2 = e64.clone().requires_grad_(True)
            loss2 = pfc(emb2, labels.clone(), None, norms=emb2.detach().norm(dim=1))
            loss2.backward()
            assert float(loss2.detach()) == float(loss)
            _, _, reg = margins(e64.norm(dim=1))
            assert float(LAMBDA_G * reg) > 1.0                                # the regulariser is no rounding matter in that value
            np.testing.assert_allclose(emb2.grad.numpy(), d_hat.numpy(), rtol=1e-9, atol=1e-12)
            assert float((emb.grad - emb2.grad).abs().max()) > 1e-3 * float(emb2.grad.abs().max())
        finally:
            if own_pg:
                dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------ two real ranks on gloo
def _inputs():
    _paths()
    from magface_double import branch_case
    emb, weight, labels = branch_case(2 * B, C, D, 5200)
    return emb, weight, labels


def _worker(rank, ws, path, ret):
    _paths()
    import nets.PartialFC as P
    from magface_double import L_M, S, MagHeadKernels
    from nets.ArcFace import MagFace
    from oracle import head_ref

    class Recording(MagHeadKernels):
        seen = []

        def magface_margins(self, norms, mg):
            self.seen.append(norms.clone())
            return super().magface_margins(norms, mg)

    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="file://" + path, rank=rank, world_size=ws)
    emb, weight, labels = _inputs()
    conf = types.SimpleNamespace(emd_size=D, sample_rate=1.0, mixed_precision=False, loss_s=S, loss_m=L_M)
    kern = Recording()
    pfc = P.PartialFC(conf, C, margin_loss=MagFace, kernels=kern)
    start, num = head_ref.shard_range(C, ws, rank)
    with torch.no_grad():
        pfc.weight_activated.data.copy_(weight[start:start + num])
    mine = slice(rank * B, (rank + 1) * B)
    e = emb[mine].double().clone().requires_grad_(True)
    norms = emb[mine].double().norm(dim=1).requires_grad_(True)              # a leaf of its own: its .grad is the head's norm gradient
    loss = pfc(e, labels[mine].clone(), None, norms=norms)
    loss.backward()
    np.savez(os.path.join(ret, "rank%d.npz" % rank), loss=float(loss.detach()), d_emb=e.grad.numpy(), d_norm=norms.grad.numpy(),
             d_w=pfc.weight_activated.grad.numpy(), calls=len(kern.seen), gathered=kern.seen[0].numpy())
    dist.destroy_process_group()


def test_two_gloo_ranks_gather_norms_in_rank_order_and_agree_with_one_process():
    _paths()
    from magface_double import assert_branches, head_reference
    from oracle import head_ref
    ws = 2
    emb, weight, labels = _inputs()
    assert_branches(emb, weight, labels)
    loss, d_emb, d_w, d_norm = head_reference(emb, weight, labels)           # the ONE-process evaluation of the double
    assert float(d_norm.abs().max()) > 0
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_worker, args=(ws, os.path.join(td, "pg"), td), nprocs=ws, join=True)
        out = [dict(np.load(os.path.join(td, "rank%d.npz" % r))) for r in range(ws)]
    for r in range(ws):
        o = out[r]
        assert int(o["calls"]) == 1                                                   # once per forward
        assert np.array_equal(o["gathered"], emb.double().norm(dim=1).numpy())        # rank order, every rank
        assert float(o["loss"]) == float(out[0]["loss"])
        np.testing.assert_allclose(float(o["loss"]), float(loss), rtol=1e-12)
        # both gradients come back x world_size (the reference's AllGatherFunc, nets/PartialFC.py:504-522)
        np.testing.assert_allclose(o["d_norm"], ws * d_norm[r * B:(r + 1) * B].numpy(), rtol=1e-9, atol=1e-15)
        np.testing.assert_allclose(o["d_emb"], ws * d_emb[r * B:(r + 1) * B].numpy(), rtol=1e-9, atol=1e-12)
        start, num = head_ref.shard_range(C, ws, r)
        ref = d_w[start:start + num].numpy()
        np.testing.assert_allclose(o["d_w"], ref, rtol=1e-6, atol=1e-7 * np.abs(ref).max())      # the parameter is fp32
