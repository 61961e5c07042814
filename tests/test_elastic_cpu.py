"""ElasticFace (random per-row margins, ranked for the "+" variants) without a GPU: the generator's known answers and statistics, the
descriptor, the C ABI's refusal of bad arguments, and the distributed host logic on real gloo ranks with the float64 kernel double of
tests/elastic_double.py -- the same margins and the same loss at world sizes 1 and 2, the step counter, eval mode, checkpoints."""
import ctypes
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
S = 64.0
C, B, D = 150, 37, 64
SEED = 77


# ------------------------------------------------------------------------------------------------ the generator
def test_philox_known_answers():
    from elastic_double import philox4x32_10
    kats = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
            ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
            ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"))
    for counter, key, want in kats:
        assert " ".join("%08x" % int(x) for x in philox4x32_10(counter, key)) == want


def test_sample_margins_prefix_property_and_statistics():
    from elastic_double import draws, normals
    got = draws(4, 0.5, 0.05, 0, 0).numpy()
    assert got.dtype == np.float32
    assert np.array_equal(got, np.array([0.5495569, 0.4923181, 0.4406821, 0.47022966], dtype=np.float32))
    # a draw depends on (seed, step, row) alone, not on n
    assert torch.equal(draws(1000, 0.5, 0.05, 5, 3)[:37], draws(37, 0.5, 0.05, 5, 3))
    assert not torch.equal(draws(37, 0.5, 0.05, 5, 3), draws(37, 0.5, 0.05, 5, 4))
    assert not torch.equal(draws(37, 0.5, 0.05, 5, 3), draws(37, 0.5, 0.05, 6, 3))
    assert not torch.equal(draws(37, 0.5, 0.05, 5, 3), draws(37, 0.5, 0.05, 5, 3 + 2 ** 32))       # the step's high word counts
    assert not torch.equal(draws(37, 0.5, 0.05, 5, 3), draws(37, 0.5, 0.05, 5 + 2 ** 32, 3))       # and the seed's
    n = 4096
    z = normals(n, 1234, 1)
    print("seed 1234 step 1: mean %.4f std %.4f" % (z.mean(), z.std()))
    assert abs(z.mean()) < 4 / math.sqrt(n) and abs(z.std() - 1) < 0.05
    assert torch.equal(draws(5, 0.35, 0.05, 0, 0, update=False), torch.full((5,), float(np.float32(0.35))))


def test_ranking_gives_the_largest_cosine_the_smallest_margin():
    from elastic_double import assign, ranks
    tcos = torch.tensor([[0.25, -2.0, 0.25, -2.0, 0.75], [-2.0, 0.125, -2.0, -2.0, -2.0]])
    g = torch.tensor([0.5, 0.125, 0.375, 0.25, 0.3125])
    c, r = ranks(tcos)
    assert c.tolist() == [0.25, 0.125, 0.25, -2.0, 0.75] and r.tolist() == [1, 3, 2, 4, 0]   # equal cosines in row order, unowned last
    assert assign(tcos, g).tolist() == [0.25, 0.375, 0.3125, 0.5, 0.125]


# ------------------------------------------------------------------------------------------------ descriptor, module, ABI
def test_margin_descriptor_and_module_surface():
    from nets.ArcFace import SUPPORTED, ElasticFace, ElasticMargin, is_plain_arcface, margin_of
    mod = ElasticFace(48.0, 0.35, std=0.025, kind="cos", plus=True, seed=9)
    assert margin_of(mod) == ElasticMargin(48.0, 0.35, 0.025, "cos", True, 9, 1e-3)
    assert margin_of(ElasticFace()) == ElasticMargin(64.0, 0.5, 0.05, "arc", False, 0, 1e-3)
    assert (mod.scale, mod.margin) == (48.0, 0.35) and not is_plain_arcface(margin_of(mod))
    assert "ElasticFace" in SUPPORTED and "MagFace" in SUPPORTED
    assert not getattr(mod, "needs_norms", False)
    assert set(dict(mod.named_buffers())) == {"step"} and mod.step.dtype == torch.int64 and mod.step.tolist() == [0]
    assert "step" in mod.state_dict()                    # checkpointed
    mod.std = 0.05                                       # read at call time, like the other modules
    assert margin_of(mod).std == 0.05
    with pytest.raises(ValueError, match="kind"):
        ElasticFace(kind="sphere")
    with pytest.raises(ValueError, match="std"):
        ElasticFace(std=-0.1)
    via_partial = functools.partial(ElasticFace, std=0.0175, plus=True)(64.0, 0.5)
    assert margin_of(via_partial) == ElasticMargin(64.0, 0.5, 0.0175, "arc", True, 0, 1e-3)


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

    refused(lib.frhip_elastic_margins(0, 0, 0.5, 0.05, 0, p, 1, p, p, None), b"frhip_elastic_margins", b"n=0")
    refused(lib.frhip_elastic_margins(8, 0, 0.5, -0.05, 0, p, 1, p, p, None), b"frhip_elastic_margins", b"std")
    refused(lib.frhip_elastic_margins(8, 0, 0.5, float("nan"), 0, p, 1, p, p, None), b"frhip_elastic_margins", b"std")
    refused(lib.frhip_elastic_margins(8, 2, 0.5, 0.05, 0, p, 1, p, p, None), b"frhip_elastic_margins", b"kind 2")
    for hole in range(3):
        a = [p] * 3
        a[hole] = None
        refused(lib.frhip_elastic_margins(8, 0, 0.5, 0.05, 0, a[0], 1, a[1], a[2], None), b"frhip_elastic_margins", b"non-null")
    refused(lib.frhip_elastic_draws(8, 0.5, 0.05, 0, None, 1, p, None), b"frhip_elastic_draws", b"non-null")
    refused(lib.frhip_elastic_draws(8, 0.5, 0.05, 0, p, 1, None, None), b"frhip_elastic_draws", b"non-null")
    refused(lib.frhip_head_target_cos(1, p, p, p, 4, 10, 48, 1, p, None), b"frhip_head_target_cos", b"d=48")
    refused(lib.frhip_head_target_cos(0, p, p, p, 4, 10, 64, 0, p, None), b"frhip_head_target_cos", b"subcenters=0")
    refused(lib.frhip_head_target_cos(0, p, p, None, 4, 10, 64, 1, p, None), b"frhip_head_target_cos", b"non-null")
    assert lib.frhip_elastic_assign_workspace(0) == 0 and lib.frhip_elastic_assign_workspace(65537) == 0
    assert lib.frhip_elastic_assign_workspace(1) == 8 and lib.frhip_elastic_assign_workspace(65536) == 8 * 65536
    refused(lib.frhip_elastic_assign(p, 1, 0, p, 0, p, p, p, 64, None), b"frhip_elastic_assign", b"n=0")
    refused(lib.frhip_elastic_assign(p, 1, 65537, p, 0, p, p, p, 1 << 20, None), b"frhip_elastic_assign", b"n=65537")
    refused(lib.frhip_elastic_assign(p, 0, 4, p, 0, p, p, p, 64, None), b"frhip_elastic_assign", b"world_size")
    refused(lib.frhip_elastic_assign(p, 1, 4, p, 3, p, p, p, 64, None), b"frhip_elastic_assign", b"kind")
    refused(lib.frhip_elastic_assign(p, 1, 4, p, 0, p, p, p, 31, None), b"frhip_elastic_assign", b"workspace")
    refused(lib.frhip_elastic_assign(p, 1, 4, p, 0, p, p, None, 64, None), b"frhip_elastic_assign", b"workspace")
    refused(lib.frhip_elastic_assign(None, 1, 4, p, 0, p, p, p, 64, None), b"frhip_elastic_assign", b"non-null")
    with pytest.raises(_abi.FrhipError):
        _abi.check(-1, "frhip_elastic_assign")
    cpu = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError, match="elastic_margins: step must be a tensor on the GPU"):
        ops.elastic_margins(4, "arc", 0.5, 0.05, 0, cpu, True)
    with pytest.raises(ValueError, match="head_target_cos: ehat must be a tensor on the GPU"):
        ops.head_target_cos(torch.zeros(4, 64), torch.zeros(8, 64), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="elastic_assign: tcos must be a tensor on the GPU"):
        ops.elastic_assign(torch.zeros(1, 4), torch.zeros(4), "arc")


# ------------------------------------------------------------------------------------------------ PartialFC on gloo with the double
def _inputs():
    from elastic_double import case
    emb, weight, labels = case(2 * B, C, D, 5200)
    return emb.double(), weight, labels


def _margin(plus):
    from nets.ArcFace import ElasticFace
    m, std = (0.5, 0.0175) if plus else (0.5, 0.05)
    return functools.partial(ElasticFace, std=std, kind="arc", plus=plus, seed=SEED), m, std


def _worker(rank, ws, path, ret, plus):
    for p in (ROOT, os.path.join(ROOT, "face-recognition-pytorch_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="file://" + path, rank=rank, world_size=ws)
    np.savez(os.path.join(ret, "rank%d.npz" % rank), **_run(rank, ws, plus))
    dist.destroy_process_group()


def _run(rank, ws, plus):
    """one rank's part of a two-step run: its rows of the shared batch (2 B rows in all, at either world size)"""
    import nets.PartialFC as P
    from elastic_double import ElasticHeadKernels
    from oracle import head_ref

    class Recording(ElasticHeadKernels):
        def __init__(self):
            self.margins, self.gathered = [], []

        def forward_stats(self, ehat, what, labels_i32, s, m, margin=None):
            self.margins.append(torch.stack([margin.m_ang.float(), margin.m_add.float()]).clone())
            return super().forward_stats(ehat, what, labels_i32, s, m, margin=margin)

        def elastic_assign(self, tcos, g, mg):
            self.gathered.append(tcos.clone())
            return super().elastic_assign(tcos, g, mg)

    factory, m, std = _margin(plus)
    emb, weight, labels = _inputs()
    conf = types.SimpleNamespace(emd_size=D, sample_rate=1.0, mixed_precision=False, loss_s=S, loss_m=m)
    kern = Recording()
    pfc = P.PartialFC(conf, C, margin_loss=factory, kernels=kern)
    start, num = head_ref.shard_range(C, ws, rank)
    with torch.no_grad():
        pfc.weight_activated.data.copy_(weight[start:start + num])
    rows = 2 * B // ws
    mine = slice(rank * rows, (rank + 1) * rows)
    out = {}
    for st in range(2):
        e = emb[mine].clone().requires_grad_(True)
        loss = pfc(e, labels[mine].clone(), None)
        loss.backward()
        out["loss%d" % st], out["step%d" % st] = float(loss.detach()), int(pfc.margin_softmax.step)
        if st == 0:
            out["d_emb"], out["d_w"] = e.grad.numpy(), pfc.weight_activated.grad.numpy().copy()
            pfc.weight_activated.grad = None
            sd = {k: v.clone() for k, v in pfc.state_dict().items()}                   # after step 0: the counter stands at 1
    out["saved_step"] = int(sd["margin_softmax.step"])
    # a fresh head from the checkpoint repeats step 1's margins; one from a checkpoint without the counter starts at 0 again
    for name, state in (("fresh", sd), ("bare", {"weight": sd["weight"]})):
        k2 = Recording()
        fresh = P.PartialFC(conf, C, margin_loss=factory, kernels=k2)
        fresh.load_state_dict(state)
        out[name + "_step"] = int(fresh.margin_softmax.step)
        fresh(emb[mine].clone(), labels[mine].clone(), None)
        out[name + "_margins"] = k2.margins[0].numpy()
    # eval: every margin is m, the counter stands still, nothing is ranked
    pfc.eval()
    calls = len(kern.gathered)
    pfc(emb[mine].clone(), labels[mine].clone(), None)
    out["eval_margins"], out["eval_step"], out["eval_ranked"] = kern.margins[2].numpy(), int(pfc.margin_softmax.step), len(kern.gathered) - calls
    out["margins0"], out["margins1"] = kern.margins[0].numpy(), kern.margins[1].numpy()
    out["gathered"] = kern.gathered[0].numpy() if kern.gathered else np.zeros(0)
    with pytest.raises(ValueError, match="does not take"):
        pfc(emb[mine].clone(), labels[mine].clone(), None, norms=torch.ones(rows))
    return out


def _one_process(plus):
    with tempfile.TemporaryDirectory() as td:
        dist.init_process_group("gloo", init_method="file://" + os.path.join(td, "pg"), rank=0, world_size=1)
        try:
            return _run(0, 1, plus)
        finally:
            dist.destroy_process_group()


@pytest.mark.parametrize("plus", [False, True], ids=["arc", "arc_plus"])
def test_same_margins_and_loss_at_world_sizes_1_and_2(plus):
    from elastic_double import assert_case, row_margins
    from adaface_double import head_reference
    from oracle import head_ref
    _, m, std = _margin(plus)
    emb, weight, labels = _inputs()
    n = 2 * B
    tcos = assert_case(emb, weight, labels, m, std, "arc")
    want = [torch.stack(row_margins(n, m, std, "arc", plus, SEED, st, tcos)) for st in range(2)]
    assert float((want[0][0] - m).abs().max()) < 5 * std and not torch.equal(want[0], want[1])
    loss, d_emb, d_w = head_reference(emb, weight, labels, S, want[0][0], want[0][1])
    one = _one_process(plus)
    ws = 2
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_worker, args=(ws, os.path.join(td, "pg"), td, plus), nprocs=ws, join=True)
        two = [dict(np.load(os.path.join(td, "rank%d.npz" % r))) for r in range(ws)]
    for r, o in [(0, one)] + list(enumerate(two)):
        world = 1 if o is one else ws
        for st in range(2):
            assert np.array_equal(o["margins%d" % st], want[st].numpy()), (world, r, st)         # the same margins at both world sizes
            assert int(o["step%d" % st]) == st + 1                                               # one per training call
        np.testing.assert_allclose(float(o["loss0"]), float(loss), rtol=1e-12)
        np.testing.assert_allclose(float(o["loss0"]), float(one["loss0"]), rtol=1e-12)
        np.testing.assert_allclose(float(o["loss1"]), float(one["loss1"]), rtol=1e-12)
        assert float(o["loss1"]) != float(o["loss0"])
        rows = n // world
        np.testing.assert_allclose(o["d_emb"], world * d_emb[r * rows:(r + 1) * rows].numpy(), rtol=1e-9, atol=1e-12)
        start, num = head_ref.shard_range(C, world, r)
        ref = d_w[start:start + num].numpy()
        np.testing.assert_allclose(o["d_w"], ref, rtol=1e-6, atol=1e-7 * np.abs(ref).max())      # the parameter is fp32
        assert int(o["saved_step"]) == 1 and int(o["fresh_step"]) == 1 and int(o["bare_step"]) == 0
        assert np.array_equal(o["fresh_margins"], want[1].numpy()) and np.array_equal(o["bare_margins"], want[0].numpy())
        assert int(o["eval_step"]) == 2 and int(o["eval_ranked"]) == 0
        assert np.array_equal(o["eval_margins"], np.stack([np.full(n, np.float32(m)), np.zeros(n, np.float32)]))
        if plus:
            # every rank ranked the cosines of ALL ranks: [world, n], -2 where the shard does not own the row, their maximum the batch's
            g = o["gathered"]
            assert g.shape == (world, n) and np.array_equal(g, two[0]["gathered"] if world == ws else g)
            np.testing.assert_allclose(g.max(axis=0), tcos.numpy(), rtol=0, atol=1e-12)
            if world == ws:
                assert int((g == -2.0).sum()) == n + 1          # each row is owned by one shard; the label -1 row by none
