"""UniFace (the sigmoid / binary cross-entropy head with one learnable threshold) without a GPU: the float64 double of
tests/uniface_double.py against torch autograd of the same expression, the module and descriptor surface, the C ABI's refusal of bad
arguments before any launch, the distributed host logic on real gloo ranks with the double's kernels -- the same loss and the same
bias gradient at world sizes 1 and 2, checkpoints -- and the optimizer groups model.FR_PartialFC.Model builds."""
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
S, M = 64.0, 0.4
C, B, D = 150, 37, 64


def _mg(kind, m_neg=0.0, w_pos=1.0, w_neg=1.0):
    from uniface_double import KINDS
    return (KINDS[kind], S, M, m_neg, w_pos, w_neg)


# ------------------------------------------------------------------------------------------------ the double against autograd
@pytest.mark.parametrize("m_neg", [0.0, 0.2])
@pytest.mark.parametrize("bias", [0.0, math.log(10 * C)])
@pytest.mark.parametrize("kind", ["arc", "cos"])
def test_double_equals_float64_autograd(kind, bias, m_neg):
    """the rule written out (value, d/dcos, d/db) against torch autograd of the same expression: loss, d_emb, d_w, dbias to 1e-10,
    with unequal weights, on inputs where no branch is decided by rounding (asserted)"""
    from uniface_double import ARC, T_LOW, assert_case, case, cosines, head_reference
    emb, weight, labels = case(2 * B, C, D, 8100)
    raw = cosines(emb, weight)
    mg = _mg(kind, m_neg, 0.7, 1.3)
    assert_case(raw, labels, mg[0], M)
    own = torch.nonzero(labels >= 0).flatten()
    tc = raw[own, labels[own]]
    assert float(tc.min()) < math.cos(math.pi - M) < float(tc.max()) and T_LOW < math.cos(math.pi - M)       # both arc branches occur
    auto = head_reference(emb, weight, labels, mg, bias, autograd=True)
    mine = head_reference(emb, weight, labels, mg, bias, autograd=False)
    assert mine["a"].min() < -20 and mine["a"].max() > 20                          # both tails of the sigmoid
    for key in ("loss", "dbias", "d_emb", "d_w"):
        a, b = mine[key].numpy(), auto[key].numpy()
        np.testing.assert_allclose(a, b, rtol=1e-10, atol=1e-10 * float(np.abs(b).max()), err_msg=key)
    assert float(auto["dbias"]) != 0.0 and (kind == "arc") == (mg[0] == ARC)


def test_double_clamp_padding_and_softplus_tails():
    """where the clamp binds d/dcos is 0 while the loss and bias terms count; a label -1 row has no target column; softplus keeps its
    relative accuracy where log(1 + e) is 0 in fp32"""
    from uniface_double import COS, _softplus, terms
    raw = torch.tensor([[1.5, 0.25, -1.5], [0.5, 0.25, 0.0]], dtype=torch.float64)
    term, dcos, db, a = terms(raw, torch.tensor([0, -1]), (COS, 2.0, 0.25, 0.5, 3.0, 0.5), 0.5)
    assert a.tolist() == [[2 * 0.75 - 0.5, 2 * 0.75 - 0.5, 2 * -0.5 - 0.5], [2 * 1.0 - 0.5, 2 * 0.75 - 0.5, 2 * 0.5 - 0.5]]
    assert dcos[0].tolist()[0] == 0.0 and dcos[0].tolist()[2] == 0.0 and dcos[0, 1] > 0 and bool((dcos[1] > 0).all())
    sig = lambda x: 1.0 / (1.0 + math.exp(-x))      # noqa: E731
    assert float(term[0, 0]) == pytest.approx(3.0 * math.log1p(math.exp(-1.0))) and float(db[0, 0]) == pytest.approx(3.0 * sig(-1.0))
    assert float(term[1, 0]) == pytest.approx(0.5 * math.log1p(math.exp(1.5))) and float(db[1, 0]) == pytest.approx(-0.5 * sig(1.5))
    assert float(dcos[1, 2]) == pytest.approx(0.5 * sig(0.5) * 2.0)
    tiny = float(_softplus(torch.tensor(-40.0, dtype=torch.float64)))
    assert tiny == pytest.approx(math.exp(-40.0), rel=1e-12) and np.log(np.float32(1.0) + np.exp(np.float32(-40.0))) == 0.0


# ------------------------------------------------------------------------------------------------ descriptor, module, ABI
def test_margin_descriptor_and_module_surface():
    from nets.ArcFace import ARCFACE, COSFACE, SUPPORTED, BceMargin, UniFace, UniMargin, is_plain_arcface, margin_of
    mod = UniFace(48.0, 0.35, kind="arc", w_pos=0.5, w_neg=2.0, m_neg=0.1)
    assert margin_of(mod) == UniMargin(ARCFACE, 48.0, 0.35, 0.1, 0.5, 2.0)
    assert margin_of(UniFace()) == UniMargin(COSFACE, 64.0, 0.4, 0.0, 1.0, 1.0)
    assert (mod.scale, mod.margin) == (48.0, 0.35) and not is_plain_arcface(margin_of(mod))
    assert "UniFace" in SUPPORTED and "CurricularFace" in SUPPORTED
    assert not getattr(mod, "needs_norms", False)
    assert BceMargin._fields == ("kind", "s", "m", "m_neg", "w_pos", "w_neg", "bias")
    # the threshold: a [1] fp32 Parameter, or a buffer with learn_bias=False; checkpointed either way
    assert [n for n, _ in mod.named_parameters()] == ["bias"] and mod.bias.dtype == torch.float32 and mod.bias.shape == (1,)
    fixed = UniFace(learn_bias=False, bias_init=3.0)
    assert list(fixed.parameters()) == [] and set(dict(fixed.named_buffers())) == {"bias"} and fixed.bias.tolist() == [3.0]
    assert "bias" in mod.state_dict() and "bias" in fixed.state_dict()
    mod.reset_bias(1000)
    assert float(mod.bias.detach()) == pytest.approx(math.log(10 * 1000), rel=1e-6)
    fixed.reset_bias(1000)
    assert fixed.bias.tolist() == [3.0]                          # an explicit bias_init stands
    mod.w_neg = 1.5                                              # read at call time, like the other modules
    assert margin_of(mod).w_neg == 1.5
    for kw, word in ((dict(kind="sphere"), "kind"), (dict(s=0.0), "s must"), (dict(s=float("nan")), "s must"), (dict(m=float("inf")), "finite"),
                     (dict(m_neg=float("nan")), "finite"), (dict(kind="arc", m=4.0), "pi"), (dict(kind="arc", m=-0.1), "pi"),
                     (dict(w_pos=-1.0), "w_pos"), (dict(w_neg=float("nan")), "w_pos"), (dict(w_pos=0.0, w_neg=0.0), "not both 0"),
                     (dict(bias_init=float("inf")), "bias_init")):
        with pytest.raises(ValueError, match=word):
            UniFace(**kw)
    UniFace(kind="cos", m=4.0)                                   # no angle: any finite margin
    with pytest.raises(RuntimeError, match="no CPU path"):
        UniFace()(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))
    # the module of another package is still refused by name
    with pytest.raises(NotImplementedError, match="UniFace"):
        margin_of(torch.nn.Linear(2, 2))


def test_entry_points_refuse_bad_arguments_before_any_launch():
    import __graft_entry__ as ge
    ge.build()
    from frhip import _abi, ops
    from nets.ArcFace import BceMargin
    lib = _abi.lib()
    host = (ctypes.c_float * 8)()                        # never dereferenced: every call below must return before a launch
    p = ctypes.addressof(host)
    nan, inf = float("nan"), float("inf")

    def refused(rc, name, *words):
        err = lib.frhip_last_error()
        assert rc == -1 and name in err and all(w in err for w in words), (rc, err)

    D_ = ops._MarginBceDesc
    good = D_(1, 64.0, 0.4, 0.0, 1.0, 1.0, p)
    bad = [(None, b"null descriptor"), (D_(1, 64.0, 0.4, 0.0, 1.0, 1.0, None), b"null bias"), (D_(2, 64.0, 0.4, 0.0, 1.0, 1.0, p), b"kind"),
           (D_(-1, 64.0, 0.4, 0.0, 1.0, 1.0, p), b"kind"), (D_(1, 0.0, 0.4, 0.0, 1.0, 1.0, p), b"s must"), (D_(1, -1.0, 0.4, 0.0, 1.0, 1.0, p), b"s must"),
           (D_(1, nan, 0.4, 0.0, 1.0, 1.0, p), b"s must"), (D_(0, 64.0, -0.1, 0.0, 1.0, 1.0, p), b"[0, pi)"), (D_(0, 64.0, math.pi, 0.0, 1.0, 1.0, p), b"[0, pi)"),
           (D_(0, 64.0, 4.0, 0.0, 1.0, 1.0, p), b"[0, pi)"), (D_(1, 64.0, nan, 0.0, 1.0, 1.0, p), b"finite"), (D_(1, 64.0, inf, 0.0, 1.0, 1.0, p), b"finite"),
           (D_(1, 64.0, 0.4, nan, 1.0, 1.0, p), b"finite"), (D_(1, 64.0, 0.4, -inf, 1.0, 1.0, p), b"finite"), (D_(1, 64.0, 0.4, 0.0, -1.0, 1.0, p), b"w_pos"),
           (D_(1, 64.0, 0.4, 0.0, 1.0, -0.5, p), b"w_pos"), (D_(1, 64.0, 0.4, 0.0, nan, 1.0, p), b"w_pos"), (D_(1, 64.0, 0.4, 0.0, 1.0, nan, p), b"w_pos"),
           (D_(1, 64.0, 0.4, 0.0, 0.0, 0.0, p), b"both 0")]
    ref = lambda d: None if d is None else ctypes.byref(d)      # noqa: E731
    for desc, word in bad:
        w = (b"BCE descriptor", word)
        refused(lib.frhip_head_fwd_bce(1, p, p, p, 4, 10, 64, ref(desc), p, p, p, p, p, None), b"frhip_head_fwd_bce", *w)
        refused(lib.frhip_head_bwd_dt_bce(1, p, p, p, 4, 10, 64, ref(desc), 0.25, None, p, 12, None, 0, None), b"frhip_head_bwd_dt_bce", *w)
        refused(lib.frhip_head_fwd_sub_bce(1, p, p, p, 4, 10, 64, 3, ref(desc), p, p, p, p, p, p, None), b"frhip_head_fwd_sub_bce", *w)
        refused(lib.frhip_head_bwd_dt_sub_bce(1, p, p, p, 4, 10, 64, 3, ref(desc), 0.25, None, p, 36, 12, None, 0, None),
                b"frhip_head_bwd_dt_sub_bce", *w)
        refused(lib.frhip_bce_fwd(p, p, 4, 10, ref(desc), p, p, None), b"frhip_bce_fwd", *w)
        refused(lib.frhip_bce_bwd(p, p, 4, 10, ref(desc), 0.25, None, p, None), b"frhip_bce_bwd", *w)
    # a good descriptor does not rescue a bad shape, dtype, pitch, sub-centre count or operand
    g = ctypes.byref(good)
    refused(lib.frhip_head_fwd_bce(2, p, p, p, 4, 10, 64, g, p, p, p, p, p, None), b"frhip_head_fwd_bce", b"bad dtype 2")
    refused(lib.frhip_head_fwd_bce(1, p, p, p, 4, 10, 48, g, p, p, p, p, p, None), b"frhip_head_fwd_bce", b"d=48")
    refused(lib.frhip_head_fwd_bce(1, p, p, p, 0, 10, 64, g, p, p, p, p, p, None), b"frhip_head_fwd_bce", b"n=0")
    refused(lib.frhip_head_fwd_bce(1, None, p, p, 4, 10, 64, g, p, p, p, p, p, None), b"frhip_head_fwd_bce", b"null pointer")
    refused(lib.frhip_head_fwd_bce(1, p, p, p, 4, 10, 64, g, p, None, p, p, p, None), b"frhip_head_fwd_bce", b"null pointer")
    refused(lib.frhip_head_fwd_sub_bce(1, p, p, p, 4, 10, 64, 3, g, p, p, p, None, p, p, None), b"frhip_head_fwd_sub_bce", b"null pointer")
    for k in (0, lib.frhip_head_sub_max() + 1):
        refused(lib.frhip_head_fwd_sub_bce(1, p, p, p, 4, 10, 64, k, g, p, p, p, p, p, p, None), b"frhip_head_fwd_sub_bce", b"%d sub-centres" % k)
        refused(lib.frhip_head_bwd_dt_sub_bce(1, p, p, p, 4, 10, 64, k, g, 0.25, None, p, 36, 12, None, 0, None), b"frhip_head_bwd_dt_sub_bce",
                b"%d sub-centres" % k)
    refused(lib.frhip_head_bwd_dt_bce(1, p, p, p, 4, 10, 64, g, 0.25, None, p, 10, None, 0, None), b"frhip_head_bwd_dt_bce", b"bad dT pitch 10")
    refused(lib.frhip_head_bwd_dt_bce(1, p, p, p, 4, 10, 64, g, 0.25, None, p, 12, p, 3, None), b"frhip_head_bwd_dt_bce", b"bad transposed pitch 3")
    refused(lib.frhip_head_bwd_dt_bce(1, p, p, p, 4, 10, 64, g, 0.25, None, None, 12, None, 0, None), b"frhip_head_bwd_dt_bce", b"null pointer")
    refused(lib.frhip_head_bwd_dt_sub_bce(1, p, p, p, 4, 10, 64, 3, g, 0.25, None, p, 24, 12, None, 0, None), b"frhip_head_bwd_dt_sub_bce",
            b"bad dT pitches")
    refused(lib.frhip_bce_fwd(None, p, 4, 10, g, p, p, None), b"frhip_bce_fwd", b"non-null")
    refused(lib.frhip_bce_fwd(p, p, 0, 10, g, p, p, None), b"frhip_bce_fwd", b"n=0")
    refused(lib.frhip_bce_bwd(p, p, 4, 0, g, 0.25, None, p, None), b"frhip_bce_bwd", b"c=0")
    refused(lib.frhip_bce_bwd(p, p, 4, 10, g, 0.25, None, None, None), b"frhip_bce_bwd", b"non-null")
    refused(lib.frhip_bce_reduce(p, p, 0, p, None), b"frhip_bce_reduce", b"n=0")
    refused(lib.frhip_bce_reduce(p, None, 4, p, None), b"frhip_bce_reduce", b"non-null")
    refused(lib.frhip_bce_merge(p, 0, 4, p, p, None), b"frhip_bce_merge", b"world_size >= 1 (0)")
    refused(lib.frhip_bce_merge(p, 2, 0, p, p, None), b"frhip_bce_merge", b"n_global >= 1 (0)")
    refused(lib.frhip_bce_merge(None, 2, 4, p, p, None), b"frhip_bce_merge", b"non-null")
    refused(lib.frhip_bce_merge(p, 2, 4, p, None, None), b"frhip_bce_merge", b"non-null")
    with pytest.raises(ValueError, match="bce_fwd: logits must be a tensor on the GPU"):
        ops.bce_fwd(torch.zeros(4, 10), torch.zeros(4, dtype=torch.int64), BceMargin(1, 64.0, 0.4, 0.0, 1.0, 1.0, torch.zeros(1)))
    with pytest.raises(ValueError, match="bce_reduce: rowloss must be a tensor on the GPU"):
        ops.bce_reduce(torch.zeros(4), torch.zeros(4))
    # the header declares exactly the eight new entry points
    names = {n for _, n, _ in _abi.prototypes()}
    new = {"frhip_head_fwd_bce", "frhip_head_bwd_dt_bce", "frhip_head_fwd_sub_bce", "frhip_head_bwd_dt_sub_bce", "frhip_bce_reduce",
           "frhip_bce_merge", "frhip_bce_fwd", "frhip_bce_bwd"}
    assert new <= names and len(names) == 172


# ------------------------------------------------------------------------------------------------ PartialFC on gloo with the double
KIND, M_NEG, W_POS, W_NEG = "arc", 0.1, 0.7, 1.3


def _factory(s, m):
    from nets.ArcFace import UniFace
    return UniFace(s, m, kind=KIND, w_pos=W_POS, w_neg=W_NEG, m_neg=M_NEG)


def _inputs():
    from uniface_double import case
    emb, weight, labels = case(2 * B, C, D, 8200)
    return emb.double(), weight, labels


def _worker(rank, ws, path, ret):
    for p in (ROOT, os.path.join(ROOT, "face-recognition-pytorch_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="file://" + path, rank=rank, world_size=ws)
    np.savez(os.path.join(ret, "rank%d.npz" % rank), **_run(rank, ws))
    dist.destroy_process_group()


def _run(rank, ws):
    """one rank's part: its rows of the shared batch (2 B rows in all, at either world size), one forward / backward, checkpoints"""
    import nets.PartialFC as P
    from nets.ArcFace import UniFace
    from oracle import head_ref
    from uniface_double import UniHeadKernels

    class Recording(UniHeadKernels):
        def __init__(self):
            self.pairs = []

        def bce_merge(self, gathered, n_global):
            self.pairs.append(gathered.clone())
            return super().bce_merge(gathered, n_global)

    emb, weight, labels = _inputs()
    conf = types.SimpleNamespace(emd_size=D, sample_rate=1.0, mixed_precision=False, loss_s=S, loss_m=M)
    kern = Recording()
    pfc = P.PartialFC(conf, C, margin_loss=_factory, kernels=kern)
    mod = pfc.margin_softmax
    assert isinstance(mod, UniFace) and float(mod.bias.detach()) == pytest.approx(math.log(10 * C), rel=1e-6)     # reset_bias(num_classes), the GLOBAL count
    assert [n for n, _ in pfc.named_parameters()] == ["weight_activated", "margin_softmax.bias"]
    start, num = head_ref.shard_range(C, ws, rank)
    with torch.no_grad():
        pfc.weight_activated.data.copy_(weight[start:start + num])
    rows = 2 * B // ws
    mine = slice(rank * rows, (rank + 1) * rows)
    e = emb[mine].clone().requires_grad_(True)
    loss = pfc(e, labels[mine].clone(), None)
    (3.0 * loss).backward()                                      # an upstream factor reaches every gradient
    out = dict(loss=float(loss.detach()), d_emb=e.grad.numpy(), d_w=pfc.weight_activated.grad.numpy().copy(), dbias=mod.bias.grad.numpy().copy(),
               pairs=kern.pairs[0].numpy(), bias0=mod.bias.detach().numpy().copy())
    # the checkpoint carries the threshold next to the weight; one without it is refused, not silently reset
    with torch.no_grad():
        mod.bias.fill_(1.25)
    sd = {k: v.clone() for k, v in pfc.state_dict().items()}
    assert set(sd) == {"weight", "margin_softmax.bias"}
    fresh = P.PartialFC(conf, C, margin_loss=_factory, kernels=Recording())
    fresh.load_state_dict(sd)
    out["fresh_bias"] = fresh.margin_softmax.bias.detach().numpy().copy()
    assert torch.equal(fresh.weight_activated.data, pfc.weight_activated.data)
    with pytest.raises(KeyError, match="margin_softmax.bias"):
        fresh.load_state_dict({"weight": sd["weight"]})
    with pytest.raises(ValueError, match="does not take"):
        pfc(emb[mine].clone(), labels[mine].clone(), None, norms=torch.ones(rows))
    return out


def _one_process():
    with tempfile.TemporaryDirectory() as td:
        dist.init_process_group("gloo", init_method="file://" + os.path.join(td, "pg"), rank=0, world_size=1)
        try:
            return _run(0, 1)
        finally:
            dist.destroy_process_group()


def test_same_loss_and_bias_gradient_at_world_sizes_1_and_2():
    from oracle import head_ref
    from uniface_double import assert_case, cosines, head_reference
    emb, weight, labels = _inputs()
    n = 2 * B
    mg = _mg(KIND, M_NEG, W_POS, W_NEG)
    assert_case(cosines(emb, weight), labels, mg[0], M)
    b0 = float(np.float32(math.log(10 * C)))                     # the parameter is fp32
    ref = head_reference(emb, weight, labels, mg, b0)
    one = _one_process()
    ws = 2
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_worker, args=(ws, os.path.join(td, "pg"), td), nprocs=ws, join=True)
        two = [dict(np.load(os.path.join(td, "rank%d.npz" % r))) for r in range(ws)]
    assert two[0]["loss"] == two[1]["loss"] and np.array_equal(two[0]["dbias"], two[1]["dbias"])       # equal across ranks, bit for bit
    assert np.array_equal(two[0]["pairs"], two[1]["pairs"]) and two[0]["pairs"].shape == (ws, 2) and one["pairs"].shape == (1, 2)
    for r, o in [(0, one)] + list(enumerate(two)):
        world = 1 if o is one else ws
        assert float(o["bias0"][0]) == b0
        np.testing.assert_allclose(float(o["loss"]), float(ref["loss"]), rtol=1e-12)
        np.testing.assert_allclose(float(o["dbias"][0]), 3.0 * float(ref["dbias"]), rtol=1e-6)          # the parameter's gradient is fp32
        rows = n // world
        np.testing.assert_allclose(o["d_emb"], 3.0 * world * ref["d_emb"][r * rows:(r + 1) * rows].numpy(), rtol=1e-9, atol=1e-12)
        start, num = head_ref.shard_range(C, world, r)
        want = 3.0 * ref["d_w"][start:start + num].numpy()
        np.testing.assert_allclose(o["d_w"], want, rtol=1e-6, atol=1e-7 * np.abs(want).max())           # the parameter is fp32
        assert o["fresh_bias"].tolist() == [1.25]
    # the ranks' pairs add up to the single rank's: the loss is a plain sum over shards
    np.testing.assert_allclose(two[0]["pairs"].sum(axis=0), one["pairs"][0], rtol=1e-12)


def test_adamw_flavour_with_sampling_and_two_subcenters():
    """PartialFCAdamW, sample_rate 0.3, conf.subcenters = 2 on the double's kernels: "all classes" are the activated ones, the pooled cosine
    enters the rule, the sampled rows carry their Adam state into the optimizer's LAST group while the threshold sits in the one before"""
    import nets.PartialFC as P
    from subcenter_double import case
    from uniface_double import UniHeadKernels, assert_case, head_reference
    n, K = 2 * B, 2
    emb, weight, labels, res = case(n, C, D, K, 7300)
    own = torch.nonzero(labels >= 0).flatten()
    with tempfile.TemporaryDirectory() as td:
        dist.init_process_group("gloo", init_method="file://" + os.path.join(td, "pg"), rank=0, world_size=1)
        try:
            conf = types.SimpleNamespace(emd_size=D, sample_rate=0.3, mixed_precision=False, loss_s=S, loss_m=M, subcenters=K)
            pfc = P.PartialFCAdamW(conf, C, margin_loss=_factory, kernels=UniHeadKernels())
            with torch.no_grad():
                pfc.weight.copy_(weight)
            dummy = torch.nn.Parameter(torch.zeros(1))
            bias = pfc.margin_softmax.bias
            opt = torch.optim.AdamW([{"params": [dummy]}, {"params": [bias], "weight_decay": 0.0}, {"params": [pfc.weight_activated]}], lr=1e-2)
            e = emb.double().requires_grad_(True)
            torch.manual_seed(5)
            loss = pfc(e, labels.clone(), opt)
            loss.backward()
            index = pfc.weight_index.clone()
            assert opt.param_groups[-1]["params"][0] is pfc.weight_activated and pfc.weight_activated.grad.shape == (K * index.numel(), D)
            assert opt.state[pfc.weight_activated]["exp_avg"] is pfc.weight_activated_exp_avg
            assert opt.param_groups[1]["params"][0] is bias and bias.grad is not None
            tsub = pfc.last_target_sub.clone()
            b0, dbias = float(bias.detach()), float(bias.grad)
        finally:
            dist.destroy_process_group()
    assert index.numel() == int(0.3 * C) and bool(torch.isin(labels[own], index).all())
    pos = torch.full_like(labels, -1)
    pos[own] = torch.searchsorted(index, labels[own])
    rows = torch.cat([index + k * C for k in range(K)])
    ref = head_reference(emb, weight[rows], pos, _mg(KIND, M_NEG, W_POS, W_NEG), b0, K=K)
    assert_case(ref["raw"], pos, _mg(KIND)[0], M)
    np.testing.assert_allclose(float(loss.detach()), float(ref["loss"]), rtol=1e-12)
    np.testing.assert_allclose(dbias, float(ref["dbias"]), rtol=1e-6)
    np.testing.assert_allclose(e.grad.numpy(), ref["d_emb"].numpy(), rtol=1e-9, atol=1e-12)
    want = torch.full((n,), -1, dtype=torch.int64)
    want[own] = res["win"][own, labels[own]]
    assert torch.equal(tsub.long(), want)


# ------------------------------------------------------------------------------------------------ the Model's optimizer groups
def _model_groups(margin_loss):
    """configure_optimizers on a stand-in Model (no encoder is built: the grouping reads self.encoder / self.loss / self.conf alone)"""
    import nets.PartialFC as P
    from model.FR_PartialFC import Model
    from uniface_double import UniHeadKernels
    conf = types.SimpleNamespace(emd_size=D, sample_rate=1.0, mixed_precision=False, loss_s=S, loss_m=M, optimizer="SGD", lr=0.1, mom=0.9,
                                 wd=5e-4, lr_scheduler=None)
    extra = {} if margin_loss is None else {"margin_loss": margin_loss}
    me = types.SimpleNamespace(conf=conf, lr=conf.lr, encoder=torch.nn.Linear(4, 3), loss=P.PartialFC(conf, C, kernels=UniHeadKernels(), **extra))
    opt, _ = Model.configure_optimizers(me)
    return me, opt


def test_model_optimizer_groups():
    from nets.ArcFace import ArcFace, UniFace
    with tempfile.TemporaryDirectory() as td:
        dist.init_process_group("gloo", init_method="file://" + os.path.join(td, "pg"), rank=0, world_size=1)
        try:
            me, opt = _model_groups(UniFace)
            groups = opt.param_groups
            assert len(groups) == 3
            assert [id(p) for p in groups[0]["params"]] == [id(p) for p in me.encoder.parameters()]
            assert len(groups[1]["params"]) == 1 and groups[1]["params"][0] is me.loss.margin_softmax.bias and groups[1]["weight_decay"] == 0.0
            assert len(groups[2]["params"]) == 1 and groups[2]["params"][0] is me.loss.weight_activated and groups[2]["weight_decay"] == 5e-4
            # a threshold that is not learned is a buffer: the groups are the two of every other margin
            me, opt = _model_groups(lambda s, m: UniFace(s, m, learn_bias=False))
            assert len(opt.param_groups) == 2 and opt.param_groups[1]["params"][0] is me.loss.weight_activated
            for factory in (None, ArcFace):
                me, opt = _model_groups(factory)
                groups = opt.param_groups
                assert len(groups) == 2 and [id(p) for p in groups[1]["params"]] == [id(p) for p in me.loss.parameters()]
                assert len(groups[1]["params"]) == 1 and groups[1]["params"][0] is me.loss.weight_activated
        finally:
            dist.destroy_process_group()
