"""Sub-centre head (K centres per class) without a GPU: the float64 restatement (tests/subcenter_double.py) against oracle.head_ref at
K = 1 and against naive autograd at K = 2, 3; the host logic of nets.PartialFC at K = 3 on gloo with real ranks and the restatement as
its kernels (plane-major tables, per-plane expansion of the sampled index, optimizer-state rows, sub_hits, checkpoints, collapse); and
the new entry points of the C ABI."""
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

from oracle import head_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, M = 30.0, 0.35
N, CLASSES, D = 37, 150, 64


@pytest.fixture(scope="module")
def pg():
    own = not dist.is_initialized()
    if own:
        d = tempfile.mkdtemp()
        dist.init_process_group("gloo", init_method="file://" + os.path.join(d, "pg"), rank=0, world_size=1)
    yield
    if own and dist.is_initialized():
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------ 1. / 2. the double itself
def _atol(ref):
    """A gradient element is a sum of up to CLASSES (rows: N) products, some of which cancel: two float64 evaluations in different orders
    differ by up to the number of terms x 2^-52 x the largest element, whatever the size of the element itself."""
    return CLASSES * 2.0 ** -52 * float(ref.abs().max())


def test_double_equals_the_oracle_at_one_centre():
    from subcenter_double import case, pooled_head
    emb, weight, labels, _ = case(N, CLASSES, D, 1, 4100)
    got = pooled_head(emb, weight, labels, 1, S, M)
    ref = head_ref.head_all_shards([emb.double()], [labels], [weight.double()], CLASSES, S, M)
    np.testing.assert_allclose(float(got["loss"]), float(ref["loss"]), rtol=1e-12)
    np.testing.assert_allclose(got["d_emb"].numpy(), ref["d_emb"][0].numpy(), rtol=1e-12, atol=_atol(ref["d_emb"][0]))
    np.testing.assert_allclose(got["d_w"].numpy(), ref["d_w_act"][0].numpy(), rtol=1e-12, atol=_atol(ref["d_w_act"][0]))


@pytest.mark.parametrize("K", [2, 3])
def test_double_equals_naive_autograd_and_ties_go_to_the_lowest_plane(K):
    from subcenter_double import TIE_CLASS, assert_case, case, cross_entropy, logits, pooled_head
    emb, weight, labels, res = case(N, CLASSES, D, K, 4100 + K)
    assert_case(emb, weight, labels, K, res)
    # the exact-tie class: the copies beyond plane 0 never win a row, so they get an exact zero and plane 0 the whole gradient
    d_w = res["d_w"].view(K, CLASSES, D)
    assert bool((res["win"][:, TIE_CLASS] != 1).all())
    assert not d_w[1, TIE_CLASS].any() and float(d_w[0, TIE_CLASS].abs().max()) > 0
    # no ties: the copies become centres of their own
    w2 = weight.clone().view(K, CLASSES, D)
    w2[1:, TIE_CLASS] = torch.randn((K - 1, D), generator=torch.Generator().manual_seed(5)) * 0.05
    w2 = w2.reshape(K * CLASSES, D)
    got = pooled_head(emb, w2, labels, K, S, M)
    assert float(got["gap"].min()) > 0
    e = emb.double().requires_grad_(True)
    w = w2.double().requires_grad_(True)
    eh = e / e.norm(dim=1, keepdim=True).clamp_min(head_ref.NORM_EPS)
    wh = w / w.norm(dim=1, keepdim=True).clamp_min(head_ref.NORM_EPS)
    raw = torch.stack([eh @ wh[k * CLASSES:(k + 1) * CLASSES].t() for k in range(K)]).max(dim=0).values
    loss = cross_entropy(logits(raw, labels, S, M), labels)
    loss.backward()
    np.testing.assert_allclose(float(got["loss"]), float(loss.detach()), rtol=1e-12)
    np.testing.assert_allclose(got["d_emb"].numpy(), e.grad.numpy(), rtol=1e-10, atol=_atol(e.grad))
    np.testing.assert_allclose(got["d_w"].numpy(), w.grad.numpy(), rtol=1e-10, atol=_atol(w.grad))


# ------------------------------------------------------------------------------------------------ 3. / 5. host logic on gloo
K3, STEPS, LR, WD = 3, 2, 0.1, 5e-4


class PlainAdamW(torch.optim.AdamW):
    """AdamW restated (decoupled decay, bias-corrected) on whatever `step` count the state holds: the sampled head writes its own integer
    count into the state before every step (nets/PartialFC.py, as the reference does), which torch's implementation refuses.  The test is
    about the moment ROWS travelling with the sampled centres, and the single-process reference runs this same update."""

    @torch.no_grad()
    def step(self):
        for g in self.param_groups:
            b1, b2 = g["betas"]
            for p in g["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if "exp_avg" not in st:
                    st["exp_avg"], st["exp_avg_sq"], st["step"] = torch.zeros_like(p), torch.zeros_like(p), 0
                st["step"] = t = int(st["step"]) + 1
                p.mul_(1.0 - g["lr"] * g["weight_decay"])
                st["exp_avg"].mul_(b1).add_(p.grad, alpha=1.0 - b1)
                st["exp_avg_sq"].mul_(b2).addcmul_(p.grad, p.grad, value=1.0 - b2)
                denom = (st["exp_avg_sq"].sqrt() / math.sqrt(1.0 - b2 ** t)).add_(g["eps"])
                p.addcdiv_(st["exp_avg"], denom, value=-g["lr"] / (1.0 - b1 ** t))


def _make_opt(adamw, params):
    groups = [{"params": [torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))]}, {"params": params}]
    if adamw:
        return PlainAdamW(groups, lr=5e-3, weight_decay=WD)
    return torch.optim.SGD(groups, lr=LR, momentum=0.9, weight_decay=WD)


def _shard_table(weight, K, classes, start, num):
    """rows of the plane-major [K classes, d] table that the shard [start, start + num) owns, plane-major again"""
    return weight.view(K, classes, -1)[:, start:start + num].reshape(K * num, -1).clone()


def _worker(rank, ws, path, ret, rate, adamw):
    for p in (ROOT, os.path.join(ROOT, "face-recognition-pytorch_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import nets.PartialFC as P
    from subcenter_double import SubcenterOracleKernels, case
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="file://" + path, rank=rank, world_size=ws)
    cls = P.PartialFCAdamW if adamw else P.PartialFC
    conf = types.SimpleNamespace(emd_size=D, sample_rate=rate, mixed_precision=False, loss_s=S, loss_m=M, subcenters=K3,
                                 subcenter_track=True)
    pfc = cls(conf, CLASSES, kernels=SubcenterOracleKernels()).double()
    one = cls(types.SimpleNamespace(emd_size=D, sample_rate=rate, mixed_precision=False, loss_s=S, loss_m=M), CLASSES,
              kernels=SubcenterOracleKernels()).double()                # the head as it is today, for the sampled index
    assert pfc.subcenters == K3 and one.subcenters == 1 and one.sub_hits is None
    weight = case(ws * N, CLASSES, D, K3, 4200)[1].double()
    start, num = head_ref.shard_range(CLASSES, ws, rank)
    table = pfc.weight if rate < 1 else pfc.weight_activated.data
    assert table.shape == (K3 * num, D)
    with torch.no_grad():
        table.copy_(_shard_table(weight, K3, CLASSES, start, num))
        (one.weight if rate < 1 else one.weight_activated.data).copy_(weight[start:start + num])
    opt, opt1 = _make_opt(adamw, pfc.parameters()), _make_opt(adamw, one.parameters())
    out = {}
    names = pfc._state_names
    for st in range(STEPS):
        emb, _, labels, _ = case(ws * N, CLASSES, D, K3, 4200 + 50 * st)
        mine = slice(rank * N, (rank + 1) * N)
        e = emb[mine].double().requires_grad_(True)
        opt.zero_grad()
        torch.manual_seed(1000 + rank + 100 * st)                     # the sampling draws come from the CPU generator
        loss = pfc(e, labels[mine].clone(), opt)
        loss.backward()
        ok = opt.param_groups[-1]["params"][0] is pfc.weight_activated
        if rate < 1:
            assert pfc.weight_activated.shape == (K3 * pfc.weight_index.numel(), D)
            key = {"mom": "momentum_buffer"}
            ok = ok and all(opt.state[pfc.weight_activated][key.get(nm, nm)] is getattr(pfc, "weight_activated_" + nm) for nm in names)
        opt.step()
        torch.manual_seed(1000 + rank + 100 * st)
        one(emb[mine].double(), labels[mine].clone(), opt1)
        idx = pfc.weight_index if rate < 1 else torch.arange(num)
        idx1 = one.weight_index if rate < 1 else torch.arange(num)
        out["loss%d" % st], out["d_emb%d" % st], out["index%d" % st] = float(loss.detach()), e.grad.numpy(), idx.numpy()
        out["index_one%d" % st], out["tsub%d" % st], out["ok%d" % st] = idx1.numpy(), pfc.last_target_sub.numpy(), bool(ok)
    pfc.update()
    if rate < 1:
        out["weight"] = pfc.weight.numpy()
        for nm in names:
            out[nm] = getattr(pfc, "weight_" + nm).numpy()
    else:
        out["weight"] = pfc.weight_activated.detach().numpy()
        key = {"mom": "momentum_buffer"}
        for nm in names:
            out[nm] = opt.state[pfc.weight_activated][key.get(nm, nm)].numpy()
    out["sub_hits"] = pfc.sub_hits.numpy()
    assert "sub_hits" in pfc.state_dict() and torch.equal(pfc.dominant_subcenters(), _dominant(pfc.sub_hits))
    np.savez(os.path.join(ret, "rank%d.npz" % rank), **out)
    dist.destroy_process_group()


def _dominant(hits):
    """first index of the maximum over the planes, restated with a loop"""
    k, c = hits.shape
    dom = torch.zeros(c, dtype=torch.int64)
    for j in range(c):
        col = hits[:, j].tolist()
        dom[j] = col.index(max(col))
    return dom


@pytest.mark.parametrize("adamw", [False, True], ids=["sgd", "adamw"])
@pytest.mark.parametrize("rate", [1.0, 0.3])
@pytest.mark.parametrize("ws", [1, 2])
def test_partial_fc_three_centres_on_gloo_vs_single_process_double(ws, rate, adamw):
    from subcenter_double import case, pooled_head
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_worker, args=(ws, os.path.join(td, "pg"), td, rate, adamw), nprocs=ws, join=True)
        outs = [dict(np.load(os.path.join(td, "rank%d.npz" % r))) for r in range(ws)]
    names = ("exp_avg", "exp_avg_sq") if adamw else ("mom",)
    weight = case(ws * N, CLASSES, D, K3, 4200)[1].double()
    shards = [head_ref.shard_range(CLASSES, ws, r) for r in range(ws)]
    full = [_shard_table(weight, K3, CLASSES, s0, num) for s0, num in shards]
    state = [{nm: torch.zeros_like(full[r]) for nm in names} for r in range(ws)]
    hits = [torch.zeros((K3, num), dtype=torch.int64) for _, num in shards]
    for st in range(STEPS):
        emb, _, labels, _ = case(ws * N, CLASSES, D, K3, 4200 + 50 * st)
        # the activated classes of all ranks in rank order (plane-major over the concatenation), every label as its position in that list
        index = [torch.from_numpy(outs[r]["index%d" % st]).long() for r in range(ws)]
        pos, offset = torch.full_like(labels, -1), 0
        for r, (s0, num) in enumerate(shards):
            assert outs[r]["ok%d" % st]
            assert np.array_equal(outs[r]["index%d" % st], outs[r]["index_one%d" % st]), "the sampled classes differ from the K = 1 head's"
            own = (labels >= s0) & (labels < s0 + num)
            assert bool(torch.isin(labels[own] - s0, index[r]).all())
            pos[own] = torch.searchsorted(index[r], labels[own] - s0) + offset
            offset += index[r].numel()
        if rate < 1:
            assert all(i.numel() == int(rate * num) for i, (_, num) in zip(index, shards))
        rows = [torch.cat([index[r] + k * shards[r][1] for k in range(K3)]) for r in range(ws)]
        act = torch.cat([torch.cat([full[r][index[r] + k * shards[r][1]] for r in range(ws)]) for k in range(K3)])
        ref = pooled_head(emb, act, pos, K3, S, M)
        d_w = ref["d_w"].view(K3, offset, D)
        offset = 0
        for r, (s0, num) in enumerate(shards):
            o, cnt = outs[r], index[r].numel()
            np.testing.assert_allclose(o["loss%d" % st], float(ref["loss"]), rtol=1e-12)
            np.testing.assert_allclose(o["d_emb%d" % st], ws * ref["d_emb"][r * N:(r + 1) * N].numpy(), rtol=1e-9, atol=1e-16)
            # winners of the targets over the global batch, -1 for rows another shard owns; and the counts they add up to
            own = torch.nonzero((labels >= s0) & (labels < s0 + num)).flatten()
            tsub = torch.full((ws * N,), -1, dtype=torch.int64)
            tsub[own] = ref["win"][own, pos[own]]
            assert np.array_equal(o["tsub%d" % st], tsub.numpy())
            got_tsub = torch.from_numpy(o["tsub%d" % st]).long()
            for m_ in own.tolist():
                hits[r][got_tsub[m_], labels[m_] - s0] += 1
            # this rank's step in the single process: the same optimizer on its activated rows and their state rows
            p = torch.nn.Parameter(full[r][rows[r]].clone())
            p.grad = d_w[:, offset:offset + cnt].reshape(K3 * cnt, D).clone()
            offset += cnt
            opt = _make_opt(adamw, [p])
            key = {"mom": "momentum_buffer"}
            for nm in names:
                opt.state[p][key.get(nm, nm)] = state[r][nm][rows[r]].clone()
            if adamw:
                opt.state[p]["step"] = st + 1 if rate < 1 else st          # the sampled head writes its own count (one ahead)
            opt.step()
            full[r][rows[r]] = p.data
            for nm in names:
                state[r][nm][rows[r]] = opt.state[p][key.get(nm, nm)]
    for r in range(ws):
        np.testing.assert_allclose(outs[r]["weight"], full[r].numpy(), rtol=1e-9, atol=1e-15)
        for nm in names:
            np.testing.assert_allclose(outs[r][nm], state[r][nm].numpy(), rtol=1e-8, atol=1e-18, err_msg=nm)
        assert np.array_equal(outs[r]["sub_hits"], hits[r].numpy()) and int(hits[r].sum()) > 0
        if rate < 1:                # rows of classes never sampled: untouched table, zero state -- in every plane
            seen = torch.unique(torch.cat([torch.from_numpy(outs[r]["index%d" % st]).long() for st in range(STEPS)]))
            never = torch.tensor(sorted(set(range(shards[r][1])) - set(seen.tolist())))
            assert never.numel() > 0
            for k in range(K3):
                assert not outs[r][names[0]][never + k * shards[r][1]].any()


# ------------------------------------------------------------------------------------------------ 4. / 6. checkpoints, collapse
def _head(K, rate=1.0, track=False, classes=CLASSES):
    import nets.PartialFC as P
    from subcenter_double import SubcenterOracleKernels
    conf = types.SimpleNamespace(emd_size=D, sample_rate=rate, mixed_precision=False, loss_s=S, loss_m=M)
    if K is not None:
        conf.subcenters = K
    if track:
        conf.subcenter_track = True
    return P.PartialFC(conf, classes, kernels=SubcenterOracleKernels())


@pytest.mark.parametrize("rate", [1.0, 0.3])
def test_state_dict_round_trip_and_row_count_refusal(pg, rate):
    a, b = _head(3, rate, track=True), _head(3, rate, track=True)
    with torch.no_grad():
        a.sub_hits.copy_(torch.arange(3 * CLASSES).view(3, CLASSES))
    sd = a.state_dict()
    assert sd["weight"].shape == (3 * CLASSES, D) and sd["sub_hits"].shape == (3, CLASSES)
    b.load_state_dict({k: v.clone() for k, v in sd.items()})
    assert torch.equal(b.state_dict()["weight"], sd["weight"]) and torch.equal(b.sub_hits, a.sub_hits)
    b.load_state_dict({"weight": sd["weight"].clone()})                   # written without the counts: they start from zero
    assert not b.sub_hits.any()
    for rows in (CLASSES, 2 * CLASSES, 3 * CLASSES + 1):
        with pytest.raises(ValueError, match="3 sub-centre"):
            b.load_state_dict({"weight": torch.zeros(rows, D)})
    one = _head(None, rate)                                               # conf.subcenters absent: today's head and today's tensor
    assert one.subcenters == 1 and one.state_dict()["weight"].shape == (CLASSES, D) and "sub_hits" not in one.state_dict()
    with pytest.raises(ValueError, match="1 sub-centre"):
        one.load_state_dict({"weight": sd["weight"]})
    with pytest.raises(RuntimeError, match="subcenter_track"):
        _head(3, rate).dominant_subcenters()


def test_collapse_loads_into_a_one_centre_head(pg):
    from subcenter_double import case, pooled_head
    emb, weight, labels, res = case(N, CLASSES, D, 3, 4103)
    head = _head(3, 1.0, track=True).double()
    with torch.no_grad():
        head.weight_activated.data.copy_(weight.double())
    dummy = torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))
    opt = torch.optim.SGD([{"params": [dummy]}, {"params": head.parameters()}], lr=0.0)
    head(emb.double(), labels.clone(), opt)
    own = torch.nonzero(labels >= 0).flatten()
    assert torch.equal(head.last_target_sub[own].long(), res["win"][own, labels[own]]) and int(head.last_target_sub[labels < 0]) == -1
    head.eval()
    head(emb.double(), labels.clone(), opt)                              # not a training step: the counts stay
    want = torch.zeros((3, CLASSES), dtype=torch.int64)
    for m_ in own.tolist():
        want[res["win"][m_, labels[m_]], labels[m_]] += 1
    assert torch.equal(head.sub_hits, want)
    dom = head.dominant_subcenters()
    assert torch.equal(dom, _dominant(want)) and len(set(dom.tolist())) == 3
    table = head.collapse_subcenters()
    planes = weight.double().view(3, CLASSES, D)
    assert table.shape == (CLASSES, D) and all(torch.equal(table[c], planes[dom[c], c]) for c in range(CLASSES))
    one = _head(1, 1.0).double()
    one.load_state_dict({"weight": table})
    assert torch.equal(one.weight_activated.data, table)
    got = float(one(emb.double(), labels.clone(), opt).detach())
    np.testing.assert_allclose(got, float(pooled_head(emb, table, labels, 1, S, M)["loss"]), rtol=1e-12)


# ------------------------------------------------------------------------------------------------ 7. ABI
SUB_ENTRY_POINTS = {
    "frhip_head_sub_max": [],
    "frhip_head_fwd_sub": ["i", "p", "p", "p", "i", "i", "i", "i", "p", "p", "p", "p", "p", "p", "p", "p"],
    "frhip_head_fwd_sub_rows": ["i", "p", "p", "p", "i", "i", "i", "i", "p", "p", "p", "p", "p", "p", "p", "p"],
    "frhip_head_bwd_dt_sub": ["i", "p", "p", "p", "i", "i", "i", "i", "p", "p", "p", "f", "p", "p", "i", "i", "p", "i", "p"],
    "frhip_head_bwd_dt_sub_rows": ["i", "p", "p", "p", "i", "i", "i", "i", "p", "p", "p", "f", "p", "p", "i", "i", "p", "i", "p"],
}


def test_abi_prototypes_and_argument_guards():
    import __graft_entry__ as ge
    ge.build()
    from frhip import _abi
    protos = _abi.parse_header()
    code = {"i": ctypes.c_int, "p": ctypes.c_void_p, "f": ctypes.c_float}
    handle = ctypes.CDLL(_abi.LIB_PATH)
    for name, args in SUB_ENTRY_POINTS.items():
        assert name in protos and hasattr(handle, name), name
        assert protos[name] == (ctypes.c_int, [code[a] for a in args]), name
    lib = _abi.lib()
    kmax = lib.frhip_head_sub_max()
    assert kmax >= 4
    margin = (ctypes.c_float * 5)()                                        # never read: the guards come first
    for k in (0, -1, kmax + 1):
        calls = {
            "frhip_head_fwd_sub": lambda: lib.frhip_head_fwd_sub(1, None, None, None, 8, 16, 64, k, margin, None, None, None, None, None, None, None),
            "frhip_head_fwd_sub_rows": lambda: lib.frhip_head_fwd_sub_rows(1, None, None, None, 8, 16, 64, k, margin, None, None, None, None, None,
                                                                          None, None),
            "frhip_head_bwd_dt_sub": lambda: lib.frhip_head_bwd_dt_sub(1, None, None, None, 8, 16, 64, k, margin, None, None, 1.0, None, None,
                                                                      16 * max(k, 1), 16, None, 0, None),
            "frhip_head_bwd_dt_sub_rows": lambda: lib.frhip_head_bwd_dt_sub_rows(1, None, None, None, 8, 16, 64, k, margin, None, None, 1.0, None,
                                                                                None, 16 * max(k, 1), 16, None, 0, None),
        }
        for name, call in calls.items():
            assert call() == -1, (name, k)
            assert b"sub-centres per class" in lib.frhip_last_error(), (name, k)
    # a table that does not fit: every plane is below 2 GiB, the four of them together are not
    assert lib.frhip_head_fwd_sub(1, None, None, None, 8, 3_000_000, 64, 4, margin, None, None, None, None, None, None, None) == -1
    assert b"exceed 2 GiB" in lib.frhip_last_error()
    # pitches: the planes' pitch must hold a plane in whole 16-byte vectors, the row pitch all planes
    for ldt, ldp in ((300, 150), (456, 152 + 1), (2 * 152, 152)):
        assert lib.frhip_head_bwd_dt_sub(1, None, None, None, 8, 150, 64, 3, margin, None, None, 1.0, None, None, ldt, ldp, None, 0, None) == -1
        assert b"bad dT pitches" in lib.frhip_last_error()


def test_binding_refuses_a_table_that_is_not_whole_planes():
    import __graft_entry__ as ge
    ge.build()
    from frhip import ops
    with pytest.raises(ValueError, match="plane-major"):
        ops.head_fwd(torch.zeros(8, 64), torch.zeros(151, 64), torch.zeros(8, dtype=torch.int32), S, M, subcenters=3)
    with pytest.raises(ValueError, match="plane-major"):
        ops.head_bwd_dt(torch.zeros(8, 64), torch.zeros(151, 64), torch.zeros(8, dtype=torch.int32), S, M, None, None, 1.0, subcenters=2)
