"""Cross-matching evaluation from histograms (frhip_cross_hist, utils.eval.cross_histograms / cross_accuracy): bit-identity with the
pair-list route (cross_score + performance_acc), the reference fixture, more than 2^31 pairs, bounded device memory, poisoned memory
and the Model route."""
import numpy as np
import pytest
import torch

from oracle import eval_ref

pytestmark = pytest.mark.gpu


def _embeddings(n, d, seed, ids=None, dup=True, scaled=True):
    """unit rows around `ids` identity centres; some rows duplicated (score exactly 1), some scaled x2 (scores below 0)"""
    r = np.random.default_rng(seed)
    ids = ids or max(1, n // 8)
    lab = r.integers(0, ids, size=n)
    centres = r.standard_normal((ids, d))
    e = centres[lab] * 0.6 + r.standard_normal((n, d))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    e = e.astype(np.float32)
    perm = r.permutation(n)
    k_dup, k_scaled = (max(1, n // 20) if dup else 0), (max(1, n // 10) if scaled else 0)
    if n >= 4 and 2 * k_dup + k_scaled <= n:
        src, dst, big = perm[:k_dup], perm[k_dup:2 * k_dup], perm[2 * k_dup:2 * k_dup + k_scaled]
        e[dst], lab[dst] = e[src], lab[src]
        e[big] *= 2.0
    return e, lab.astype(np.int64)


def _slot(s):
    """the smallest integer th with s <= th / 1e5 (Python's own division), as the threshold slots define it"""
    t = int(np.ceil(s * 1e5))
    while s <= (t - 1) / 1e5:
        t -= 1
    while not s <= t / 1e5:
        t += 1
    return t


def _fresh(ev):
    ev._CROSS_CACHE.clear()


CASES = [(2, 512), (3, 512), (17, 512), (1000, 512), (4099, 512), (20000, 512), (17, 3), (1000, 3), (4099, 100), (1000, 100)]


@pytest.mark.parametrize("n,d", CASES, ids=["n%d_d%d" % c for c in CASES])
def test_bit_identical_to_the_pair_list(n, d):
    from utils import eval as ev
    _fresh(ev)
    e, lab = _embeddings(n, d, seed=n * 7 + d, ids=max(2, n // 50))       # few identities: many genuine pairs
    hg, hi, scores, plab = ev.cross_score(e, lab)
    sg, si = ev.cross_histograms(e, lab)
    assert sg.dtype == np.float64 and sg.shape == (100001,) and si.shape == (100001,)
    assert np.array_equal(sg, hg) and np.array_equal(si, hi)
    if n >= 4:
        assert (scores < 0).any() and (scores == 1.0).any()                   # skipped bins and the clamped slot 0 are exercised
    eer_th = 100000
    if hg.sum() > 0 and hi.sum() > 0:
        _, eer_th = ev.performance_roc(hg, hi, min_level=1, max_level=3)
    ths = {eer_th, 1, 100000, 0, 99999, 50000}
    for s in scores[:: max(1, scores.size // 5)][:5]:
        t = min(max(_slot(float(s)), 0), 100000)
        ths |= {t, max(t - 1, 0)}                                             # bin edges straddling real scores
    for th in sorted(ths):
        assert ev.cross_accuracy(e, lab, th) == ev.performance_acc(scores, plab, th), th


def test_reference_fixture(golden):
    from test_eval import _cross_inputs
    from utils import eval as ev
    _fresh(ev)
    g = golden("cross_eval")
    emb, labels = _cross_inputs(g)
    hg, hi = ev.cross_histograms(emb, labels)
    assert np.array_equal(hg, g["hist_genuine"]) and np.array_equal(hi, g["hist_imposter"])
    roc, eer_th = ev.performance_roc(hg, hi, min_level=1, max_level=3)
    assert eer_th == int(g["eer_th"]) and roc == str(g["roc"])
    np.testing.assert_allclose(ev.cross_accuracy(emb, labels, eer_th), g["acc"], rtol=1e-12)


def _torch_oracle(e, lab, i0, i1):
    """bins and threshold slots of the pairs (i in [i0, i1), j < i), summed over k one column at a time in a Python loop"""
    n, d = e.shape
    rows = e[i0:i1]
    s = torch.zeros((i1 - i0, n), dtype=torch.float64, device=e.device)
    for k in range(d):
        dd = (e[None, :, k] - rows[:, None, k]).double()                      # fp32 difference, then fp64
        s += dd * dd
    score = 1.0 - s / 4.0
    ii = torch.arange(i0, i1, device=e.device)[:, None]
    keep = torch.arange(n, device=e.device)[None, :] < ii
    gen = (lab[None, :] == lab[i0:i1, None])
    score, gen = score[keep], gen[keep]
    idx = ((1e5 - 1.0) * score).to(torch.int64)
    t = torch.ceil(score * 1e5).clamp(0, 100001).to(torch.int64)
    for _ in range(2):
        t = torch.where((t > 0) & (score <= (t - 1).double() / 1e5), t - 1, t)
        t = torch.where((t < 100000) & ~(score <= t.double() / 1e5), t + 1, t)
    t = torch.where(score <= 0, torch.zeros_like(t), torch.where(score > 1, torch.full_like(t, 100001), t))
    ok = (idx >= 0) & (idx <= 100000)
    out = []
    for m in (gen & ok, ~gen & ok):
        out.append(torch.bincount(idx[m], minlength=100001))
    for m in (gen, ~gen):
        out.append(torch.bincount(t[m], minlength=100002))
    return out


def test_past_2_pow_31_pairs():
    from frhip import ops
    from frhip._abi import check, lib
    n, d = 70000, 512
    pairs = n * (n - 1) // 2
    assert pairs > 2 ** 31
    e_np, lab_np = _embeddings(n, d, seed=70000, ids=3000, dup=False, scaled=False)
    e, lab = torch.from_numpy(e_np).cuda(), torch.from_numpy(lab_np).cuda()
    hg, hi, tg, ti = ops.cross_hist(e, lab)
    assert int(tg.sum()) + int(ti.sum()) == pairs
    scores_in_range = int(hg.sum()) + int(hi.sum())
    assert scores_in_range == pairs                                          # unit rows: every score in [0, 1], every bin counted
    for bounds in ([0, 1, 12345, 40000, n], [0, n - 3, n], ops.cross_hist_bands(n, 1 << 28)):
        other = ops.cross_hist(e, lab, bounds)
        assert all(torch.equal(a, b) for a, b in zip((hg, hi, tg, ti), other)), bounds
    i0 = n - 3
    band = [torch.zeros((100001,), dtype=torch.int64, device="cuda") for _ in range(2)]
    band += [torch.zeros((100002,), dtype=torch.int64, device="cuda") for _ in range(2)]
    check(lib().frhip_cross_hist(e.data_ptr(), lab.data_ptr(), n, d, i0, n, *[h.data_ptr() for h in band], ops._s()),
          "frhip_cross_hist")
    want = _torch_oracle(e, lab, i0, n)
    for got, ref in zip(band, want):
        assert torch.equal(got, ref)
    assert int(sum(int(h.sum()) for h in band[2:])) == 3 * n - 6


def test_device_memory_stays_small_at_100k():
    from utils import eval as ev
    _fresh(ev)
    n, d = 100000, 512
    e, lab = _embeddings(n, d, seed=100000, ids=5000, dup=False, scaled=False)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    hg, hi = ev.cross_histograms(e, lab)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < 1 << 30, peak
    (_, _, tg, ti), _ = ev._cross_counts(e, lab)
    assert int(tg.sum()) + int(ti.sum()) == n * (n - 1) // 2
    assert hg.sum() + hi.sum() == n * (n - 1) // 2
    _fresh(ev)


@pytest.mark.parametrize("pattern", [float("nan"), 3e38, 0.75], ids=["nan", "3e38", "0.75"])
def test_poisoned_memory(pattern):
    from poison import assert_poison_applies, poisoned_empty, reset_frhip_caches
    from frhip import ops
    e_np, lab_np = _embeddings(4099, 100, seed=41, ids=60)
    e, lab = torch.from_numpy(e_np).cuda(), torch.from_numpy(lab_np).cuda()
    clean = ops.cross_hist(e, lab)
    with poisoned_empty(pattern):
        assert_poison_applies(pattern, torch.float32)
        reset_frhip_caches()
        got = ops.cross_hist(e, lab)
    assert all(torch.equal(a, b) for a, b in zip(clean, got))


def test_model_streaming_route_matches_list_route():
    """Model.cross_test_epoch_end with conf.cross_test_streaming returns the list route's dict on the outputs of cross_test_step"""
    import os
    import tempfile
    import types

    import torch.distributed as dist
    from model.FR_PartialFC import Model
    from utils import eval as ev
    _fresh(ev)
    if not dist.is_initialized():
        dist.init_process_group("gloo", init_method="file://" + os.path.join(tempfile.mkdtemp(), "pg"), rank=0, world_size=1)
    conf = types.SimpleNamespace(network="ResNet18", emd_size=512, img_size=112, local_rank=0, world_size=1, sample_rate=1.0,
                                 mixed_precision=True, loss_s=30.0, loss_m=0.35, n_classes=16, optimizer="SGD", lr=0.1, wd=5e-4,
                                 mom=0.9, lr_scheduler=None, frhip_dtype="bf16", ckpt_path=None, cross_test_dataset=["synt"],
                                 min_level=1, max_level=3)
    torch.manual_seed(3)
    model = Model(conf, None, "test")
    gen = torch.Generator().manual_seed(5)
    outs = []
    for k in range(3):
        img = torch.randn((4, 3, 112, 112), generator=gen).clamp_(-1, 1)
        outs.append(model.cross_test_step((img, torch.tensor([0, 1, 0, 2]) + k), 0))
    listed = model.cross_test_epoch_end(outs)
    conf.cross_test_streaming = True
    streamed = model.cross_test_epoch_end(outs)
    assert streamed == listed
    emb = np.concatenate([o["synt_embedding"].numpy() for o in outs])
    lab = np.concatenate([o["synt_label_list"].numpy() for o in outs])
    scores, plab = eval_ref.cross_scores(emb, lab)
    _, hg, hi = eval_ref.histograms(scores, plab)
    eer_th, _, _ = eval_ref.roc(hg, hi, 1, 3)
    assert streamed["eer_th"] == eer_th
