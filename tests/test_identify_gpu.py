"""1:N identification on the device (frhip_gallery_topk, ops.gallery_topk, utils.eval.identify, Model.cross_test_epoch_end): equality,
scores and indices, with the CPU double (tests/identify_double.py); the leave-one-out search against frhip_cross_score's own
scores; invariance under the band split, the launch order and the in-launch gallery split; poisoned memory; bounded device memory;
the rates end to end.  Every comparison is np.array_equal: the arithmetic is exact by construction."""
import numpy as np
import pytest
import torch

import identify_double
from test_cross_hist_gpu import _embeddings

pytestmark = pytest.mark.gpu


def _case(p, g, d, seed):
    """probe [p,d] and gallery [g,d] cut from one _embeddings set (shared identities, duplicated rows -> exact ties, rows scaled x 2
    -> negative scores), plus: probe 0 equal to a gallery row present three times, one NaN gallery row, one NaN probe row"""
    e, _ = _embeddings(p + g, d, seed=seed)
    probe, gallery = e[:p].copy(), e[p:].copy()
    if g >= 4:
        gallery[0] = gallery[g // 2] = gallery[g - 1]
        probe[0] = gallery[g - 1]
    if g >= 5:
        gallery[g // 3, d // 2] = np.nan
    if p >= 3:
        probe[p - 1, 0] = np.nan
    return probe, gallery


def _search(probe, gallery, k, exclude=None, bounds=None):
    from frhip import ops
    ex = None if exclude is None else torch.from_numpy(exclude).cuda()
    ts, ti = ops.gallery_topk(torch.from_numpy(probe).cuda(), torch.from_numpy(gallery).cuda(), k, ex, bounds)
    assert ts.dtype == torch.float64 and ti.dtype == torch.int64 and ts.shape == (probe.shape[0], k) and ti.shape == ts.shape
    return ts.cpu().numpy(), ti.cpu().numpy()


def _same(got, want, what=""):
    assert np.array_equal(got[1], want[1]), "%s: indices differ in %d rows" % (what, int((got[1] != want[1]).any(axis=1).sum()))
    assert np.array_equal(got[0], want[0]), "%s: scores differ in %d rows" % (what, int((got[0] != want[0]).any(axis=1).sum()))


CASES = [(1, 1, 512, 1), (1, 5000, 512, 10), (257, 5000, 512, 10), (130, 129, 100, 64), (5, 3, 3, 8), (300, 1000, 3, 1)]


@pytest.mark.parametrize("p,g,d,k", CASES, ids=["p%d_g%d_d%d_k%d" % c for c in CASES])
def test_equal_to_the_double(p, g, d, k):
    probe, gallery = _case(p, g, d, seed=p * 31 + g * 7 + d + k)
    want = identify_double.topk(probe, gallery, k)
    got = _search(probe, gallery, k)
    _same(got, want, "search")
    if g >= 4:                                                   # the triplicated row: score 1 three times, indices ascending
        assert got[1][0, :min(k, 3)].tolist() == [0, g // 2, g - 1][:min(k, 3)] and got[0][0, 0] == 1.0
    if g >= 5:
        assert not (got[1] == g // 3).any()                      # the NaN gallery row is never returned
    if p >= 3:
        assert (got[1][p - 1] == -1).all() and np.isneginf(got[0][p - 1]).all()      # the NaN probe returns nothing
    if g < k:
        assert (got[1][:, g:] == -1).all() and np.isneginf(got[0][:, g:]).all()      # padding at the end


def test_exclude_and_agreement_with_cross_score():
    from frhip import ops
    n, d, k = 1000, 512, 10
    e, lab = _embeddings(n, d, seed=77)
    me = np.arange(n, dtype=np.int64)
    got = _search(e, e, k, exclude=me)
    _same(got, identify_double.topk(e, e, k, exclude=me), "leave-one-out")
    assert not (got[1] == me[:, None]).any()
    free = _search(e, e, k)
    assert (free[1] == me[:, None]).any(axis=1).all() and (free[0][:, 0] == 1.0).all()     # without it every row finds itself
    some = me.copy()
    some[::2] = -1                                               # -1: nothing excluded for that probe
    _same(_search(e, e, k, exclude=some), identify_double.topk(e, e, k, exclude=some), "partial exclude")
    # the same device functions: every listed score is cross_score's entry of that unordered pair, to the bit
    scores = ops.cross_score(torch.from_numpy(e).cuda(), torch.from_numpy(lab).cuda())[0].cpu().numpy()
    hi, lo = np.maximum(me[:, None], got[1]), np.minimum(me[:, None], got[1])
    assert np.array_equal(got[0], scores[hi * (hi - 1) // 2 + lo])


def test_band_invariance():
    from frhip import ops
    from frhip._abi import check, lib
    p, g, d, k = 300, 50000, 512, 10
    probe, gallery = _case(p, g, d, seed=5)
    whole = _search(probe, gallery, k, bounds=[0, g])
    assert (whole[1][:p - 1] >= 0).all()
    for bounds in ([0, 1, 12345, 40000, g], [0, g - 3, g], None, ops.gallery_topk_bands(p, g, 1 << 20)):
        _same(_search(probe, gallery, k, bounds=bounds), whole, str(bounds)[:40])
    # the bands in reverse order, through the raw call
    pt, gt = torch.from_numpy(probe).cuda(), torch.from_numpy(gallery).cuda()
    ts = torch.full((p, k), float("-inf"), dtype=torch.float64, device="cuda")
    ti = torch.full((p, k), -1, dtype=torch.int64, device="cuda")
    ws = ops.gallery_topk_workspace(p, k, "cuda")
    b = [0, 1, 12345, 40000, g]
    for g0, g1 in reversed(list(zip(b, b[1:]))):
        check(lib().frhip_gallery_topk(pt.data_ptr(), gt.data_ptr(), None, p, g, d, k, g0, g1, ts.data_ptr(), ti.data_ptr(),
                                       ws.data_ptr(), ws.numel() * 8, ops._s()), "frhip_gallery_topk")
    _same((ts.cpu().numpy(), ti.cpu().numpy()), whole, "reversed bands")
    # a band merged a second time changes nothing (the lists hold every entry once)
    check(lib().frhip_gallery_topk(pt.data_ptr(), gt.data_ptr(), None, p, g, d, k, 0, 12345, ts.data_ptr(), ti.data_ptr(),
                                   ws.data_ptr(), ws.numel() * 8, ops._s()), "frhip_gallery_topk")
    _same((ts.cpu().numpy(), ti.cpu().numpy()), whole, "band merged twice")


def test_split_invariance_at_few_probes():
    p, g, d, k = 512, 200000, 512, 10
    probe, gallery = _case(p, g, d, seed=9)
    few = _search(probe[:16], gallery, k)                        # one probe tile: the gallery is split over the whole chip
    _same(few, identify_double.topk(probe[:16], gallery, k), "16 probes")
    many = _search(probe, gallery, k)                            # four probe tiles: another grid, another split
    _same((many[0][:16], many[1][:16]), few, "rows 0..15 of 512 probes")


@pytest.mark.parametrize("pattern", [float("nan"), 3e38, 0.75], ids=["nan", "3e38", "0.75"])
def test_poisoned_memory(pattern):
    from poison import assert_poison_applies, poisoned_empty, reset_frhip_caches
    probe, gallery = _case(130, 4099, 100, seed=41)
    me = np.arange(130, dtype=np.int64)
    clean = _search(probe, gallery, 10, exclude=me)
    with poisoned_empty(pattern):
        assert_poison_applies(pattern, torch.float64)
        reset_frhip_caches()                                     # the workspace is allocated again, poisoned
        got = _search(probe, gallery, 10, exclude=me)
        banded = _search(probe, gallery, 10, exclude=me, bounds=[0, 128, 1000, 4099])
    _same(got, clean, "poisoned")
    _same(banded, clean, "poisoned, banded")


def test_device_memory_stays_small():
    from poison import reset_frhip_caches
    from frhip import ops
    p, g, d, k = 4096, 200000, 512, 10
    gen = torch.Generator(device="cuda").manual_seed(3)
    probe = torch.nn.functional.normalize(torch.randn((p, d), device="cuda", generator=gen)).contiguous()
    gallery = torch.nn.functional.normalize(torch.randn((g, d), device="cuda", generator=gen)).contiguous()
    reset_frhip_caches()                                         # the workspace counts: it is allocated inside the measured call
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ts, ti = ops.gallery_topk(probe, gallery, k)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    outputs = ts.numel() * 8 + ti.numel() * 8
    print("peak over inputs %d bytes, outputs %d bytes" % (peak, outputs))
    assert peak - outputs < 64 << 20, (peak, outputs)            # a P x G float64 matrix would be 6.5 GB
    assert (ti >= 0).all() and (ti < g).all() and (ts[:, :-1] >= ts[:, 1:]).all()


def _known_mates(seed, ids, per_id, n_mated, n_non, d):
    """gallery: per_id noisy images of each of `ids` identities; probes: n_mated further images of gallery identities and n_non images
    of identities the gallery does not hold"""
    r = np.random.default_rng(seed)
    centres = r.standard_normal((ids + n_non, d))
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)       # noqa: E731
    gl = np.repeat(np.arange(ids), per_id)
    gallery = unit(centres[gl] + 0.5 * r.standard_normal((gl.size, d)))
    pl = np.concatenate([r.integers(0, ids, size=n_mated), ids + np.arange(n_non)])
    probe = unit(centres[pl] + 0.5 * r.standard_normal((pl.size, d)))
    return probe, pl.astype(np.int64), gallery, gl.astype(np.int64)


def test_identify_and_rates_end_to_end():
    from utils import eval as ev
    probe, pl, gallery, gl = _known_mates(13, ids=400, per_id=5, n_mated=300, n_non=100, d=512)
    ts, ti = ev.identify(probe, gallery, k=10)
    assert isinstance(ts, np.ndarray) and ts.dtype == np.float64 and ti.dtype == np.int64
    want = identify_double.topk(probe, gallery, 10)
    _same((ts, ti), want, "identify")
    _same(ev.identify(torch.from_numpy(probe), torch.from_numpy(gallery).cuda(), k=10), want, "identify, tensors")
    got = ev.identification_rates(ts, ti, pl, gl, fpirs=(1e-1, 1e-2))
    ref = ev.identification_rates(want[0], want[1], pl, gl, fpirs=(1e-1, 1e-2))
    assert got == ref
    assert got["n_mated"] == 300 and got["n_nonmated"] == 100
    mate_first = gl[want[1][:300, 0]] == pl[:300]                # the figures from the double's lists, restated here
    assert got["cmc"][1] == float(np.mean(mate_first)) and got["cmc"][1] > 0.9
    s = np.sort(want[0][300:, 0])[::-1]
    for f in (1e-1, 1e-2):
        tau = s[int(np.floor(f * 100))]
        assert got["threshold"][f] == tau and got["fpir"][f] <= f
        assert got["tpir"][f] == float(np.mean(mate_first & (want[0][:300, 0] > tau)))
    assert got["tpir"][1e-1] > 0.5
    # leave-one-out on one set
    e = np.concatenate([probe, gallery])
    lab = np.concatenate([pl, gl])
    ts, ti = ev.identify(e, e, k=5, exclude_self=True)
    _same((ts, ti), identify_double.topk(e, e, 5, exclude=np.arange(e.shape[0])), "exclude_self")
    loo = ev.identification_rates(ts, ti, lab, lab, ranks=(1, 5), exclude_self=True)
    assert loo["n_nonmated"] == 100 and loo["n_mated"] == e.shape[0] - 100
    with pytest.raises(ValueError, match="same length"):
        ev.identify(probe, gallery, k=5, exclude_self=True)


def test_model_cross_test_identification():
    """Model.cross_test_epoch_end with conf.cross_test_identification = 5 adds the leave-one-out rates; without it: today's keys"""
    import os
    import tempfile
    import types

    import torch.distributed as dist
    from model.FR_PartialFC import Model
    from utils import eval as ev
    ev._CROSS_CACHE.clear()
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
    plain = model.cross_test_epoch_end(outs)
    assert sorted(plain) == ["acc", "dataset_name", "eer_th", "infer_time", "roc"]
    conf.cross_test_identification = 5
    with_id = model.cross_test_epoch_end(outs)
    assert sorted(with_id) == ["acc", "dataset_name", "eer_th", "identification", "infer_time", "roc"]
    assert all(with_id[key] == plain[key] for key in plain)
    emb = np.concatenate([o["synt_embedding"].numpy() for o in outs])
    lab = np.concatenate([o["synt_label_list"].numpy() for o in outs])
    want = identify_double.topk(emb, emb, 5, exclude=np.arange(12))
    ref = ev.identification_rates(want[0], want[1], lab, lab, ranks=(1, 5), exclude_self=True)
    assert with_id["identification"] == ref
    assert ref["n_probe"] == 12 and ref["n_nonmated"] == 1 and ref["n_mated"] == 11       # label 4 occurs once: the non-mated probe
