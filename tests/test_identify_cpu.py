"""CPU-side checks of the 1:N identification path: frhip_gallery_topk declared, exported and bound; bad arguments reported through
frhip_last_error before any device work; utils.eval.identification_rates against a brute-force restatement; the CPU double's own
tie rule; no CPU fallback."""
import ctypes
import math

import numpy as np
import pytest
import torch

import identify_double


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from frhip import _abi
    return _abi


def test_declared_exported_and_bound():
    _abi = _lib()
    protos = _abi.parse_header()
    assert "frhip_gallery_topk" in protos and "frhip_gallery_topk_workspace" in protos
    res, args = protos["frhip_gallery_topk"]
    assert res is ctypes.c_int and len(args) == 14
    assert args[3] is ctypes.c_int64 and args[4] is ctypes.c_int64 and args[7] is ctypes.c_int64 and args[8] is ctypes.c_int64
    assert args[5] is ctypes.c_int and args[6] is ctypes.c_int and args[12] is ctypes.c_size_t
    assert hasattr(ctypes.CDLL(_abi.LIB_PATH), "frhip_gallery_topk")
    assert hasattr(_abi.lib(), "frhip_gallery_topk")
    from frhip import ops
    from utils import eval as ev
    assert callable(ops.gallery_topk) and callable(ops.gallery_topk_bands)
    assert callable(ev.identify) and callable(ev.identification_rates)


def _call(lib, p, g, d, k, g0, g1, ptr=None, ws_bytes=0):
    return lib.frhip_gallery_topk(ptr, ptr, None, p, g, d, k, g0, g1, ptr, ptr, ptr, ws_bytes, None)


@pytest.mark.parametrize("p,g,d,k,g0,g1,what", [
    (-1, 10, 512, 5, 0, 10, b"p = -1"),
    (4, -2, 512, 5, 0, 0, b"g = -2"),
    (4, 10, 0, 5, 0, 10, b"d = 0"),
    (4, 10, -3, 5, 0, 10, b"d = -3"),
    (4, 10, (1 << 27) + 1, 5, 0, 10, b"d = 134217729"),
    (4, 10, 512, 0, 0, 10, b"k = 0"),
    (4, 10, 512, 65, 0, 10, b"k = 65"),
    (4, 10, 512, -1, 0, 10, b"k = -1"),
    (4, 10, 512, 5, -1, 10, b"band [-1, 10)"),
    (4, 10, 512, 5, 0, 11, b"band [0, 11)"),
    (4, 10, 512, 5, 7, 3, b"band [7, 3)"),
    (4, 3_000_000_000, 512, 5, 2_999_999_999, 3_000_000_001, b"band [2999999999, 3000000001)"),
])
def test_bad_arguments_return_an_error(p, g, d, k, g0, g1, what):
    _abi = _lib()
    lib = _abi.lib()
    rc = _call(lib, p, g, d, k, g0, g1)
    assert rc == -1
    msg = lib.frhip_last_error()
    assert b"frhip_gallery_topk" in msg and what in msg, msg
    with pytest.raises(_abi.FrhipError):
        _abi.check(rc, "frhip_gallery_topk")


def test_null_pointers_and_nothing_to_do():
    _abi = _lib()
    lib = _abi.lib()
    assert _call(lib, 4, 10, 512, 5, 0, 10) == -1
    msg = lib.frhip_last_error()
    assert b"frhip_gallery_topk" in msg and b"null pointer" in msg, msg
    assert _call(lib, 0, 10, 512, 5, 0, 10) == 0               # no probe
    assert _call(lib, 4, 10, 512, 5, 4, 4) == 0                # empty band
    assert _call(lib, 4, 0, 512, 5, 0, 0) == 0                 # empty gallery


def test_workspace_size_and_a_workspace_too_small():
    _abi = _lib()
    lib = _abi.lib()
    need = ctypes.c_int64(-1)
    assert lib.frhip_gallery_topk_workspace(0, 10, ctypes.byref(need)) == 0 and need.value == 0
    sizes = {}
    for p in (1, 128, 4096, 200_000, 1_000_000):
        assert lib.frhip_gallery_topk_workspace(p, 10, ctypes.byref(need)) == 0
        sizes[p] = need.value
        per_row = 10 * 16
        assert need.value >= (p + 127) // 128 * 128 * per_row          # at least one list per probe row
        assert need.value <= max(1024, (p + 127) // 128) * 128 * per_row   # O(P k) + a fixed part: never O(P G)
    assert sizes[1] == sizes[4096]                                         # the fixed part
    assert lib.frhip_gallery_topk_workspace(4, 65, ctypes.byref(need)) == -1
    assert b"frhip_gallery_topk_workspace" in lib.frhip_last_error() and b"k = 65" in lib.frhip_last_error()
    assert lib.frhip_gallery_topk_workspace(4, 5, None) == -1
    assert b"null pointer" in lib.frhip_last_error()
    # a real (host) address for every pointer: the size check fails before anything is launched or dereferenced
    buf = ctypes.create_string_buffer(64)
    rc = _call(lib, 4, 10, 512, 5, 0, 10, ctypes.addressof(buf), ws_bytes=64)
    assert rc == -1
    msg = lib.frhip_last_error()
    assert b"frhip_gallery_topk" in msg and b"workspace of 64 bytes is too small" in msg, msg


def test_cpu_tensors_raise():
    _lib()
    from frhip import ops
    with pytest.raises(AssertionError, match="contiguous CUDA tensors"):
        ops.gallery_topk(torch.randn(8, 16), torch.randn(20, 16), 3)
    with pytest.raises(ValueError, match="bounds"):
        ops.gallery_topk(torch.zeros(4, 2), torch.zeros(9, 2), 3, bounds=[0, 3])
    with pytest.raises(ValueError, match="bounds"):
        ops.gallery_topk(torch.zeros(4, 2), torch.zeros(9, 2), 3, bounds=[0, 5, 4, 9])


def test_bands_cover_the_gallery_in_tile_multiples():
    _lib()
    from frhip import ops
    for p, g in ((0, 0), (0, 1000), (1, 1), (128, 1_000_000), (10_000, 100_000), (20_000, 20_000), (300, 50_000), (1 << 31, 1000)):
        b = ops.gallery_topk_bands(p, g)
        assert b[0] == 0 and b[-1] == g and all(x < y for x, y in zip(b, b[1:])), (p, g, b[:4])
        assert all(x % 128 == 0 for x in b[:-1])
        assert all((y - x) * p <= max(ops.GALLERY_TOPK_PAIRS_PER_LAUNCH, 128 * p) for x, y in zip(b, b[1:]))
    assert len(ops.gallery_topk_bands(128, 1_000_000)) == 2                 # 1.28e8 pairs: one launch
    assert len(ops.gallery_topk_bands(20_000, 20_000, 1 << 26)) > 2


def test_eval_has_no_cpu_path(monkeypatch):
    _lib()
    from utils import eval as ev
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.identify(np.ones((4, 16), np.float32), np.ones((8, 16), np.float32), k=3)


# ---- the double's own rules, pinned on a case small enough to work out by hand
def test_double_on_a_hand_written_case():
    gallery = np.array([[1, 0], [0, 1], [1, 0], [-1, 0]], dtype=np.float32)          # rows 0 and 2 are duplicates
    probe = np.array([[1, 0], [0, 1], [0, -1]], dtype=np.float32)
    s = identify_double.scores(probe, gallery)
    assert s.dtype == np.float64
    assert np.array_equal(s, np.array([[1.0, 0.5, 1.0, 0.0], [0.5, 1.0, 0.5, 0.5], [0.5, 0.0, 0.5, 0.5]]))
    ts, ti = identify_double.topk(probe, gallery, 3)
    assert np.array_equal(ti, [[0, 2, 1], [1, 0, 2], [0, 2, 3]])                    # ties: lowest index first
    assert np.array_equal(ts, [[1.0, 1.0, 0.5], [1.0, 0.5, 0.5], [0.5, 0.5, 0.5]])
    ts, ti = identify_double.topk(probe, gallery, 5, exclude=np.array([0, -1, 2]))
    assert np.array_equal(ti, [[2, 1, 3, -1, -1], [1, 0, 2, 3, -1], [0, 3, 1, -1, -1]])
    assert np.array_equal(ts, [[1.0, 0.5, 0.0, -np.inf, -np.inf], [1.0, 0.5, 0.5, 0.5, -np.inf], [0.5, 0.5, 0.0, -np.inf, -np.inf]])
    gallery[1] = np.nan                                                             # a NaN gallery row is never listed
    probe[2] = np.nan                                                               # a NaN probe lists nothing
    ts, ti = identify_double.topk(probe, gallery, 2)
    assert np.array_equal(ti, [[0, 2], [0, 2], [-1, -1]])
    assert np.array_equal(ts[:2], [[1.0, 1.0], [0.5, 0.5]]) and np.all(np.isneginf(ts[2]))


def test_double_sums_sequentially_not_pairwise():
    r = np.random.default_rng(0)
    p, g = r.standard_normal((3, 512)).astype(np.float32), r.standard_normal((5, 512)).astype(np.float32)
    want = np.empty((3, 5))
    for i in range(3):
        for j in range(5):
            acc = 0.0
            for c in range(512):
                dd = float(np.float32(g[j, c] - p[i, c]))
                acc += dd * dd
            want[i, j] = 1.0 - acc / 4.0
    assert np.array_equal(identify_double.scores(p, g), want)


# ---- identification_rates against a restatement in plain Python
def _brute(top_score, top_index, pl, gl, ranks, fpirs, exclude_self):
    n, k = len(top_index), len(top_index[0])
    mated = []
    for i in range(n):
        mated.append(any(gl[j] == pl[i] and not (exclude_self and j == i) for j in range(len(gl))))
    n_m, n_n = sum(mated), n - sum(mated)
    cmc = {}
    for r in ranks:
        good = 0
        for i in range(n):
            if mated[i] and any(top_index[i][q] >= 0 and gl[top_index[i][q]] == pl[i] for q in range(r)):
                good += 1
        cmc[r] = good / n_m if n_m else None
    s = sorted((top_score[i][0] for i in range(n) if not mated[i]), reverse=True)
    tpir, thr, fp = {}, {}, {}
    for f in fpirs:
        if not s:
            tpir[f] = thr[f] = fp[f] = None
            continue
        tau = s[int(math.floor(f * len(s)))]
        thr[f] = tau
        fp[f] = sum(1 for x in s if x > tau) / len(s)
        good = sum(1 for i in range(n) if mated[i] and top_index[i][0] >= 0 and gl[top_index[i][0]] == pl[i] and top_score[i][0] > tau)
        tpir[f] = good / n_m if n_m else None
    return {"cmc": cmc, "tpir": tpir, "threshold": thr, "fpir": fp, "n_probe": n, "n_mated": n_m, "n_nonmated": n_n}


def _random_lists(seed, n, n_g, k, exclude_self=False, nonmated=True):
    """lists as a search would return them (descending scores, distinct indices, some -1 padded) with every case the rates must
    tell apart: mate at rank 1, at a later rank, beyond k (absent from the list), non-mated probes, tied top-1 scores"""
    r = np.random.default_rng(seed)
    gl = r.integers(0, max(2, n_g // 3), size=n_g)
    if exclude_self:
        pl = gl.copy()                                          # the probes ARE the gallery; singletons are the non-mated ones
        assert n == n_g
    else:
        pl = r.choice(gl, size=n)
        if nonmated:
            pl[r.random(n) < 0.3] += 10_000                     # identities the gallery does not hold
    top_index = np.full((n, k), -1, dtype=np.int64)
    top_score = np.full((n, k), -np.inf)
    for i in range(n):
        fill = k if r.random() < 0.8 else int(r.integers(0, k + 1))           # some short (padded) lists, some empty
        cand = np.array([j for j in r.permutation(n_g) if not (exclude_self and j == i)][:fill], dtype=np.int64)
        sc = np.sort(np.round(r.random(cand.size), 2))[::-1]                  # two decimals: many ties, also among top-1 scores
        top_index[i, :cand.size], top_score[i, :cand.size] = cand, sc
    return top_score, top_index, pl, gl


@pytest.mark.parametrize("seed,n,n_g,k,exclude_self,nonmated", [
    (1, 200, 60, 10, False, True), (2, 200, 60, 5, False, True), (3, 90, 90, 10, True, True), (4, 150, 40, 10, False, False),
    (5, 7, 9, 3, False, True), (6, 400, 30, 1, False, True),
])
def test_identification_rates_match_the_brute_force(seed, n, n_g, k, exclude_self, nonmated):
    _lib()
    from utils import eval as ev
    ts, ti, pl, gl = _random_lists(seed, n, n_g, k, exclude_self, nonmated)
    ranks = tuple(r for r in (1, 2, 5, 10) if r <= k)
    fpirs = (0.5, 1e-1, 1e-2, 1e-3)
    got = ev.identification_rates(ts, ti, pl, gl, ranks=ranks, fpirs=fpirs, exclude_self=exclude_self)
    want = _brute(ts.tolist(), ti.tolist(), pl.tolist(), gl.tolist(), ranks, fpirs, exclude_self)
    for key, val in want.items():
        assert got[key] == val, key
    if nonmated and n >= 90:
        assert want["n_mated"] > 0 and want["n_nonmated"] > 0
        assert all(got["fpir"][f] <= f for f in fpirs)          # ties at the cut only lower the realised rate
    if not nonmated:
        assert want["n_nonmated"] == 0 and all(got["tpir"][f] is None and got["threshold"][f] is None for f in fpirs)
    assert isinstance(got["report"], str) and "Rank-1" in got["report"] and "TPIR @ FPIR" in got["report"]
    assert "Total probe count = {:,}".format(n) in got["report"]


def test_identification_rates_hand_case():
    _lib()
    from utils import eval as ev
    gl = np.array([0, 0, 1, 2])
    pl = np.array([0, 1, 2, 7, 8, 9])                            # three mated probes, three non-mated
    ti = np.array([[0, 1, 2], [3, 2, 0], [0, 1, -1], [2, 0, 1], [1, 2, 3], [3, -1, -1]])
    ts = np.array([[0.9, 0.8, 0.1], [0.7, 0.6, 0.2], [0.3, 0.2, -np.inf], [0.5, 0.4, 0.3], [0.5, 0.1, 0.0], [0.2, -np.inf, -np.inf]])
    out = ev.identification_rates(ts, ti, pl, gl, ranks=(1, 2, 3), fpirs=(0.5, 0.1))
    assert out["n_probe"] == 6 and out["n_mated"] == 3 and out["n_nonmated"] == 3
    assert out["cmc"] == {1: 1 / 3, 2: 2 / 3, 3: 2 / 3}          # probe 0 at rank 1, probe 1 at rank 2, probe 2's mate beyond the list
    # non-mated top-1 scores: 0.5, 0.5, 0.2.  f = 0.5: tau = s[1] = 0.5, nothing accepted above it (tie at the cut); f = 0.1: s[0] = 0.5
    assert out["threshold"] == {0.5: 0.5, 0.1: 0.5} and out["fpir"] == {0.5: 0.0, 0.1: 0.0}
    assert out["tpir"] == {0.5: 1 / 3, 0.1: 1 / 3}               # only probe 0: right at rank 1 and 0.9 > 0.5
    none = ev.identification_rates(ts[:3], ti[:3], pl[:3], gl, ranks=(1,), fpirs=(0.1,))
    assert none["n_nonmated"] == 0 and none["tpir"] == {0.1: None} and none["threshold"] == {0.1: None} and none["fpir"] == {0.1: None}
    assert none["cmc"] == {1: 1 / 3}
    lone = ev.identification_rates(ts[3:], ti[3:], pl[3:], gl, ranks=(1,), fpirs=(0.5,))
    assert lone["n_mated"] == 0 and lone["cmc"] == {1: None} and lone["tpir"] == {0.5: None} and lone["threshold"] == {0.5: 0.5}
    with pytest.raises(ValueError, match="ranks"):
        ev.identification_rates(ts, ti, pl, gl, ranks=(1, 5))
    with pytest.raises(ValueError, match="ranks"):
        ev.identification_rates(ts, ti, pl, gl, ranks=(0,))
    # exclude_self: the probes are the gallery; label 0 (rows 0, 1) is mated, labels 1 and 2 are singletons
    ti = np.array([[1, 2], [0, 3], [0, 1], [2, 1]])
    ts = np.array([[0.9, 0.1], [0.9, 0.2], [0.4, 0.3], [0.6, 0.5]])
    loo = ev.identification_rates(ts, ti, gl, gl, ranks=(1,), fpirs=(0.5,), exclude_self=True)
    assert loo["n_mated"] == 2 and loo["n_nonmated"] == 2 and loo["cmc"] == {1: 1.0}
    assert loo["threshold"] == {0.5: 0.4} and loo["fpir"] == {0.5: 0.5} and loo["tpir"] == {0.5: 1.0}
