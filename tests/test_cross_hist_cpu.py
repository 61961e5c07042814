"""CPU-side checks of frhip_cross_hist (cross-matching histograms without the pair list): declared and exported, bad arguments
reported through frhip_last_error before any device work, and no CPU fallback."""
import ctypes

import numpy as np
import pytest
import torch


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from frhip import _abi
    return _abi


def test_declared_and_exported():
    _abi = _lib()
    protos = _abi.parse_header()
    assert "frhip_cross_hist" in protos
    res, args = protos["frhip_cross_hist"]
    assert res is ctypes.c_int and len(args) == 11
    assert args[2] is ctypes.c_int64 and args[4] is ctypes.c_int64 and args[5] is ctypes.c_int64
    assert hasattr(ctypes.CDLL(_abi.LIB_PATH), "frhip_cross_hist")
    assert hasattr(_abi.lib(), "frhip_cross_hist")


@pytest.mark.parametrize("n,d,i0,i1,what", [
    (-1, 512, 0, 0, b"n = -1"),
    (10, 0, 0, 10, b"d = 0"),
    (10, -3, 0, 10, b"d = -3"),
    (10, 512, -1, 10, b"band [-1, 10)"),
    (10, 512, 0, 11, b"band [0, 11)"),
    (10, 512, 7, 3, b"band [7, 3)"),
    (3_000_000_000, 512, 2_999_999_999, 3_000_000_001, b"band [2999999999, 3000000001)"),
])
def test_bad_arguments_return_an_error(n, d, i0, i1, what):
    _abi = _lib()
    lib = _abi.lib()
    rc = lib.frhip_cross_hist(None, None, n, d, i0, i1, None, None, None, None, None)
    assert rc == -1
    msg = lib.frhip_last_error()
    assert b"frhip_cross_hist" in msg and what in msg, msg
    with pytest.raises(_abi.FrhipError):
        _abi.check(rc, "frhip_cross_hist")


def test_null_pointers_with_pairs_to_count_are_an_error():
    _abi = _lib()
    lib = _abi.lib()
    assert lib.frhip_cross_hist(None, None, 10, 512, 0, 10, None, None, None, None, None) == -1
    assert b"null pointer" in lib.frhip_last_error()
    assert lib.frhip_cross_hist(None, None, 10, 512, 4, 4, None, None, None, None, None) == 0     # empty band: nothing to do
    assert lib.frhip_cross_hist(None, None, 1, 512, 0, 1, None, None, None, None, None) == 0      # one row: no pair


def test_cpu_tensors_raise():
    _lib()
    from frhip import ops
    e, lab = torch.randn(8, 16), torch.arange(8)
    with pytest.raises(AssertionError, match="contiguous CUDA tensors"):
        ops.cross_hist(e, lab)


def test_eval_has_no_cpu_path(monkeypatch):
    _lib()
    from utils import eval as ev
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    e, lab = np.ones((8, 16), np.float32), np.arange(8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.cross_histograms(e, lab)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.cross_accuracy(e, lab, 50000)


@pytest.mark.parametrize("th", [-1, 100001, 0.5, float("nan")])
def test_cross_accuracy_rejects_thresholds_it_cannot_answer(th):
    _lib()
    from utils import eval as ev
    with pytest.raises(ValueError, match="th ="):
        ev.cross_accuracy(np.ones((8, 16), np.float32), np.arange(8), th)


def test_bands_cover_the_rows_in_tile_multiples():
    _lib()
    from frhip import ops
    for n in (0, 1, 2, 127, 128, 129, 20000, 100000, 1_000_000):
        b = ops.cross_hist_bands(n)
        assert b[0] == 0 and b[-1] == n and all(x < y for x, y in zip(b, b[1:]))
        assert all(x % 128 == 0 for x in b[:-1])
        assert all(y * (y - 1) // 2 - x * (x - 1) // 2 <= ops.CROSS_HIST_PAIRS_PER_LAUNCH + 128 * y for x, y in zip(b, b[1:]))
    with pytest.raises(ValueError):
        ops.cross_hist(torch.zeros(4, 2), torch.zeros(4, dtype=torch.int64), [0, 3])
