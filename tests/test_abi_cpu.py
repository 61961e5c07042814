"""CPU-side checks of the C-ABI boundary: the library builds for gfx950, loads without a GPU and exports every
symbol include/frhip.h declares (no compute calls here)."""
import ctypes
import os

import pytest


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as ge
    ge.build()
    from frhip import _abi
    protos = _abi.parse_header()
    assert len(protos) >= 35
    handle = ctypes.CDLL(_abi.LIB_PATH)
    missing = [n for n in protos if not hasattr(handle, n)]
    assert not missing, missing
    lib = _abi.lib()
    assert lib.frhip_abi_version() == 1
    assert lib.frhip_nt_block_m(64) == 256 and lib.frhip_nt_block_m(128) == 128
    assert lib.frhip_head_groups(122000) == 1908


def test_bad_arguments_are_reported_not_thrown():
    from frhip import _abi
    lib = _abi.lib()
    # channel count that is not a multiple of the K step: must return FRHIP_EINVAL before touching the GPU
    rc = lib.frhip_conv_fwd(0, None, None, None, None, 1, 8, 8, 3, 64, 3, 3, 1, 1, None)
    assert rc == -1
    assert b"unsupported shape" in lib.frhip_last_error()
    with pytest.raises(_abi.FrhipError):
        _abi.check(rc, "frhip_conv_fwd")


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from frhip import _abi
    monkeypatch.setattr(_abi, "_LIB", None)
    monkeypatch.setattr(_abi, "LIB_PATH", os.path.join(tmp_path, "nope.so"))
    with pytest.raises(_abi.FrhipError):
        _abi.lib()


def test_unknown_dtype_is_refused_first_in_one_wording():
    """Every prototype of frhip.h whose first parameter is `int dtype` and whose last is the stream, called with dtype 2 and zero / NULL
    for the rest: it must say exactly "<name>: bad dtype 2" and return FRHIP_EINVAL before it reads another argument (a NULL dereference
    or a division by a zero size would end the process, not the test)"""
    from frhip import _abi
    lib = _abi.lib()
    protos = _abi.parse_header()
    names = [name for _, name, params in _abi.prototypes()
             if params and params[0] == "int dtype" and params[-1] == "frhip_stream_t stream"]
    assert len(names) >= 60, names
    names.append("frhip_wgrad_plan")            # no stream: a read-only query, behind the same guard as the weight gradients it plans
    names.append("frhip_dgrad_route")           # likewise for the data-gradients; its `int out[5]` binds as a pointer
    assert protos["frhip_dgrad_route"][1][-1] is ctypes.c_void_p and len(protos["frhip_dgrad_route"][1]) == 13
    names.append("frhip_conv_fwd_route")        # and for the forward convolutions
    assert protos["frhip_conv_fwd_route"][1][-1] is ctypes.c_void_p and len(protos["frhip_conv_fwd_route"][1]) == 12
    for name in names:
        args = [2] + [None if t is ctypes.c_void_p else t(0) for t in protos[name][1][1:]]
        rc = getattr(lib, name)(*args)
        assert rc == -1, (name, rc)
        assert lib.frhip_last_error() == name.encode() + b": bad dtype 2", (name, lib.frhip_last_error())
