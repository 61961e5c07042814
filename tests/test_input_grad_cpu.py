"""CPU-side checks of the image-gradient / eval-mode backward surface: the new C-ABI entry points are declared and exported, the ops
wrappers refuse what the kernels cannot take before touching a GPU, and an fp8 model refuses eval-mode differentiation."""
import ctypes
import types

import pytest
import torch

NEW_SYMBOLS = ("frhip_bn_eval_state", "frhip_bn_bwd_finalize_eval", "frhip_stem_dx", "frhip_stem_dx_s2")


def test_new_entry_points_are_declared_and_exported():
    import __graft_entry__ as ge
    ge.build()
    from frhip import _abi
    protos = _abi.parse_header()
    for name in NEW_SYMBOLS:
        assert name in protos, name
    handle = ctypes.CDLL(_abi.LIB_PATH)
    assert all(hasattr(handle, n) for n in NEW_SYMBOLS)
    assert len(protos["frhip_stem_dx"][1]) == 14 and len(protos["frhip_stem_dx_s2"][1]) == 9


def test_entry_points_report_bad_arguments():
    from frhip import _abi
    lib = _abi.lib()
    # recompute form without x / cb: FRHIP_EINVAL before any launch
    assert lib.frhip_stem_dx(0, None, 1, 1, 1, 1, 1, 1, None, 2, 8, 8, 1, None) == -1
    assert b"frhip_stem_dx" in lib.frhip_last_error()
    assert lib.frhip_stem_dx_s2(0, 1, 1, 20, 2, 8, 8, 1, None) == -1          # kp < 27
    assert lib.frhip_stem_dx_s2(5, 1, 1, 64, 2, 8, 8, 1, None) == -1          # unknown dtype
    assert lib.frhip_bn_eval_state(0, None, None, None, None, 1e-5, None, None, None, None, None) == -1


def _stem_operands(b=2, h=9, w=11, dt=torch.bfloat16, device="cpu"):
    hp, wp_ = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return dict(x=torch.zeros(b, 3, h, w, device=device), wp=torch.zeros(64, 1, 1, 32, dtype=dt, device=device),
                dpool=torch.zeros(b, hp, wp_, 64, dtype=dt, device=device), arg=torch.zeros(b, hp, wp_, 64, dtype=torch.uint8, device=device),
                pooled=torch.zeros(b, hp, wp_, 64, dtype=dt, device=device), coef=torch.zeros(3, 64, device=device))


def test_stem_dx_wrapper_rejects_cpu_tensors():
    from frhip import ops
    with pytest.raises(ValueError, match="GPU"):
        ops.stem_dx(**_stem_operands())
    with pytest.raises(ValueError, match="GPU"):
        ops.stem_dx_s2(torch.zeros(2, 5, 6, 64, dtype=torch.bfloat16), torch.zeros(64, 1, 1, 64, dtype=torch.bfloat16), 9, 11)


def _fake_cuda(t):
    """a CPU tensor that claims to live on the GPU: shape checks run before anything reads its memory"""
    class T(torch.Tensor):
        @property
        def is_cuda(self):
            return True
    return t.as_subclass(T)


def test_stem_dx_wrapper_rejects_mismatched_shapes():
    from frhip import ops
    ops_ = {k: _fake_cuda(v) for k, v in _stem_operands().items()}
    bad = dict(ops_, dpool=_fake_cuda(torch.zeros(2, 4, 6, 64, dtype=torch.bfloat16)))       # one pooled row short
    with pytest.raises(ValueError, match="dpool"):
        ops.stem_dx(**bad)
    bad = dict(ops_, pooled=_fake_cuda(torch.zeros(2, 5, 6, 64, dtype=torch.float32)))       # dtype differs from wp's
    with pytest.raises(ValueError, match="pooled"):
        ops.stem_dx(**bad)
    bad = dict(ops_, x=_fake_cuda(torch.zeros(2, 4, 9, 11)))
    with pytest.raises(ValueError, match="x must be"):
        ops.stem_dx(**bad)
    bad = dict(ops_, wp=_fake_cuda(torch.zeros(64, 1, 1, 64, dtype=torch.bfloat16)))          # the im2col pack (kp 64), not kp 32
    with pytest.raises(ValueError, match="wp"):
        ops.stem_dx(**bad)
    dy0 = _fake_cuda(torch.zeros(2, 5, 6, 64, dtype=torch.bfloat16))
    wp = _fake_cuda(torch.zeros(64, 1, 1, 64, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="does not match"):
        ops.stem_dx_s2(dy0, wp, 12, 11)
    with pytest.raises(ValueError, match="wp"):
        ops.stem_dx_s2(dy0, _fake_cuda(torch.zeros(64, 1, 1, 64, dtype=torch.float32)), 9, 11)


def test_fp8_model_refuses_eval_mode_differentiation():
    import nets.resnet as R
    net = R.Encoder(types.SimpleNamespace(network="ResNet18", emd_size=512, frhip_dtype="bf16", frhip_fp8=True))
    net.eval()
    x = torch.zeros(2, 3, 112, 112, requires_grad=True)
    with pytest.raises(NotImplementedError, match="fp8"):
        net(x)
    net.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="fp8"):
        net(x)
    # without anything to differentiate it is the inference path (which has no CPU route)
    with torch.no_grad(), pytest.raises(RuntimeError, match="MI355X"):
        net(x)
