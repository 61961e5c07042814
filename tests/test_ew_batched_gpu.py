"""The batched element-wise BatchNorm passes (four rows' loads in flight per thread, the default) against the row-at-a-time
kernels they replace (frhip_set_ew_batch(0)): the same expression per element, so every output must agree BIT FOR BIT --
both dtypes, every mode of the four entry points (ReLU mask on / off, residual with and without its own scale / shift, per-sample
rowscale, in place), the four ResNet50 shapes at B = 512, ragged row counts (not a multiple of a block's row lanes, fewer rows than one
block holds) at C = 64 and C = 512, and once with a weight gradient resident on a second stream -- the case the kernels are for."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "face-recognition-pytorch_amd")) if p not in sys.path]

pytestmark = pytest.mark.gpu

RESNET = [(512 * 56 * 56, 64), (512 * 28 * 28, 128), (512 * 14 * 14, 256), (512 * 7 * 7, 512)]
# ragged: fewer rows than one block's row lanes; one short of / one past a whole batch; an odd count of several blocks; rows_per = 7
RAGGED = [(3, 64), (7, 512), (32 * 8 - 1, 64), (4 * 4 + 1, 512), (7 * 1231, 64), (7 * 307, 512), (7 * 93, 128), (7 * 150, 256)]
SENTINEL = -77.0


@pytest.fixture()
def hook():
    from frhip._abi import lib
    old = lib().frhip_set_ew_batch(-1)
    assert old == 1, "the batched kernels are the default"
    yield lib().frhip_set_ew_batch
    lib().frhip_set_ew_batch(old)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _inputs(rows, c, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn((rows, c), generator=g, device="cuda").to(dtype)
    b = torch.randn((rows, c), generator=g, device="cuda").to(dtype)
    coef = torch.randn((7, c), generator=g, device="cuda")
    return a, b, coef


def _bwd_apply(a, b, coef, mask, rowscale=None, rows_per=0):
    from frhip import ops
    from frhip._abi import check, lib
    p = ops._p
    rows, c = a.shape
    out = torch.full_like(a, SENTINEL)
    if rowscale is not None:
        check(lib().frhip_bn_bwd_apply_rs(ops.dt_of(a), p(a), p(b), p(coef[0]), p(coef[1]), p(coef[2]), p(rowscale), rows_per, p(out), rows, c,
                                          ops._s()), "frhip_bn_bwd_apply_rs")
    else:
        check(lib().frhip_bn_bwd_apply(ops.dt_of(a), p(a), p(b), p(coef[0]), p(coef[1]), p(coef[2]), p(coef[3]) if mask else None,
                                       p(coef[4]) if mask else None, p(out), rows, c, ops._s()), "frhip_bn_bwd_apply")
    return out


def _apply(y, res, coef, mode):
    """mode: plain | relu | res | res_relu | res_affine | inplace | inplace_res | rs | rs_res"""
    from frhip import ops
    from frhip._abi import check, lib
    p = ops._p
    rows, c = y.shape
    relu = int(mode in ("relu", "res_relu"))
    if mode.startswith("rs"):
        rows_per = 7
        keep = (torch.arange(rows // rows_per, device="cuda") % 3).float() * 0.75
        out = torch.full_like(y, SENTINEL)
        check(lib().frhip_bn_apply_rs(ops.dt_of(y), p(y), p(coef[0]), p(coef[1]), p(res) if mode == "rs_res" else None, p(keep), rows_per,
                                      p(out), rows, c, ops._s()), "frhip_bn_apply_rs")
        return out
    use_res = mode in ("res", "res_relu", "res_affine", "inplace_res")
    affine = mode == "res_affine"
    out = y.clone() if mode.startswith("inplace") else torch.full_like(y, SENTINEL)
    src = out if mode.startswith("inplace") else y
    check(lib().frhip_bn_apply(ops.dt_of(y), p(src), p(coef[0]), p(coef[1]), p(res) if use_res else None, p(coef[5]) if affine else None,
                               p(coef[6]) if affine else None, relu, p(out), rows, c, ops._s()), "frhip_bn_apply")
    return out


def _compare(hook, fn):
    hook(0)
    ref = fn()
    torch.cuda.synchronize()
    assert not (ref.float() == SENTINEL).any(), "the reference left elements unwritten"
    hook(1)
    got = fn()
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(ref))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("rows,c", RESNET + RAGGED)
def test_bwd_apply_batched_is_bit_identical(hook, rows, c, dtype):
    a, b, coef = _inputs(rows, c, dtype, 5)
    for mask in (True, False):
        _compare(hook, lambda: _bwd_apply(a, b, coef, mask))
    if rows % 7 == 0:
        keep = (torch.arange(rows // 7, device="cuda") % 3).float() * 0.75
        _compare(hook, lambda: _bwd_apply(a, b, coef, False, keep, 7))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("rows,c", RESNET + RAGGED)
def test_apply_batched_is_bit_identical(hook, rows, c, dtype):
    y, res, coef = _inputs(rows, c, dtype, 6)
    modes = ["plain", "relu", "res", "res_relu", "res_affine", "inplace", "inplace_res"]
    if rows % 7 == 0:
        modes += ["rs", "rs_res"]
    for mode in modes:
        _compare(hook, lambda: _apply(y, res, coef, mode))


def test_batched_passes_beside_a_resident_weight_gradient(hook):
    """the same comparison while a 14 x 14 x 256 weight gradient occupies every CU from a second stream"""
    from frhip import ops
    rows, c = 512 * 14 * 14, 256
    a, b, coef = _inputs(rows, c, torch.bfloat16, 7)
    hook(0)
    ref_bwd, ref_fwd = _bwd_apply(a, b, coef, True), _apply(a, b, coef, "res_relu")
    torch.cuda.synchronize()
    x = torch.randn((512, 14, 14, 256), device="cuda").to(torch.bfloat16)
    dy = torch.randn((512, 14, 14, 256), device="cuda").to(torch.bfloat16)
    dw = torch.zeros((256, 3, 3, 256), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    hook(1)
    for _ in range(2):
        started, done = torch.cuda.Event(), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            ops.conv_wgrad(dy, x, dw, 3, 3, 1, 1)
            started.record()
            for _ in range(12):
                ops.conv_wgrad(dy, x, dw, 3, 3, 1, 1)
            done.record()
        torch.cuda.current_stream().wait_event(started)
        got_bwd, got_fwd = _bwd_apply(a, b, coef, True), _apply(a, b, coef, "res_relu")
        mine = torch.cuda.Event(enable_timing=True)
        mine.record()
        torch.cuda.synchronize()
        assert mine.elapsed_time(done) > 0, "the weight gradients ended before the passes did: nothing was resident beside them"
        assert torch.equal(_bits(got_bwd), _bits(ref_bwd)) and torch.equal(_bits(got_fwd), _bits(ref_fwd))
