"""The hot launches of the two bench configurations besides ResNet50 -- Swin34 (bf16, B = 512, 112 x 112) and AlterNet50 (bf16,
B = 256, 192 x 192) -- against float64, at the shapes those steps really launch.

The census test records every distinct launch of one training-mode forward + backward pass of each network and holds it to the committed
lists SWIN34_LAUNCHES / ALTERNET50_LAUNCHES, so that a change to a network or to the dispatch forces this file to follow.  Every committed
signature has a float64 check here at that exact shape (CHECKED_BY names it per entry point); none of them is one of the B = 512 ResNet50
convolutions tests/test_poisoned_kernels_gpu.py already checks.

Bounds are per element, never a fraction of the tensor maximum.  With u = 2^-24 (fp32) and h(x) = 2^-8 |x| (half a bf16 step of x):
  * every bf16 rounding the kernel performs on the way to a stored value costs h() of that value;
  * an fp32 accumulation over K products costs acc(K) = 2^-23 sqrt(K) * sum |a b|, the sum of magnitudes formed in float64 beside the
    reference (sqrt(K): the worst-case K u is vacuous at K = 100 352);
  * a partial sum over the rows of one 256-row tile costs 258 u * sum |term| (the worst case: the tiles are short);
  * an intermediate the kernel rounds to bf16 whose rounding may come out the other way than the reference's (it lies within the
    kernel's fp32 error of a rounding boundary) costs one bf16 step of itself, carried through the products it enters;
  * an attention probability below the smallest normal fp32 number (a key behind the -100 shift mask) may come out as 0: 2^-126, absolute.
Each test's docstring states the bound it applies.  The negative controls at the end show that these bounds reject plausible defects."""
import inspect
import math
import types

import pytest
import torch

from ref64 import ref_conv, ref_dgrad, ref_wgrad, window_index

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
U32 = 2.0 ** -24
HALF = 2.0 ** -8
GELU_VALUE, GELU_SLOPE = 3.5e-4, 6.8e-4          # logistic GELU against the erf form (test_bf16_gelu_pair_stays_within_...)


def _ops():
    from frhip import ops
    return ops


def _lib():
    from frhip._abi import lib
    return lib()


def rnd(seed, shape, std=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, generator=g, device="cuda") * std


# ================================================================================================ A. launch census
CENSUS_ENTRIES = ("linear_fwd", "linear_dgrad_gelu", "gemm_nt", "gemm_tn", "conv_fwd", "conv_fwd_bnrelu", "conv_dgrad", "conv_wgrad",
                  "conv_wgrad_bnrelu", "winattn_fwd", "winattn_bwd")


def _dt(t):
    return "bf16" if t.dtype == BF else "fp32"


def signature(name, a):
    """one launch of frhip.ops.<name> with bound arguments `a` -> a hashable tuple of its shapes and flags"""
    if name == "linear_fwd":
        m, k = a["a"].shape
        return (name, _dt(a["a"]), m, a["w"].shape[0], k, a["bias"] is not None, bool(a["want_act"]), bool(a["want_stats"]))
    if name == "linear_dgrad_gelu":
        m, k = a["dy"].shape
        return (name, _dt(a["dy"]), m, a["wt"].shape[0], k, bool(a["want_colsum"]), a["colsum_into"] is not None)
    if name == "gemm_nt":
        m, k = a["a"].shape
        return (name, _dt(a["a"]), m, a["b"].shape[0], k, int(a["splits"]), bool(a["atomic_f32"]))
    if name == "gemm_tn":
        m, ldp = a["p"].shape
        return (name, _dt(a["p"]), m, ldp if a["kc"] is None else int(a["kc"]), ldp, a["q"].shape[1], int(a["splits"]), bool(a["overwrite"]))
    if name in ("conv_fwd", "conv_fwd_bnrelu"):
        n, h, w, c = a["x"].shape
        k, r, s, _ = a["w"].shape
        sig = (name, _dt(a["x"]), n, h, w, c, k, r, s, int(a["stride"]), int(a["pad"]), bool(a["want_stats"]))
        return sig + ((a["act_out"] is not None,) if name == "conv_fwd_bnrelu" else ())
    if name == "conv_dgrad":
        n, h, w, c = a["x_shape"]
        br = a["bnred"]
        bn = "-" if br is None else ("bn+relu" if bool(br[2]) else "bn")
        rs = int(br[4]) if br is not None and len(br) > 3 and br[3] is not None else 0       # rows per sample of the stochastic-depth factor
        return (name, _dt(a["dy"]), n, h, w, c, a["dy"].shape[3], int(a["r"]), int(a["s"]), int(a["stride"]), int(a["pad"]),
                a["residual"] is not None, int(a["residual_stride"]), bn, rs)
    if name in ("conv_wgrad", "conv_wgrad_bnrelu"):
        n, h, w, c = a["x"].shape
        return (name, _dt(a["x"]), n, h, w, c, a["dy"].shape[3], int(a["r"]), int(a["s"]), int(a["stride"]), int(a["pad"]), int(a["splits"]))
    if name in ("winattn_fwd", "winattn_bwd"):
        sig = (name, _dt(a["qkv"]), int(a["b"]), int(a["h"]), int(a["w"]), a["qkv"].shape[1] // 3, int(a["heads"]), int(a["ws"]),
               int(a["shift"]))
        if name == "winattn_bwd":
            sig += (bool(a["want_colsum"]), a["qv_grads"] is not None, a["dbias"] is not None)
        return sig
    raise KeyError(name)


def record_launches(network):
    """one training-mode forward + backward of the bf16 encoder at its bench size (stochastic depth as the product has it, a fixed upstream
    gradient), every call of the CENSUS_ENTRIES recorded -> set of signatures"""
    ops = _ops()
    seen = set()
    saved = {name: getattr(ops, name) for name in CENSUS_ENTRIES}

    def wrap(name, fn):
        sig_of = inspect.signature(fn)

        def call(*args, **kw):
            b = sig_of.bind(*args, **kw)
            b.apply_defaults()
            seen.add(signature(name, b.arguments))
            return fn(*args, **kw)
        return call

    if network == "Swin34":
        import nets.SwinV2 as mod
        batch, img = 512, 112
    else:
        import nets.AlterNet_SwinV2_FAN as mod
        batch, img = 256, 192
    try:
        for name, fn in saved.items():
            setattr(ops, name, wrap(name, fn))
        torch.manual_seed(1234)
        net = mod.Encoder(types.SimpleNamespace(network=network, emd_size=512, img_size=img, frhip_dtype="bf16", frhip_fp8=False)).cuda()
        net.train()
        gen = torch.Generator().manual_seed(1234)
        x = torch.randn((batch, 3, img, img), generator=gen).clamp_(-1, 1).cuda()
        y = net(x)
        y.backward((torch.randn(tuple(y.shape), generator=gen) * 0.05).cuda())
        torch.cuda.synchronize()
        del net, x, y
    finally:
        for name, fn in saved.items():
            setattr(ops, name, fn)
        torch.cuda.empty_cache()
    return seen


SWIN34_LAUNCHES = {
    ('conv_dgrad', 'bf16', 512, 14, 14, 256, 512, 2, 2, 2, 0, False, 1, '-', 0),
    ('conv_dgrad', 'bf16', 512, 28, 28, 128, 256, 2, 2, 2, 0, False, 1, '-', 0),
    ('conv_dgrad', 'bf16', 512, 56, 56, 64, 128, 2, 2, 2, 0, False, 1, 'bn+relu', 0),
    ('conv_dgrad', 'bf16', 25088, 1, 1, 512, 1536, 1, 1, 1, 0, True, 1, '-', 0),
    ('conv_dgrad', 'bf16', 25088, 1, 1, 512, 1536, 1, 1, 1, 0, True, 1, 'bn', 0),
    ('conv_dgrad', 'bf16', 25088, 1, 1, 512, 2048, 1, 1, 1, 0, True, 1, 'bn', 0),
    ('conv_dgrad', 'bf16', 100352, 1, 1, 256, 768, 1, 1, 1, 0, True, 1, '-', 0),
    ('conv_dgrad', 'bf16', 100352, 1, 1, 256, 768, 1, 1, 1, 0, True, 1, 'bn', 0),
    ('conv_dgrad', 'bf16', 100352, 1, 1, 256, 1024, 1, 1, 1, 0, True, 1, 'bn', 0),
    ('conv_fwd', 'bf16', 512, 14, 14, 256, 512, 2, 2, 2, 0, False),
    ('conv_fwd', 'bf16', 512, 28, 28, 128, 256, 2, 2, 2, 0, False),
    ('conv_fwd', 'bf16', 512, 56, 56, 64, 128, 2, 2, 2, 0, False),
    ('conv_wgrad', 'bf16', 512, 14, 14, 256, 512, 2, 2, 2, 0, 0),
    ('conv_wgrad', 'bf16', 512, 28, 28, 128, 256, 2, 2, 2, 0, 0),
    ('conv_wgrad', 'bf16', 512, 56, 56, 64, 128, 2, 2, 2, 0, 0),
    ('gemm_nt', 'bf16', 512, 25088, 512, 1, False),
    ('gemm_nt', 'bf16', 25088, 512, 512, 1, False),
    ('gemm_nt', 'bf16', 100352, 256, 256, 1, False),
    ('gemm_tn', 'bf16', 512, 512, 512, 25088, 0, True),
    ('gemm_tn', 'bf16', 25088, 512, 512, 512, 0, False),
    ('gemm_tn', 'bf16', 25088, 512, 512, 2048, 0, False),
    ('gemm_tn', 'bf16', 25088, 1536, 1536, 512, 0, False),
    ('gemm_tn', 'bf16', 25088, 2048, 2048, 512, 0, False),
    ('gemm_tn', 'bf16', 100352, 256, 256, 256, 0, False),
    ('gemm_tn', 'bf16', 100352, 256, 256, 1024, 0, False),
    ('gemm_tn', 'bf16', 100352, 768, 768, 256, 0, False),
    ('gemm_tn', 'bf16', 100352, 1024, 1024, 256, 0, False),
    ('linear_dgrad_gelu', 'bf16', 25088, 2048, 512, True, True),
    ('linear_dgrad_gelu', 'bf16', 100352, 1024, 256, True, True),
    ('linear_fwd', 'bf16', 25088, 512, 512, True, False, True),
    ('linear_fwd', 'bf16', 25088, 512, 2048, True, False, True),
    ('linear_fwd', 'bf16', 25088, 1536, 512, True, False, False),
    ('linear_fwd', 'bf16', 25088, 2048, 512, True, True, False),
    ('linear_fwd', 'bf16', 100352, 256, 256, True, False, True),
    ('linear_fwd', 'bf16', 100352, 256, 1024, True, False, True),
    ('linear_fwd', 'bf16', 100352, 768, 256, True, False, False),
    ('linear_fwd', 'bf16', 100352, 1024, 256, True, True, False),
    ('winattn_bwd', 'bf16', 512, 7, 7, 512, 16, 7, 0, True, True, True),
    ('winattn_bwd', 'bf16', 512, 14, 14, 256, 8, 7, 0, True, True, True),
    ('winattn_fwd', 'bf16', 512, 7, 7, 512, 16, 7, 0),
    ('winattn_fwd', 'bf16', 512, 14, 14, 256, 8, 7, 0),
}
ALTERNET50_LAUNCHES = {
    ('conv_dgrad', 'bf16', 256, 6, 6, 256, 512, 1, 1, 1, 0, False, 1, '-', 0),
    ('conv_dgrad', 'bf16', 256, 6, 6, 512, 512, 3, 3, 1, 1, False, 1, 'bn+relu', 0),
    ('conv_dgrad', 'bf16', 256, 6, 6, 512, 512, 3, 3, 1, 1, True, 1, 'bn', 0),
    ('conv_dgrad', 'bf16', 256, 12, 12, 128, 256, 1, 1, 1, 0, False, 1, '-', 0),
    ('conv_dgrad', 'bf16', 256, 12, 12, 256, 256, 3, 3, 1, 1, False, 1, 'bn+relu', 0),
    ('conv_dgrad', 'bf16', 256, 12, 12, 256, 256, 3, 3, 1, 1, True, 1, 'bn', 0),
    ('conv_dgrad', 'bf16', 256, 12, 12, 256, 256, 3, 3, 1, 1, True, 1, 'bn', 144),
    ('conv_dgrad', 'bf16', 256, 12, 12, 256, 256, 3, 3, 1, 1, True, 2, 'bn', 144),
    ('conv_dgrad', 'bf16', 256, 12, 12, 256, 512, 3, 3, 2, 1, False, 1, 'bn+relu', 0),
    ('conv_dgrad', 'bf16', 256, 24, 24, 64, 128, 1, 1, 1, 0, False, 1, '-', 0),
    ('conv_dgrad', 'bf16', 256, 24, 24, 128, 128, 3, 3, 1, 1, False, 1, 'bn+relu', 0),
    ('conv_dgrad', 'bf16', 256, 24, 24, 128, 128, 3, 3, 1, 1, True, 1, 'bn', 0),
    ('conv_dgrad', 'bf16', 256, 24, 24, 128, 128, 3, 3, 1, 1, True, 2, 'bn', 576),
    ('conv_dgrad', 'bf16', 256, 24, 24, 128, 256, 3, 3, 2, 1, False, 1, 'bn+relu', 0),
    ('conv_dgrad', 'bf16', 256, 48, 48, 64, 64, 3, 3, 1, 1, False, 1, 'bn+relu', 0),
    ('conv_dgrad', 'bf16', 256, 48, 48, 64, 64, 3, 3, 1, 1, True, 1, '-', 0),
    ('conv_dgrad', 'bf16', 256, 48, 48, 64, 64, 3, 3, 1, 1, True, 1, 'bn', 0),
    ('conv_dgrad', 'bf16', 256, 48, 48, 64, 64, 3, 3, 1, 1, True, 2, 'bn', 0),
    ('conv_dgrad', 'bf16', 256, 48, 48, 64, 128, 3, 3, 2, 1, False, 1, 'bn+relu', 0),
    ('conv_dgrad', 'bf16', 9216, 1, 1, 512, 1536, 1, 1, 1, 0, True, 1, 'bn', 0),
    ('conv_dgrad', 'bf16', 9216, 1, 1, 512, 1536, 1, 1, 1, 0, True, 1, 'bn', 36),
    ('conv_dgrad', 'bf16', 36864, 1, 1, 256, 768, 1, 1, 1, 0, True, 1, 'bn', 0),
    ('conv_dgrad', 'bf16', 36864, 1, 1, 256, 768, 1, 1, 1, 0, True, 1, 'bn', 144),
    ('conv_dgrad', 'bf16', 147456, 1, 1, 128, 384, 1, 1, 1, 0, True, 1, 'bn', 0),
    ('conv_dgrad', 'bf16', 147456, 1, 1, 128, 384, 1, 1, 1, 0, True, 1, 'bn', 576),
    ('conv_fwd', 'bf16', 256, 6, 6, 512, 512, 3, 3, 1, 1, True),
    ('conv_fwd', 'bf16', 256, 12, 12, 256, 256, 3, 3, 1, 1, True),
    ('conv_fwd', 'bf16', 256, 12, 12, 256, 512, 1, 1, 2, 0, True),
    ('conv_fwd', 'bf16', 256, 12, 12, 256, 512, 3, 3, 2, 1, True),
    ('conv_fwd', 'bf16', 256, 24, 24, 128, 128, 3, 3, 1, 1, True),
    ('conv_fwd', 'bf16', 256, 24, 24, 128, 256, 1, 1, 2, 0, True),
    ('conv_fwd', 'bf16', 256, 24, 24, 128, 256, 3, 3, 2, 1, True),
    ('conv_fwd', 'bf16', 256, 48, 48, 64, 64, 3, 3, 1, 1, True),
    ('conv_fwd', 'bf16', 256, 48, 48, 64, 128, 1, 1, 2, 0, True),
    ('conv_fwd', 'bf16', 256, 48, 48, 64, 128, 3, 3, 2, 1, True),
    ('conv_fwd', 'bf16', 2359296, 1, 1, 64, 64, 1, 1, 1, 0, True),
    ('conv_fwd_bnrelu', 'bf16', 256, 6, 6, 512, 512, 3, 3, 1, 1, True, True),
    ('conv_fwd_bnrelu', 'bf16', 256, 12, 12, 256, 256, 3, 3, 1, 1, True, True),
    ('conv_fwd_bnrelu', 'bf16', 256, 24, 24, 128, 128, 3, 3, 1, 1, True, True),
    ('conv_fwd_bnrelu', 'bf16', 256, 48, 48, 64, 64, 3, 3, 1, 1, True, True),
    ('conv_wgrad', 'bf16', 256, 6, 6, 512, 512, 3, 3, 1, 1, 0),
    ('conv_wgrad', 'bf16', 256, 12, 12, 256, 256, 3, 3, 1, 1, 0),
    ('conv_wgrad', 'bf16', 256, 12, 12, 256, 512, 1, 1, 2, 0, 0),
    ('conv_wgrad', 'bf16', 256, 12, 12, 256, 512, 3, 3, 2, 1, 0),
    ('conv_wgrad', 'bf16', 256, 24, 24, 128, 128, 3, 3, 1, 1, 0),
    ('conv_wgrad', 'bf16', 256, 24, 24, 128, 256, 1, 1, 2, 0, 0),
    ('conv_wgrad', 'bf16', 256, 24, 24, 128, 256, 3, 3, 2, 1, 0),
    ('conv_wgrad', 'bf16', 256, 48, 48, 64, 64, 3, 3, 1, 1, 0),
    ('conv_wgrad', 'bf16', 256, 48, 48, 64, 128, 1, 1, 2, 0, 0),
    ('conv_wgrad', 'bf16', 256, 48, 48, 64, 128, 3, 3, 2, 1, 0),
    ('conv_wgrad', 'bf16', 2359296, 1, 1, 64, 64, 1, 1, 1, 0, 0),
    ('gemm_nt', 'bf16', 256, 18432, 512, 1, False),
    ('gemm_nt', 'bf16', 9216, 512, 512, 1, False),
    ('gemm_nt', 'bf16', 36864, 256, 256, 1, False),
    ('gemm_nt', 'bf16', 147456, 128, 128, 1, False),
    ('gemm_tn', 'bf16', 256, 512, 512, 18432, 0, True),
    ('gemm_tn', 'bf16', 9216, 512, 512, 512, 0, False),
    ('gemm_tn', 'bf16', 9216, 1536, 1536, 512, 0, False),
    ('gemm_tn', 'bf16', 36864, 256, 256, 256, 0, False),
    ('gemm_tn', 'bf16', 36864, 768, 768, 256, 0, False),
    ('gemm_tn', 'bf16', 147456, 128, 128, 128, 0, False),
    ('gemm_tn', 'bf16', 147456, 384, 384, 128, 0, False),
    ('linear_fwd', 'bf16', 9216, 512, 512, True, False, True),
    ('linear_fwd', 'bf16', 9216, 1536, 512, True, False, False),
    ('linear_fwd', 'bf16', 36864, 256, 256, True, False, True),
    ('linear_fwd', 'bf16', 36864, 768, 256, True, False, False),
    ('linear_fwd', 'bf16', 147456, 128, 128, True, False, True),
    ('linear_fwd', 'bf16', 147456, 384, 128, True, False, False),
    ('winattn_bwd', 'bf16', 256, 6, 6, 512, 16, 3, 0, True, True, True),
    ('winattn_bwd', 'bf16', 256, 6, 6, 512, 16, 3, 1, True, True, True),
    ('winattn_bwd', 'bf16', 256, 12, 12, 256, 8, 6, 0, True, True, True),
    ('winattn_bwd', 'bf16', 256, 12, 12, 256, 8, 6, 3, True, True, True),
    ('winattn_bwd', 'bf16', 256, 24, 24, 128, 4, 6, 0, True, True, True),
    ('winattn_bwd', 'bf16', 256, 24, 24, 128, 4, 6, 3, True, True, True),
    ('winattn_fwd', 'bf16', 256, 6, 6, 512, 16, 3, 0),
    ('winattn_fwd', 'bf16', 256, 6, 6, 512, 16, 3, 1),
    ('winattn_fwd', 'bf16', 256, 12, 12, 256, 8, 6, 0),
    ('winattn_fwd', 'bf16', 256, 12, 12, 256, 8, 6, 3),
    ('winattn_fwd', 'bf16', 256, 24, 24, 128, 4, 6, 0),
    ('winattn_fwd', 'bf16', 256, 24, 24, 128, 4, 6, 3),
}


def test_launch_census_matches_the_committed_lists():
    """the launches of one bf16 Swin34 (B = 512) and one bf16 AlterNet50 (B = 256, 192 x 192, fp8 off) training step are exactly the
    committed lists, and every one of them has a float64 check below"""
    got = {"Swin34": record_launches("Swin34"), "AlterNet50": record_launches("AlterNet50")}
    for net, want in (("Swin34", SWIN34_LAUNCHES), ("AlterNet50", ALTERNET50_LAUNCHES)):
        assert got[net] == want, "%s: launches not in the committed list %r; committed but not launched %r" % (
            net, sorted(got[net] - want), sorted(want - got[net]))
    for sig in SWIN34_LAUNCHES | ALTERNET50_LAUNCHES:
        # every entry point has its float64 check; the attention backward runs in the form check_winattn exercises (column sums fused,
        # q / v bias gradients and d(bias) / d(scale) accumulated in place)
        assert sig[0] in CHECKS or sig[0] in ("winattn_fwd", "winattn_bwd"), sig
        if sig[0] == "winattn_bwd":
            assert sig[9:] == (True, True, True), sig


# ================================================================================================ per-element bounds
def ulp(x):
    """one bf16 step at |x| (float64): 2^(e - 8) for |x| in [2^(e-1), 2^e), 0 at 0"""
    _, e = torch.frexp(x.abs())
    return torch.ldexp(torch.ones_like(x), e - 8) * (x != 0)


def rb(x):
    """round a float64 tensor to bf16 (through fp32, as the kernels' fp32 values are) and back"""
    return x.float().to(BF).double()


def may_flip(x, d):
    """the bf16 rounding of a value known to within +-d of x can come out either way"""
    return rb(x - d) != rb(x + d)


def acc(mag, k):
    """fp32 accumulation of k products whose magnitudes sum to mag"""
    return 2.0 ** -23 * math.sqrt(k) * mag


def violations(got, ref, bound):
    """number of elements outside their bound (NaN counts)"""
    err = (got.double() - ref).abs()
    return int((~(err <= bound)).sum())


def within(got, ref, bound, what):
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    nbad = int(bad.sum())
    if nbad:
        i = int(torch.argmax(torch.where(bad, (err - bound).nan_to_num(float("inf")), torch.zeros_like(err))).item())
        f = lambda t: float(t.reshape(-1)[i])
        raise AssertionError("%s: %d of %d elements outside their bound; worst at flat index %d: got %.6g, float64 %.6g, bound %.3g"
                             % (what, nbad, err.numel(), i, f(got.double()), f(ref), f(bound)))


def tile_rows(m):
    return (m + 255) // 256


def assert_256_row_tile(m, n, k):
    """the automatic dispatch puts this linear on the 256 x 256 tile (its BatchNorm partial buffer has one row per 256 output rows)"""
    assert n % 256 == 0
    assert _lib().frhip_conv_stat_rows(0, m, n, 1, 1, k, 1, 1, 1, 0) == tile_rows(m), (m, n, k)


def partial_bound(terms_abs, rows=256):
    """column sums over per-tile partials: rows u per tile (sequential worst case) + 2 u for the tile sums and the store"""
    return (rows + 2) * U32 * terms_abs.sum(0)


def check_partials(part, terms, terms_abs, what, extra=None):
    """part [tiles, 2, n] fp32 against float64 column sums of terms = (t0 [rows, n], t1 [rows, n])"""
    s = part.double().sum(0)
    for j in (0, 1):
        bound = partial_bound(terms_abs[j]) + (extra[j] if extra is not None else 0.0)
        within(s[j], terms[j].sum(0), bound, "%s: partial sum %d" % (what, j))


def gelu64(x):
    return x * 0.5 * (1 + torch.erf(x / math.sqrt(2)))


def gelu_slope64(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-x * x / 2) / math.sqrt(2 * math.pi)


# ================================================================================================ B. the linear family
def _linear_operands(m, n, k, seed):
    a = rnd(seed, (m, k)).to(BF)
    w = (rnd(seed + 1, (n, k)) / math.sqrt(k)).to(BF)
    return a, w


def _gemm64(a, w):
    """float64 a @ w^T and sum |a| |w|^T (rows chunked)"""
    ref = torch.empty((a.shape[0], w.shape[0]), dtype=torch.float64, device="cuda")
    mag = torch.empty_like(ref)
    wd = w.double()
    for i in range(0, a.shape[0], 32768):
        ad = a[i:i + 32768].double()
        ref[i:i + 32768] = ad @ wd.t()
        mag[i:i + 32768] = ad.abs() @ wd.abs().t()
    return ref, mag


def linear_fwd_bounds(a, w, bias, want_act):
    """float64 (out, bound) of frhip_linear_fwd: out = bf16(bf16(a w^T) + bias) -> h(acc) + h(out) + acc(K)"""
    k = a.shape[1]
    g, mag = _gemm64(a, w)
    e = acc(mag, k)
    ref = g + (bias.double() if bias is not None else 0.0)
    bound = HALF * (g.abs() + e) + e
    if bias is not None:
        bound = bound + HALF * (ref.abs() + bound)
    return ref, bound


def check_linear_fwd(sig, seed=11):
    """frhip_linear_fwd at a census shape.  out: h(a w^T) + h(out) + acc(K) (two roundings with a bias: the tile is staged in bf16, then
    biased); GELU output against the exact erf form of the STORED out: 3.5e-4 + h(act) + 1.13 h(out) (the GELU input may be the value before
    its last rounding); BatchNorm partials against float64 sums of the stored out: 258 u sum |term| per column."""
    ops = _ops()
    _, _, m, n, k, has_bias, want_act, want_stats = sig
    a, w = _linear_operands(m, n, k, seed)
    bias = rnd(seed + 2, (n,)) * 0.5 if has_bias else None
    out, act, part = ops.linear_fwd(a, w, bias, want_act=want_act, want_stats=want_stats)
    ref, bound = linear_fwd_bounds(a, w, bias, want_act)
    within(out, ref, bound, "linear_fwd out %r" % (sig,))
    o = out.double()
    if want_act:
        ga = gelu64(o)
        within(act, ga, GELU_VALUE + HALF * (ga.abs() + GELU_VALUE) + 1.13 * HALF * o.abs(), "linear_fwd gelu %r" % (sig,))
    if want_stats:
        check_partials(part, (o, o * o), (o.abs(), o * o), "linear_fwd stats %r" % (sig,))
    if n % 256 == 0 and m >= 256 * 64:
        assert_256_row_tile(m, n, k)
        if want_stats:
            assert part.shape[0] == tile_rows(m)
    return out, ref, bound


def gemm_nt_bounds(a, b):
    g, mag = _gemm64(a, b)
    e = acc(mag, a.shape[1])
    return g, HALF * (g.abs() + e) + e


def check_gemm_nt(sig, seed=21):
    """frhip_gemm_nt (bf16 out, one K split): h(out) + acc(K)"""
    ops = _ops()
    _, _, m, n, k, splits, atomic = sig
    a, b = _linear_operands(m, n, k, seed)
    out = ops.gemm_nt(a, b, splits=splits, atomic_f32=atomic)
    ref, bound = gemm_nt_bounds(a, b)
    within(out, ref, bound, "gemm_nt %r" % (sig,))
    if n % 256 == 0 and m >= 256 * 64:
        assert_256_row_tile(m, n, k)
    return out, ref, bound


def linear_dgrad_gelu_bounds(dy, wt, pre):
    """dx = bf16(bf16(dy wt^T) * gelu'(pre)), kernel slope logistic: h(dx) + |slope| (h(acc) + acc(K)) + 6.8e-4 |acc|"""
    g, mag = _gemm64(dy, wt)
    e = acc(mag, dy.shape[1])
    sl = gelu_slope64(pre.double())
    ref = g * sl
    bound = sl.abs() * (HALF * (g.abs() + e) + e) + GELU_SLOPE * (g.abs() + e)
    return ref, bound + HALF * (ref.abs() + bound)


def check_linear_dgrad_gelu(sig, seed=31):
    """frhip_linear_dgrad_gelu: dx within h(dx) + |gelu'| (h(acc) + acc(K)) + 6.8e-4 |acc| of acc * exact-erf gelu'(pre); the column sums
    ADDED into a non-zero fp32 accumulator (as nets.SwinV2 does into the fc1.bias gradient) within (258 + tiles) u sum |dx| + 2 u |sum|
    of the float64 sums of the STORED dx"""
    ops = _ops()
    _, _, m, n, k, want_colsum, into = sig
    dy, wt = _linear_operands(m, n, k, seed)
    pre = (rnd(seed + 2, (m, n)) * 1.5).to(BF)
    acc0 = rnd(seed + 3, (n,)) if into else None
    dx, colsum = ops.linear_dgrad_gelu(dy, wt, pre, want_colsum=want_colsum, colsum_into=acc0.clone() if into else None)
    ref, bound = linear_dgrad_gelu_bounds(dy, wt, pre)
    within(dx, ref, bound, "linear_dgrad_gelu dx %r" % (sig,))
    if want_colsum:
        d = dx.double()
        want = d.sum(0) + (acc0.double() if into else 0.0)
        b = (258 + tile_rows(m)) * U32 * d.abs().sum(0) + 2 * U32 * want.abs()
        within(colsum, want, b, "linear_dgrad_gelu column sums %r" % (sig,))
    if n % 256 == 0 and m >= 256 * 64:
        assert_256_row_tile(m, n, k)
    return dx, ref, bound


def gemm_tn_bounds(p, q, acc0):
    """out[kc][c] = acc0 + sum_m p[m][kc] q[m][c] in fp32: acc(M) + 4 u (|out| + |acc0|)"""
    ref = acc0.double().clone()
    mag = torch.zeros_like(ref)
    for i in range(0, p.shape[0], 32768):
        pd, qd = p[i:i + 32768].double(), q[i:i + 32768].double()
        ref += pd.t() @ qd
        mag += pd.abs().t() @ qd.abs()
    return ref, acc(mag, p.shape[0]) + 4 * U32 * (ref.abs() + acc0.double().abs())


def check_gemm_tn(sig, seed=41):
    """frhip_gemm_tn weight gradient added into a NON-ZERO accumulator (overwrite launches: into NaN, the accumulator plays no part):
    acc(M) + 4 u (|out| + |acc0|)"""
    ops = _ops()
    _, _, m, kc, ldp, c, splits, overwrite = sig
    p = rnd(seed, (m, ldp)).to(BF)
    q = (rnd(seed + 1, (m, c)) * 0.1).to(BF)
    if overwrite:
        out = torch.full((kc, c), float("nan"), device="cuda")
        acc0 = torch.zeros((kc, c), device="cuda")
    else:
        acc0 = rnd(seed + 2, (kc, c))
        out = acc0.clone()
    ops.gemm_tn(p, q, out, kc=kc, splits=splits, overwrite=overwrite)
    ref, bound = gemm_tn_bounds(p[:, :kc], q, acc0)
    within(out, ref, bound, "gemm_tn %r" % (sig,))
    return out, ref, bound


# ================================================================================================ C. convolutions
def _chunk(n, ho, wo, ckk):
    """images per chunk of the float64 references: about 2^25 unfolded elements"""
    return max(1, min(n, (1 << 25) // max(1, ho * wo * ckk)))


def _conv_operands(sig, seed):
    n, h, w, c, k, r, s = sig[2:9]
    x = rnd(seed, (n, h, w, c)).to(BF)
    wt = (rnd(seed + 1, (k, r, s, c)) / math.sqrt(r * s * c)).to(BF)
    return x, wt


def conv_fwd_bounds(x, wt, stride, pad):
    n, h, w, c = x.shape
    k, r, s, _ = wt.shape
    ho, wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1
    ch = _chunk(n, ho, wo, c * r * s)
    ref = ref_conv(x, wt, stride, pad, chunk=ch)
    e = acc(ref_conv(x.abs(), wt.abs(), stride, pad, chunk=ch), r * s * c)
    return ref, HALF * (ref.abs() + e) + e


def _rows_per_partial(m, part):
    return max(256, -(-m // part.shape[0]))


def check_conv_fwd(sig, seed=51):
    """frhip_conv_fwd: y = bf16(conv) within h(y) + acc(R S C); the BatchNorm partials within 258 u sum |term| of float64 sums over the
    STORED y (rows per partial: M / partial rows, at least 256)"""
    ops = _ops()
    _, _, n, h, w, c, k, r, s, stride, pad, want_stats = sig
    x, wt = _conv_operands(sig, seed)
    y, part = ops.conv_fwd(x, wt, stride, pad, want_stats=want_stats)
    ref, bound = conv_fwd_bounds(x, wt, stride, pad)
    within(y, ref, bound, "conv_fwd %r" % (sig,))
    if want_stats:
        yy = y.double().reshape(-1, k)
        rows = _rows_per_partial(yy.shape[0], part)
        s_ = part.double().sum(0)
        for j, t in enumerate((yy, yy * yy)):
            within(s_[j], t.sum(0), (rows + 2) * U32 * t.abs().sum(0), "conv_fwd stats %d %r" % (j, sig))
    return y, ref, bound


def check_conv_fwd_bnrelu(sig, seed=61):
    """frhip_conv_fwd_bnrelu: the activated operand it writes out within one bf16 step of relu(x scale + shift) (fp32 FMA or not: the
    rounding may flip); y within h(y) + acc(R S C) of the float64 convolution of that operand; partials as check_conv_fwd"""
    ops = _ops()
    _, _, n, h, w, c, k, r, s, stride, pad, want_stats, want_act = sig
    x, wt = _conv_operands(sig, seed)
    x = (x.float() * 0.8 + 0.3).to(BF)
    rows = n * h * w
    st = ops.bn_finalize(ops.colstats(x.view(rows, c)), rows, 1 + 0.1 * rnd(seed + 2, (c,)), 0.1 * rnd(seed + 3, (c,)), None, None)
    act = torch.empty_like(x) if want_act else None
    y, part = ops.conv_fwd_bnrelu(x, st, wt, stride, pad, want_stats=want_stats, act_out=act)
    a64 = (x.double() * st.scale.double() + st.shift.double()).clamp_min(0)
    within(act, a64, 2 * HALF * a64.abs() + 2.0 ** -20 * ((x.double() * st.scale.double()).abs() + st.shift.double().abs()),
           "conv_fwd_bnrelu activation %r" % (sig,))
    ref, bound = conv_fwd_bounds(act, wt, stride, pad)
    within(y, ref, bound, "conv_fwd_bnrelu %r" % (sig,))
    if want_stats:
        yy = y.double().reshape(-1, k)
        rr = _rows_per_partial(yy.shape[0], part)
        s_ = part.double().sum(0)
        for j, t in enumerate((yy, yy * yy)):
            within(s_[j], t.sum(0), (rr + 2) * U32 * t.abs().sum(0), "conv_fwd_bnrelu stats %d %r" % (j, sig))
    return y, ref, bound


def dgrad_bounds(dy, wt, x_shape, stride, pad, res=None, residual_stride=1):
    n, h, w, c = x_shape
    k, r, s, _ = wt.shape
    ch = _chunk(n, h, w, c * r * s)
    g = ref_dgrad(dy, wt, x_shape, stride, pad, chunk=ch)
    e = acc(ref_dgrad(dy.abs(), wt.abs(), x_shape, stride, pad, chunk=ch), k * r * s)
    bound = HALF * (g.abs() + e) + e
    ref = g
    if res is not None:
        ref = g.clone()
        if residual_stride == 1:
            ref += res.double()
        else:
            ref[:, ::2, ::2, :] += res.double()
        bound = bound + HALF * (ref.abs() + bound)
    return ref, bound


def check_conv_dgrad(sig, seed=71):
    """frhip_conv_dgrad[_fused[_rs]] at a census shape.  dx = bf16(bf16(dy * w) + residual): h(acc) + h(dx) + acc(K R S) (one rounding
    less without a residual).  BatchNorm-backward partials (sum d, sum d xhat) with d the STORED dx through the ReLU mask (formed in fp32 as
    the kernels form it) and the per-sample stochastic-depth factor: 258 u per tile times sum |d| and sum |d xhat| + invstd (sum |d y| +
    |mean| sum |d|) -- the lean epilogue forms sum d xhat as invstd (sum d y - mean sum d)"""
    ops = _ops()
    _, _, n, h, w, c, k, r, s, stride, pad, has_res, rstride, bn, rows_per = sig
    ho, wo = ops.conv_out_hw(h, w, r, s, stride, pad)
    wt = (rnd(seed, (k, r, s, c)) / math.sqrt(r * s * k)).to(BF)
    dy = rnd(seed + 1, (n, ho, wo, k)).to(BF)
    wpack = ops.pack_wt(wt.float(), BF)
    res = None
    if has_res:
        res = rnd(seed + 2, (n, h, w, c) if rstride == 1 else (n, (h + 1) // 2, (w + 1) // 2, c)).to(BF)
    rows = n * h * w
    bnred = None
    if bn != "-":
        y_bn = (rnd(seed + 3, (n, h, w, c)) * 0.8 + 0.5).to(BF)
        st = ops.bn_finalize(ops.colstats(y_bn.view(rows, c)), rows, 1 + 0.1 * rnd(seed + 4, (c,)), 0.1 * rnd(seed + 5, (c,)), None, None)
        bnred = (y_bn, st, bn == "bn+relu")
        if rows_per:
            kp = 0.9
            keep = ((torch.rand(rows // rows_per, generator=torch.Generator().manual_seed(seed + 6)) < 0.6).float() / kp).cuda()
            bnred = bnred + (keep, rows_per, 1.0 / kp)
    got = ops.conv_dgrad(dy, wpack, (n, h, w, c), r, s, stride, pad, residual=res, bnred=bnred, residual_stride=rstride)
    dx, part = got if bnred is not None else (got, None)
    ref, bound = dgrad_bounds(dy, wt, (n, h, w, c), stride, pad, res, rstride)
    within(dx, ref, bound, "conv_dgrad %r" % (sig,))
    if bnred is not None:
        d = dx.double().reshape(rows, c)
        yb = y_bn.double().reshape(rows, c)
        if bn == "bn+relu":
            d = d * ((y_bn.float().reshape(rows, c) * st.scale + st.shift) > 0)
        if rows_per:
            d = d * keep.double().repeat_interleave(rows_per).view(rows, 1)
        mean, invstd = st.mean.double(), st.invstd.double()
        xh = (yb - mean) * invstd
        cancel = invstd * ((d * yb).abs().sum(0) + mean.abs() * d.abs().sum(0))
        rpp = _rows_per_partial(rows, part)
        s_ = part.double().sum(0)
        within(s_[0], d.sum(0), (rpp + 2) * U32 * d.abs().sum(0), "conv_dgrad BN-backward sum d %r" % (sig,))
        within(s_[1], (d * xh).sum(0), (rpp + 2) * U32 * ((d * xh).abs().sum(0) + cancel), "conv_dgrad BN-backward sum d xhat %r" % (sig,))
    if r == 1 and h == 1 and c % 256 == 0 and n >= 256 * 64:
        assert_256_row_tile(n, c, k)
    return dx, ref, bound


def check_conv_wgrad(sig, seed=81):
    """frhip_conv_wgrad into a caller-zeroed fp32 accumulator: acc(N Ho Wo) + 4 u |dw|"""
    ops = _ops()
    _, _, n, h, w, c, k, r, s, stride, pad, splits = sig
    ho, wo = ops.conv_out_hw(h, w, r, s, stride, pad)
    x = rnd(seed, (n, h, w, c)).to(BF)
    dy = (rnd(seed + 1, (n, ho, wo, k)) * 0.1).to(BF)
    dw = torch.zeros((k, r, s, c), device="cuda")
    ops.conv_wgrad(dy, x, dw, r, s, stride, pad, splits)
    ch = _chunk(n, ho, wo, c * r * s)
    ref = ref_wgrad(dy, x, r, s, stride, pad, chunk=ch)
    bound = acc(ref_wgrad(dy.abs(), x.abs(), r, s, stride, pad, chunk=ch), n * ho * wo) + 4 * U32 * ref.abs()
    within(dw, ref, bound, "conv_wgrad %r" % (sig,))
    return dw, ref, bound


# ================================================================================================ F. window attention (MFMA kernels)
def wm_chunks(nwin, heads, target_wgs):
    """csrc/winattn_mfma.hip wm_chunks: (chunks, windows per chunk)"""
    chunks = -(-target_wgs // heads)
    wpb = max(4, -(-nwin // chunks))
    return -(-nwin // wpb), wpb


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _normalised(x):
    """x^ = bf16(x / max(|x|, 1e-12)) and the deviation the kernel's x^ may have from it: one bf16 step where its fp32 value (2^-20 relative)
    may round the other way"""
    nrm = x.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)
    xn = x / nrm
    d = xn.abs() * 2.0 ** -20
    return rb(xn), 1.0 / nrm, may_flip(xn, d) * (ulp(xn) + d)


def attn_reference(qkv, dout, bias, scale, b, H, W, heads, ws, shift, use_mask=True):
    """float64 window attention written out by hand, with the bf16 roundings of the MFMA kernels (q^ / k^ after normalisation, P before
    P V, dS before the dq^ / dk^ products, the stored outputs) and per-element bounds.  Returns dict of (value, bound) pairs in the
    kernels' layouts; `dout` None: forward only."""
    C = qkv.shape[1] // 3
    n = ws * ws
    pix, region = window_index(b, H, W, ws, shift)
    if not use_mask:
        region = torch.zeros_like(region)
    nw = pix.shape[0]
    X = qkv[pix.reshape(-1)].view(nw, n, 3, heads, 32).permute(2, 0, 3, 1, 4).double()        # [3, nw, heads, n, 32]
    q, k, v = X[0], X[1], X[2]
    qh, qinv, fq = _normalised(q)
    kh, kinv, fk = _normalised(k)
    T = lambda t: t.transpose(-1, -2)
    cos = qh @ T(kh)                                                               # [nw, heads, i, j]
    dcos = fq @ T(kh.abs()) + qh.abs() @ T(fk) + 2.0 ** -19 * (qh.abs() @ T(kh.abs()))
    sc = scale.double().view(1, heads, 1, 1)
    masked = (region[:, None, :, None] != region[:, None, None, :]).double()
    bb = bias.double().view(1, heads, n, n)
    logit = cos * sc + bb - 100.0 * masked
    dl = sc * dcos + 2.0 ** -20 * ((cos * sc).abs() + bb.abs() + 100.0 * masked)
    P = torch.softmax(logit, -1)
    dP = P * (torch.expm1(dl + dl.amax(-1, keepdim=True)) + 2.0 ** -18)            # logit errors + the fp32 exp / sum / divide
    # fp32 underflow: a pair the shift mask separates in EVERY window of the map (maps one window wide or high) has P of order
    # e^-100 = 3.7e-44, below the smallest normal fp32 number 2^-126; the kernel's exponential returns 0 for it (at most 2^-126 lost,
    # the sum being >= 1), and the product P (dP - rd) may underflow the same way.  Relative terms cannot carry that: it is absolute.
    FLUSH = 2.0 ** -126
    dP = dP + FLUSH
    Pb = rb(P)
    tP = may_flip(P, dP) * (dP + ulp(P))                                            # the kernel's bf16 P may differ from Pb by this
    O = Pb @ v
    dO = tP @ v.abs() + 2.0 ** -19 * (Pb @ v.abs())
    res = {}

    def scatter(val, bnd, third=None):
        width = C if third is None else 3 * C
        vo = torch.empty((b * H * W, width), dtype=torch.float64, device="cuda")
        bo = torch.empty_like(vo)
        cols = slice(None) if third is None else slice(third * C, (third + 1) * C)
        vo[pix.reshape(-1), cols] = val.permute(0, 2, 1, 3).reshape(nw * n, C)
        bo[pix.reshape(-1), cols] = bnd.permute(0, 2, 1, 3).reshape(nw * n, C)
        return vo, bo

    res["out"] = scatter(O, dO + HALF * (O.abs() + dO))
    res["nwin"] = nw
    res["pix"] = pix
    if dout is None:
        return res
    G = dout[pix.reshape(-1)].view(nw, n, heads, 32).permute(0, 2, 1, 3).double()   # dO [nw, heads, i, 32]
    dPm = G @ T(v)                                                                  # dP[i][j] = <dO_i, v_j>
    ddP = 2.0 ** -19 * (G.abs() @ T(v.abs()))
    rd = (P * dPm).sum(-1, keepdim=True)
    drd = (dP * dPm.abs()).sum(-1, keepdim=True) + (P * ddP).sum(-1, keepdim=True) + 2.0 ** -19 * (P * dPm).abs().sum(-1, keepdim=True)
    dS = P * (dPm - rd)
    ddS = dP * (dPm - rd).abs() + P * (ddP + drd) + 2.0 ** -22 * dS.abs() + FLUSH
    chunks, wpb = wm_chunks(nw, heads, _cus())
    nacc = wpb + chunks + 8
    res["dbias"] = (dS.sum(0), ddS.sum(0) + nacc * U32 * dS.abs().sum(0))
    dsc = (dS * cos).sum((0, 2, 3))
    res["dscale"] = (dsc, (ddS * cos.abs() + dS.abs() * dcos).sum((0, 2, 3)) + (64 * wpb + chunks + 64) * U32 * (dS * cos).abs().sum((0, 2, 3)))
    dSb = rb(dS)
    tS = may_flip(dS, ddS) * (ddS + ulp(dS))
    dqh = dSb @ kh
    ddqh = tS @ kh.abs() + dSb.abs() @ fk + 2.0 ** -19 * (dSb.abs() @ kh.abs())
    dkh = T(dSb) @ qh
    ddkh = T(tS) @ qh.abs() + T(dSb.abs()) @ fq + 2.0 ** -19 * (T(dSb.abs()) @ qh.abs())
    dvv = T(Pb) @ G
    ddv = T(tP) @ G.abs() + 2.0 ** -19 * (T(Pb) @ G.abs())

    def unnormalise(dxh, ddxh, xh, fx, inv):
        """dx = inv (sc dx^ - x^ <sc dx^, x^>) (the kernel uses its bf16 x^ and its fp32 inv)"""
        dv = sc * dxh
        dot = (dv * xh).sum(-1, keepdim=True)
        r = (dv - xh * dot) * inv
        ddot = (sc * ddxh * xh.abs() + dv.abs() * fx).sum(-1, keepdim=True) + 2.0 ** -21 * (dv * xh).abs().sum(-1, keepdim=True)
        dr = inv * (sc * ddxh + fx * dot.abs() + xh.abs() * ddot) + 2.0 ** -20 * inv * (dv.abs() + (xh * dot).abs())
        return r, dr + HALF * (r.abs() + dr)

    dq, bq = unnormalise(dqh, ddqh, qh, fq, qinv)
    dk, bk = unnormalise(dkh, ddkh, kh, fk, kinv)
    dqkv = torch.empty((b * H * W, 3 * C), dtype=torch.float64, device="cuda")
    bqkv = torch.empty_like(dqkv)
    for t, (val, bnd) in enumerate(((dq, bq), (dk, bk), (dvv, ddv + HALF * (dvv.abs() + ddv)))):
        vo, bo = scatter(val, bnd, third=t)
        dqkv[:, t * C:(t + 1) * C] = vo[:, t * C:(t + 1) * C]
        bqkv[:, t * C:(t + 1) * C] = bo[:, t * C:(t + 1) * C]
    res["dqkv"] = (dqkv, bqkv)
    res["colsum_terms"] = n * wpb + chunks + 64
    return res


def _attn_inputs(b, H, W, C, heads, ws, seed):
    n = ws * ws
    qkv = rnd(seed, (b * H * W, 3 * C)).to(BF)
    bias = 16 * torch.sigmoid(rnd(seed + 1, (heads, n, n)))
    scale = 5 + 15 * torch.rand(heads, generator=torch.Generator().manual_seed(seed + 2)).cuda()     # exp(logit_scale) in [5, 20]
    dout = rnd(seed + 3, (b * H * W, C)).to(BF)
    return qkv, bias, scale, dout


def check_winattn(b, H, W, C, heads, ws, shift, seed=91, backward=True):
    """frhip_winattn_fwd / _bwd (MFMA kernels) against attn_reference.  out, dqkv: the stored value's h() + the deviations the kernel's
    bf16 q^, k^, P, dS may carry (one bf16 step where their rounding may flip, first-order propagation of the logit errors through the
    softmax) through the products they enter + 2^-19 sum |a b| per 32-product MFMA accumulation.  d(bias), d(scale): summed over ALL windows
    in float64, bounded by the summed per-window deviations + (windows per chunk + chunks) u sum |term|.  The product's accumulate form
    (d(bias), d(scale), the q / v bias gradients added into non-zero accumulators) and the fused [3C] column sums of the stored dqkv
    ((n windows per chunk + chunks + 64) u sum |dqkv|) are both checked; dqkv is the same bits in both."""
    ops = _ops()
    assert _lib().frhip_set_winattn_mfma(-1) == 1
    qkv, bias, scale, dout = _attn_inputs(b, H, W, C, heads, ws, seed)
    what = "winattn b=%d %dx%d C=%d heads=%d ws=%d shift=%d" % (b, H, W, C, heads, ws, shift)
    out = ops.winattn_fwd(qkv, bias, scale, b, H, W, heads, ws, shift)
    ref = attn_reference(qkv, dout if backward else None, bias, scale, b, H, W, heads, ws, shift)
    within(out, *ref["out"], what + ": out")
    if not backward:
        return out, ref
    db0, ds0 = rnd(seed + 4, bias.shape), rnd(seed + 5, scale.shape)
    gq0, gv0 = rnd(seed + 6, (C,)), rnd(seed + 7, (C,))
    gq, gv = gq0.clone(), gv0.clone()
    dqkv, dbias, dscale, flag = ops.winattn_bwd(qkv, dout, bias, scale, b, H, W, heads, ws, shift, want_colsum=True, dbias=db0.clone(),
                                                dscale=ds0.clone(), qv_grads=(gq, gv))
    assert flag is True
    dqkv2, dbias2, dscale2, colsum = ops.winattn_bwd(qkv, dout, bias, scale, b, H, W, heads, ws, shift, want_colsum=True)
    assert torch.equal(dqkv, dqkv2)
    within(dqkv, *ref["dqkv"], what + ": dqkv")
    vb, bb = ref["dbias"]
    within(dbias2, vb, bb, what + ": dbias")
    within(dbias, vb + db0.double(), bb + 2 * U32 * (vb.abs() + db0.double().abs()), what + ": dbias accumulated")
    vs, bs = ref["dscale"]
    within(dscale2, vs, bs, what + ": dscale")
    within(dscale, vs + ds0.double(), bs + 2 * U32 * (vs.abs() + ds0.double().abs()), what + ": dscale accumulated")
    d = dqkv.double()
    cs = d.sum(0)
    cb = ref["colsum_terms"] * U32 * d.abs().sum(0) + 2 * U32 * cs.abs()
    within(colsum, cs, cb, what + ": column sums")
    within(gq, cs[:C] + gq0.double(), cb[:C] + 2 * U32 * gq0.double().abs(), what + ": q bias gradient accumulated")
    within(gv, cs[2 * C:] + gv0.double(), cb[2 * C:] + 2 * U32 * gv0.double().abs(), what + ": v bias gradient accumulated")
    return out, ref


# ================================================================================================ the census signatures, checked
CHECKS = {"linear_fwd": check_linear_fwd, "gemm_nt": check_gemm_nt, "linear_dgrad_gelu": check_linear_dgrad_gelu, "gemm_tn": check_gemm_tn,
          "conv_fwd": check_conv_fwd, "conv_fwd_bnrelu": check_conv_fwd_bnrelu, "conv_dgrad": check_conv_dgrad, "conv_wgrad": check_conv_wgrad}
CHECKED_BY = {name: "test_census_launch_against_float64 (%s)" % fn.__name__ for name, fn in CHECKS.items()}
CHECKED_BY.update(winattn_fwd="test_window_attention_against_float64", winattn_bwd="test_window_attention_against_float64")
ALL_SIGS = SWIN34_LAUNCHES | ALTERNET50_LAUNCHES
GEMM_SIGS = sorted(s for s in ALL_SIGS if s[0] in CHECKS)
ATTN_GEOMS = sorted({s[2:9] for s in ALL_SIGS if s[0] in ("winattn_fwd", "winattn_bwd")})
EDGE_GEOMS = [(37, 56, 56, 64, 2, 7, 0)]             # 2 368 windows: the last forward chunk holds 3 windows, the last backward chunk 12


def _id(sig):
    return "-".join(str(int(v)) if isinstance(v, bool) else str(v) for v in sig)


@pytest.mark.parametrize("sig", GEMM_SIGS, ids=[_id(s) for s in GEMM_SIGS])
def test_census_launch_against_float64(sig):
    """every linear / GEMM / convolution launch of the two census lists at its exact bench shape and flags, fresh operands; the bounds are
    those stated by the check_* function of its entry point, and every Nout % 256 == 0 launch of M >= 16 384 rows asserts its 256-row tile"""
    CHECKS[sig[0]](sig)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("geom", ATTN_GEOMS + EDGE_GEOMS, ids=[_id(g) for g in ATTN_GEOMS + EDGE_GEOMS])
def test_window_attention_against_float64(geom):
    """every window-attention geometry of the census at full bench batch (several windows per wave in both kernels; AlterNet50's shifted
    ws 6 / shift 3 and ws 3 / shift 1 layers) and a ragged last chunk, with the bounds of check_winattn"""
    b, H, W, C, heads, ws, shift = geom
    nwin = b * (H // ws) * (W // ws)
    check_winattn(b, H, W, C, heads, ws, shift)
    if geom in EDGE_GEOMS and _cus() == 256:
        assert nwin - (wm_chunks(nwin, heads, 4 * 256)[0] - 1) * wm_chunks(nwin, heads, 4 * 256)[1] == 3
        assert nwin - (wm_chunks(nwin, heads, 256)[0] - 1) * wm_chunks(nwin, heads, 256)[1] == 12
    torch.cuda.empty_cache()


# ================================================================================================ D. NT GEMM dispatch boundaries
# automatic dispatch throughout.  M = 16 128 stays on the 128-row tiles; 16 384 is the first 256 x 256 launch (lean, persistent, 64 tiles: fewer
# than the CUs); 16 512 is tile 4 with a ragged last row tile (the general EPI_STORE epilogue); 76 800 x 512 makes 600 tiles, 2.3 per
# persistent workgroup (walks of 2 and 3 tiles).
NT_BOUNDARY = [(16128, 256, 256, False), (16384, 256, 256, True), (16512, 512, 256, True), (76800, 512, 128, True)]


@pytest.mark.parametrize("case", NT_BOUNDARY, ids=["M%d-N%d-K%d" % c[:3] for c in NT_BOUNDARY])
def test_nt_dispatch_boundaries_against_float64(case):
    """linear_fwd (bias + GELU, bias + stats), gemm_nt and linear_dgrad_gelu on either side of the 256 x 256 tile threshold, with the bounds
    of check_linear_fwd / check_gemm_nt / check_linear_dgrad_gelu; the dispatched row tile is asserted from the partial-buffer rows"""
    m, n, k, tile4 = case
    rows = _lib().frhip_conv_stat_rows(0, m, n, 1, 1, k, 1, 1, 1, 0)
    assert rows == (tile_rows(m) if tile4 else -(-m // 128))
    check_linear_fwd(("linear_fwd", "bf16", m, n, k, True, True, False))
    check_linear_fwd(("linear_fwd", "bf16", m, n, k, True, False, True))
    check_gemm_nt(("gemm_nt", "bf16", m, n, k, 1, False))
    check_linear_dgrad_gelu(("linear_dgrad_gelu", "bf16", m, n, k, True, True))
    check_conv_dgrad(("conv_dgrad", "bf16", m, 1, 1, n, k, 1, 1, 1, 0, True, 1, "bn", 64))


# ================================================================================================ G. negative controls
def test_negative_controls_linear_and_partials():
    """the linear bounds reject a reference missing one 32-wide K step and an output with one 256 x 256 tile shifted by a row; the partial-sum
    bound rejects a buffer with one tile's partial row dropped"""
    m, n, k = 16384, 256, 256
    a, w = _linear_operands(m, n, k, 11)
    out, ref, bound = check_linear_fwd(("linear_fwd", "bf16", m, n, k, True, False, False))
    step = a[:, 32:64].double() @ w[:, 32:64].double().t()
    assert violations(out, ref - step, bound) > out.numel() // 2
    shifted = out.clone()
    shifted[256:512, :256] = out[257:513, :256]
    assert violations(shifted, ref, bound) > 256 * 200
    o2, _, part = _ops().linear_fwd(a, w, rnd(13, (n,)) * 0.5, want_stats=True)
    o = o2.double()
    check_partials(part, (o, o * o), (o.abs(), o * o), "intact")
    dropped = part.clone()
    dropped[5] = 0
    with pytest.raises(AssertionError):
        check_partials(dropped, (o, o * o), (o.abs(), o * o), "one tile dropped")
    # the gemm_tn bound at the largest census K (100 352): a 32-row K step left out of the reference is still seen
    sig = ("gemm_tn", "bf16", 100352, 256, 256, 256, 0, False)
    out, ref, bound = check_gemm_tn(sig)
    p = rnd(41, (100352, 256)).to(BF)
    q = (rnd(42, (100352, 256)) * 0.1).to(BF)
    assert violations(out, ref - p[32:64].double().t() @ q[32:64].double(), bound) > out.numel() // 4


def test_negative_controls_convolution():
    """the convolution bound rejects a reference missing one 32-channel K step of one tap and an output with one 256 x 256 tile shifted by
    a row (AlterNet50's 12 x 12 / 256-channel body convolution)"""
    sig = ("conv_fwd", "bf16", 256, 12, 12, 256, 256, 3, 3, 1, 1, True)
    y, ref, bound = check_conv_fwd(sig)
    x, wt = _conv_operands(sig, 51)
    part = torch.zeros_like(wt)
    part[:, 1, 1, 32:64] = wt[:, 1, 1, 32:64]
    assert violations(y, ref - ref_conv(x, part, 1, 1), bound) > y.numel() // 2
    flat = y.view(-1, 256)
    shifted = flat.clone()
    shifted[512:768] = flat[513:769]
    assert violations(shifted, ref.view(-1, 256), bound.view(-1, 256)) > 256 * 200


def test_negative_controls_window_attention():
    """the attention bounds reject a reference without the shift mask (AlterNet50's shifted 12 x 12 layer) and a forward output in which
    every chunk's last window holds its first window's values"""
    b, H, W, C, heads, ws, shift = 256, 12, 12, 256, 8, 6, 3
    out, ref = check_winattn(b, H, W, C, heads, ws, shift, backward=False)
    qkv, bias, scale, _ = _attn_inputs(b, H, W, C, heads, ws, 91)
    nomask = attn_reference(qkv, None, bias, scale, b, H, W, heads, ws, shift, use_mask=False)
    val, bound = ref["out"]
    assert violations(out, nomask["out"][0], bound) > 1000
    nw, pix = ref["nwin"], ref["pix"]
    chunks, wpb = wm_chunks(nw, heads, 4 * _cus())
    bad = out.clone()
    for c in range(chunks):
        first, last = c * wpb, min(nw, (c + 1) * wpb) - 1
        bad[pix[last]] = out[pix[first]]
    assert violations(bad, val, bound) > chunks * 36 * C // 2
