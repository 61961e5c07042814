"""Exact-operand cases of the forward convolutions (frhip_conv_fwd, frhip_conv_fwd_affine, frhip_conv_fwd_bnrelu: csrc/igemm_nt.hip and
csrc/igemm_halo.hip), one per route and map edge, with their exact reference.  Shared by tests/test_fwd_cases_cpu.py (routes, references
and bounds, no GPU) and tests/test_fwd_exact_gpu.py.  Nothing here calls into frhip for a reference value.  The switches, the guarded
buffers and the integer generators are those of tests/dgrad_cases.py.

Operands are small integers, drawn per case from a generator seeded with the case name: x and w sparse from {-2 .. 2}, their density set
per case so that about 16 products per output element are not zero; the residual from {-8 .. 8}, the affine scale from {-1, 1, 2}, shift
from {-3 .. 3}.  For frhip_conv_fwd_bnrelu x is dense from {-4 .. 4}, in_scale from {-1, 1, 2}, in_shift from {-3 .. 3} (so the operand
a = relu(x * in_scale + in_shift) is an integer of at most 11, zero for about every second element, and relu(in_shift) is positive for
three channels in seven: padding that went through the transform shows) and w sparser, to keep the product count.  No halves anywhere:
an odd value times 0.5 above 128 is not a bf16 number.  Then, per case (asserted by the CPU test, not assumed):
  * every stored element of y, of the affine output and of act_out is unchanged by a round trip through the case's dtype, and every y is
    an integer of magnitude <= 256;
  * |x| (*) |w| + 8 < 2^24 (|a| (*) |w| for _bnrelu): every partial sum of the contraction, in any order, is exact;
  * for every statistics row -- one per block of BM output rows -- sum |y| < 2^24 and sum y^2 < 2^24 per channel: the terms of the second
    are not negative, so any order of summation is exact.
The comparison is therefore torch.equal against the reference, with no tolerance.

The reference is computed twice, independently: torch.nn.functional.conv2d in float64, and an int64 loop over the filter taps written
from the text of include/frhip.h, y[ho][wo] = sum_taps x[ho * stride - pad + fr][wo * stride - pad + fs] . w[:, fr, fs, :].  The second
also forms the _bnrelu operand (zero padding applied AFTER the transform), the affine output [relu](y * scale + shift + residual) and the
per-block sums {sum y, sum y^2}, one row per BM output rows, the last block ragged.  The two largest cases (16 384 and 33 024 rows) take
the tap's matrix product in float64, exact under the bounds above, because an int64 product of that size costs seconds.

A case: (n, h, w, c, k) with x [n,h,w,c] and y [n,ho,wo,k]; the filter (r x r, stride, pad); the four switches it runs under
(frhip_set_conv_halo, frhip_set_halo_wide_dirs, frhip_set_nt_tile, frhip_set_epi_lean); the route it claims for frhip_conv_fwd, as
frhip_conv_fwd_route reports it: (family, NT tile, epilogue, stat rows); and the variants it runs (VARIANTS).  frhip_conv_fwd_affine takes
the same kernel in one launch where that is a lean halo kernel -- the folded BatchNorm exists in the lean epilogue only -- and everywhere
else two launches, the convolution and frhip_bn_apply in place.  frhip_conv_fwd_bnrelu always runs the 4-wave halo tile.

Two notes on the table.  The forward direction of the 64 x 128-per-wave halo tile is off by default (frhip_set_halo_wide_dirs: 2), so its
cases run under 1 or 3.  And every listed shape of the two 8-wave tiles has a ragged last row tile, so each has a forced case of one
whole tile beside it.

The persistent case is sized as in tests/dgrad_cases.py: (256 / 2 + 1) x 2 = 258 tiles on the 256 workgroups of an MI355X.  Forward sums
are per 256-row block, so unlike there the bound on the sums holds and the case runs WITH statistics."""
import collections
import functools
import zlib

import torch

from dgrad_cases import (GENERIC, HALO_4WAVE, HALO_4X2, HALO_8X1, HALO_WIDE, PERSISTENT_CUS, POISON, _guarded, _ints, _sparse,  # noqa: F401
                         guards_untouched, switches)

EPI_GENERAL, EPI_LEAN = 0, 1
MODE_FWD, MODE_AFFINE, MODE_BNRELU = 0, 1, 2
# variant -> (mode of frhip_conv_fwd_route, statistics, ReLU and residual (affine) / act_out (bnrelu))
VARIANTS = {
    "plain": (MODE_FWD, False, False),
    "stats": (MODE_FWD, True, False),
    "affine": (MODE_AFFINE, False, True),
    "affine_bare": (MODE_AFFINE, False, False),
    "bnrelu": (MODE_BNRELU, False, False),
    "bnrelu_act": (MODE_BNRELU, True, True),
}
BASE = ("plain", "stats")
AFF = ("affine", "affine_bare")
BNR = ("bnrelu", "bnrelu_act")
BIG_ROWS = 16384          # from here on the tap products are taken in float64

Case = collections.namedtuple("Case", "name dtype n h w c k r stride pad halo wide tile lean route variants")


def _case(name, dims, route, more=(), dtype="bf16", f=(3, 1, 1), halo=1, wide=2, tile=0, lean=1):
    n, h, w, c, k = dims
    return Case(name, dtype, n, h, w, c, k, f[0], f[1], f[2], halo, wide, tile, lean, route, BASE + tuple(more))


S2 = (3, 2, 1)
ONE = (1, 1, 0)
CASES = [
    # ---- halo kernels, 4-wave tile <4,1,4,1> (bf16, default switches)
    _case("4-wave, one ragged tile over three images", (3, 7, 7, 64, 64), (1, 0, 0, 1), AFF + BNR),
    _case("4-wave, lean, one tile", (4, 8, 8, 64, 64), (1, 0, 1, 1), AFF + BNR),
    _case("4-wave, one whole tile, lean off", (4, 8, 8, 64, 64), (1, 0, 0, 1), AFF, lean=0),
    _case("4-wave, lean, 2 x 2 tiles", (8, 8, 8, 64, 128), (1, 0, 1, 2), AFF + BNR),
    _case("4-wave, three K chunks", (3, 7, 7, 192, 64), (1, 0, 0, 1), BNR),
    _case("4-wave, ragged channel tile: 72 of 128 columns", (3, 7, 7, 64, 72), (1, 0, 0, 1)),
    # ---- halo kernels, map edges
    _case("H = 1, W = 56", (2, 1, 56, 64, 64), (1, 0, 0, 1), ("bnrelu",)),
    _case("W = 1, H = 56", (2, 56, 1, 64, 64), (1, 0, 0, 1), ("bnrelu",)),
    _case("1 x 1 maps: every tap but the centre is padding", (130, 1, 1, 64, 64), (1, 0, 0, 1), ("bnrelu",)),
    _case("W = 56: widest halo map", (1, 5, 56, 64, 64), (1, 0, 0, 2), ("bnrelu",)),
    _case("W = 57: handed to the generic kernel", (1, 5, 57, 64, 64), (0, 2, 0, 2)),
    # ---- halo kernels, the 64 x 128-per-wave tile (bf16, k % 128 == 0, c >= 128, W <= 28, forward direction on)
    _case("wide, ragged tile", (3, 7, 7, 128, 128), (4, 0, 0, 1), wide=1),
    _case("wide, lean", (1, 16, 16, 128, 128), (4, 0, 1, 1), AFF, wide=1),
    _case("wide at its width limit W = 28, both directions on", (1, 10, 28, 128, 128), (4, 0, 0, 2), wide=3),
    _case("W = 29 leaves the wide tile", (1, 9, 29, 128, 128), (1, 0, 0, 2), wide=1),
    _case("wide direction off by default: 4-wave, lean", (1, 16, 16, 128, 128), (1, 0, 1, 1), AFF),
    # ---- halo kernels, the two 8-wave tiles
    _case("<8,1,2,2> forced under bf16", (3, 7, 7, 128, 64), (2, 0, 0, 1), AFF, halo=3),
    _case("<8,1,2,2> forced, one whole tile", (4, 8, 8, 128, 64), (2, 0, 0, 1), halo=3),
    _case("<8,1,2,2> automatic: nine K chunks", (1, 5, 5, 576, 64), (2, 0, 0, 1)),
    _case("<8,1,2,2> fp32", (3, 7, 7, 32, 64), (2, 0, 0, 1), AFF, dtype="fp32"),
    _case("<4,2,4,2> forced under bf16", (3, 7, 7, 128, 128), (3, 0, 0, 1), halo=3),
    _case("<4,2,4,2> forced, one whole tile", (4, 8, 8, 128, 128), (3, 0, 0, 1), halo=3),
    _case("<4,2,4,2> automatic: nine K chunks", (1, 5, 5, 576, 128), (3, 0, 0, 1)),
    _case("<4,2,4,2> fp32", (3, 7, 7, 32, 128), (3, 0, 0, 1), dtype="fp32"),
    # ---- generic kernel on 3x3 / stride 1 (halo off), every NT tile; tile 3 is never chosen automatically
    _case("generic 3x3, tile 1 automatic", (3, 7, 7, 64, 128), (0, 1, 0, 2), AFF, halo=0),
    _case("generic 3x3, tile 1 forced", (3, 7, 7, 64, 64), (0, 1, 0, 2), halo=0, tile=1),
    _case("generic 3x3, tile 2 automatic", (3, 7, 7, 64, 64), (0, 2, 0, 1), halo=0),
    _case("generic 3x3, tile 2 forced", (3, 7, 7, 64, 128), (0, 2, 0, 1), halo=0, tile=2),
    _case("generic 3x3, tile 3 forced, 64 columns", (3, 7, 7, 64, 64), (0, 3, 0, 1), halo=0, tile=3),
    _case("generic 3x3, tile 3 forced, 128 columns", (3, 7, 7, 64, 128), (0, 3, 0, 1), halo=0, tile=3),
    _case("generic 3x3, tile 4 forced, 64 columns", (3, 7, 7, 64, 64), (0, 4, 0, 1), halo=0, tile=4),
    _case("generic 3x3, tile 4 forced, 128 columns", (3, 7, 7, 64, 128), (0, 4, 0, 1), halo=0, tile=4),
    _case("generic 3x3, fp32: tile 3 forced resolves to tile 1", (3, 7, 7, 32, 64), (0, 1, 0, 2), dtype="fp32", halo=0, tile=3),
    # ---- generic kernel, 1x1 / stride 1
    _case("1x1, tile 2", (3, 7, 7, 64, 64), (0, 2, 0, 1), AFF, f=ONE),
    _case("1x1, tile 1", (3, 7, 7, 64, 128), (0, 1, 0, 2), f=ONE),
    _case("1x1, tile 1, ragged third column tile", (3, 7, 7, 64, 264), (0, 1, 0, 2), f=ONE),
    _case("1x1, tile 2, ragged third column tile", (3, 7, 7, 64, 136), (0, 2, 0, 1), f=ONE),
    _case("1x1 on 1 x 1 maps, as the stem calls it: 300 rows", (300, 1, 1, 64, 64), (0, 2, 0, 2), f=ONE),
    _case("tile 4 automatic, lean", (64, 16, 16, 64, 256), (0, 4, 1, 64), f=ONE),
    _case("tile 4 automatic, lean off", (64, 16, 16, 64, 256), (0, 4, 0, 64), f=ONE, lean=0),
    _case("tile 4 lean, persistent loop takes a second tile", (PERSISTENT_CUS // 2 + 1, 16, 16, 64, 512),
          (0, 4, 1, PERSISTENT_CUS // 2 + 1), f=ONE),
    # ---- generic kernel, the stride-2 gather: 3x3 / pad 1
    _case("3x3 / s2, 9x9, tile 2 automatic", (2, 9, 9, 64, 64), (0, 2, 0, 1), AFF, f=S2),
    _case("3x3 / s2, 9x9, tile 1 forced", (2, 9, 9, 64, 64), (0, 1, 0, 1), f=S2, tile=1),
    _case("3x3 / s2, 10x6", (2, 10, 6, 64, 128), (0, 1, 0, 1), f=S2),
    _case("3x3 / s2, H = 1", (2, 1, 7, 64, 64), (0, 2, 0, 1), f=S2),
    _case("3x3 / s2, 1 x 1 maps", (3, 1, 1, 64, 64), (0, 2, 0, 1), f=S2),
    _case("3x3 / s2, 2 x 2 map: one output pixel", (1, 2, 2, 64, 64), (0, 2, 0, 1), f=S2),
    _case("3x3 / s2, fp32", (2, 9, 9, 32, 64), (0, 2, 0, 1), dtype="fp32", f=S2),
    # ---- 2x2 / s2 / pad 0 and 1x1 / s2
    _case("2x2 / s2", (3, 14, 14, 64, 128), (0, 1, 0, 2), f=(2, 2, 0)),
    _case("2x2 / s2, odd map: last row and column are read by no output", (2, 15, 13, 64, 64), (0, 2, 0, 1), f=(2, 2, 0)),
    _case("1x1 / s2", (2, 8, 8, 64, 128), (0, 1, 0, 1), f=(1, 2, 0)),
    _case("1x1 / s2, odd map", (2, 9, 7, 64, 64), (0, 2, 0, 1), f=(1, 2, 0)),
]
BY_NAME = {case.name: case for case in CASES}
RUNS = [(case.name, variant) for case in CASES for variant in case.variants]


def dt_code(case):
    return 0 if case.dtype == "bf16" else 1


def torch_dtype(case):
    return torch.bfloat16 if case.dtype == "bf16" else torch.float32


def kstep(case):
    """channels of x per K step: one 128-byte row"""
    return 64 if case.dtype == "bf16" else 32


def out_hw(case):
    return (case.h + 2 * case.pad - case.r) // case.stride + 1, (case.w + 2 * case.pad - case.r) // case.stride + 1


def rows(case):
    ho, wo = out_hw(case)
    return case.n * ho * wo


def is_halo(case):
    return case.route[0] != GENERIC


def block_rows(case):
    """BM: output rows per statistics row"""
    return 256 if is_halo(case) else {1: 128, 2: 256, 3: 256, 4: 256}[case.route[1]]


def shape_args(case):
    return (dt_code(case), case.n, case.h, case.w, case.c, case.k, case.r, case.r, case.stride, case.pad)


def stat_rows_args(case):
    """the arguments of frhip_conv_stat_rows: (dtype, m, k, h, w, c, r, s, stride, pad)"""
    return (dt_code(case), rows(case), case.k, case.h, case.w, case.c, case.r, case.r, case.stride, case.pad)


def claimed_route(case, variant):
    """(family, tile, epilogue, launches, stat rows) as frhip_conv_fwd_route reports the run"""
    family, tile, epi, stat_rows = case.route
    mode = VARIANTS[variant][0]
    if mode == MODE_BNRELU:
        return (HALO_4WAVE, 0, epi, 1, stat_rows)
    folded = family in (HALO_4WAVE, HALO_WIDE) and epi == EPI_LEAN
    return (family, tile, epi, 2 if mode == MODE_AFFINE and not folded else 1, stat_rows)


def density(case, bnrelu=False):
    """of x and of w (bnrelu: of w alone, x being dense): about 16 non-zero products per output element of an interior pixel"""
    terms = case.r * case.r * case.c
    if bnrelu:
        return min(1.0, 16.0 / (0.8 * 0.5 * terms))          # a drawn w is 0 one time in five, a = relu(..) about every second time
    return min(1.0, (16.0 / (0.64 * terms)) ** 0.5)


@functools.lru_cache(maxsize=None)
def operands(name):
    """CPU tensors of a case, int64: x [n][h][w][c], w [k][r][r][c], res [n][ho][wo][k], scale / shift [k], and for the _bnrelu variants
    xd [n][h][w][c] (dense), wb [k][r][r][c], in_scale / in_shift [c]"""
    case = BY_NAME[name]
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    ho, wo = out_hw(case)
    p = density(case)
    steps = torch.tensor([-1, 1, 2])
    ops = {"x": _sparse(gen, (case.n, case.h, case.w, case.c), p), "w": _sparse(gen, (case.k, case.r, case.r, case.c), p),
           "res": _ints(gen, (case.n, ho, wo, case.k), -8, 8),
           "scale": steps[_ints(gen, (case.k,), 0, 2)], "shift": _ints(gen, (case.k,), -3, 3)}
    if any(VARIANTS[v][0] == MODE_BNRELU for v in case.variants):
        ops["xd"] = _ints(gen, (case.n, case.h, case.w, case.c), -4, 4)
        ops["wb"] = _sparse(gen, (case.k, case.r, case.r, case.c), density(case, True))
        ops["in_scale"], ops["in_shift"] = steps[_ints(gen, (case.c,), 0, 2)], _ints(gen, (case.c,), -3, 3)
    return ops


def transform(xd, in_scale, in_shift):
    """the _bnrelu operand a = relu(x * in_scale[c] + in_shift[c]), int64"""
    return (xd * in_scale + in_shift).clamp(min=0)


def conv_i64(case, x, w, skip_tap=None, base=0, pad_value=None):
    """[n][ho][wo][k] int64: y[ho][wo] = sum over the taps (fr, fs) of x[ho * stride - pad + fr][wo * stride - pad + fs] . w[:, fr, fs, :],
    x zero outside the map.  The three keywords build deliberately WRONG results: one tap left out; the gather base `base` pixels further
    down and right; the padding holding pad_value[c] instead of zero."""
    ho, wo = out_hw(case)
    hp, wp = case.h + 2 * case.pad + base, case.w + 2 * case.pad + base
    xp = torch.zeros((case.n, hp, wp, case.c), dtype=torch.int64)
    if pad_value is not None:
        xp += pad_value
    xp[:, case.pad:case.pad + case.h, case.pad:case.pad + case.w] = x
    y = torch.zeros((case.n * ho * wo, case.k), dtype=torch.int64)
    for fr in range(case.r):
        for fs in range(case.r):
            if (fr, fs) == skip_tap:
                continue
            tap = xp[:, base + fr:base + fr + case.stride * (ho - 1) + 1:case.stride,
                     base + fs:base + fs + case.stride * (wo - 1) + 1:case.stride].reshape(-1, case.c)
            if rows(case) >= BIG_ROWS:
                y += (tap.double() @ w[:, fr, fs, :].double().t()).long()
            else:
                y += tap @ w[:, fr, fs, :].t()
    return y.reshape(case.n, ho, wo, case.k)


def _conv2d_f64(case, x, w):
    y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), w.permute(0, 3, 1, 2).double(), None, case.stride, case.pad)
    return y.permute(0, 2, 3, 1).contiguous()


def inputs(name, bnrelu):
    """(the convolution's operand on the CPU, its weights): x, w or relu(xd * in_scale + in_shift), wb"""
    ops = operands(name)
    if bnrelu:
        return transform(ops["xd"], ops["in_scale"], ops["in_shift"]), ops["wb"]
    return ops["x"], ops["w"]


@functools.lru_cache(maxsize=None)
def y_f64(name, bnrelu=False):
    """[n][ho][wo][k] float64: torch.nn.functional.conv2d, the _bnrelu operand formed in float64 as well"""
    case, ops = BY_NAME[name], operands(name)
    if bnrelu:
        a = torch.relu(ops["xd"].double() * ops["in_scale"].double() + ops["in_shift"].double())
        return _conv2d_f64(case, a, ops["wb"])
    return _conv2d_f64(case, ops["x"], ops["w"])


@functools.lru_cache(maxsize=None)
def y_i64(name, bnrelu=False):
    return conv_i64(BY_NAME[name], *inputs(name, bnrelu))


def affine(name, y, relu, residual, channel_shift=0):
    """[relu](y * scale[k] + shift[k] + residual), int64; channel_shift: scale and shift indexed that many channels off (WRONG)"""
    ops = operands(name)
    out = y * ops["scale"].roll(channel_shift) + ops["shift"].roll(channel_shift)
    if residual:
        out = out + ops["res"]
    return out.clamp(min=0) if relu else out


def block_sums(case, y, beyond=False):
    """float64 [ceil(rows / BM)][2][k]: {sum y, sum y^2} over each block of BM output rows, the last one ragged.  beyond (WRONG): the last
    block runs on over BM whole rows, into what the next images would hold (the batch repeated)"""
    flat = y.reshape(-1, case.k)
    m, bm = flat.shape[0], block_rows(case)
    short = (-m) % bm
    if beyond:
        flat = flat.repeat((m + short + m - 1) // m, 1)[:m + short]
    else:
        flat = torch.nn.functional.pad(flat, (0, 0, 0, short))
    blocks = flat.reshape(-1, bm, case.k)
    return torch.stack([blocks.sum(1), (blocks * blocks).sum(1)], 1).double()


@functools.lru_cache(maxsize=None)
def expected(name, variant):
    """{"y": int64 [n][ho][wo][k], what the run stores; "act": int64 [n][h][w][c] or None; "rows": float64 [stat rows][2][k] or None}"""
    case = BY_NAME[name]
    mode, stats, extra = VARIANTS[variant]
    y = y_i64(name, mode == MODE_BNRELU)
    out = {"y": y, "act": None, "rows": block_sums(case, y) if stats else None}
    if mode == MODE_AFFINE:
        out["y"] = affine(name, y, relu=extra, residual=extra)
    if mode == MODE_BNRELU and extra:
        out["act"] = inputs(name, True)[0]
    return out


@functools.lru_cache(maxsize=None)
def bound(name):
    """{"contraction": max |x| (*) |w| + 8 over the operand pairs the case runs, "y": largest magnitude of a convolution result, "stored":
    largest magnitude of anything stored, "sum": largest per-block, per-channel sum |y|, "sumsq": largest such sum y^2}"""
    case = BY_NAME[name]
    modes = {VARIANTS[v][0] == MODE_BNRELU for v in case.variants}
    out = {"contraction": 0, "y": 0, "stored": 0, "sum": 0, "sumsq": 0}
    for bnrelu in modes:
        a, w = inputs(name, bnrelu)
        y = y_i64(name, bnrelu)
        sums = block_sums(case, y.abs())
        out["contraction"] = max(out["contraction"], int(_conv2d_f64(case, a.abs(), w.abs()).max()) + 8)
        out["y"] = max(out["y"], int(y.abs().max()))
        out["sum"], out["sumsq"] = max(out["sum"], float(sums[:, 0].max())), max(out["sumsq"], float(sums[:, 1].max()))
    for variant in case.variants:
        want = expected(name, variant)
        out["stored"] = max(out["stored"], int(want["y"].abs().max()), 0 if want["act"] is None else int(want["act"].abs().max()))
    return out


# ------------------------------------------------------------------------------------------ the launch (GPU)
def _between_guards(t, guard_elems, dtype, device):
    """`t` on the device as `dtype`, inside a buffer whose elements before and after it are NaN: a read outside the tensor poisons the result"""
    flat = t.to(dtype).reshape(-1)
    buf = torch.full((flat.numel() + 2 * guard_elems,), POISON, dtype=dtype, device=device)
    buf[guard_elems:guard_elems + flat.numel()] = flat.to(device)
    return buf, buf[guard_elems:guard_elems + flat.numel()]


def launch(name, variant, device="cuda"):
    """One launch of the run through its C entry point, under the switches the CALLER has set.  y, act_out and the partial rows live inside
    larger buffers, poisoned with NaN, between guards of 256 rows (y, act_out) / 8 rows (partials) on either side; x, w and the residual
    lie between NaN guards of 256 rows.
    -> (y [n][ho][wo][k] on the CPU as float64, act_out [n][h][w][c] as float64 or None, partial rows [rows][2][k] as float64 or None,
        guards untouched)"""
    from frhip import ops as fops
    from frhip._abi import check, lib
    case, data = BY_NAME[name], operands(name)
    mode, stats, extra = VARIANTS[variant]
    dtype = torch_dtype(case)
    ho, wo = out_hw(case)
    m = rows(case)
    x_cpu, w_cpu = (data["xd"], data["wb"]) if mode == MODE_BNRELU else (data["x"], data["w"])
    keep = [_between_guards(x_cpu, 256 * case.c, dtype, device), _between_guards(w_cpu, 256 * case.c, dtype, device)]
    x, w = keep[0][1], keep[1][1]
    f32 = lambda key: data[key].to(torch.float32).to(device).contiguous()
    ptr = lambda t: None if t is None else t.data_ptr()
    y_buf, y = _guarded(m * case.k, 256 * case.k, dtype, device)
    act_buf = act = part_buf = part = None
    stat_rows = lib().frhip_conv_stat_rows(*stat_rows_args(case))
    if stats:
        part_buf, part = _guarded(stat_rows * 2 * case.k, 8 * 2 * case.k, torch.float32, device)
    shape = shape_args(case)[1:]
    dt = dt_code(case)
    if mode == MODE_FWD:
        rc, entry = lib().frhip_conv_fwd(dt, ptr(x), ptr(w), ptr(y), ptr(part), *shape, fops._s()), "frhip_conv_fwd"
    elif mode == MODE_AFFINE:
        res = None
        if extra:
            keep.append(_between_guards(data["res"], 256 * case.k, dtype, device))
            res = keep[-1][1]
        scale, shift = f32("scale"), f32("shift")
        rc, entry = lib().frhip_conv_fwd_affine(dt, ptr(x), ptr(w), ptr(y), ptr(scale), ptr(shift), int(extra), ptr(res), *shape,
                                                fops._s()), "frhip_conv_fwd_affine"
    else:
        if extra:
            act_buf, act = _guarded(case.n * case.h * case.w * case.c, 256 * case.c, dtype, device)
        in_scale, in_shift = f32("in_scale"), f32("in_shift")
        rc, entry = lib().frhip_conv_fwd_bnrelu(dt, ptr(x), ptr(in_scale), ptr(in_shift), ptr(w), ptr(y), ptr(part), ptr(act), *shape,
                                                fops._s()), "frhip_conv_fwd_bnrelu"
    check(rc, entry)
    torch.cuda.synchronize()
    clean = guards_untouched(y_buf, m * case.k, 256 * case.k)
    if part is not None:
        clean = clean and guards_untouched(part_buf, stat_rows * 2 * case.k, 8 * 2 * case.k)
    if act is not None:
        clean = clean and guards_untouched(act_buf, act.numel(), 256 * case.c)
    return (y.cpu().double().reshape(case.n, ho, wo, case.k),
            None if act is None else act.cpu().double().reshape(case.n, case.h, case.w, case.c),
            None if part is None else part.cpu().double().reshape(stat_rows, 2, case.k), clean)
