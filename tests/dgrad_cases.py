"""Exact-operand cases of the data-gradient convolutions (frhip_conv_dgrad, _fused, _fused_rs, _bnred: csrc/igemm_nt.hip and
csrc/igemm_halo.hip), one per route and map edge, with their exact reference.  Shared by tests/test_dgrad_cases_cpu.py (routes, references
and bounds, no GPU) and tests/test_dgrad_exact_gpu.py.  Nothing here calls into frhip for a reference value.

Operands are small integers, drawn per case from a generator seeded with the case name: dy and w sparse from {-2 .. 2}, the dense and the
compact residual from {-8 .. 8}, y_bn from {-4 .. 4}, mean from {-2 .. 2}, invstd from {0.5, 1, 2}, mask_scale from {-1, 1, 2} and mask_shift
from {-3 .. 3} (so y * scale + shift is 0 for about one element in seven: `>` against `>=` shows), rowscale from {0, 2} with keep_scale 2.
The density of dy and w is set per case so that about 16 products per output element are not zero.  Then, per case (`bound`, asserted by
the CPU test):
  * every element of the convolution and of every stored dx (residual included) is an integer of magnitude <= 256: bf16 holds it exactly,
    both where the kernel rounds the convolution and where it rounds the sum with the residual;
  * every partial sum of the contraction, in any order, stays below max |dy| (*) |w| + 8 < 2^24;
  * every partial sum, in any order, of sum d, sum d * (y_bn - mean) * invstd over all rows, and of the lean epilogue's form of the latter,
    invstd * (sum d * y_bn - mean * sum d), stays below 2 * max_c sum_rows |dx| * (|y_bn| + |mean| + 1) * max(invstd, 1) < 2^24 (the 2 is
    keep_scale).  invstd is a power of two, so the sums are integers or halves, which fp32 holds just as exactly.
The comparison is therefore torch.equal against the reference, with no tolerance.

The reference is computed twice, independently: torch.nn.grad.conv2d_input in float64, and an int64 loop over the filter taps that
scatters dy . w[:, r, s, :] into the zero-padded dx, written from the text of include/frhip.h.  The second also places the compact
residual (even pixels only), applies the ReLU mask d = dx * (y_bn * mask_scale + mask_shift > 0), and forms the two per-channel sums -- for
frhip_conv_dgrad_fused_rs the sums of dx * rowscale[row / rows_per], dx itself unscaled.

A case: (n, h, w, c, k) with dx [n,h,w,c] and dy [n,ho,wo,k]; the filter (r x r, stride, pad); the four switches it runs under
(frhip_set_conv_halo, frhip_set_halo_wide_dirs, frhip_set_nt_tile, frhip_set_epi_lean); the route it claims, as frhip_dgrad_route reports
it: (family, NT tile, epilogue letter, launches, stat rows), the letter being G (general whatever the epilogue does), L (lean) or H (lean,
and in two 64-row halves once the launch carries BatchNorm-backward partials); and the epilogue variants it runs with (VARIANTS).  A
compact residual always takes the general epilogue.

Three notes on the table.  NT tile 3 (256 x 128) is never chosen automatically (nt_pick_tile names 1, 2 and 4): only frhip_set_nt_tile(3)
reaches it.  The parity shapes with 64 channels get tile 2 automatically, so their second run forces tile 1: every parity shape runs on
tiles 1 and 2, one of the two automatic.  And the 2 x 2 map (1,2,2,64,64) has NO empty parity class -- each of its four pixels is a class
of one row -- so (3,1,1,64,64), whose classes (0,1), (1,0) and (1,1) are empty, stands beside (2,1,7,64,64), which has two empty ones.

The persistent case (the lean loop of the 256 x 256 tile taking a second tile) is sized for the 256 compute units of an MI355X:
(256 / 2 + 1) x 2 = 258 tiles on 256 workgroups; the GPU test asserts that the device has fewer workgroups than the case has tiles.  Its
33 024 rows are beyond what the BatchNorm sums bound allows, so it runs without them."""
import collections
import contextlib
import functools
import zlib

import torch

GENERIC, HALO_4WAVE, HALO_8X1, HALO_4X2, HALO_WIDE = 0, 1, 2, 3, 4
EPI_GENERAL, EPI_LEAN, EPI_LEAN_HALVES = 0, 1, 2
KEEP_SCALE = 2.0
PERSISTENT_CUS = 256
# variant -> (entry point, residual stride or 0, BatchNorm partials, masked, rowscale)
VARIANTS = {
    "plain": ("frhip_conv_dgrad", 0, False, False, False),
    "res": ("frhip_conv_dgrad", 1, False, False, False),
    "res_bn": ("frhip_conv_dgrad_fused", 1, True, True, False),
    "res_bn_unmasked": ("frhip_conv_dgrad_bnred", 1, True, False, False),
    "compact": ("frhip_conv_dgrad_fused", 2, False, False, False),
    "compact_bn": ("frhip_conv_dgrad_fused", 2, True, True, False),
    "rs": ("frhip_conv_dgrad_fused_rs", 1, True, True, True),
}
BASE = ("plain", "res_bn")
COMPACT = ("compact", "compact_bn")

Case = collections.namedtuple("Case", "name dtype n h w c k r stride pad halo wide tile lean route variants")


def _case(name, dims, route, more=(), dtype="bf16", f=(3, 1, 1), halo=1, wide=2, tile=0, lean=1, variants=None):
    n, h, w, c, k = dims
    return Case(name, dtype, n, h, w, c, k, f[0], f[1], f[2], halo, wide, tile, lean, route, tuple(variants or BASE + tuple(more)))


S2 = (3, 2, 1)          # 3x3 / stride 2 / pad 1: four parity classes
CASES = [
    # ---- halo kernels, 4-wave tile <4,1,4,1>
    _case("4-wave, one ragged tile over three images", (3, 7, 7, 64, 64), (1, 0, "G", 1, 1), COMPACT + ("res_bn_unmasked", "rs")),
    _case("4-wave, lean, one tile", (4, 8, 8, 64, 64), (1, 0, "L", 1, 1), COMPACT + ("rs",)),
    _case("4-wave, one whole tile, lean off", (4, 8, 8, 64, 64), (1, 0, "G", 1, 1), lean=0),
    _case("4-wave, lean, 2 x 2 tiles", (8, 8, 8, 128, 64), (1, 0, "L", 1, 2)),
    _case("4-wave, 2 x 2 whole tiles, lean off", (8, 8, 8, 128, 64), (1, 0, "G", 1, 2), lean=0),
    _case("4-wave, three K chunks", (3, 7, 7, 64, 192), (1, 0, "G", 1, 1)),
    # ---- halo kernels, the 64 x 128-per-wave tile (bf16, c % 128 == 0, k >= 128, W <= 28, data-gradient direction on)
    _case("wide, ragged tile", (3, 7, 7, 128, 128), (4, 0, "G", 1, 1), COMPACT + ("rs",)),
    _case("wide, lean", (1, 16, 16, 128, 128), (4, 0, "L", 1, 1)),
    _case("wide, lean, four images", (4, 8, 8, 128, 128), (4, 0, "L", 1, 1), ("rs",)),
    _case("wide at its width limit W = 28", (1, 10, 28, 128, 128), (4, 0, "G", 1, 2)),
    _case("W = 29 leaves the wide tile", (1, 9, 29, 128, 128), (1, 0, "G", 1, 2)),
    _case("wide direction off: 4-wave, lean", (1, 16, 16, 128, 128), (1, 0, "L", 1, 1), wide=0),
    # ---- halo kernels, the two 8-wave tiles
    _case("<8,1,2,2> forced under bf16", (3, 7, 7, 64, 128), (2, 0, "G", 1, 1), halo=3),
    _case("<8,1,2,2> automatic: nine K chunks", (1, 5, 5, 64, 576), (2, 0, "G", 1, 1)),
    _case("<8,1,2,2> fp32", (3, 7, 7, 64, 32), (2, 0, "G", 1, 1), dtype="fp32"),
    _case("<4,2,4,2> forced under bf16", (3, 7, 7, 128, 128), (3, 0, "G", 1, 1), halo=3),
    _case("<4,2,4,2> automatic: nine K chunks, wide direction off", (1, 5, 5, 128, 576), (3, 0, "G", 1, 1), wide=0),
    _case("<4,2,4,2> fp32", (3, 7, 7, 128, 32), (3, 0, "G", 1, 1), dtype="fp32"),
    # ---- halo kernels, map edges
    _case("H = 1, W = 56", (2, 1, 56, 64, 64), (1, 0, "G", 1, 1)),
    _case("W = 1, H = 56", (2, 56, 1, 64, 64), (1, 0, "G", 1, 1)),
    _case("1 x 1 maps: every tap but the centre is padding", (130, 1, 1, 64, 64), (1, 0, "G", 1, 1)),
    _case("W = 56: widest halo map", (1, 5, 56, 64, 64), (1, 0, "G", 1, 2)),
    _case("W = 57: handed to the generic kernel", (1, 5, 57, 64, 64), (0, 2, "G", 1, 2)),
    # ---- generic kernel on 3x3 / stride 1 (halo off), every NT tile; tile 3 is never chosen automatically
    _case("generic 3x3, tile 1 automatic", (3, 7, 7, 128, 64), (0, 1, "G", 1, 2), COMPACT + ("res_bn_unmasked",), halo=0),
    _case("generic 3x3, tile 1 forced", (3, 7, 7, 64, 64), (0, 1, "G", 1, 2), halo=0, tile=1),
    _case("generic 3x3, tile 2 automatic", (3, 7, 7, 64, 64), (0, 2, "G", 1, 1), COMPACT, halo=0),
    _case("generic 3x3, tile 2 forced", (3, 7, 7, 128, 64), (0, 2, "G", 1, 1), halo=0, tile=2),
    _case("generic 3x3, tile 3 forced, 128 channels", (3, 7, 7, 128, 64), (0, 3, "G", 1, 1), halo=0, tile=3),
    _case("generic 3x3, tile 3 forced, 64 channels", (3, 7, 7, 64, 64), (0, 3, "G", 1, 1), halo=0, tile=3),
    _case("generic 3x3, tile 4 forced, 128 channels", (3, 7, 7, 128, 64), (0, 4, "G", 1, 1), halo=0, tile=4),
    _case("generic 3x3, tile 4 forced, 64 channels", (3, 7, 7, 64, 64), (0, 4, "G", 1, 1), halo=0, tile=4),
    # ---- generic kernel, tile 4 chosen automatically (1x1 / stride 1, M = 16 384, c % 256 == 0): lean, and in two halves with partials
    _case("tile 4 automatic, lean", (64, 16, 16, 256, 64), (0, 4, "H", 1, 64), ("rs",), f=(1, 1, 0)),
    _case("tile 4 automatic, lean off", (64, 16, 16, 256, 64), (0, 4, "G", 1, 64), ("rs",), f=(1, 1, 0), lean=0),
    _case("tile 4 lean, persistent loop takes a second tile", (PERSISTENT_CUS // 2 + 1, 16, 16, 512, 64),
          (0, 4, "H", 1, PERSISTENT_CUS // 2 + 1), f=(1, 1, 0), variants=("plain", "res")),
    # ---- parity classes (3x3 / stride 2 / pad 1), each shape on tiles 1 and 2
    _case("parity 9x9, tile 2 automatic", (2, 9, 9, 64, 64), (0, 2, "G", 4, 4), COMPACT, f=S2),
    _case("parity 9x9, tile 1 forced", (2, 9, 9, 64, 64), (0, 1, "G", 4, 4), f=S2, tile=1),
    _case("parity 10x6, tile 2 automatic", (2, 10, 6, 64, 128), (0, 2, "G", 4, 4), f=S2),
    _case("parity 10x6, tile 1 forced", (2, 10, 6, 64, 128), (0, 1, "G", 4, 4), f=S2, tile=1),
    _case("parity H = 1: two empty classes, tile 2 automatic", (2, 1, 7, 64, 64), (0, 2, "G", 2, 2), f=S2),
    _case("parity H = 1: two empty classes, tile 1 forced", (2, 1, 7, 64, 64), (0, 1, "G", 2, 2), f=S2, tile=1),
    _case("parity 2x2: four classes of one pixel, tile 2 automatic", (1, 2, 2, 64, 64), (0, 2, "G", 4, 4), f=S2),
    _case("parity 2x2: four classes of one pixel, tile 1 forced", (1, 2, 2, 64, 64), (0, 1, "G", 4, 4), f=S2, tile=1),
    _case("parity 1x1: three empty classes, tile 2 automatic", (3, 1, 1, 64, 64), (0, 2, "G", 1, 1), f=S2),
    _case("parity 1x1: three empty classes, tile 1 forced", (3, 1, 1, 64, 64), (0, 1, "G", 1, 1), f=S2, tile=1),
    _case("parity 20x20: three tiles per class, tile 1 automatic", (3, 20, 20, 128, 64), (0, 1, "G", 4, 12), f=S2),
    _case("parity 20x20: two tiles per class, tile 2 forced", (3, 20, 20, 128, 64), (0, 2, "G", 4, 8), f=S2, tile=2),
    # ---- the other strided filters: full-grid gather, pixels no tap reaches receive only the residual
    _case("2x2 / stride 2", (3, 14, 14, 64, 128), (0, 2, "G", 1, 3), f=(2, 2, 0)),
    _case("2x2 / stride 2, odd map: last row and column get the residual only", (2, 15, 13, 64, 64), (0, 2, "G", 1, 2), f=(2, 2, 0)),
    _case("1x1 / stride 2", (2, 8, 8, 64, 128), (0, 2, "G", 1, 1), f=(1, 2, 0)),
    _case("1x1 / stride 2, odd map", (2, 9, 7, 64, 64), (0, 2, "G", 1, 1), f=(1, 2, 0)),
]
BY_NAME = {case.name: case for case in CASES}
RUNS = [(case.name, variant) for case in CASES for variant in case.variants]


def dt_code(case):
    return 0 if case.dtype == "bf16" else 1


def kstep(case):
    """channels of dy per K step: one 128-byte row"""
    return 64 if case.dtype == "bf16" else 32


def out_hw(case):
    return (case.h + 2 * case.pad - case.r) // case.stride + 1, (case.w + 2 * case.pad - case.r) // case.stride + 1


def rows(case):
    return case.n * case.h * case.w


def is_halo(case):
    return case.route[0] != GENERIC


def is_parity(case):
    return (case.r, case.stride, case.pad) == S2


def claimed_epilogue(case, variant):
    _, res_stride, bn, _, _ = VARIANTS[variant]
    letter = case.route[2]
    if letter == "G" or res_stride == 2:
        return EPI_GENERAL
    return EPI_LEAN_HALVES if letter == "H" and bn else EPI_LEAN


def claimed_route(case, variant):
    family, tile, _, launches, stat_rows = case.route
    return (family, tile, claimed_epilogue(case, variant), launches, stat_rows)


def shape_args(case):
    return (dt_code(case), case.n, case.h, case.w, case.c, case.k, case.r, case.r, case.stride, case.pad)


def route_args(case, variant):
    """the arguments of frhip_dgrad_route (without `out`) for this run"""
    _, res_stride, bn, _, _ = VARIANTS[variant]
    return shape_args(case) + (res_stride, int(bn))


@contextlib.contextmanager
def switches(lib, case):
    """the case's four switches, put back whatever happens inside"""
    old = (lib.frhip_set_conv_halo(case.halo), lib.frhip_set_halo_wide_dirs(case.wide), lib.frhip_set_nt_tile(case.tile),
           lib.frhip_set_epi_lean(case.lean))
    try:
        yield
    finally:
        lib.frhip_set_conv_halo(old[0]), lib.frhip_set_halo_wide_dirs(old[1]), lib.frhip_set_nt_tile(old[2]), lib.frhip_set_epi_lean(old[3])


def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen, dtype=torch.int64)


def _sparse(gen, shape, density):
    return _ints(gen, shape, -2, 2) * (torch.rand(shape, generator=gen, dtype=torch.float64) < density)


def density(case):
    """of dy and of w: about 16 non-zero products per output element of an interior pixel, at most every second operand element"""
    taps = ((case.r + case.stride - 1) // case.stride) ** 2
    return min(0.5, (16.0 / (0.64 * taps * case.k)) ** 0.5)          # 0.64: a drawn value is itself 0 one time in five


@functools.lru_cache(maxsize=None)
def operands(name):
    """CPU tensors of a case.  int64: dy [n][ho][wo][k], w [k][r][r][c], res [n][h][w][c], resc [n][(h+1)/2][(w+1)/2][c], y [n][h][w][c],
    mean / mscale / mshift [c]; float64: invstd [c], rowscale [n] (first and last sample dropped)"""
    case = BY_NAME[name]
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    ho, wo = out_hw(case)
    p = density(case)
    ops = {"dy": _sparse(gen, (case.n, ho, wo, case.k), p), "w": _sparse(gen, (case.k, case.r, case.r, case.c), p),
           "res": _ints(gen, (case.n, case.h, case.w, case.c), -8, 8),
           "resc": _ints(gen, (case.n, (case.h + 1) // 2, (case.w + 1) // 2, case.c), -8, 8),
           "y": _ints(gen, (case.n, case.h, case.w, case.c), -4, 4), "mean": _ints(gen, (case.c,), -2, 2),
           "invstd": torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[_ints(gen, (case.c,), 0, 2)],
           "mscale": torch.tensor([-1, 1, 2])[_ints(gen, (case.c,), 0, 2)], "mshift": _ints(gen, (case.c,), -3, 3)}
    rowscale = KEEP_SCALE * _ints(gen, (case.n,), 0, 1).double()
    if case.n >= 3:
        rowscale[0] = rowscale[-1] = 0.0
        rowscale[1] = KEEP_SCALE
    ops["rowscale"] = rowscale
    return ops


def _conv2d_input_f64(case, dy, w):
    g = torch.nn.grad.conv2d_input((case.n, case.c, case.h, case.w), w.permute(0, 3, 1, 2).double(), dy.permute(0, 3, 1, 2).double(),
                                   case.stride, case.pad)
    return g.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def conv_f64(name):
    """[n][h][w][c] float64: torch.nn.grad.conv2d_input"""
    return _conv2d_input_f64(BY_NAME[name], operands(name)["dy"], operands(name)["w"])


def scatter_i64(case, dy, w, skip_tap=None):
    """[n][h][w][c] int64: y[ho][wo] = sum_taps x[ho * stride - pad + fr][wo * stride - pad + fs] . w[:, fr, fs], so tap (fr, fs) of the
    data-gradient adds dy[ho][wo] . w[:, fr, fs, :] to dx at that pixel; pixels in the padding are cut off at the end"""
    ho, wo = out_hw(case)
    hp = max(case.h + 2 * case.pad, case.stride * (ho - 1) + case.r)
    wp = max(case.w + 2 * case.pad, case.stride * (wo - 1) + case.r)
    buf = torch.zeros((case.n, hp, wp, case.c), dtype=torch.int64)
    flat = dy.reshape(-1, case.k)
    for fr in range(case.r):
        for fs in range(case.r):
            if (fr, fs) != skip_tap:
                buf[:, fr:fr + case.stride * (ho - 1) + 1:case.stride, fs:fs + case.stride * (wo - 1) + 1:case.stride] += \
                    (flat @ w[:, fr, fs, :]).reshape(case.n, ho, wo, case.c)
    return buf[:, case.pad:case.pad + case.h, case.pad:case.pad + case.w].contiguous()


@functools.lru_cache(maxsize=None)
def conv_i64(name):
    return scatter_i64(BY_NAME[name], operands(name)["dy"], operands(name)["w"])


def finish(name, variant, conv, odd_compact=False, mask_ge=False, scale_dx=False):
    """The epilogue of a run on the int64 convolution `conv` -> {"dx": int64 [n][h][w][c]} and with BatchNorm partials also "d" (int64
    [rows][c], the gradient behind the mask, times rowscale for _rs), "dyc" (float64 [rows][c]: d * (y_bn - mean) * invstd) and the
    per-channel sums "s1", "s2" (float64 [c]).  The three flags build deliberately WRONG results for the sensitivity checks."""
    case, ops = BY_NAME[name], operands(name)
    _, res_stride, bn, masked, rs = VARIANTS[variant]
    dx = conv.clone()
    if res_stride == 1:
        dx += ops["res"]
    elif res_stride == 2 and not odd_compact:
        dx[:, 0::2, 0::2] += ops["resc"]
    elif res_stride == 2:
        dx[:, 1::2, 1::2] += ops["resc"][:, :case.h // 2, :case.w // 2]
    out = {"dx": dx}
    if bn:
        d = dx.reshape(-1, case.c)
        y = ops["y"].reshape(-1, case.c)
        if masked:
            act = y * ops["mscale"] + ops["mshift"]
            d = d * (act >= 0 if mask_ge else act > 0)
        if rs:
            scale = ops["rowscale"].long().repeat_interleave(case.h * case.w)[:, None]
            d = d * scale
            if scale_dx:
                out["dx"] = dx * scale.reshape(case.n, case.h, case.w, 1)
        out["d"] = d
        out["dyc"] = (d * (y - ops["mean"])).double() * ops["invstd"]
        out["s1"], out["s2"] = d.sum(0).double(), out["dyc"].sum(0)
    return out


@functools.lru_cache(maxsize=None)
def expected(name, variant):
    return finish(name, variant, conv_i64(name))


def tile_rows(name, variant, per=256):
    """float64 [ceil(rows / per)][2][c]: the two sums over each run of `per` output rows (what a halo launch writes, one row per tile)"""
    want = expected(name, variant)
    c = BY_NAME[name].c
    pad = (-want["d"].shape[0]) % per
    d = torch.nn.functional.pad(want["d"].double(), (0, 0, 0, pad)).reshape(-1, per, c).sum(1)
    t = torch.nn.functional.pad(want["dyc"], (0, 0, 0, pad)).reshape(-1, per, c).sum(1)
    return torch.stack([d, t], 1)


@functools.lru_cache(maxsize=None)
def bound(name):
    """{"contraction": max |dy| (*) |w| + 8, "dx": largest magnitude of the convolution and of any variant's stored dx,
    "sums": 2 * max_c sum_rows |dx| (|y_bn| + |mean| + 1) max(invstd, 1), or None for a case that runs without BatchNorm partials}"""
    case, ops = BY_NAME[name], operands(name)
    out = {"contraction": int(_conv2d_input_f64(case, ops["dy"].abs(), ops["w"].abs()).max()) + 8}
    conv = conv_i64(name)
    largest = conv.abs()
    for variant in case.variants:
        largest = torch.maximum(largest, expected(name, variant)["dx"].abs())
    out["dx"] = int(largest.max())
    out["sums"] = None
    if any(VARIANTS[v][2] for v in case.variants):
        weight = (ops["y"].abs() + ops["mean"].abs() + 1).double() * ops["invstd"].clamp(min=1.0)
        out["sums"] = float(KEEP_SCALE * (largest.double() * weight).reshape(-1, case.c).sum(0).max())
    return out


# ------------------------------------------------------------------------------------------ the launch (GPU)
GUARD, POISON = 1024.0, float("nan")


def _guarded(elems, guard_elems, dtype, device):
    """a buffer of `elems` poisoned elements between two guards of `guard_elems` elements each -> (whole buffer, interior view)"""
    buf = torch.full((elems + 2 * guard_elems,), GUARD, dtype=dtype, device=device)
    inner = buf[guard_elems:guard_elems + elems]
    inner.fill_(POISON)
    return buf, inner


def guards_untouched(buf, elems, guard_elems):
    return bool((buf[:guard_elems] == GUARD).all()) and bool((buf[guard_elems + elems:] == GUARD).all())


def launch(name, variant, device="cuda"):
    """One launch of the run through its C entry point, under the switches the CALLER has set.  dx and the partial rows live inside larger
    buffers, poisoned with NaN, between guards of 256 rows (dx) / 8 rows (partials) on either side.
    -> (dx [n][h][w][c] on the CPU as float64, partial rows [rows][2][c] as float64 or None, guards untouched)"""
    from frhip import ops as fops
    from frhip._abi import check, lib
    case, data = BY_NAME[name], operands(name)
    entry, res_stride, bn, masked, rs = VARIANTS[variant]
    dtype = torch.bfloat16 if case.dtype == "bf16" else torch.float32
    dev = lambda t, dt=dtype: t.to(dt).to(device).contiguous()
    dy, wt = dev(data["dy"]), dev(data["w"].permute(3, 1, 2, 0))           # wt = frhip_pack_wt(w) = [c][r][s][k]
    res = dev(data["res"]) if res_stride == 1 else dev(data["resc"]) if res_stride == 2 else None
    m = rows(case)
    dx_buf, dx = _guarded(m * case.c, 256 * case.c, dtype, device)
    part_buf = part = None
    stat_rows = lib().frhip_dgrad_stat_rows(*shape_args(case))
    ptr = lambda t: None if t is None else t.data_ptr()
    shape = shape_args(case)[1:]
    if bn:
        part_buf, part = _guarded(stat_rows * 2 * case.c, 8 * 2 * case.c, torch.float32, device)
        y = dev(data["y"])
        f32 = lambda key: dev(data[key], torch.float32)
        mean, invstd, mscale, mshift = f32("mean"), f32("invstd"), f32("mscale") if masked else None, f32("mshift") if masked else None
    dt = dt_code(case)
    if entry == "frhip_conv_dgrad":
        rc = lib().frhip_conv_dgrad(dt, ptr(dy), ptr(wt), ptr(dx), ptr(res), *shape, fops._s())
    elif entry == "frhip_conv_dgrad_bnred":
        rc = lib().frhip_conv_dgrad_bnred(dt, ptr(dy), ptr(wt), ptr(dx), ptr(res), ptr(y), ptr(mean), ptr(invstd), ptr(mscale), ptr(mshift),
                                          ptr(part), *shape, fops._s())
    elif entry == "frhip_conv_dgrad_fused_rs":
        rowscale = dev(data["rowscale"], torch.float32)
        rc = lib().frhip_conv_dgrad_fused_rs(dt, ptr(dy), ptr(wt), ptr(dx), ptr(res), res_stride, ptr(y), ptr(mean), ptr(invstd), ptr(mscale),
                                             ptr(mshift), ptr(rowscale), case.h * case.w, KEEP_SCALE, ptr(part), *shape, fops._s())
    else:
        rc = lib().frhip_conv_dgrad_fused(dt, ptr(dy), ptr(wt), ptr(dx), ptr(res), res_stride or 1, ptr(y) if bn else None,
                                          ptr(mean) if bn else None, ptr(invstd) if bn else None, ptr(mscale) if bn else None,
                                          ptr(mshift) if bn else None, ptr(part), *shape, fops._s())
    check(rc, entry)
    torch.cuda.synchronize()
    clean = guards_untouched(dx_buf, m * case.c, 256 * case.c)
    if bn:
        clean = clean and guards_untouched(part_buf, stat_rows * 2 * case.c, 8 * 2 * case.c)
    return (dx.cpu().double().reshape(case.n, case.h, case.w, case.c),
            part.cpu().double().reshape(stat_rows, 2, case.c) if bn else None, clean)
