"""Exact-operand cases of the recompute-style stem (csrc/stem_fused.hip, csrc/stem_algebra.hip) with their exact reference.  TEST-ONLY.
Shared by tests/test_stem_cases_cpu.py (the reference, the value bounds and the coverage of every case, no GPU) and
tests/test_stem_exact_gpu.py.

Operands are small integers and halves, drawn from a seeded generator per case:
  x {-1, 0, 1} fp32 NCHW; w [64][27] {-1, 0, 1}; scale {0.5, 1, 2, -1} per channel; shift -4 .. 4; dpool -2 .. 2; mean -2 .. 2;
  invstd {0.5, 1, 2}; ca {1, 2, -1}; cb {0, 1, -1, 0.5}; cc -3 .. 3; the starting dw a non-zero integer pattern (the entry points add).
Then |y| <= 27, |a| = relu(y scale + shift) <= 58 in steps of 0.5 (7 significant bits), |d| <= 8 (at most four windows reach a pixel),
|dy| = |ca d + cb y + cc| <= 46.5 in steps of 0.5 -- also every intermediate of the scatter kernel's bf16 read-modify-write -- and every
sum (sum y, sum y^2, sum d, sum d y, dW, G, s, D, dx) is an integer or a half far below 2^24: bf16 holds every element and fp32 every
sum of every order of additions exactly.  The comparison is therefore torch.equal, with no tolerance: one dropped pixel, one window read
from the wrong neighbour tile or a ReLU mask that differs at y scale + shift == 0 is at least a half off.  `bounds` computes the worst
magnitudes per case and the CPU test asserts them.

The reference below is plain torch in float64 (exact on these operands: every value is a multiple of 1/8 below 2^30) with no call into
frhip, written from the specification in include/frhip.h and the header comments of the two .hip files:
  col[p][j] = the 27 inputs under pixel p, zero padded, j = (fr 3 + fs) 3 + ci;  y = col w^T;  a = relu(y scale + shift);
  pooled = max over the in-image taps of the 3x3 / stride 2 / pad 1 window, arg = the FIRST maximum in row-major tap order (also where
  the maximum is 0);  d = dpool routed to its arg-max pixel, times (y scale + shift > 0);
  reduce = { sum d, invstd (sum d y - mean sum d) };  dy = ca d + cb y + cc;  dW = sum_p dy col;
  G = sum_p col col^T, s = sum_p col, D = sum over pooled elements with pooled > 0 of dpool col[arg-max pixel], dW = ca D + cb (w G) + cc s;
  dx = conv^T(dy0) with dy0 = ca d (+ cb y + cc), d masked by pooled > 0;  stride 2: dx = col2im(dy0 w^T).

A case is (b, h, w) and what it is there for; CASES lists the reason next to each.  `only` restricts a case to one entry point and
`dtypes` to one element type (the widest rows the statistics and Gram kernels accept)."""
import collections
import functools
import zlib

import torch

PH, PW = 4, 28              # pooled tile of the forward / backward kernels: 8 x 56 activation pixels
STATS_ROWS, STATS_STEP = 8, 16
DX_TILE, DG_TILE = 16, 8
STEM_BLOCKS_CAP, GRAM_BLOCKS_CAP, GRAM_ROWS = 1024, 512, 8
GRAM_FLOATS, GRAM_OUT = 27 * 27 + 27, 7 * 81

Case = collections.namedtuple("Case", "name b h w why only dtypes salt")


def _case(b, h, w, why, only=None, dtypes=("fp32", "bf16"), salt=0):
    return Case("%dx%dx%d" % (b, h, w), b, h, w, why, only, dtypes, salt)


CASES = [
    # ---- degenerate maps
    _case(1, 1, 1, "one pixel: every tap but the centre is padding"),
    _case(2, 1, 5, "one row"),
    _case(2, 5, 1, "one column"),
    _case(2, 2, 2, "one pooled pixel per image"),
    # ---- pooled-tile edges in H: Hp = 4 | 4 | 5, the second tile row has one pooled row whose window reaches past the image
    _case(2, 7, 6, "H below the tile edge"),
    _case(2, 8, 6, "H at the tile edge"),
    _case(2, 9, 6, "H past the tile edge: second tile row of one pooled row"),
    # ---- pooled-tile edges in W
    _case(1, 3, 55, "W below the tile edge"),
    _case(1, 3, 56, "W at the tile edge"),
    _case(1, 3, 57, "W past the tile edge: second tile column of one pooled column"),
    _case(2, 9, 57, "both edges: arg-max pixels in the tile above, to the left and diagonally"),
    _case(1, 17, 113, "three tile rows and three tile columns"),
    # ---- the 16-pixel step of the statistics kernel and the wave row pairs of its 8-row band
    _case(1, 2, 15, "statistics: W below the 16-pixel step"),
    _case(1, 2, 16, "statistics: W at the 16-pixel step"),
    _case(1, 2, 17, "statistics: W past the 16-pixel step"),
    _case(1, 3, 4, "statistics: a wave with one row of its pair"),
    _case(1, 8, 4, "statistics: a full 8-row band"),
    _case(1, 9, 4, "statistics: second band of one row"),
    # ---- stem_dx_kernel's 16 x 16 tile
    _case(2, 16, 16, "dx: one whole tile"),
    _case(2, 17, 16, "dx: second tile row of one pixel row"),
    _case(2, 16, 17, "dx: second tile column of one pixel column"),
    # ---- stem_dgather_kernel's 8 x 8 pooled tile against the 4 x 28 grid that launches it
    _case(1, 3, 40, "gather: 1 workgroup, 3 tiles (strides with the register prefetch)"),
    _case(1, 20, 3, "gather: 3 workgroups, 2 tiles (the idle workgroup writes a zero slab)"),
    _case(1, 16, 16, "gather: one whole tile"),
    _case(1, 17, 17, "gather: past the tile edge both ways"),
    # ---- both grid caps: 1030 tiles over 1024 workgroups, 1030 Gram bands over 512
    _case(1030, 3, 3, "second (and third) trip of every grid-stride loop"),
    # ---- widest accepted rows
    _case(1, 2, 544, "statistics: widest fp32 row", only="stats", dtypes=("fp32",)),
    _case(1, 2, 1090, "statistics: widest bf16 row", only="stats", dtypes=("bf16",)),
    _case(1, 2, 510, "Gram: widest row", only="gram"),
]
BY_NAME = {case.name: case for case in CASES}
FULL = [case for case in CASES if case.only is None]

# one past the widest rows: refused on the host, before any device call -> (entry point, dtype, b, h, w, message)
DT_BF16, DT_F32 = 0, 1
REFUSALS = [
    ("frhip_stem_stats", DT_F32, 1, 2, 545, "frhip_stem_stats: image too wide (545)"),
    ("frhip_stem_stats", DT_BF16, 1, 2, 1091, "frhip_stem_stats: image too wide (1091)"),
    ("frhip_stem_gram", DT_F32, 1, 2, 511, "frhip_stem_gram: unsupported dtype / shape (dtype=1 b=1 h=2 w=511)"),
    ("frhip_stem_gram", DT_BF16, 1, 2, 511, "frhip_stem_gram: unsupported dtype / shape (dtype=0 b=1 h=2 w=511)"),
]

# frhip_stem_dx_s2 (stride-2 im2col stem): (b, h, w, kp)
S2_CASES = [(b, h, w, kp) for (b, h, w) in ((1, 1, 1), (2, 2, 2), (2, 5, 4), (2, 4, 5), (3, 9, 7)) for kp in (32, 64)]


def pooled_hw(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def tiles(case):
    """(tile rows, tile columns) of the 4 x 28 pooled grid"""
    hp, wp = pooled_hw(case.h, case.w)
    return (hp + PH - 1) // PH, (wp + PW - 1) // PW


def stem_blocks(case):
    th, tw = tiles(case)
    return min(case.b * th * tw, STEM_BLOCKS_CAP)


def gram_blocks(case):
    return min(case.b * ((case.h + GRAM_ROWS - 1) // GRAM_ROWS), GRAM_BLOCKS_CAP)


def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen, dtype=torch.int64).double()


def _pick(gen, values, shape):
    return torch.tensor(values, dtype=torch.float64)[torch.randint(0, len(values), shape, generator=gen)]


@functools.lru_cache(maxsize=None)
def operands(name):
    """float64 CPU tensors of a case: x [b][3][h][w], w [64][27], dpool [b][hp][wp][64], dw0 [64][27], the per-channel vectors [64]"""
    case = BY_NAME[name]
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()) + case.salt)
    hp, wp = pooled_hw(case.h, case.w)
    ops = {"x": _ints(gen, (case.b, 3, case.h, case.w), -1, 1), "w": _ints(gen, (64, 27), -1, 1),
           "scale": _pick(gen, (0.5, 1.0, 2.0, -1.0), (64,)), "shift": _ints(gen, (64,), -4, 4),
           "dpool": _ints(gen, (case.b, hp, wp, 64), -2, 2), "mean": _ints(gen, (64,), -2, 2),
           "invstd": _pick(gen, (0.5, 1.0, 2.0), (64,)), "ca": _pick(gen, (1.0, 2.0, -1.0), (64,)),
           "cb": _pick(gen, (0.0, 1.0, -1.0, 0.5), (64,)), "cc": _ints(gen, (64,), -3, 3)}
    j = torch.arange(64 * 27, dtype=torch.float64).reshape(64, 27)
    ops["dw0"] = (j % 7 + 1) * (1 - 2 * (j % 2))             # 1 .. 7 with alternating sign: never zero
    return ops


@functools.lru_cache(maxsize=None)
def s2_operands(b, h, w):
    """dy0 [b][ho][wo][64]: halves within +-46.5, the range of the stem's dy;  w [64][27] {-1, 0, 1}"""
    gen = torch.Generator().manual_seed(zlib.crc32(("s2 %d %d %d" % (b, h, w)).encode()))
    ho, wo = pooled_hw(h, w)
    return {"dy0": _ints(gen, (b, ho, wo, 64), -93, 93) / 2, "w": _ints(gen, (64, 27), -1, 1)}


# ---------------------------------------------------------------------------------------------------------------------- the reference
def im2col(x):
    """x [b][3][h][w] -> col [b][h][w][27], j = (fr 3 + fs) 3 + ci, zero padded"""
    b, _, h, w = x.shape
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1))
    col = x.new_empty((b, h, w, 27))
    for fr in range(3):
        for fs in range(3):
            for ci in range(3):
                col[..., (fr * 3 + fs) * 3 + ci] = xp[:, ci, fr:fr + h, fs:fs + w]
    return col


def pool_first_max(a):
    """a [b][h][w][c] -> (pooled [b][hp][wp][c], arg int64: tap index r 3 + s of the first maximum among the in-image taps)"""
    b, h, w, c = a.shape
    hp, wp = pooled_hw(h, w)
    ap = a.new_full((b, h + 2, w + 2, c), float("-inf"))
    ap[:, 1:h + 1, 1:w + 1] = a
    taps = torch.stack([ap[:, r:r + 2 * hp - 1:2, s:s + 2 * wp - 1:2] for r in range(3) for s in range(3)])
    pooled = taps.max(0).values
    index = torch.arange(9).view(9, 1, 1, 1, 1).expand_as(taps)
    arg = torch.where(taps == pooled, index, torch.full_like(index, 9)).min(0).values
    return pooled, arg, taps


def argmax_pixel(arg):
    """arg [b][hp][wp][c] -> image coordinates (hh, ww) of the arg-max pixel of every pooled element"""
    _, hp, wp, _ = arg.shape
    hh = 2 * torch.arange(hp).view(1, hp, 1, 1) - 1 + arg // 3
    ww = 2 * torch.arange(wp).view(1, 1, wp, 1) - 1 + arg % 3
    return hh, ww


def route(dpool, arg, h, w):
    """the max-pool backward: [b][h][w][c], every pooled gradient added at its arg-max pixel"""
    b, hp, wp, c = dpool.shape
    hh, ww = argmax_pixel(arg)
    out = dpool.new_zeros((b, h * w, c))
    out.scatter_add_(1, (hh * w + ww).reshape(b, hp * wp, c), dpool.reshape(b, hp * wp, c))
    return out.view(b, h, w, c)


def col2im(t, h, w, stride):
    """t [b][ho][wo][27] -> [b][3][h][w]: entry j = (fr 3 + fs) 3 + ci of output pixel (a, b) lands on input pixel
    (stride a - 1 + fr, stride b - 1 + fs) of channel ci (conv3x3 / pad 1)"""
    b, ho, wo, _ = t.shape
    out = t.new_zeros((b, 3, stride * ho + 2, stride * wo + 2))
    for fr in range(3):
        for fs in range(3):
            for ci in range(3):
                out[:, ci, fr:fr + stride * (ho - 1) + 1:stride, fs:fs + stride * (wo - 1) + 1:stride] += t[..., (fr * 3 + fs) * 3 + ci]
    return out[:, :, 1:h + 1, 1:w + 1].contiguous()


def stem_forward(x, w27, scale, shift):
    """-> dict(col, y [b][h][w][64], sum_y, sum_y2, a, pooled, arg, taps)"""
    col = im2col(x)
    y = col @ w27.t()
    a = (y * scale + shift).clamp_min(0.0)
    pooled, arg, taps = pool_first_max(a)
    return dict(col=col, y=y, sum_y=y.sum((0, 1, 2)), sum_y2=(y * y).sum((0, 1, 2)), a=a, pooled=pooled, arg=arg, taps=taps)


def stem_reduce(fwd, scale, shift, dpool, mean, invstd):
    """-> (d [b][h][w][64], reduce [2][64] = { sum d, invstd (sum d y - mean sum d) }): the sums of the BatchNorm backward"""
    y = fwd["y"]
    d = route(dpool, fwd["arg"], y.shape[1], y.shape[2]) * (y * scale + shift > 0)
    sd, sdy = d.sum((0, 1, 2)), (d * y).sum((0, 1, 2))
    return d, torch.stack([sd, invstd * (sdy - mean * sd)])


def stem_backward(x, w27, scale, shift, fwd, dpool, mean, invstd, ca, cb, cc):
    """-> dict(d, reduce [2][64], dy, dw [64][27], gram [756], D, dw_gram, dx, dx_eval) from the forward's dict and the coefficients"""
    b, _, h, w = x.shape
    col, y, arg, pooled = fwd["col"], fwd["y"], fwd["arg"], fwd["pooled"]
    d, reduce = stem_reduce(fwd, scale, shift, dpool, mean, invstd)
    dy = ca * d + cb * y + cc
    dw = torch.einsum("bhwk,bhwj->kj", dy, col)
    flat = col.reshape(-1, 27)
    g, s = flat.t() @ flat, flat.sum(0)
    # D from the pooled side: the im2col row of every pooled element's arg-max pixel, under the mask pooled > 0
    hh, ww = argmax_pixel(arg)
    rows = col[torch.arange(b).view(b, 1, 1, 1), hh, ww]                          # [b][hp][wp][64][27]
    dmat = torch.einsum("bpqk,bpqkj->kj", dpool * (pooled > 0), rows)
    dw_gram = ca[:, None] * dmat + cb[:, None] * (w27 @ g) + cc[:, None] * s[None, :]
    d_pooled = route(dpool * (pooled > 0), arg, h, w)
    dx = col2im((ca * d_pooled + cb * y + cc) @ w27, h, w, 1)
    dx_eval = col2im((ca * d_pooled) @ w27, h, w, 1)
    return dict(d=d, d_pooled=d_pooled, reduce=reduce, dy=dy, dw=dw,
                gram=torch.cat([g.reshape(-1), s]), D=dmat, dw_gram=dw_gram, dx=dx, dx_eval=dx_eval)


def stem_dx_s2(dy0, w27, h, w):
    """dx [b][3][h][w] = col2im(dy0 w^T) of conv3x3 / stride 2 / pad 1"""
    return col2im(dy0 @ w27, h, w, 2)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the forward and backward dicts of a case, merged; computed once, shared, never changed by a test"""
    ops = operands(name)
    fwd = stem_forward(ops["x"], ops["w"], ops["scale"], ops["shift"])
    if BY_NAME[name].only is not None:                     # the wide rows: statistics and Gram only
        flat = fwd["col"].reshape(-1, 27)
        return dict(fwd, gram=torch.cat([(flat.t() @ flat).reshape(-1), flat.sum(0)]))
    bwd = stem_backward(ops["x"], ops["w"], ops["scale"], ops["shift"], fwd, ops["dpool"], ops["mean"], ops["invstd"], ops["ca"], ops["cb"],
                        ops["cc"])
    return dict(fwd, **bwd)


@functools.lru_cache(maxsize=None)
def bounds(name):
    """the largest magnitude of each quantity of a case, and of every sum in any order of additions (the sum of the magnitudes)"""
    ops, ref = operands(name), reference(name)
    out = {"y": float(ref["y"].abs().max()), "a": float(ref["a"].abs().max()),
           "sum_y": float(ref["y"].abs().sum((0, 1, 2)).max()), "sum_y2": float(ref["sum_y2"].max()),
           "gram": float(ref["col"].abs().reshape(-1, 27).sum(0).max())}     # |col| <= 1: bounds G and s alike
    if BY_NAME[name].only is None:
        col, y, w27 = ref["col"].abs(), ref["y"].abs(), ops["w"].abs()
        ca, cb, cc = ops["ca"].abs(), ops["cb"].abs(), ops["cc"].abs()
        dabs = route(ops["dpool"].abs(), ref["arg"], BY_NAME[name].h, BY_NAME[name].w)
        dyabs = ca * dabs + cb * y + cc                                        # every intermediate of the read-modify-write
        g = col.reshape(-1, 27).t() @ col.reshape(-1, 27)
        out.update(d=float(dabs.max()), dy=float(dyabs.max()), sum_d=float(dabs.sum((0, 1, 2)).max()),
                   sum_dy=float((dabs * y).sum((0, 1, 2)).max()),
                   reduce=float((ops["invstd"] * ((dabs * y).sum((0, 1, 2)) + ops["mean"].abs() * dabs.sum((0, 1, 2)))).max()),
                   dw=float(torch.einsum("bhwk,bhwj->kj", dyabs, col).max()) + 7,
                   dw_gram=float((ca[:, None] * torch.einsum("bhwk,bhwj->kj", dabs, col) + cb[:, None] * (w27 @ g) +
                                  cc[:, None] * col.reshape(-1, 27).sum(0)[None, :]).max()) + 7,
                   dx=float(col2im(dyabs @ w27, BY_NAME[name].h, BY_NAME[name].w, 1).max()))
    return out


def claims(case):
    """what the case must exercise, from its geometry alone (tests/test_stem_cases_cpu.py asserts each against the reference)"""
    th, tw = tiles(case)
    out = {"zero", "mask"}
    if case.h * case.w > 1:
        out.add("tie")
    if case.h >= 3 and case.w >= 3:
        out.add("taps")
    if case.h >= 3:
        out.add("two windows, row pair")
    if case.w >= 3:
        out.add("two windows, column pair")
    if case.h >= 3 and case.w >= 3:
        out.add("two windows, diagonal")
    if th > 1:
        out.add("arg-max in the tile above")
    if tw > 1:
        out.add("arg-max in the tile to the left")
    if th > 1 and tw > 1:
        out.add("arg-max in the tile diagonally")
    return out


@functools.lru_cache(maxsize=None)
def coverage(name):
    """the claims the reference of the case fulfils"""
    case, ops, ref = BY_NAME[name], operands(name), reference(name)
    arg, pooled, taps, dpool = ref["arg"], ref["pooled"], ref["taps"], ops["dpool"]
    hp, wp = pooled_hw(case.h, case.w)
    out = set()
    if set(arg.unique().tolist()) == set(range(9)):
        out.add("taps")
    if bool((((taps == pooled).sum(0) > 1) & (pooled > 0) & (dpool != 0)).any()):      # a tie whose choice the backward pass sees
        out.add("tie")
    if bool((pooled == 0).any()):
        out.add("zero")
    unmasked = route(dpool, arg, case.h, case.w)
    if bool(((ref["y"] * ops["scale"] + ops["shift"] == 0) & (unmasked != 0)).any()):
        out.add("mask")
    # windows whose arg-max is the same pixel: compare the pixel of window (p, q) with that of (p + 1, q), (p, q + 1), (p + 1, q + 1)
    hh, ww = argmax_pixel(arg)
    pix = (hh * case.w + ww).expand_as(arg)
    if hp > 1 and bool((pix[:, 1:] == pix[:, :-1]).any()):
        out.add("two windows, row pair")
    if wp > 1 and bool((pix[:, :, 1:] == pix[:, :, :-1]).any()):
        out.add("two windows, column pair")
    if hp > 1 and wp > 1 and bool(((pix[:, 1:, 1:] == pix[:, :-1, :-1]) | (pix[:, 1:, :-1] == pix[:, :-1, 1:])).any()):
        out.add("two windows, diagonal")
    # the tile of a window against the tile that owns its arg-max pixel (a 4 x 28 pooled tile owns 8 x 56 activation pixels); only
    # windows that carry a gradient the ReLU mask lets through count
    live = (dpool != 0) & (pooled > 0)
    dth = (hh // (2 * PH) - torch.arange(hp).view(1, hp, 1, 1) // PH).expand_as(arg)
    dtw = (ww // (2 * PW) - torch.arange(wp).view(1, 1, wp, 1) // PW).expand_as(arg)
    assert int(dth.min()) >= -1 and int(dth.max()) <= 0 and int(dtw.min()) >= -1 and int(dtw.max()) <= 0
    if bool((live & (dth == -1) & (dtw == 0)).any()):
        out.add("arg-max in the tile above")
    if bool((live & (dth == 0) & (dtw == -1)).any()):
        out.add("arg-max in the tile to the left")
    if bool((live & (dth == -1) & (dtw == -1)).any()):
        out.add("arg-max in the tile diagonally")
    return out


# ---------------------------------------------------------------------------------------------------------------------- device side
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
PAD_BYTES = 256


def packed_weights(w27, dtype, kp=32):
    """what frhip_pack_stem(w, 64, 27, kp) writes: [64][kp] in `dtype`, zeros from column 27 on"""
    out = torch.zeros((64, kp), dtype=torch.float64)
    out[:, :27] = w27
    return out.to(dtype)


class Guarded:
    """Device buffers between canaries.  Every buffer is carved out of an allocation made under tests/poison.py's poisoned_empty(nan)
    with PAD_BYTES on both sides: floating-point buffers start as NaN, byte buffers as 0xFF, canaries included.  `put` copies an operand
    in, `out` leaves the poison for the kernel to overwrite; `check` asserts that no canary changed."""

    def __init__(self, device="cuda"):
        self.device, self.items = device, []

    def out(self, shape, dtype, what):
        import poison
        n = 1
        for s in shape:
            n *= s
        pad = PAD_BYTES // torch.empty((), dtype=dtype).element_size()
        with poison.poisoned_empty(float("nan")):
            raw = torch.empty((n + 2 * pad,), dtype=dtype, device=self.device)
        if not dtype.is_floating_point:
            raw.fill_(0xFF)
        assert poison.holds(raw, float("nan") if dtype.is_floating_point else 0xFF), what
        self.items.append((what, raw, pad, n))
        return raw[pad:pad + n].view(shape)

    def put(self, t, dtype, what):
        buf = self.out(tuple(t.shape), dtype, what)
        buf.copy_(t.to(dtype))
        return buf

    def check(self):
        import poison
        for what, raw, pad, n in self.items:
            pattern = float("nan") if raw.dtype.is_floating_point else 0xFF
            assert poison.holds(raw[:pad], pattern), "the canary in front of %s changed" % what
            assert poison.holds(raw[pad + n:], pattern), "the canary behind %s changed" % what
