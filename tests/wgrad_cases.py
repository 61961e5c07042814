"""Exact-operand cases of the weight gradients (csrc/igemm_tn.hip), one per branch of the launch plan (csrc/tn_plan.h), with their exact
reference.  Shared by tests/test_wgrad_cases_cpu.py (the plans and the references, no GPU) and tests/test_wgrad_exact_gpu.py.

Operands are small integers: x and dy from {-4 .. 4}, the starting dw from {-8 .. 8} (the entry points accumulate), and for the operand
transform scale from {-2, -1, 1, 2} and shift from {-3 .. 3}, so relu(x * scale + shift) <= 11 is an integer bf16 holds.  Every
partial sum of every order of additions is then an integer below 2^24 (`bound` computes max |dy|^T |x| + 8 per case and the CPU test
asserts it; 16 M + 8 at most, M <= 16900 GEMM-K rows): fp32 holds each of them exactly, whatever the K split, the slab layout or the reduce tree.  The comparison is
therefore torch.equal against integers, with no tolerance; one dropped or doubled pixel or one wrong padding lane is an integer off.

The reference is computed twice, independently: torch.nn.grad.conv2d_weight in float64, and a loop over the taps that slices the
zero-padded input and contracts in int64.

A case names the public op, its arguments, the nine-tap switch it runs under and the plan it is meant to hit, as frhip_wgrad_plan reports it:
(family, instantiation, splits, ksteps, ksteps_per_split, store, reduce groups, slabs per group), plus three claims derived from it:
`tree` (groups > 1: the two-level reduce), `short` (ksteps % ksteps_per_split != 0: a short last split) and `mid` (a split of a nine-tap
launch starts inside the lane-mask period: ks_begin % period != 0).

frhip_gemm_tn_overwrite takes no `splits` argument, so its branch "clear `out`, then slabs through the two-level tree" cannot be forced
at m = 4200: the search picks at most (ksteps + 7) / 8 splits and the tree needs more than 32.  The case "gemm overwrite, searched splits,
tree" therefore has m = 16900 rows (34 searched splits, groups 2 x 17), the largest M of the table; its sums stay below 2^24 all the same."""
import collections
import functools
import math
import zlib

import torch

WORKSPACE_BYTES = 160 << 20
TAP128, TAP256, TAPS9, ROWS = 0, 1, 2, 3
OUT, SLABS, OVERWRITE = 0, 1, 2
MAX_TABLE_PERIOD, TABLE_GEOMETRIES = 64, 8

Case = collections.namedtuple("Case", "name op dtype n h w c kc ldp r s stride pad splits taps9 workspace plan tree short mid")


def _conv(name, dims, splits, plan, flags="", op="conv", taps9=1, r=3, stride=1, pad=1):
    n, h, w, c, k = dims
    return Case(name, op, "bf16", n, h, w, c, k, k, r, r, stride, pad, splits, taps9, True, plan, "tree" in flags, "short" in flags, "mid" in flags)


def _gemm(name, dims, splits, plan, flags="", op="gemm", dtype="bf16", workspace=True):
    m, kc, ldp, c = dims
    return Case(name, op, dtype, m, 1, 1, c, kc, ldp, 1, 1, 1, 0, splits, 1, workspace, plan, "tree" in flags, "short" in flags, False)


CASES = [
    # ---- nine-tap kernel: stages 4 / 3 / 2 (instantiation 14 / 13 / 12 with the lane-mask table wanted)
    _conv("8x8, one split into dw", (2, 8, 8, 64, 64), 0, (2, 14, 1, 2, 2, 0, 0, 0)),
    _conv("1x1 maps: every tap but the centre is padding", (130, 1, 1, 64, 64), 3, (2, 14, 3, 3, 1, 1, 1, 3)),
    _conv("3x2 maps: ten images per K step", (50, 3, 2, 64, 64), 100000, (2, 14, 5, 5, 1, 1, 1, 5), "mid"),
    _conv("5x7 maps, ragged c / k / M, short last split", (9, 5, 7, 72, 40), 3, (2, 14, 3, 5, 2, 1, 1, 3), "short mid"),
    _conv("H = 1", (3, 1, 56, 64, 64), 2, (2, 12, 2, 3, 2, 1, 1, 2), "short mid"),
    _conv("W = 1", (3, 56, 1, 64, 64), 2, (2, 14, 2, 3, 2, 1, 1, 2), "short mid"),
    _conv("9x9 maps: period 81, never a table", (4, 9, 9, 64, 64), 2, (2, 14, 2, 6, 3, 1, 1, 2)),
    _conv("W = 15: last width of four stages", (5, 4, 15, 64, 64), 2, (2, 14, 2, 5, 3, 1, 1, 2), "short mid"),
    _conv("W = 16: first width of three stages", (5, 4, 16, 64, 64), 2, (2, 13, 2, 5, 3, 1, 1, 2), "short"),
    _conv("W = 31: last width of three stages, period 93", (5, 3, 31, 64, 64), 2, (2, 13, 2, 8, 4, 1, 1, 2)),
    _conv("W = 32: first width of two stages", (5, 3, 32, 64, 64), 2, (2, 12, 2, 8, 4, 1, 1, 2), "mid"),
    _conv("W = 56: widest nine-tap map", (5, 2, 56, 64, 64), 2, (2, 12, 2, 9, 5, 1, 1, 2), "short mid"),
    _conv("W = 57: handed to the per-tap kernel", (5, 2, 57, 64, 64), 2, (0, 0, 2, 9, 5, 1, 1, 2), "short"),
    _conv("28x28, a split per K step, two-level tree", (5, 28, 28, 64, 64), 100000, (2, 13, 62, 62, 1, 1, 2, 31), "tree mid"),
    _conv("28x28, four splits, short last", (5, 28, 28, 64, 64), 4, (2, 13, 4, 62, 16, 1, 1, 4), "short mid"),
    _conv("28x28, searched splits", (5, 28, 28, 64, 64), 0, (2, 13, 7, 62, 9, 1, 1, 7), "short mid"),
    # ---- nine-tap kernel with the BatchNorm + ReLU operand transform (102 / 103: never a table)
    _conv("transform, two stages", (5, 3, 32, 64, 64), 2, (2, 102, 2, 8, 4, 1, 1, 2), op="bnrelu"),
    _conv("transform, three stages, ragged last K step", (5, 3, 31, 64, 128), 2, (2, 103, 2, 8, 4, 1, 1, 2), op="bnrelu"),
    _conv("transform, one split into dw", (3, 14, 14, 128, 64), 0, (2, 103, 1, 10, 10, 0, 0, 0), op="bnrelu"),
    _conv("transform, two-level tree", (5, 28, 28, 64, 64), 100000, (2, 103, 62, 62, 1, 1, 2, 31), "tree", op="bnrelu"),
    _conv("transform, short last split, ragged last K step", (9, 5, 7, 64, 64), 3, (2, 103, 3, 5, 2, 1, 1, 3), "short", op="bnrelu"),
    # ---- per-tap kernel on 3x3 / stride 1 (nine-tap switch off): 128- and 256-byte tile, nine taps, two-level tree
    _conv("per-tap 3x3, 128-byte tile, tree", (5, 28, 28, 64, 64), 100000, (0, 0, 62, 62, 1, 1, 2, 31), "tree", taps9=0),
    _conv("per-tap 3x3, 256-byte tile, tree", (5, 28, 28, 128, 128), 100000, (1, 0, 62, 62, 1, 1, 2, 31), "tree", taps9=0),
    # ---- per-tap kernel as a plain P^T Q
    _gemm("gemm 64x64, tree", (4200, 64, 64, 64), 100000, (0, 0, 66, 66, 1, 1, 4, 17), "tree"),
    _gemm("gemm 128x128, tree", (4200, 128, 128, 128), 100000, (1, 0, 66, 66, 1, 1, 4, 17), "tree"),
    _gemm("gemm overwrite, searched splits", (4200, 128, 128, 128), 0, (1, 0, 9, 66, 8, 1, 1, 9), "short", op="gemm_overwrite"),
    _gemm("gemm overwrite, searched splits, tree", (16900, 128, 128, 128), 0, (1, 0, 34, 265, 8, 1, 2, 17), "tree short", op="gemm_overwrite"),
    _gemm("gemm overwrite, no workspace", (4200, 128, 128, 128), 0, (1, 0, 1, 66, 66, 2, 0, 0), op="gemm_overwrite", workspace=False),
    _gemm("gemm padded pitch, ragged tiles", (4200, 200, 208, 72), 0, (0, 0, 9, 66, 8, 1, 1, 9), "short"),
    _gemm("gemm fp32, 256-byte tile, tree", (4200, 64, 64, 64), 100000, (1, 0, 66, 66, 1, 1, 4, 17), "tree", dtype="fp32"),
    _gemm("gemm fp32, 128-byte tile, tree", (4200, 64, 64, 32), 100000, (0, 0, 66, 66, 1, 1, 4, 17), "tree", dtype="fp32"),
    # ---- per-tap kernel on the strided convolutions
    _conv("3x3 / stride 2, short last split", (3, 29, 29, 64, 128), 7, (0, 0, 6, 11, 2, 1, 1, 6), "short", r=3, stride=2, pad=1),
    _conv("2x2 / stride 2, one split", (3, 14, 14, 64, 128), 0, (0, 0, 1, 3, 3, 0, 0, 0), r=2, stride=2, pad=0),
    _conv("1x1 / stride 2", (7, 15, 15, 128, 256), 5, (1, 0, 4, 7, 2, 1, 1, 4), "short", r=1, stride=2, pad=0),
    # ---- rows kernel (14 x 14 maps): a split per image
    _conv("rows, 37 images, tree", (37, 14, 14, 64, 128), 0, (3, 0, 37, 37, 1, 1, 2, 19), "tree"),
    _conv("rows, 3 images", (3, 14, 14, 64, 64), 0, (3, 0, 3, 3, 1, 1, 1, 3)),
]
BY_NAME = {case.name: case for case in CASES}

# the fresh process of test_wgrad_exact_gpu.py: eight geometries that can have a lane-mask table, every staged instantiation among them,
# then a ninth, which finds the cache full
CHILD_TABLE_CASES = ["1x1 maps: every tap but the centre is padding", "3x2 maps: ten images per K step",
                     "5x7 maps, ragged c / k / M, short last split", "W = 1", "W = 16: first width of three stages",
                     "28x28, four splits, short last", "H = 1", "W = 32: first width of two stages"]
CHILD_NINTH_CASE = "W = 56: widest nine-tap map"


def period(h, w):
    """K steps after which the padding lane masks of h x w maps repeat"""
    return h * w // math.gcd(h * w, 64)


def nine_tap(case):
    return case.plan[0] == TAPS9


def wants_table(case):
    return nine_tap(case) and case.plan[1] in (12, 13, 14)


def table_capable(case):
    """the launch asks for a lane-mask table and its geometry can have one (whether the cache has room is known at the launch only)"""
    return wants_table(case) and period(case.h, case.w) <= MAX_TABLE_PERIOD


def overwrite(case):
    return case.op == "gemm_overwrite"


def clears_output(case):
    return overwrite(case) and case.plan[2] > 1


def plan_args(case):
    """the arguments of frhip_wgrad_plan for this case"""
    dt = 0 if case.dtype == "bf16" else 1
    return (dt, case.n, case.h, case.w, case.c, case.kc, case.ldp, case.r, case.s, case.stride, case.pad, case.splits,
            int(case.workspace), WORKSPACE_BYTES if case.workspace else 0, int(overwrite(case)), int(case.op == "bnrelu"))


def derived_claims(case):
    """(tree, short, mid) from the case's plan and geometry"""
    family, inst, splits, ksteps, per, store, groups, per_group = case.plan
    mid = table_capable(case) and any((i * per) % period(case.h, case.w) for i in range(splits))
    return groups > 1, ksteps % per != 0, mid


def out_hw(case):
    return (case.h + 2 * case.pad - case.r) // case.stride + 1, (case.w + 2 * case.pad - case.s) // case.stride + 1


def gemm_rows(case):
    ho, wo = out_hw(case)
    return case.n * ho * wo


def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def operands(name):
    """int64 CPU tensors of a case: x [n][h][w][c], dy [n][ho][wo][kc], dw0 [kc][r][s][c], and for the transform scale [c], shift [c]"""
    case = BY_NAME[name]
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    ho, wo = out_hw(case)
    ops = {"x": _ints(gen, (case.n, case.h, case.w, case.c), -4, 4), "dy": _ints(gen, (case.n, ho, wo, case.kc), -4, 4),
           "dw0": _ints(gen, (case.kc, case.r, case.s, case.c), -8, 8)}
    if case.op == "bnrelu":
        ops["scale"] = torch.tensor([-2, -1, 1, 2])[_ints(gen, (case.c,), 0, 3)]
        ops["shift"] = _ints(gen, (case.c,), -3, 3)
    return ops


def activated(name):
    """the int64 tensor the gradient contracts dy with: x, or relu(x * scale + shift) under the operand transform"""
    ops = operands(name)
    return (ops["x"] * ops["scale"] + ops["shift"]).clamp_(min=0) if "scale" in ops else ops["x"]


def _conv2d_weight_f64(case, q, p):
    if case.h == 1 and case.w == 1 and case.r == 1:
        return (p.reshape(case.n, case.kc).double().t() @ q.reshape(case.n, case.c).double()).reshape(case.kc, 1, 1, case.c)
    g = torch.nn.grad.conv2d_weight(q.permute(0, 3, 1, 2).double(), (case.kc, case.c, case.r, case.s), p.permute(0, 3, 1, 2).double(),
                                    case.stride, case.pad)
    return g.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def reference_f64(name):
    """[kc][r][s][c] float64: torch.nn.grad.conv2d_weight (a matrix product where the case is one)"""
    return _conv2d_weight_f64(BY_NAME[name], activated(name), operands(name)["dy"])


@functools.lru_cache(maxsize=None)
def reference_i64(name):
    """[kc][r][s][c] int64: tap by tap, slices of the zero-padded input against dy"""
    case = BY_NAME[name]
    ho, wo = out_hw(case)
    q = torch.nn.functional.pad(activated(name), (0, 0, case.pad, case.pad, case.pad, case.pad))
    p = operands(name)["dy"].reshape(-1, case.kc).t().contiguous()
    out = torch.empty((case.kc, case.r, case.s, case.c), dtype=torch.int64)
    for fr in range(case.r):
        for fs in range(case.s):
            tap = q[:, fr:fr + case.stride * (ho - 1) + 1:case.stride, fs:fs + case.stride * (wo - 1) + 1:case.stride]
            out[:, fr, fs] = p @ tap.reshape(-1, case.c)
    return out


@functools.lru_cache(maxsize=None)
def bound(name):
    """an upper bound of the magnitude of every partial sum the launch can form, in any order: max over dw of |dy|^T |x| + |dw0|"""
    return int(_conv2d_weight_f64(BY_NAME[name], activated(name).abs(), operands(name)["dy"].abs()).max()) + 8


@functools.lru_cache(maxsize=None)
def expected(name):
    """float64 [kc][r][s][c]: what dw must hold after one launch, to the bit"""
    ref = reference_i64(name)
    return (ref if overwrite(BY_NAME[name]) else ref + operands(name)["dw0"]).double()


def launch(name, device="cuda"):
    """One launch of the case through its public op, under its nine-tap switch; -> dw on the CPU, float64.  The mask-table switch is the
    caller's.  P of the gemm cases has NaN in its padding columns kc .. ldp; `out` of the overwrite cases starts as NaN."""
    import ctypes
    from frhip import ops
    from frhip._abi import check, lib
    case = BY_NAME[name]
    data = operands(name)
    dtype = torch.bfloat16 if case.dtype == "bf16" else torch.float32
    ho, wo = out_hw(case)
    p = torch.full((case.n, ho, wo, case.ldp), float("nan"), dtype=dtype)
    p[..., :case.kc] = data["dy"].to(dtype)
    p, x = p.to(device), data["x"].to(dtype).to(device)
    dw = data["dw0"].float().to(device)
    if overwrite(case):
        dw.fill_(float("nan"))
    old = lib().frhip_set_wgrad_taps9(case.taps9)
    try:
        if case.op == "conv":
            ops.conv_wgrad(p, x, dw, case.r, case.s, case.stride, case.pad, case.splits)
        elif case.op == "bnrelu":
            st = ops.BNState()
            st.scale, st.shift = data["scale"].float().to(device), data["shift"].float().to(device)
            ops.conv_wgrad_bnrelu(p, x, st, dw, case.r, case.s, case.stride, case.pad, case.splits)
        elif case.workspace:
            ops.gemm_tn(p.reshape(case.n, case.ldp), x.reshape(case.n, case.c), dw.reshape(case.kc, case.c), kc=case.kc, splits=case.splits,
                        overwrite=overwrite(case))
        else:
            assert overwrite(case)
            check(lib().frhip_gemm_tn_overwrite(ops.dt_of(p), p.data_ptr(), x.data_ptr(), dw.data_ptr(), case.n, case.kc, case.ldp, case.c,
                                                None, ctypes.c_size_t(0), ops._s()), "frhip_gemm_tn_overwrite")
    finally:
        lib().frhip_set_wgrad_taps9(old)
    return dw.cpu().double()
