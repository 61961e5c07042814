"""The BatchNorm statistic reductions (csrc/bn.hip and the store epilogues that produce the same partial rows) held to EXACT sums.

With small-integer data every partial and every total is an integer (or a dyadic fraction) below 2^24, so fp32 adds it without rounding in
any order: whatever tree a kernel uses, its result must be the bits of the float64 / int64 sum.  Each test asserts those conditions on its
inputs before it calls a kernel.  Values behind a rounded operation are held to  (rounded operations + 1) * 2^-24  (+ 2^-23 behind rsqrtf,
which is documented at 1 ulp); the operations are counted beside each assertion.  tests/bn_double.py is the reference of the formulas
(tests/test_bn_double_cpu.py holds it against float64 F.batch_norm and autograd)."""
import functools
import math

import numpy as np
import pytest
import torch

import bn_double

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                      # unit roundoff of fp32
EXACT = 2 ** 24                     # integers below it are fp32 values
CANARY = -24680.0
GUARD = 256                         # floats of canary beside every buffer
EPS = float(np.float32(1e-5))       # the constants as the kernels receive them (float arguments)
M01 = float(np.float32(0.1))


def _ops():
    from frhip import ops
    return ops


def _lib():
    from frhip._abi import lib
    return lib()


class Guarded:
    """a device buffer of `shape` with GUARD canary floats in front of it and behind it"""

    def __init__(self, shape, fill=None, dtype=torch.float32):
        assert dtype == torch.float32
        n = int(np.prod(shape))
        self.full = torch.full((GUARD + n + GUARD,), CANARY, dtype=dtype, device="cuda")
        self.t = self.full[GUARD:GUARD + n].view(shape)
        if fill is not None:
            if torch.is_tensor(fill):
                self.t.copy_(fill.to(dtype).reshape(shape))
            else:
                self.t.fill_(fill)

    @property
    def p(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.full[:GUARD] == CANARY).all()) and bool((self.full[-GUARD:] == CANARY).all())


def _close(got, want, rel, what):
    """|got - want| <= rel * |want|, element-wise"""
    got, want = got.double().cpu(), want.double()
    err = (got - want).abs()
    lim = rel * want.abs()
    assert bool((err <= lim).all()), (what, float((err / want.abs().clamp_min(1e-300)).max() / U), "units of 2^-24; allowed", rel / U)


def _close_abs(got, want, rel, mag, what):
    """|got - want| <= rel * mag: for differences, mag = the sum of the magnitudes of their terms"""
    got, want = got.double().cpu(), want.double()
    err = (got - want).abs()
    assert bool((err <= rel * mag).all()), (what, float((err / mag.clamp_min(1e-300)).max() / U), "units of 2^-24; allowed", rel / U)


def _is_pow2(v):
    m, _ = np.frexp(np.asarray(v, dtype=np.float64))
    return bool(np.all(m == 0.5))


def _ints(seed, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed))


def _pick(seed, n, values):
    return torch.tensor(values, dtype=torch.float64)[_ints(seed, (n,), 0, len(values) - 1)]


# =============================================================================================== (a) finalize trees
@functools.lru_cache(maxsize=2)
def _partials(nparts, c):
    """[nparts][2][c] integer partial rows: sum rows in [-8, 8], sum-of-squares rows in [8, 16] (no row is zero, so no row can go missing
    unseen)"""
    s1 = _ints(1000 + nparts * 7 + c, (nparts, c), -8, 8)
    s2 = _ints(2000 + nparts * 7 + c, (nparts, c), 8, 16)
    return torch.stack([s1, s2], dim=1).double()


def _assert_exact_partials(p, count):
    assert torch.equal(p, p.round())
    assert float(p[:, 0].abs().max()) <= 8 and float(p[:, 1].min()) >= 0 and float(p[:, 1].max()) <= 16
    assert float(p.abs().sum(0).max()) < EXACT
    assert count >= 1 and _is_pow2(count)


def _count_for(nparts):
    """a power of two >= 16 nparts: with |s1 row| <= 8 and s2 row >= 8,  2 mean^2 <= 128 n^2 / count^2 <= 8 n / count <= E[x^2], i.e.
    mean^2 <= var -- the rounding of mean * mean is then at most 2^-24 var and counts as ONE rounded operation on var (the cancellation of
    E[x^2] - mean^2 at large mean / sigma is a property of the design and not this test's subject)"""
    return float(2 ** math.ceil(math.log2(16 * nparts)))


def _finalize(p, c, count, gamma, beta, rm, rv, momentum):
    """frhip_bn_finalize on guarded buffers -> dict of CPU results; asserts every canary and that the inputs are unchanged"""
    ops, lib = _ops(), _lib()
    nparts = p.shape[0]
    parts, scratch = Guarded((nparts, 2, c), p), Guarded((64 * 2 * c,), float("nan"))
    g, b = Guarded((c,), gamma), Guarded((c,), beta)
    out = {k: Guarded((c,), float("nan")) for k in ("mean", "invstd", "scale", "shift")}
    run = {k: Guarded((c,), v) for k, v in (("rm", rm), ("rv", rv))} if rm is not None else {}
    ops.check(lib.frhip_bn_finalize(parts.p, nparts, scratch.p, c, float(count), g.p, b.p, run["rm"].p if run else None,
                                    run["rv"].p if run else None, float(momentum), EPS, out["mean"].p, out["invstd"].p, out["scale"].p,
                                    out["shift"].p, ops._s()), "frhip_bn_finalize")
    torch.cuda.synchronize()
    for name, buf in [("partials", parts), ("scratch", scratch), ("gamma", g), ("beta", b)] + list(out.items()) + list(run.items()):
        assert buf.intact(), "canary beside %s" % name
    assert torch.equal(parts.t.cpu().double(), p)
    res = {k: v.t.cpu() for k, v in out.items()}
    res.update({k: v.t.cpu() for k, v in run.items()})
    return res


def _check_forward(p, c, count, momentum=M01, running=True, seed=0, generic=True):
    _assert_exact_partials(p, count)
    gamma = _pick(31 + seed, c, [0.5, 1.0, 2.0, 4.0])
    beta = _ints(32 + seed, (c,), -3, 3).double()
    assert _is_pow2(gamma.numpy())
    rm = _ints(33 + seed, (c,), -4, 4).double() * 0.25 if running else None
    rv = _ints(34 + seed, (c,), 1, 8).double() * 0.25 if running else None
    s = p.sum(0)
    ref = bn_double.forward(s[0], s[1], count, gamma, beta, rm, rv, momentum, EPS)
    if generic:
        assert bool((ref["mean"] ** 2 <= ref["var"]).all())          # see _count_for
    got = _finalize(p, c, count, gamma, beta, rm, rv, momentum)
    # mean = s1 / count: an exact sum divided by a power of two
    assert torch.equal(got["mean"], ref["mean"].float()) and torch.equal(got["mean"].double(), ref["mean"])
    # invstd = rsqrtf(s2 / count - mu * mu + eps): mu * mu, the subtraction, the addition of eps = 3 rounded operations, + rsqrtf
    _close(got["invstd"], ref["invstd"], (3 + 1) * U + 2 * U, "invstd")
    # scale = gamma * invstd: one more
    _close(got["scale"], ref["scale"], (4 + 1) * U + 2 * U, "scale")
    # shift = beta - mu * scale: two more; a difference, so absolute on |beta| + |mu scale|
    _close_abs(got["shift"], ref["shift"], (6 + 1) * U + 2 * U, beta.abs() + (ref["mean"] * ref["scale"]).abs(), "shift")
    if running:
        mom = float(momentum)
        # (1 - m), (1 - m) * rm, m * mu, the addition = 4 rounded operations
        _close_abs(got["rm"], ref["running_mean"], (4 + 1) * U, ((1 - mom) * rm).abs() + (mom * ref["mean"]).abs(), "running_mean")
        # mu * mu, the subtraction, var * count, / (count - 1), (1 - m), (1 - m) * rv, m * unbiased, the addition = 8
        unb = ref["var"] * count / (count - 1) if count > 1 else ref["var"]
        _close_abs(got["rv"], ref["running_var"], (8 + 1) * U, ((1 - mom) * rv).abs() + (mom * unb).abs(), "running_var")
        if mom == 1.0:          # 0 * rm + 1 * mu
            assert torch.equal(got["rm"], got["mean"])
    return got, ref


def _check_backward(p, c, count, eval_mode, seed=0):
    """frhip_bn_bwd_finalize / _eval: += into non-zero accumulators, then once more with NULL accumulators"""
    ops, lib = _ops(), _lib()
    _assert_exact_partials(p, count)
    nparts = p.shape[0]
    gamma = _pick(41 + seed, c, [0.5, 1.0, 2.0])
    invstd = _pick(42 + seed, c, [0.25, 0.5, 1.0, 2.0])
    mean = _ints(43 + seed, (c,), -3, 3).double()
    assert _is_pow2(gamma.numpy()) and _is_pow2(invstd.numpy()) and torch.equal(mean, mean.round())
    dg0, db0 = _ints(44 + seed, (c,), -50, 50).double(), _ints(45 + seed, (c,), 1, 50).double()
    s = p.sum(0)
    assert float((s.abs() + 50).max()) < EXACT
    ref = bn_double.backward(s[0], s[1], count, gamma, mean, invstd, eval_mode)
    fn = lib.frhip_bn_bwd_finalize_eval if eval_mode else lib.frhip_bn_bwd_finalize
    parts, scratch = Guarded((nparts, 2, c), p), Guarded((64 * 2 * c,), float("nan"))
    g, mu, isd = Guarded((c,), gamma), Guarded((c,), mean), Guarded((c,), invstd)
    dg, db = Guarded((c,), dg0), Guarded((c,), db0)
    for null in (False, True):
        coef = {k: Guarded((c,), float("nan")) for k in ("ca", "cb", "cc")}
        scratch.t.fill_(float("nan"))
        ops.check(fn(parts.p, nparts, scratch.p, c, float(count), g.p, mu.p, isd.p, None if null else dg.p, None if null else db.p,
                     coef["ca"].p, coef["cb"].p, coef["cc"].p, ops._s()), "frhip_bn_bwd_finalize")
        torch.cuda.synchronize()
        for name, buf in [("partials", parts), ("scratch", scratch), ("gamma", g), ("mean", mu), ("invstd", isd), ("dgamma", dg),
                          ("dbeta", db)] + list(coef.items()):
            assert buf.intact(), "canary beside %s" % name
        # exact sums added to the non-zero start; the NULL call leaves both vectors as the first call left them
        assert torch.equal(dg.t.cpu().double(), dg0 + ref["dgamma"]), "dgamma (NULL call: %s)" % null
        assert torch.equal(db.t.cpu().double(), db0 + ref["dbeta"]), "dbeta (NULL call: %s)" % null
        ca, cb, cc = (coef[k].t.cpu() for k in ("ca", "cb", "cc"))
        if eval_mode:
            assert torch.equal(ca.double(), gamma * invstd)          # a product of two powers of two
            assert torch.equal(cb, torch.zeros(c)) and torch.equal(cc, torch.zeros(c))
            continue
        # ca = gamma * invstd: 1 rounded operation
        _close(ca, ref["ca"], (1 + 1) * U, "ca")
        # cb = -(gamma * invstd) * invstd * (s2 / count): 4
        _close(cb, ref["cb"], (4 + 1) * U, "cb")
        # cc = gi * (mean * invstd * (s2 / count) - s1 / count): gi, mean * invstd, s2 / count, * m2, s1 / count, the subtraction, * gi = 7;
        # a difference: absolute on gi * (|mean invstd m2| + |m1|)
        mag = ref["ca"].abs() * ((mean * invstd * s[1] / count).abs() + (s[0] / count).abs())
        _close_abs(cc, ref["cc"], (7 + 1) * U, mag, "cc")
    assert torch.equal(parts.t.cpu().double(), p)


def _check_sum_partials(p, c, seed=0):
    ops, lib = _ops(), _lib()
    nparts = p.shape[0]
    parts = Guarded((nparts, 2, c), p)
    s = p.sum(0)
    for which in (0, 1):
        start = _ints(51 + seed + which, (c,), 1, 50).double()
        assert float((s[which].abs() + 50).max()) < EXACT
        out = Guarded((c,), start)
        ops.check(lib.frhip_sum_partials(parts.p, nparts, c, which, out.p, ops._s()), "frhip_sum_partials")
        torch.cuda.synchronize()
        assert out.intact() and parts.intact()
        assert torch.equal(out.t.cpu().double(), start + s[which]), "which = %d" % which
    assert torch.equal(parts.t.cpu().double(), p)


TREE_64x4 = [1, 2, 3, 4, 5, 12, 13, 16, 17, 28, 29, 32, 33, 60, 61, 63, 64]              # 8-unrolled, 4-unrolled, remainder loop
TREE_16x16 = [65, 112, 113, 127, 128, 129, 240, 241, 256, 257, 511, 512]                 # 8-unrolled, remainder
FOLDED = [513, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 12544, 16385]                   # fold to 64 rows, wraps every 4096
FINALIZE_CASES = [(n, 64) for n in TREE_64x4 + TREE_16x16 + FOLDED] + [(n, c) for c in (8, 72, 512) for n in (3, 64, 200, 513, 4097)] + \
    [(16385, 512)]                  # the largest partial buffer of this file: 67 MB


@pytest.mark.parametrize("nparts,c", FINALIZE_CASES)
def test_finalize_trees_return_the_exact_sums(nparts, c):
    """all four finalize entry points at every loop boundary of the three reduction trees and at widths that are no multiple of the 16-
    and 64-channel blocks"""
    p = _partials(nparts, c)
    count = _count_for(nparts)
    _check_forward(p, c, count)
    _check_backward(p, c, count, eval_mode=False)
    _check_backward(p, c, count, eval_mode=True)
    _check_sum_partials(p, c)


def test_finalize_without_running_statistics():
    _check_forward(_partials(61, 64), 64, _count_for(61), running=False)


@pytest.mark.parametrize("nparts", [29, 200, 1025])
def test_finalize_with_momentum_one_replaces_the_running_statistics(nparts):
    _check_forward(_partials(nparts, 64), 64, _count_for(nparts), momentum=1.0)


@pytest.mark.parametrize("momentum", [M01, 1.0])
def test_finalize_of_a_single_value_per_channel_skips_the_unbiased_correction(momentum):
    """count = 1: running_var takes var itself (var * 1 / 0 otherwise).  s1 in [-2, 2] and s2 in [8, 16]: var = s2 - s1^2 >= 4 >= s1^2"""
    c = 64
    p = torch.stack([_ints(71, (1, c), -2, 2), _ints(72, (1, c), 8, 16)], dim=1).double()
    got, ref = _check_forward(p, c, 1.0, momentum=momentum)
    assert torch.equal(ref["var"], p[0, 1] - p[0, 0] ** 2)
    assert bool(torch.isfinite(got["rv"]).all())
    if momentum == 1.0:
        assert torch.equal(got["rv"].double(), ref["var"])           # 0 * rv + 1 * var, var an integer


def test_finalize_of_constant_and_of_impossible_columns():
    """64 partial rows of four values each.  Columns 0-15 hold the constant 2 (s1 = 8, s2 = 16 per row): var is exactly 0 and invstd =
    rsqrt(eps).  Columns 16-31 claim s2 = 8 per row with the same s1: E[x^2] - mean^2 = 2 - 4 < 0 is clamped to 0.  The other columns are
    ordinary."""
    c, nparts, count = 64, 64, 256.0
    p = _partials(nparts, c).clone()
    p[:, 0, :32] = 8
    p[:, 1, :16] = 16
    p[:, 1, 16:32] = 8
    # the 32 special columns do not satisfy mean^2 <= var; their mean * mean = 4 is exact, so the count of rounded operations holds
    got, ref = _check_forward(p, c, count, generic=False)
    assert bool((ref["mean"][32:] ** 2 <= ref["var"][32:]).all())
    assert torch.equal(ref["var"][:32], torch.zeros(32, dtype=torch.float64)) and torch.equal(got["mean"][:32], torch.full((32,), 2.0))
    # invstd = rsqrtf(0 + eps): no rounded operation in front of rsqrtf
    _close(got["invstd"][:32], torch.full((32,), EPS ** -0.5, dtype=torch.float64), U + 2 * U, "invstd of a constant column")
    assert torch.equal(got["invstd"][:32], got["invstd"][:1].expand(32))


# =============================================================================================== (b) accuracy on inexact data
@pytest.mark.parametrize("nparts", [64, 512, 12544])
def test_finalize_trees_on_inexact_partials(nparts):
    """|kernel sum - float64 sum| <= 2^-24 (ceil(nparts / 64) + 24) sum |p|.  A sum whose every element passes through at most d rounded
    additions is within d 2^-24 sum |p| of the exact one (to first order; (1 + 2^-24)^220 - 1 exceeds 220 * 2^-24 by 1e-5 of itself, the
    bracket has at least that much room).  d from the launch geometry, counting additions to a zero accumulator although they are exact:
      nparts = 64     64-channel x 4-lane block: a lane owns 16 rows = two trips of the 8-unrolled loop: 3 levels of the pairwise tree + 2
                      accumulations, then 4 lanes: d = 9 <= 25
      nparts = 512    16-channel x 16-lane block: 32 rows per lane = four trips: 3 + 4, then 16 lanes: d = 23 <= 32;
                      frhip_sum_partials always runs this tree
      nparts = 12544  the fold has 64 groups x 4 lanes = 256 lanes of 49 rows, added one after the other (four trips of 16 with the last
                      padded by zeros): 49, 3 more for its four lanes, then the first tree on 64 rows: d = 49 + 3 + 9 = 61 <= 220;
                      frhip_sum_partials on 12544 rows: 784 rows per lane = 98 trips: 3 + 98 + 16 = 117 <= 220
    At other sizes: a lane of r rows passes an element through at most 3 + floor(r / 8) + r mod 8 additions (r of them when r < 8; the
    4-lane block has a 4-unrolled loop between the two, at most 3 + 1 + 1 + 3 at its largest r = 15).  r = ceil(nparts / 16) <= 32 in the
    16-lane tree, so that is at most ceil(nparts / 64) + 8, and its lanes add 16.  A fold lane adds ceil(nparts / 256) rows, then come its
    3 lanes and the 9 of the first tree."""
    ops, lib = _ops(), _lib()
    c, count = 64, 1024.0
    g = torch.Generator().manual_seed(90 + nparts)
    p = torch.stack([torch.randn((nparts, c), generator=g), torch.rand((nparts, c), generator=g) * 3 + 0.01], dim=1)     # fp32 values
    assert float(p[:, 1].min()) > 0
    want, mag = p.double().sum(0), p.double().abs().sum(0)
    lim = U * (-(-nparts // 64) + 24) * mag
    parts, scratch = Guarded((nparts, 2, c), p), Guarded((64 * 2 * c,), float("nan"))
    ones, zeros = Guarded((c,), 1.0), Guarded((c,), 0.0)
    out = {k: Guarded((c,), 0.0) for k in ("mean", "invstd", "scale", "shift", "dgamma", "dbeta", "ca", "cb", "cc", "sum0", "sum1")}
    ops.check(lib.frhip_bn_finalize(parts.p, nparts, scratch.p, c, count, ones.p, zeros.p, None, None, M01, EPS, out["mean"].p,
                                    out["invstd"].p, out["scale"].p, out["shift"].p, ops._s()), "frhip_bn_finalize")
    ops.check(lib.frhip_bn_bwd_finalize(parts.p, nparts, scratch.p, c, count, ones.p, zeros.p, ones.p, out["dgamma"].p, out["dbeta"].p,
                                        out["ca"].p, out["cb"].p, out["cc"].p, ops._s()), "frhip_bn_bwd_finalize")
    for which in (0, 1):
        ops.check(lib.frhip_sum_partials(parts.p, nparts, c, which, out["sum%d" % which].p, ops._s()), "frhip_sum_partials")
    torch.cuda.synchronize()
    assert all(b.intact() for b in [parts, scratch, ones, zeros] + list(out.values()))
    got = {"mean * count": (out["mean"].t.cpu().double() * count, 0),          # a division by a power of two and back: exact
           "dbeta": (out["dbeta"].t.cpu().double(), 0), "dgamma": (out["dgamma"].t.cpu().double(), 1),
           "sum_partials 0": (out["sum0"].t.cpu().double(), 0), "sum_partials 1": (out["sum1"].t.cpu().double(), 1)}
    for name, (v, which) in got.items():
        err = (v - want[which]).abs()
        print("%s: nparts %d, worst error %.2f of the bound" % (name, nparts, float((err / lim[which]).max())))
        assert bool((err <= lim[which]).all()), (name, float((err / lim[which]).max()))


# =============================================================================================== (c) colreduce_kernel
RAGGED = [(1, 64), (3, 64), (7, 512), (129, 64), (1001, 128), (7 * 93, 128)]
PAST_THE_CAP = {torch.float32: [(16401, 512), (131089, 64)], torch.bfloat16: [(32801, 512)]}
COLREDUCE_CASES = [(dt, rc) for dt in (torch.float32, torch.bfloat16) for rc in RAGGED + PAST_THE_CAP[dt]]
ROWS_PER = 7


def _expected_blocks(rows, c, dtype):
    """eight rows per row-lane and block, at most 1024 blocks (then the kernel grid-strides)"""
    rlanes = 256 // (c // (8 if dtype == torch.bfloat16 else 4))
    return min(1024, -(-rows // (rlanes * 8)))


def _guarded_rows(nb, c):
    """[nb][2][c] of NaN between canary ROWS: a row that is not written turns the sums into NaN, one too many breaks a canary"""
    full = torch.full((2 + nb + 2, 2, c), CANARY, dtype=torch.float32, device="cuda")
    full[2:2 + nb] = float("nan")
    return full, full[2:2 + nb]


def _rows_intact(full, nb):
    return bool((full[:2] == CANARY).all()) and bool((full[2 + nb:] == CANARY).all())


@pytest.mark.parametrize("dtype,rc", COLREDUCE_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_column_reductions_are_exact(dtype, rc):
    """frhip_colstats, frhip_bn_bwd_reduce (ReLU mask off and on) and frhip_bn_bwd_reduce_rs on integers in [-3, 3]"""
    ops, lib = _ops(), _lib()
    rows, c = rc
    nb = lib.frhip_colreduce_blocks(rows, c, ops._DT[dtype])
    assert nb == _expected_blocks(rows, c, dtype)
    if rc in PAST_THE_CAP[dtype]:
        rlanes = 256 // (c // ops.epv(dtype))
        assert nb == 1024 and rows > 1024 * 8 * rlanes and rows % rlanes != 0        # grid-strides, and the last stride is ragged
    seed = rows * 3 + c
    y, dout = _ints(seed, (rows, c), -3, 3), _ints(seed + 1, (rows, c), -3, 3)
    mean = _ints(seed + 2, (c,), -2, 2).double()
    invstd = _pick(seed + 3, c, [0.5, 1.0, 2.0])
    # ReLU mask y * ms + mb > 0 with ms a power of two (either sign) and mb a half-integer: never a tie
    ms = _pick(seed + 4, c, [1.0, 2.0, -1.0])
    mb = _ints(seed + 5, (c,), -2, 2).double() + 0.5
    groups = -(-rows // ROWS_PER)
    rowscale = _ints(seed + 6, (groups,), 0, 1).double() * 2
    assert _is_pow2(invstd.numpy()) and _is_pow2(ms.abs().numpy()) and set(rowscale.tolist()) <= {0.0, 2.0}
    # |d| <= 6, |y - mean| <= 5, in units of the smallest invstd: every partial and total an fp32 value
    assert rows * 9 < EXACT and rows * 6 * 5 * 2.0 / 0.5 < EXACT
    yd, dd = y.to(dtype).cuda(), dout.to(dtype).cuda()
    assert torch.equal(yd.cpu().long(), y) and torch.equal(dd.cpu().long(), dout)
    f32 = lambda t: t.float().cuda()
    mean_d, invstd_d, ms_d, mb_d, rs_d = f32(mean), f32(invstd), f32(ms), f32(mb), f32(rowscale)
    dt, P, S = ops._DT[dtype], ops._p, ops._s

    def run(what, call, want):
        full, part = _guarded_rows(nb, c)
        ops.check(call(P(part)), what)
        torch.cuda.synchronize()
        assert part.shape[0] == lib.frhip_colreduce_blocks(rows, c, dt)
        assert _rows_intact(full, nb), what
        got = part.double().sum(0).cpu()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), what

    run("frhip_colstats", lambda p: lib.frhip_colstats(dt, P(yd), rows, c, p, S()), [y.sum(0).double(), (y * y).sum(0).double()])
    for mask in (False, True):
        _, s1, s2 = bn_double.backward_sums(dout, y, mean, invstd, *((ms, mb) if mask else (None, None)))
        run("frhip_bn_bwd_reduce, mask %s" % mask,
            lambda p: lib.frhip_bn_bwd_reduce(dt, P(dd), P(yd), P(mean_d), P(invstd_d), P(ms_d) if mask else None, P(mb_d) if mask else None,
                                              rows, c, p, S()), [s1, s2])
    scaled = dout.double() * rowscale.repeat_interleave(ROWS_PER)[:rows, None]
    _, s1, s2 = bn_double.backward_sums(scaled, y, mean, invstd)
    run("frhip_bn_bwd_reduce_rs",
        lambda p: lib.frhip_bn_bwd_reduce_rs(dt, P(dd), P(yd), P(mean_d), P(invstd_d), P(rs_d), ROWS_PER, rows, c, p, S()), [s1, s2])


# =============================================================================================== (d) epilogue statistics
def _ternary(seed, shape, density):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-1, 2, shape, generator=g) * (torch.rand(shape, generator=g) < density)).float()


def _assert_stored_is_exact(t):
    """what the kernel stored: integers of at most 256 (bf16 values) -> CPU float64"""
    t = t.float().cpu().double()
    assert torch.equal(t, t.round()) and float(t.abs().max()) <= 256, float(t.abs().max())
    return t


def _forward_stats_of_the_stored_tensor(y, full, part, rows, what):
    k = y.shape[-1]
    torch.cuda.synchronize()
    assert _rows_intact(full, rows), what
    yy = _assert_stored_is_exact(y).reshape(-1, k)
    want = [yy.sum(0), (yy * yy).sum(0)]
    assert float(want[1].max()) < EXACT and float(want[1].max()) > 0
    got = part.double().sum(0).cpu()
    assert torch.equal(got[0], want[0]), what + ": sum"
    assert torch.equal(got[1], want[1]), what + ": sum of squares"


def _conv_fwd(x, w, stride, pad):
    """frhip_conv_fwd with guarded statistics rows -> (y, full, part, rows)"""
    ops, lib = _ops(), _lib()
    n, h, wd, c = x.shape
    k, r, s, _ = w.shape
    ho, wo = ops.conv_out_hw(h, wd, r, s, stride, pad)
    y = torch.empty((n, ho, wo, k), dtype=x.dtype, device="cuda")
    rows = lib.frhip_conv_stat_rows(ops.dt_of(x), n * ho * wo, k, h, wd, c, r, s, stride, pad)
    assert rows > 0
    full, part = _guarded_rows(rows, k)
    ops.check(lib.frhip_conv_fwd(ops.dt_of(x), ops._p(x), ops._p(w), ops._p(y), ops._p(part), n, h, wd, c, k, r, s, stride, pad, ops._s()),
              "frhip_conv_fwd")
    return y, full, part, rows


def _conv_operands(seed, n, h, c, k, dtype):
    # 9 c products of density 1/8 each: a standard deviation of sqrt(9 c / 8) <= 17 for c <= 256
    return _ternary(seed, (n, h, h, c), 0.5).to(dtype).cuda(), _ternary(seed + 1, (k, 3, 3, c), 0.25).to(dtype).cuda()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_conv_epilogue_statistics_general_and_ragged(dtype):
    x, w = _conv_operands(110, 3, 7, 64, 128, dtype)
    y, full, part, rows = _conv_fwd(x, w, 1, 1)
    _forward_stats_of_the_stored_tensor(y, full, part, rows, "conv_fwd (3, 7, 7, 64 -> 128)")


def test_conv_epilogue_statistics_lean_and_general():
    lib = _lib()
    x, w = _conv_operands(120, 4, 8, 64, 64, torch.bfloat16)
    for lean in (0, 1):
        old = lib.frhip_set_epi_lean(lean)
        try:
            y, full, part, rows = _conv_fwd(x, w, 1, 1)
            _forward_stats_of_the_stored_tensor(y, full, part, rows, "conv_fwd (4, 8, 8, 64 -> 64), lean %d" % lean)
        finally:
            lib.frhip_set_epi_lean(old)


@pytest.mark.parametrize("case", [(6, 28, 128, 128), (7, 14, 256, 256)])
def test_conv_epilogue_statistics_of_the_halo_tiles(case):
    lib = _lib()
    n, h, c, k = case
    x, w = _conv_operands(130 + h, n, h, c, k, torch.bfloat16)
    for halo in (0, 2, 3):
        old = lib.frhip_set_conv_halo(halo)
        try:
            y, full, part, rows = _conv_fwd(x, w, 1, 1)
            _forward_stats_of_the_stored_tensor(y, full, part, rows, "conv_fwd %s, halo %d" % (case, halo))
        finally:
            lib.frhip_set_conv_halo(old)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mnk", [(600, 256, 64), (300, 72, 64)])
def test_linear_epilogue_statistics(dtype, mnk):
    ops, lib = _ops(), _lib()
    m, n, k = mnk
    a, w = _ternary(140, (m, k), 0.5).to(dtype).cuda(), _ternary(141, (n, k), 0.5).to(dtype).cuda()
    bias = _ints(142, (n,), -2, 2).float().cuda()
    out = torch.empty((m, n), dtype=dtype, device="cuda")
    rows = lib.frhip_conv_stat_rows(ops.dt_of(a), m, n, 1, 1, k, 1, 1, 1, 0)
    assert rows > 0
    full, part = _guarded_rows(rows, n)
    ops.check(lib.frhip_linear_fwd(ops.dt_of(a), ops._p(a), ops._p(w), ops._p(bias), ops._p(out), None, ops._p(part), m, n, k, ops._s()),
              "frhip_linear_fwd")
    _forward_stats_of_the_stored_tensor(out, full, part, rows, "linear_fwd %s" % (mnk,))


def _hand_made_state(seed, c):
    """a BNState of integer means, power-of-two invstd and scale, half-integer shift (the ReLU mask y * scale + shift > 0 never ties)"""
    ops = _ops()
    st = ops.BNState()
    v = dict(mean=_ints(seed, (c,), -2, 2).double(), invstd=_pick(seed + 1, c, [0.5, 1.0, 2.0]), scale=_pick(seed + 2, c, [1.0, 2.0, -1.0]),
             shift=_ints(seed + 3, (c,), -2, 2).double() + 0.5)
    assert torch.equal(v["mean"], v["mean"].round()) and _is_pow2(v["invstd"].numpy()) and _is_pow2(v["scale"].abs().numpy())
    for name, t in v.items():
        setattr(st, name, t.float().cuda())
    st.count = 0.0
    return st, v


def _dgrad_with_stats(dtype, n, h, c, k, stride, mask, seed, rowscale=None, rows_per=0, keep_scale=0.0):
    """frhip_conv_dgrad_fused[_rs] into guarded statistics rows; the sums must be those of the STORED dx"""
    ops, lib = _ops(), _lib()
    ho = (h + 2 - 3) // stride + 1
    dy = _ternary(seed, (n, ho, ho, k), 0.5).to(dtype).cuda()
    wt = ops.pack_wt(_ternary(seed + 1, (k, 3, 3, c), 0.25).cuda(), dtype)
    res = _ints(seed + 2, (n, h, h, c), -3, 3).to(dtype).cuda()
    y_bn = _ints(seed + 3, (n, h, h, c), -3, 3)
    yb = y_bn.to(dtype).cuda()
    st, v = _hand_made_state(seed + 4, c)
    dt = ops.dt_of(dy)
    rows = lib.frhip_dgrad_stat_rows(dt, n, h, h, c, k, 3, 3, stride, 1)
    assert rows > 0
    full, part = _guarded_rows(rows, c)
    dx = torch.empty((n, h, h, c), dtype=dtype, device="cuda")
    P = ops._p
    ms, mb = (P(st.scale), P(st.shift)) if mask else (None, None)
    if rowscale is None:
        ops.check(lib.frhip_conv_dgrad_fused(dt, P(dy), P(wt), P(dx), P(res), 1, P(yb), P(st.mean), P(st.invstd), ms, mb, P(part),
                                             n, h, h, c, k, 3, 3, stride, 1, ops._s()), "frhip_conv_dgrad_fused")
    else:
        rs = rowscale.float().cuda()
        ops.check(lib.frhip_conv_dgrad_fused_rs(dt, P(dy), P(wt), P(dx), P(res), 1, P(yb), P(st.mean), P(st.invstd), ms, mb, P(rs), rows_per,
                                                float(keep_scale), P(part), n, h, h, c, k, 3, 3, stride, 1, ops._s()),
                  "frhip_conv_dgrad_fused_rs")
    torch.cuda.synchronize()
    what = "conv_dgrad %s" % ((n, h, c, k, stride, mask),)
    assert _rows_intact(full, rows), what
    d = _assert_stored_is_exact(dx).reshape(-1, c)
    if rowscale is not None:
        d = d * rowscale.double().repeat_interleave(rows_per)[:, None]
    yy = y_bn.double().reshape(-1, c)
    # every product |d| (|y| + |mean|) invstd in units of half the smallest invstd (the lean epilogue adds d y and d apart)
    assert float((d.abs() * (yy.abs() + v["mean"].abs())).sum(0).max()) * 2.0 / 0.25 < EXACT
    d, s1, s2 = bn_double.backward_sums(d, yy, v["mean"], v["invstd"], *((v["scale"], v["shift"]) if mask else (None, None)))
    assert float(d.abs().sum()) > 0
    got = part.double().sum(0).cpu()
    assert torch.equal(got[0], s1), what + ": sum d"
    assert torch.equal(got[1], s2), what + ": sum d xhat"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", [(3, 14, 64, 128, 1, True), (3, 9, 128, 64, 2, False)])
def test_dgrad_epilogue_statistics(dtype, case):
    n, h, c, k, stride, mask = case
    _dgrad_with_stats(dtype, n, h, c, k, stride, mask, 150 + h)


@pytest.mark.parametrize("lean", [0, 1])
def test_dgrad_epilogue_statistics_lean_and_general(lean):
    """whole tiles (4 x 8 x 8 = 256 rows): the lean epilogue forms the second sum as invstd (sum d y - mean sum d)"""
    lib = _lib()
    old = lib.frhip_set_epi_lean(lean)
    try:
        for mask in (False, True):
            _dgrad_with_stats(torch.bfloat16, 4, 8, 64, 64, 1, mask, 160)
    finally:
        lib.frhip_set_epi_lean(old)


def test_dgrad_epilogue_statistics_with_a_per_sample_scale():
    """stochastic depth: rows_per = 28 * 28, one sample dropped (0), one kept (2)"""
    _dgrad_with_stats(torch.bfloat16, 2, 28, 128, 128, 1, False, 170, rowscale=torch.tensor([2.0, 0.0]), rows_per=28 * 28, keep_scale=2.0)
