"""The case table of the exact forward-convolution tests (tests/fwd_cases.py), checked without a GPU: every run still takes the route it
claims (frhip_conv_fwd_route, which asks the predicates the launches themselves use, under the case's switches), the table as a whole
claims every route the query can name, the two predicates that decide about the folded BatchNorm (halo_lean_applies in
frhip_conv_fwd_affine, halo_lean_pick in the launcher) agree over a sweep of shapes and switches, the two CPU references agree bit for
bit, every value and every sum stays exact in bf16 / fp32, and the operands can see the error classes the GPU test is there to catch: for
each, a deliberately wrong reference differs from the true one."""
import ctypes
import itertools

import pytest
import torch

import fwd_cases as fc

NAMES = [case.name for case in fc.CASES]
HALO_FAMILIES = (fc.HALO_4WAVE, fc.HALO_8X1, fc.HALO_4X2, fc.HALO_WIDE)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from frhip import _abi
    return _abi.lib()


def fresh():
    return (ctypes.c_int * 5)(*([-7] * 5))


def defaults(lib):
    tile, halo = lib.frhip_set_nt_tile(0), lib.frhip_set_conv_halo(1)           # these two setters have no query form
    lib.frhip_set_nt_tile(tile), lib.frhip_set_conv_halo(halo)
    return (lib.frhip_set_halo_wide_dirs(-1), lib.frhip_set_epi_lean(-1), tile, halo)


def test_every_run_takes_the_route_it_claims(lib):
    assert len(fc.BY_NAME) == len(fc.CASES)
    assert defaults(lib) == (2, 1, 0, 1)
    wrong = []
    for name, variant in fc.RUNS:
        case = fc.BY_NAME[name]
        out = fresh()
        with fc.switches(lib, case):
            rc = lib.frhip_conv_fwd_route(*fc.shape_args(case), fc.VARIANTS[variant][0], out)
            stat_rows = lib.frhip_conv_stat_rows(*fc.stat_rows_args(case))
        if rc != 0 or tuple(out) != fc.claimed_route(case, variant) or out[4] != stat_rows:
            wrong.append((name, variant, rc, tuple(out), fc.claimed_route(case, variant), stat_rows))
        # one statistics row per block of BM output rows
        assert stat_rows == -(-fc.rows(case) // fc.block_rows(case)), name
    assert not wrong, wrong
    assert defaults(lib) == (2, 1, 0, 1)               # the switches are back where they were


def test_the_query_checks_its_arguments_and_touches_only_out(lib):
    out = fresh()
    route = lib.frhip_conv_fwd_route
    assert route(0, 1, 8, 8, 24, 64, 3, 3, 1, 1, 0, out) == -1 and b"unsupported shape" in lib.frhip_last_error()
    assert route(0, 1, 8, 8, 64, 60, 3, 3, 1, 1, 0, out) == -1 and b"unsupported shape" in lib.frhip_last_error()
    assert route(0, 0, 8, 8, 64, 64, 3, 3, 1, 1, 1, out) == -1 and b"unsupported shape" in lib.frhip_last_error()
    assert route(0, 1, 8, 8, 64, 64, 3, 3, 3, 1, 0, out) == -1 and b"unsupported shape" in lib.frhip_last_error()
    assert route(0, 1, 8, 8, 64, 64, 3, 3, 1, 1, 3, out) == -1 and b"mode" in lib.frhip_last_error()
    assert route(0, 1, 8, 8, 64, 64, 3, 3, 1, 1, -1, out) == -1 and b"mode" in lib.frhip_last_error()
    assert route(0, 1, 8, 8, 64, 64, 3, 3, 1, 1, 0, None) == -1
    # mode 2 where frhip_conv_bnrelu_fusable says no: fp32, a strided filter, a 1x1, the nine K chunks of an 8-wave tile, W = 57
    for dtype, shape in ((1, (1, 8, 8, 64, 64, 3, 3, 1, 1)), (0, (1, 8, 8, 64, 64, 3, 3, 2, 1)), (0, (1, 8, 8, 64, 64, 1, 1, 1, 0)),
                         (0, (1, 5, 5, 576, 64, 3, 3, 1, 1)), (0, (1, 5, 57, 64, 64, 3, 3, 1, 1))):
        assert lib.frhip_conv_bnrelu_fusable(dtype, *shape[1:3], *shape[3:]) == 0, shape
        assert route(dtype, *shape, 2, out) == -1 and b"not fusable" in lib.frhip_last_error(), shape
        assert route(dtype, *shape, 0, fresh()) == 0 and route(dtype, *shape, 1, fresh()) == 0, shape
        # and the entry point itself refuses them before it touches an operand or launches anything
        assert lib.frhip_conv_fwd_bnrelu(dtype, None, None, None, None, None, None, None, *shape, None) == -1, shape
        assert b"not fusable" in lib.frhip_last_error()
    assert tuple(out) == (-7,) * 5
    # the operand transform lives in the 4-wave tile alone: with the wide tile's forward direction on, mode 0 names the wide tile, mode 2 not
    old = lib.frhip_set_halo_wide_dirs(1)
    try:
        got = []
        for mode in (0, 1, 2):
            assert route(0, 1, 16, 16, 128, 128, 3, 3, 1, 1, mode, out) == 0
            got.append(tuple(out))
    finally:
        lib.frhip_set_halo_wide_dirs(old)
    assert got == [(fc.HALO_WIDE, 0, 1, 1, 1), (fc.HALO_WIDE, 0, 1, 1, 1), (fc.HALO_4WAVE, 0, 1, 1, 1)]
    assert defaults(lib) == (2, 1, 0, 1)


def test_no_two_cases_are_the_same_launch():
    keys = [(fc.shape_args(case), case.halo, case.wide, case.tile, case.lean) for case in fc.CASES]
    assert len(set(keys)) == len(keys)
    assert all(set(case.variants) <= set(fc.VARIANTS) and len(set(case.variants)) == len(case.variants) for case in fc.CASES)


def test_the_table_claims_every_route_the_query_can_name():
    claimed = {fc.claimed_route(fc.BY_NAME[name], variant)[:3] for name, variant in fc.RUNS}
    assert claimed == ({(family, 0, epi) for family in (fc.HALO_4WAVE, fc.HALO_WIDE) for epi in (0, 1)} |
                       {(fc.HALO_8X1, 0, 0), (fc.HALO_4X2, 0, 0)} | {(0, tile, 0) for tile in (1, 2, 3, 4)} | {(0, 4, 1)})
    runs = lambda pick: {variant for case in fc.CASES if pick(case) for variant in case.variants}
    for case in fc.CASES:
        assert case.variants[:2] == ("plain", "stats"), case.name
    # the affine variants on every lean halo route, and on one case of each kind that falls back to two launches
    for case in fc.CASES:
        if case.route[0] in (fc.HALO_4WAVE, fc.HALO_WIDE) and case.route[2] == fc.EPI_LEAN:
            assert set(fc.AFF) <= set(case.variants), case.name
    fallback = {"ragged tile": lambda c: c.route[:3] == (1, 0, 0) and fc.rows(c) % 256 and c.lean,
                "lean switch off": lambda c: c.route[:3] == (1, 0, 0) and not c.lean,
                "forced 8-wave": lambda c: c.route[0] in (fc.HALO_8X1, fc.HALO_4X2) and c.halo == 3,
                "fp32": lambda c: c.dtype == "fp32",
                "generic 3x3": lambda c: not fc.is_halo(c) and (c.r, c.stride) == (3, 1),
                "stride 2": lambda c: c.stride == 2,
                "1x1": lambda c: (c.r, c.stride) == (1, 1)}
    for kind, pick in fallback.items():
        assert set(fc.AFF) <= runs(pick), kind
    assert all(fc.claimed_route(case, "affine")[3] == 2 for pick in fallback.values() for case in fc.CASES
               if pick(case) and "affine" in case.variants)
    # the operand transform on the 4-wave tile's general and lean kernels, on several K chunks, and on every map edge that tile serves
    for case in fc.CASES:
        if set(case.variants) & set(fc.BNR):
            assert case.route[:2] == (fc.HALO_4WAVE, 0) and case.dtype == "bf16" and (case.halo, case.wide) == (1, 2), case.name
    for epi in (0, 1):
        assert set(fc.BNR) <= runs(lambda c: c.route[:3] == (1, 0, epi))
    assert set(fc.BNR) <= runs(lambda c: c.c > 64 and c.route[0] == fc.HALO_4WAVE)
    assert "bnrelu_act" in runs(lambda c: c.route[:3] == (1, 0, 1) and c.k > 64 and fc.rows(c) > 256)        # 2 x 2 tiles
    halo = [case for case in fc.CASES if fc.is_halo(case)]
    edges = [case for case in halo if case.h == 1 or case.w == 1 or case.w == 56]
    assert {(case.h == 1, case.w == 1, case.w == 56) for case in edges} == {(True, False, True), (False, True, False), (True, True, False),
                                                                            (False, False, True)}
    assert all("bnrelu" in case.variants for case in edges)
    # both sides of the two width limits (the wide tile's under its forward direction)
    width = lambda wide: {case.w: case.route[0] for case in fc.CASES
                          if case.halo == 1 and case.wide in wide and (case.r, case.stride) == (3, 1) and case.w in (28, 29, 56, 57)}
    assert width((1, 3)) == {28: fc.HALO_WIDE, 29: fc.HALO_4WAVE} and width((2,)) == {56: fc.HALO_4WAVE, 57: fc.GENERIC}
    assert {case.wide for case in fc.CASES if case.route[0] == fc.HALO_WIDE} == {1, 3}
    # a ragged and a whole last row tile per family, several K chunks, both dtypes on each 8-wave tile
    for family in HALO_FAMILIES + (fc.GENERIC,):
        assert {fc.rows(case) % fc.block_rows(case) == 0 for case in fc.CASES if case.route[0] == family} == {True, False}, family
    assert any(case.c > 8 * fc.kstep(case) for case in halo)
    for family in (fc.HALO_8X1, fc.HALO_4X2):
        assert {case.dtype for case in halo if case.route[0] == family} == {"bf16", "fp32"}
        assert {case.halo for case in halo if case.route[0] == family and case.dtype == "bf16"} == {1, 3}
    # a ragged channel tile on a halo route (64 columns per tile) and on the generic tiles 1 (128) and 2 (64)
    assert any(case.k % 64 for case in halo)
    columns = {1: 128, 2: 64, 3: 128, 4: 256}
    assert {case.route[1] for case in fc.CASES if not fc.is_halo(case) and case.k % columns[case.route[1]] and case.k > 128} == {1, 2}
    # the stride-2 gather: every strided filter, odd and even maps, maps with a single output row or pixel, both tiles, both dtypes
    strided = [case for case in fc.CASES if case.stride == 2]
    assert {(case.r, case.pad) for case in strided} == {(3, 1), (2, 0), (1, 0)}
    for r in (3, 2, 1):
        assert {case.h % 2 for case in strided if case.r == r} == {0, 1}
    assert {case.route[1] for case in strided if case.r == 3} == {1, 2} and {case.dtype for case in strided} == {"bf16", "fp32"}
    assert any(fc.out_hw(case) == (1, 1) and case.h == 2 for case in strided) and any(case.h == 1 and case.w > 1 for case in strided)
    # the persistent case has more tiles than an MI355X has workgroups of the lean kernel, and runs with statistics
    big = fc.BY_NAME["tile 4 lean, persistent loop takes a second tile"]
    assert (fc.rows(big) // 256) * (big.k // 256) == fc.PERSISTENT_CUS + 2 and "stats" in big.variants


def test_the_two_lean_predicates_agree(lib):
    """frhip_conv_fwd_affine hands scale, shift, ReLU and residual to halo_run where halo_lean_applies says the launch will be a lean one;
    halo_launch decides that with halo_lean_pick.  Where the first said yes and the second no, the general epilogue would drop all four
    without an error; the other way round costs a launch.  Mode 1 of the query reports one launch where the first says yes (and then the
    epilogue the second picks), mode 0 the epilogue the second picks: the two must coincide everywhere."""
    assert defaults(lib) == (2, 1, 0, 1)
    shapes = list(itertools.product((1, 3, 4, 8, 64), (7, 8, 16, 28, 29), (64, 72, 128, 192, 576), (64, 72, 128, 192, 576)))
    fwd, aff = fresh(), fresh()
    wrong, folded, refused = [], 0, 0
    Switch = fc.Case._make([None] * len(fc.Case._fields))
    for halo, wide, tile, lean in itertools.product(range(4), range(4), range(5), range(2)):
        with fc.switches(lib, Switch._replace(halo=halo, wide=wide, tile=tile, lean=lean)):
            for n, hw, c, k in shapes:
                args = (0, n, hw, hw, c, k, 3, 3, 1, 1)
                rc0, rc1 = lib.frhip_conv_fwd_route(*args, 0, fwd), lib.frhip_conv_fwd_route(*args, 1, aff)
                if rc0 or rc1:
                    refused += 1
                    assert rc0 == rc1 == -1 and c % 64, (args, rc0, rc1)
                    continue
                lean_halo = fwd[0] in HALO_FAMILIES and fwd[2] == 1
                folded += lean_halo
                if aff[3] != (1 if lean_halo else 2) or tuple(aff)[:3] != tuple(fwd)[:3] or aff[4] != fwd[4] or fwd[3] != 1:
                    wrong.append(((halo, wide, tile, lean), args, tuple(fwd), tuple(aff)))
    assert not wrong, (len(wrong), wrong[:8])
    assert refused == 160 * 125 and folded > 1000           # c = 72 is no whole K step; the sweep does reach the folded route
    assert defaults(lib) == (2, 1, 0, 1)


def _round_trip(t, dtype):
    return torch.equal(t.to(dtype).long(), t)


@pytest.mark.parametrize("name", NAMES)
def test_the_two_references_agree_and_every_value_is_exact(name):
    case, data = fc.BY_NAME[name], fc.operands(name)
    dtype = fc.torch_dtype(case)
    limits = {"x": 2, "w": 2, "res": 8, "shift": 3, "xd": 4, "wb": 2, "in_shift": 3}
    for key, limit in limits.items():
        if key in data:
            assert data[key].dtype == torch.int64 and 0 < int(data[key].abs().max()) <= limit, key
    assert set(data["scale"].tolist()) <= {-1, 1, 2} and set(data.get("in_scale", data["scale"]).tolist()) <= {-1, 1, 2}
    ho, wo = fc.out_hw(case)
    for bnrelu in sorted({fc.VARIANTS[v][0] == fc.MODE_BNRELU for v in case.variants}):
        a, b = fc.y_f64(name, bnrelu), fc.y_i64(name, bnrelu)
        assert a.dtype == torch.float64 and b.dtype == torch.int64 and a.shape == b.shape == (case.n, ho, wo, case.k)
        assert torch.equal(a, b.double()) and torch.equal(a.long(), b) and int(b.abs().max()) > 0
        assert _round_trip(b, dtype)
        products = (fc.inputs(name, bnrelu)[0] != 0).double().mean() * (fc.inputs(name, bnrelu)[1] != 0).double().mean() * case.r ** 2 * case.c
        assert 8 <= float(products) <= 32, (name, bnrelu, float(products))         # "about 16" non-zero products per output element
    lim = fc.bound(name)
    assert lim["y"] <= 256, (name, "largest |y| %d against 256" % lim["y"])
    assert lim["contraction"] < 2 ** 24, (name, "largest |x| (*) |w| + 8 = %d against 2^24" % lim["contraction"])
    assert lim["sum"] < 2 ** 24 and lim["sumsq"] < 2 ** 24, (name, "largest block sums %r, %r against 2^24" % (lim["sum"], lim["sumsq"]))
    for variant in case.variants:
        want = fc.expected(name, variant)
        assert _round_trip(want["y"], dtype), (name, variant, "largest stored value %d" % lim["stored"])
        if want["act"] is not None:
            assert _round_trip(want["act"], dtype) and want["act"].shape == data["xd"].shape and int(want["act"].max()) <= 11
            assert int(want["act"].min()) == 0 and 0.3 < float((want["act"] == 0).double().mean()) < 0.7
            assert int(data["in_shift"].max()) > 0                                  # relu(in_shift) is not zero everywhere
        if want["rows"] is not None:
            part = want["rows"]
            assert part.shape == (case.route[3], 2, case.k) and torch.equal(part.float().double(), part)
            flat = fc.y_i64(name, fc.VARIANTS[variant][0] == fc.MODE_BNRELU).reshape(-1, case.k).double()
            assert torch.equal(part[:, 0].sum(0), flat.sum(0)) and torch.equal(part[:, 1].sum(0), (flat * flat).sum(0))
            assert float(part[:, 1].max()) > 0


def _reaches(case, size, out, f):
    return any(0 <= o * case.stride - case.pad + f < size for o in range(out))


@pytest.mark.parametrize("name", NAMES)
def test_wrong_references_differ_from_the_true_one(name):
    """Each error class the exact comparison is there to catch, built into the CPU reference where the case can have it: the result must
    differ from the true reference, so the operands cannot hide it."""
    case, data = fc.BY_NAME[name], fc.operands(name)
    ho, wo = fc.out_hw(case)
    tried = set()
    has_bnrelu = bool(set(case.variants) & set(fc.BNR))
    for bnrelu in ((False, True) if has_bnrelu else (False,)):
        a, w = fc.inputs(name, bnrelu)
        ref = fc.y_i64(name, bnrelu)
        # one tap dropped: every tap of the filter in turn (the persistent case has one tap and one chunk: without them y is zero)
        for fr in range(case.r):
            for fs in range(case.r):
                if case.r > 1 and _reaches(case, case.h, ho, fr) and _reaches(case, case.w, wo, fs):
                    assert not torch.equal(fc.conv_i64(case, a, w, skip_tap=(fr, fs)), ref), (name, bnrelu, fr, fs)
        tried.add("tap")
        # one K chunk dropped: each chunk of x's channels in turn
        for c0 in range(0, case.c if case.c > fc.kstep(case) else 0, fc.kstep(case)):
            cut = a.clone()
            cut[..., c0:c0 + fc.kstep(case)] = 0
            assert not torch.equal(fc.conv_i64(case, cut, w), ref), (name, bnrelu, c0)
        assert bool(ref.any())
        tried.add("chunk")
        # the stride-2 gather base one pixel off: ho * stride instead of ho * stride - pad
        if case.stride == 2 and case.pad == 1:
            assert not torch.equal(fc.conv_i64(case, a, w, base=1), ref), name
            tried.add("base")
        # a ragged block's statistics taken over BM whole rows, into the next image's data
        if fc.rows(case) % fc.block_rows(case):
            true, wrong = fc.block_sums(case, ref), fc.block_sums(case, ref, beyond=True)
            assert torch.equal(true[:-1], wrong[:-1]) and not torch.equal(true[-1, 0], wrong[-1, 0]), (name, bnrelu)
            assert bool((wrong[-1, 1] > true[-1, 1]).any()), (name, bnrelu)
            tried.add("beyond")
    if has_bnrelu:
        # zero padding that went through the transform: relu(0 * in_scale + in_shift) instead of 0
        a, w = fc.inputs(name, True)
        leaked = fc.conv_i64(case, a, w, pad_value=fc.transform(torch.zeros_like(data["in_shift"]), data["in_scale"], data["in_shift"]))
        assert not torch.equal(leaked, fc.y_i64(name, True)), name
        inner = (slice(None), slice(1, ho - 1), slice(1, wo - 1))
        assert torch.equal(leaked[inner], fc.y_i64(name, True)[inner])                 # ... and only the border pixels see it
        tried.add("padding")
        # act_out from the wrong channel column: the 64-channel chunks of the transformed tensor one column off
        if case.c > 64 and "bnrelu_act" in case.variants:
            assert not torch.equal(a.roll(64, -1), fc.expected(name, "bnrelu_act")["act"]), name
            tried.add("column")
        if "bnrelu_act" in case.variants:                                            # act_out is the transformed tensor, not x
            assert not torch.equal(data["xd"], fc.expected(name, "bnrelu_act")["act"])
    if "affine" in case.variants:
        y = fc.y_i64(name)
        want, bare = fc.expected(name, "affine")["y"], fc.expected(name, "affine_bare")["y"]
        assert not torch.equal(want, fc.affine(name, y, relu=False, residual=True)), name
        assert not torch.equal(want, fc.affine(name, y, relu=True, residual=False)), name
        assert not torch.equal(bare, fc.affine(name, y, relu=True, residual=False)) and not torch.equal(bare, y), name
        tried |= {"relu", "residual"}
        if case.k > 64:
            assert not torch.equal(want, fc.affine(name, y, relu=True, residual=True, channel_shift=64)), name
            assert not torch.equal(bare, fc.affine(name, y, relu=False, residual=False, channel_shift=64)), name
            # scale and shift each on their own
            shifted = y * data["scale"].roll(64) + data["shift"]
            assert not torch.equal(bare, shifted) and not torch.equal(bare, y * data["scale"] + data["shift"].roll(64)), name
            tried.add("channel")
    expect = {"tap", "chunk"}
    expect |= {"base"} if case.stride == 2 and case.pad == 1 else set()
    expect |= {"beyond"} if fc.rows(case) % fc.block_rows(case) else set()
    expect |= {"padding"} if has_bnrelu else set()
    expect |= {"column"} if case.c > 64 and "bnrelu_act" in case.variants else set()
    expect |= {"relu", "residual"} if "affine" in case.variants else set()
    expect |= {"channel"} if "affine" in case.variants and case.k > 64 else set()
    assert tried == expect, (name, tried, expect)


def test_every_error_class_has_a_case():
    count = lambda pick: sum(1 for case in fc.CASES if pick(case))
    assert count(lambda c: c.stride == 2 and c.pad == 1) >= 7
    assert count(lambda c: fc.rows(c) % fc.block_rows(c) != 0) >= 30
    assert count(lambda c: "bnrelu" in c.variants) >= 8
    assert count(lambda c: "bnrelu_act" in c.variants and c.c > 64) >= 1
    assert count(lambda c: "affine" in c.variants and c.k > 64) >= 4
