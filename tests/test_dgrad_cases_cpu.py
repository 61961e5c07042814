"""The case table of the exact data-gradient tests (tests/dgrad_cases.py), checked without a GPU: every run still takes the route it claims
(frhip_dgrad_route, which asks the predicates the launch itself uses, under the case's switches), the table as a whole claims every route
the query can name, the two CPU references agree bit for bit, every value and every sum stays exact in bf16 / fp32, and the operands can
see the error classes the GPU test is there to catch: for each, a deliberately wrong reference differs from the true one.  A later change
of the dispatch then cannot silently turn a case of tests/test_dgrad_exact_gpu.py into a duplicate of another."""
import ctypes

import pytest
import torch

import dgrad_cases as dc

NAMES = [case.name for case in dc.CASES]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from frhip import _abi
    return _abi.lib()


def query(lib, case, variant):
    out = (ctypes.c_int * 5)(*([-7] * 5))
    with dc.switches(lib, case):
        rc = lib.frhip_dgrad_route(*dc.route_args(case, variant), out)
        stat_rows = lib.frhip_dgrad_stat_rows(*dc.shape_args(case))
    return rc, tuple(out), stat_rows


def defaults(lib):
    tile, halo = lib.frhip_set_nt_tile(0), lib.frhip_set_conv_halo(1)           # these two setters have no query form
    lib.frhip_set_nt_tile(tile), lib.frhip_set_conv_halo(halo)
    return (lib.frhip_set_halo_wide_dirs(-1), lib.frhip_set_epi_lean(-1), tile, halo)


def test_every_run_takes_the_route_it_claims(lib):
    assert len(dc.BY_NAME) == len(dc.CASES)
    assert defaults(lib) == (2, 1, 0, 1)
    wrong = []
    for name, variant in dc.RUNS:
        case = dc.BY_NAME[name]
        rc, route, stat_rows = query(lib, case, variant)
        if rc != 0 or route != dc.claimed_route(case, variant) or route[4] != stat_rows:
            wrong.append((name, variant, rc, route, dc.claimed_route(case, variant), stat_rows))
    assert not wrong, wrong
    assert defaults(lib) == (2, 1, 0, 1)               # the switches are back where they were


def test_the_query_checks_its_arguments_and_touches_only_out(lib):
    out = (ctypes.c_int * 5)(*([-7] * 5))
    assert lib.frhip_dgrad_route(0, 1, 8, 8, 64, 24, 3, 3, 1, 1, 0, 0, out) == -1 and b"unsupported shape" in lib.frhip_last_error()
    assert lib.frhip_dgrad_route(0, 1, 8, 8, 64, 64, 3, 3, 1, 1, 3, 0, out) == -1 and b"residual_stride" in lib.frhip_last_error()
    assert lib.frhip_dgrad_route(0, 1, 8, 8, 64, 64, 3, 3, 1, 1, 0, 0, None) == -1
    assert tuple(out) == (-7,) * 5
    # a convolution whose parity classes straddle the 16 384-row threshold of tile 4: the first class gets tile 4, the last tile 1
    assert lib.frhip_dgrad_route(0, 65, 31, 33, 256, 64, 3, 3, 2, 1, 0, 0, out) == 0
    assert tuple(out) == (0, -1, 0, 4, lib.frhip_dgrad_stat_rows(0, 65, 31, 33, 256, 64, 3, 3, 2, 1))


def test_no_two_cases_are_the_same_launch():
    keys = [(dc.shape_args(case), case.halo, case.wide, case.tile, case.lean) for case in dc.CASES]
    assert len(set(keys)) == len(keys)
    assert all(set(case.variants) <= set(dc.VARIANTS) and len(set(case.variants)) == len(case.variants) for case in dc.CASES)


def test_the_table_claims_every_route_the_query_can_name():
    claimed = {dc.claimed_route(dc.BY_NAME[name], variant)[:3] for name, variant in dc.RUNS}
    by_family = lambda family: {route[2] for route in claimed if route[0] == family}
    # the lean instantiations exist for the 4-wave and the wide halo tile and for NT tile 4 (there also in two halves)
    assert by_family(dc.HALO_4WAVE) == by_family(dc.HALO_WIDE) == {dc.EPI_GENERAL, dc.EPI_LEAN}
    assert by_family(dc.HALO_8X1) == by_family(dc.HALO_4X2) == {dc.EPI_GENERAL}
    assert by_family(dc.GENERIC) == {dc.EPI_GENERAL, dc.EPI_LEAN, dc.EPI_LEAN_HALVES}
    assert {route[1] for route in claimed if route[0] == dc.GENERIC} == {1, 2, 3, 4}
    assert {(tile, epi) for family, tile, epi in claimed if epi != dc.EPI_GENERAL and family == dc.GENERIC} == {(4, 1), (4, 2)}
    runs = lambda pick: {variant for name, variant in dc.RUNS if pick(dc.BY_NAME[name])}
    # every case runs bare and with dense residual + masked partials, but for the persistent one, whose rows exceed the sums bound
    for case in dc.CASES:
        assert set(case.variants) >= ({"plain", "res"} if dc.rows(case) > 16384 else {"plain", "res_bn"}), case.name
    assert [case.name for case in dc.CASES if dc.rows(case) > 16384] == ["tile 4 lean, persistent loop takes a second tile"]
    # the compact residual on the 4-wave and the wide halo tile, the generic 3x3 / stride 1 route and one parity case; unmasked partials
    # on a halo and a generic route; stochastic depth on the 4-wave and the wide tile (general and lean) and on tile 4 (halves and general)
    for family in (dc.HALO_4WAVE, dc.HALO_WIDE):
        assert {"compact", "compact_bn", "rs"} <= runs(lambda case: case.route[0] == family)
        assert {"rs"} <= runs(lambda case: case.route[0] == family and case.route[2] == "L")
    assert {"compact", "compact_bn"} <= runs(lambda case: not dc.is_halo(case) and (case.r, case.stride) == (3, 1))
    assert {"compact", "compact_bn"} <= runs(dc.is_parity)
    assert "res_bn_unmasked" in runs(dc.is_halo) and "res_bn_unmasked" in runs(lambda case: not dc.is_halo(case))
    assert {"rs"} <= runs(lambda case: case.route[:3] == (0, 4, "H")) and {"rs"} <= runs(lambda case: case.route[:3] == (0, 4, "G"))
    # parity: every shape on tiles 1 and 2; 1, 2 and 4 non-empty classes; several tiles per class with partials (the per-class row offset)
    parity = [case for case in dc.CASES if dc.is_parity(case)]
    shapes = {dc.shape_args(case) for case in parity}
    assert {(dc.shape_args(case), case.route[1]) for case in parity} == {(shape, tile) for shape in shapes for tile in (1, 2)}
    assert {case.route[3] for case in parity} == {1, 2, 4}
    assert any(case.route[4] > case.route[3] and "res_bn" in case.variants for case in parity)
    # map edges of the halo kernels, and both sides of the two width limits
    halo = [case for case in dc.CASES if dc.is_halo(case)]
    assert any(case.h == 1 and case.w == 56 for case in halo) and any(case.w == 1 for case in halo) and any(case.h * case.w == 1 for case in halo)
    by_width = {case.w: case.route[0] for case in dc.CASES if case.halo == 1 and case.wide == 2 and (case.r, case.stride) == (3, 1)}
    assert [by_width[w] for w in (28, 29, 56, 57)] == [dc.HALO_WIDE, dc.HALO_4WAVE, dc.HALO_4WAVE, dc.GENERIC]
    assert any(dc.rows(case) % 256 for case in halo) and any(case.k > 8 * dc.kstep(case) for case in halo)
    assert {case.dtype for case in halo if case.route[0] in (dc.HALO_8X1, dc.HALO_4X2)} == {"bf16", "fp32"}
    # the persistent case has more tiles than an MI355X has workgroups of the lean kernel
    big = dc.BY_NAME["tile 4 lean, persistent loop takes a second tile"]
    assert (dc.rows(big) // 256) * (big.c // 256) == dc.PERSISTENT_CUS + 2


@pytest.mark.parametrize("name", NAMES)
def test_the_two_references_agree_and_every_value_is_exact(name):
    case, data = dc.BY_NAME[name], dc.operands(name)
    limits = {"dy": 2, "w": 2, "res": 8, "resc": 8, "y": 4, "mean": 2, "mshift": 3}
    for key, limit in limits.items():
        assert data[key].dtype == torch.int64 and 0 < int(data[key].abs().max()) <= limit, key
    assert set(data["invstd"].tolist()) <= {0.5, 1.0, 2.0} and set(data["mscale"].tolist()) <= {-1, 1, 2}
    assert set(data["rowscale"].tolist()) <= {0.0, dc.KEEP_SCALE}
    if case.n >= 3:
        assert data["rowscale"][0] == 0 and data["rowscale"][-1] == 0 and data["rowscale"].max() == dc.KEEP_SCALE
    a, b = dc.conv_f64(name), dc.conv_i64(name)
    assert a.dtype == torch.float64 and b.dtype == torch.int64 and a.shape == b.shape == (case.n, case.h, case.w, case.c)
    assert torch.equal(a, b.double()) and torch.equal(a.long(), b) and int(b.abs().max()) > 0
    lim = dc.bound(name)
    assert lim["dx"] <= 256 and lim["contraction"] < 2 ** 24
    if any(dc.VARIANTS[v][2] for v in case.variants):
        assert lim["sums"] < 2 ** 24
        act = data["y"] * data["mscale"] + data["mshift"]
        assert int((act == 0).sum()) * 20 > act.numel()             # the mask's boundary is hit by more than one element in twenty
    else:
        assert lim["sums"] is None
    for variant in case.variants:
        want = dc.expected(name, variant)
        dtype = torch.bfloat16 if case.dtype == "bf16" else torch.float32
        assert torch.equal(want["dx"].to(dtype).long(), want["dx"]) and torch.equal(b.to(dtype).long(), b)
        if "s1" in want:
            for key in ("s1", "s2"):
                assert torch.equal(want[key].float().double(), want[key]) and float(want[key].abs().max()) > 0
            assert float(want["s1"].abs().max()) <= lim["sums"] and float(want["s2"].abs().max()) <= lim["sums"]
            assert torch.equal(dc.tile_rows(name, variant).sum(0), torch.stack([want["s1"], want["s2"]]))


def differs(a, b, keys=("dx", "s1", "s2")):
    return [key for key in keys if key in a and key in b and not torch.equal(a[key], b[key])]


@pytest.mark.parametrize("name", NAMES)
def test_wrong_references_differ_from_the_true_one(name):
    """Each error class the exact comparison is there to catch, built into the CPU reference where the case can have it: the result must
    differ from the true reference, so the operands cannot hide it."""
    case, data = dc.BY_NAME[name], dc.operands(name)
    ref = dc.conv_i64(name)
    tried = set()
    reaches = lambda size, out, f: any(0 <= o * case.stride - case.pad + f < size for o in range(out))
    # one tap dropped: every tap of the filter in turn
    for fr in range(case.r):
        for fs in range(case.r):
            if not (reaches(case.h, dc.out_hw(case)[0], fr) and reaches(case.w, dc.out_hw(case)[1], fs)):
                continue                                          # all of this tap's pixels are padding (maps one pixel high or wide)
            assert not torch.equal(dc.scatter_i64(case, data["dy"], data["w"], skip_tap=(fr, fs)), ref), (name, fr, fs)
            tried.add("tap")
    # one K chunk dropped: each chunk of dy's channels in turn
    for k0 in range(0, case.k if case.k > dc.kstep(case) else 0, dc.kstep(case)):
        dy = data["dy"].clone()
        dy[..., k0:k0 + dc.kstep(case)] = 0
        assert not torch.equal(dc.scatter_i64(case, dy, data["w"]), ref), (name, k0)
        tried.add("chunk")
    if case.k == dc.kstep(case):
        assert bool(ref.any())                                    # the only chunk: without it dx is zero
        tried.add("chunk")
    # zero padding replaced by the neighbouring row or image (3x3 / stride 1): pixel m reads dy at m + (1 - fr) W + (1 - fs) of the flat stream
    if (case.r, case.stride, case.pad) == (3, 1, 1):
        m = dc.rows(case)
        flat = torch.nn.functional.pad(data["dy"].reshape(m, case.k), (0, 0, case.w + 1, case.w + 1))
        for fr in range(3):
            for fs in range(3):
                start = case.w + 1 + (1 - fr) * case.w + (1 - fs)
                leaky = flat[start:start + m] @ data["w"][:, fr, fs, :]
                zero = torch.zeros_like(data["w"])
                zero[:, fr, fs, :] = data["w"][:, fr, fs, :]
                same = torch.equal(leaky.reshape(ref.shape), dc.scatter_i64(case, data["dy"], zero))
                # the centre column leaks across images only: with one image there is no neighbour to read
                assert same == (fs == 1 and (fr == 1 or case.n == 1)), (name, fr, fs)
        tried.add("padding")
    # parity classes (0, 1) and (1, 0) landing on each other's pixels
    if dc.is_parity(case) and case.h > 1 and case.w > 1:
        wrong = ref.clone()
        hh, ww = min(ref[:, 0::2, 1::2].shape[1], ref[:, 1::2, 0::2].shape[1]), min(ref[:, 0::2, 1::2].shape[2], ref[:, 1::2, 0::2].shape[2])
        wrong[:, 0:2 * hh:2, 1:2 * ww:2] = ref[:, 1:2 * hh:2, 0:2 * ww:2]
        wrong[:, 1:2 * hh:2, 0:2 * ww:2] = ref[:, 0:2 * hh:2, 1:2 * ww:2]
        assert not torch.equal(wrong, ref), name
        tried.add("parity")
    for variant in case.variants:
        _, res_stride, bn, masked, rs = dc.VARIANTS[variant]
        want = dc.expected(name, variant)
        if res_stride == 2 and case.h > 1 and case.w > 1:
            assert "dx" in differs(want, dc.finish(name, variant, ref, odd_compact=True)), (name, variant)
            tried.add("compact")
        if res_stride:
            assert "dx" in differs(want, dc.expected(name, "plain")), (name, variant)
        if masked:
            assert differs(want, dc.finish(name, variant, ref, mask_ge=True)) == ["s1", "s2"], (name, variant)
            tried.add("mask")
        if rs:
            assert differs(want, dc.finish(name, variant, ref, scale_dx=True)) == ["dx"], (name, variant)
            unscaled = dc.expected(name, "res_bn")
            assert differs(want, unscaled) == ["s1", "s2"], (name, variant)
            tried.add("rowscale")
    expect = {"tap", "chunk"}
    expect |= {"padding"} if (case.r, case.stride, case.pad) == (3, 1, 1) else set()
    expect |= {"parity"} if dc.is_parity(case) and case.h > 1 and case.w > 1 else set()
    expect |= {"compact"} if "compact" in case.variants else set()
    expect |= {"mask"} if "res_bn" in case.variants else set()
    expect |= {"rowscale"} if "rs" in case.variants else set()
    assert tried == expect, (name, tried, expect)
