"""The case table of the exact stem tests (tests/stem_cases.py), checked without a GPU: the reference agrees with float64 torch autograd
of conv -> batch_norm(training) -> ReLU -> max_pool2d on generic data (including the algebraic weight gradient and both image-gradient
forms), every case keeps the value bounds that make bf16 elements and fp32 sums exact, every case has the coverage it claims -- ties the
first-max rule decides, pooled zeros, pre-activations of exactly 0 under a non-zero gradient, pixels that several windows choose, arg-max
pixels in the neighbour tiles -- and the widths one past the widest accepted rows are refused on the host."""
import pytest
import torch
import torch.nn.functional as F

import bn_double
import stem_cases as sc

EPS = 1e-5


def close(got, want, what):
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    assert got.shape == want.shape and err <= 1e-12 * scale, (what, err, scale)


@pytest.mark.parametrize("shape", [(2, 9, 11), (1, 4, 7), (3, 1, 6)])
def test_the_reference_agrees_with_float64_autograd(shape):
    b, h, w = shape
    gen = torch.Generator().manual_seed(1234 + h)
    rnd = lambda *s: torch.randn(s, generator=gen, dtype=torch.float64)
    x, w27, beta = rnd(b, 3, h, w), 0.3 * rnd(64, 27), 0.2 * rnd(64)
    gamma = (1 + 0.2 * rnd(64)) * torch.where(torch.arange(64) % 5 == 0, -1.0, 1.0)          # some gammas negative
    xl, wl, gl, bl = (t.clone().requires_grad_(True) for t in (x, w27, gamma, beta))
    y0 = F.conv2d(xl, wl.view(64, 3, 3, 3).permute(0, 3, 1, 2), None, 1, 1)
    a0 = F.relu(F.batch_norm(y0, None, None, gl, bl, True, 0.1, EPS))
    p0, idx0 = F.max_pool2d(a0, 3, 2, 1, return_indices=True)
    dp = rnd(*p0.shape)
    p0.backward(dp)
    # the reference, fed from its own statistics through the float64 BatchNorm chain of tests/bn_double.py
    count = b * h * w
    plain = sc.stem_forward(x, w27, torch.ones(64, dtype=torch.float64), torch.zeros(64, dtype=torch.float64))
    close(plain["y"], y0.detach().permute(0, 2, 3, 1), "y")
    st = bn_double.forward(plain["sum_y"], plain["sum_y2"], count, gamma, beta, eps=EPS)
    fwd = sc.stem_forward(x, w27, st["scale"], st["shift"])
    close(fwd["pooled"], p0.detach().permute(0, 2, 3, 1), "pooled")
    hh, ww = sc.argmax_pixel(fwd["arg"])
    assert torch.equal((hh * w + ww).expand_as(fwd["arg"]), idx0.permute(0, 2, 3, 1))          # generic data: no ties
    dpool = dp.permute(0, 2, 3, 1).contiguous()
    _, red = sc.stem_reduce(fwd, st["scale"], st["shift"], dpool, st["mean"], st["invstd"])
    coef = bn_double.backward(red[0], red[1], count, gamma, st["mean"], st["invstd"])
    close(coef["dbeta"], bl.grad, "dbeta")
    close(coef["dgamma"], gl.grad, "dgamma")
    bwd = sc.stem_backward(x, w27, st["scale"], st["shift"], fwd, dpool, st["mean"], st["invstd"], coef["ca"], coef["cb"], coef["cc"])
    close(bwd["dw"], wl.grad, "dW = sum dy col")
    close(bwd["dw_gram"], wl.grad, "dW = ca D + cb (W G) + cc s")
    close(bwd["dx"], xl.grad, "dx")
    assert torch.equal(bwd["d"], bwd["d_pooled"])                                              # the two ReLU masks are one mask
    # the eval-mode form: BatchNorm with fixed statistics, dy0 = ca d
    xe = x.clone().requires_grad_(True)
    ye = F.conv2d(xe, w27.view(64, 3, 3, 3).permute(0, 3, 1, 2), None, 1, 1)
    pe = F.max_pool2d(F.relu(ye * st["scale"].view(1, 64, 1, 1) + st["shift"].view(1, 64, 1, 1)), 3, 2, 1)
    pe.backward(dp)
    ev = sc.stem_backward(x, w27, st["scale"], st["shift"], fwd, dpool, st["mean"], st["invstd"], st["scale"], 0 * gamma, 0 * gamma)
    close(ev["dx_eval"], xe.grad, "dx, eval mode")
    close(ev["dx"], xe.grad, "dx with cb = cc = 0")


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 5, 4), (2, 4, 5), (3, 9, 7)])
def test_the_stride_2_reference_agrees_with_float64_autograd(shape):
    b, h, w = shape
    gen = torch.Generator().manual_seed(99 + h)
    x = torch.randn((b, 3, h, w), generator=gen, dtype=torch.float64).requires_grad_(True)
    w27 = torch.randn((64, 27), generator=gen, dtype=torch.float64)
    y = F.conv2d(x, w27.view(64, 3, 3, 3).permute(0, 3, 1, 2), None, 2, 1)
    dy0 = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    y.backward(dy0)
    close(sc.stem_dx_s2(dy0.permute(0, 2, 3, 1).contiguous(), w27, h, w), x.grad, "dx, stride 2")


def test_the_table_is_what_the_kernels_need():
    assert len(sc.BY_NAME) == len(sc.CASES) and len(set((c.b, c.h, c.w) for c in sc.CASES)) == len(sc.CASES)
    shapes = {(c.b, c.h, c.w) for c in sc.FULL}
    hp = lambda h: (h - 1) // 2 + 1
    # both sides of the pooled tile edge (8 | 9 rows, 56 | 57 columns), alone and together; three tiles each way
    assert [sc.tiles(sc.BY_NAME["2x%dx6" % h])[0] for h in (7, 8, 9)] == [1, 1, 2] and [hp(h) for h in (7, 8, 9)] == [4, 4, 5]
    assert [sc.tiles(sc.BY_NAME["1x3x%d" % w])[1] for w in (55, 56, 57)] == [1, 1, 2]
    assert sc.tiles(sc.BY_NAME["2x9x57"]) == (2, 2) and sc.tiles(sc.BY_NAME["1x17x113"]) == (3, 3)
    # one row, one column, one pixel, one pooled pixel
    assert {(1, 1, 1), (2, 1, 5), (2, 5, 1), (2, 2, 2)} <= shapes
    # the statistics kernel: 16-pixel steps and the row pairs of the four waves of an 8-row band
    assert {(1, 2, w) for w in (sc.STATS_STEP - 1, sc.STATS_STEP, sc.STATS_STEP + 1)} <= shapes
    assert {(1, 3, 4), (1, sc.STATS_ROWS, 4), (1, sc.STATS_ROWS + 1, 4)} <= shapes
    # the 16 x 16 image-gradient tile and the 8 x 8 pooled gather tile (16 x 16 pixels), both sides
    t = sc.DX_TILE
    assert {(2, t, t), (2, t + 1, t), (2, t, t + 1), (1, t, t), (1, t + 1, t + 1)} <= shapes and 2 * sc.DG_TILE == t
    gather_tiles = lambda c: c.b * -(-hp(c.h) // sc.DG_TILE) * -(-hp(c.w) // sc.DG_TILE)
    assert (sc.stem_blocks(sc.BY_NAME["1x3x40"]), gather_tiles(sc.BY_NAME["1x3x40"])) == (1, 3)
    assert (sc.stem_blocks(sc.BY_NAME["1x20x3"]), gather_tiles(sc.BY_NAME["1x20x3"])) == (3, 2)
    # both grid caps, each with a workgroup that makes a second trip
    big = sc.BY_NAME["1030x3x3"]
    assert sc.stem_blocks(big) == sc.STEM_BLOCKS_CAP < big.b * 1 and sc.gram_blocks(big) == sc.GRAM_BLOCKS_CAP < big.b
    assert all(sc.stem_blocks(c) < sc.STEM_BLOCKS_CAP and sc.gram_blocks(c) < sc.GRAM_BLOCKS_CAP for c in sc.CASES if c is not big)
    # nothing but the batch of 3 x 3 images is larger than a few thousand pixels
    assert all(c.b * c.h * c.w <= 2500 for c in sc.CASES if c is not big) and big.b * big.h * big.w < 10000
    assert [(c.h, c.w, c.only, c.dtypes) for c in sc.CASES if c.only] == [(2, 544, "stats", ("fp32",)), (2, 1090, "stats", ("bf16",)),
                                                                            (2, 510, "gram", ("fp32", "bf16"))]
    assert len(sc.S2_CASES) == 10 and {kp for *_, kp in sc.S2_CASES} == {32, 64}


def test_the_stem_block_counts_are_the_library_s():
    import __graft_entry__ as ge
    ge.build()
    from frhip._abi import lib
    for case in sc.CASES:
        assert lib().frhip_stem_blocks(case.b, case.h, case.w) == sc.stem_blocks(case), case.name
        assert lib().frhip_stem_gram_blocks(case.b, case.h, case.w) == sc.gram_blocks(case), case.name
    assert lib().frhip_stem_gram_floats() == sc.GRAM_FLOATS


def test_the_worst_case_of_the_operand_ranges_is_exact():
    """the bounds of the module docstring from the extreme values of every operand, and what they need of bf16 and fp32"""
    y = 27 * 1 * 1
    a = y * 2 + 4
    d = 4 * 2
    dy = 2 * d + 1 * y + 3
    assert (y, a, d, dy) == (27, 58, 8, 46) and dy <= 46.5
    for top in (a, 46.5):                                             # halves up to `top`: every one a bf16 value (8 significant bits)
        v = torch.arange(-2 * top, 2 * top + 1, dtype=torch.float64) / 2
        assert torch.equal(v.bfloat16().double(), v)
    pixels = max(c.b * c.h * c.w for c in sc.CASES)
    assert pixels * y * y < 2 ** 24 and pixels * dy < 2 ** 24 and pixels * d * y < 2 ** 24 and 9 * 64 * 46.5 < 2 ** 24
    assert 2 * (pixels * d * y + 2 * pixels * d) < 2 ** 24            # invstd (sum d y - mean sum d)
    assert 2 * pixels * d + 27 * pixels + 3 * pixels + 7 < 2 ** 23    # ca D + cb (W G) + cc s + dw0, halves: one bit less


@pytest.mark.parametrize("name", [case.name for case in sc.CASES])
def test_every_value_and_every_sum_of_the_case_is_exact(name):
    case, ops, ref, bound = sc.BY_NAME[name], sc.operands(name), sc.reference(name), sc.bounds(name)
    assert set(ops["x"].unique().tolist()) <= {-1.0, 0.0, 1.0} and set(ops["w"].unique().tolist()) == {-1.0, 0.0, 1.0}
    assert set(ops["scale"].tolist()) <= {0.5, 1.0, 2.0, -1.0} and float(ops["shift"].abs().max()) <= 4
    assert float(ops["dpool"].abs().max()) <= 2 and float(ops["mean"].abs().max()) <= 2 and set(ops["invstd"].tolist()) <= {0.5, 1.0, 2.0}
    assert set(ops["ca"].tolist()) <= {1.0, 2.0, -1.0} and set(ops["cb"].tolist()) <= {0.0, 1.0, -1.0, 0.5}
    assert float(ops["cc"].abs().max()) <= 3 and float(ops["dw0"].abs().min()) >= 1 and float(ops["dw0"].abs().max()) <= 7
    halves = lambda t: torch.equal(t * 2, (t * 2).round())
    exact = lambda t: halves(t) and torch.equal(t.float().double(), t)
    assert bound["y"] <= 27 and bound["a"] <= 58 and halves(ref["a"]) and torch.equal(ref["a"].bfloat16().double(), ref["a"])
    assert torch.equal(ref["pooled"].bfloat16().double(), ref["pooled"]) and float(ref["pooled"].min()) >= 0
    assert max(bound["sum_y"], bound["sum_y2"], bound["gram"]) < 2 ** 24
    assert exact(ref["sum_y"]) and exact(ref["sum_y2"]) and exact(ref["gram"])
    if case.only is not None:
        return
    assert bound["d"] <= 8 and bound["dy"] <= 46.5 and halves(ref["dy"]) and torch.equal(ref["dy"].bfloat16().double(), ref["dy"])
    dy0 = ops["ca"] * ref["d_pooled"]
    assert torch.equal(dy0.bfloat16().double(), dy0)
    assert max(bound["sum_d"], bound["sum_dy"], bound["reduce"], bound["dw"], bound["dx"]) < 2 ** 24 and bound["dw_gram"] < 2 ** 23
    for key in ("reduce", "dw", "D", "dw_gram", "dx", "dx_eval"):
        assert exact(ref[key]), key
    assert exact(ref["dw"] + ops["dw0"])
    # the same numbers by two routes: the weight gradient from dy and from the algebra, the ReLU mask from y and from pooled
    assert torch.equal(ref["dw"], ref["dw_gram"]) and torch.equal(ref["d"], ref["d_pooled"])
    assert float(ref["dw"].abs().max()) > 0 and float(ref["dx"].abs().max()) > 0 and float(ref["reduce"].abs().max(1).values.min()) > 0


@pytest.mark.parametrize("name", [case.name for case in sc.FULL])
def test_every_case_has_the_coverage_it_claims(name):
    case = sc.BY_NAME[name]
    missing = sc.claims(case) - sc.coverage(name)
    assert not missing, (name, sorted(missing))


def test_the_table_as_a_whole_has_every_claim():
    every = set().union(*(sc.claims(case) for case in sc.FULL))
    assert every == {"zero", "mask", "tie", "taps", "two windows, row pair", "two windows, column pair", "two windows, diagonal",
                     "arg-max in the tile above", "arg-max in the tile to the left", "arg-max in the tile diagonally"}
    assert sc.claims(sc.BY_NAME["1x1x1"]) == {"zero", "mask"}
    assert {"arg-max in the tile above", "arg-max in the tile to the left", "arg-max in the tile diagonally"} <= sc.claims(sc.BY_NAME["2x9x57"])


def test_the_second_trip_of_a_workgroup_sees_other_images():
    """1030 images of one tile and one Gram band each: workgroup k of the 1024 takes images k and k + 1024, workgroup k of the 512 Gram
    workgroups images k, k + 512 and k + 1024.  A kernel that forgot to re-stage on its second trip would repeat the first image's values,
    so the images of one workgroup must differ in everything it stages."""
    name = "1030x3x3"
    case, ops, ref = sc.BY_NAME[name], sc.operands(name), sc.reference(name)
    assert sc.tiles(case) == (1, 1) and case.h <= sc.GRAM_ROWS
    differ = lambda t, i, j: not torch.equal(t[i], t[j])
    for k in range(case.b - sc.STEM_BLOCKS_CAP):
        for t in (ops["x"], ops["dpool"], ref["arg"], ref["pooled"], ref["y"]):
            assert differ(t, k, k + sc.STEM_BLOCKS_CAP), k
    for k in range(sc.GRAM_BLOCKS_CAP):
        assert differ(ops["x"], k, k + sc.GRAM_BLOCKS_CAP)
        if k + 2 * sc.GRAM_BLOCKS_CAP < case.b:
            assert differ(ops["x"], k, k + 2 * sc.GRAM_BLOCKS_CAP) and differ(ops["x"], k + sc.GRAM_BLOCKS_CAP, k + 2 * sc.GRAM_BLOCKS_CAP)
    # and the carried accumulators matter: the second trip's own contribution is not zero
    late = ops["x"][sc.STEM_BLOCKS_CAP:]
    assert float(sc.im2col(late).abs().sum()) > 0 and float(ops["dpool"][sc.STEM_BLOCKS_CAP:].abs().sum()) > 0


def test_one_past_the_widest_rows_is_refused_on_the_host():
    """3 x 10 x (w + 2) elements of the statistics kernel's window must fit 64 KiB, 3 x 10 x (w + 2) floats of the Gram kernel's 60 KiB:
    544 fp32 / 1090 bf16 / 510 columns are the widest rows, and one more returns FRHIP_EINVAL with its message before any device call
    (the pointers here are NULL and there is no device)."""
    import __graft_entry__ as ge
    ge.build()
    from frhip._abi import lib
    assert 3 * 10 * (544 + 2) * 4 <= 64 * 1024 < 3 * 10 * (545 + 2) * 4 and 3 * 10 * (1090 + 2) * 2 <= 64 * 1024 < 3 * 10 * (1091 + 2) * 2
    assert 3 * 10 * (510 + 2) * 4 <= 60 * 1024 < 3 * 10 * (511 + 2) * 4
    for entry, dt, b, h, w, message in sc.REFUSALS:
        if entry == "frhip_stem_stats":
            rc = lib().frhip_stem_stats(dt, None, None, b, h, w, None, None)
        else:
            rc = lib().frhip_stem_gram(dt, None, b, h, w, None, None, None)
        assert rc == -1 and lib().frhip_last_error().decode() == message, (entry, dt, w, rc, lib().frhip_last_error())
