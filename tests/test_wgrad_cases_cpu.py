"""The case table of the exact weight-gradient tests (tests/wgrad_cases.py), checked without a GPU: every case still gets the launch plan
it claims (csrc/tn_plan.h through frhip_wgrad_plan), the table as a whole covers every branch of the plan, the two CPU references agree
bit for bit and every sum stays an integer fp32 holds.  A later change of the plan then cannot silently turn a case of
tests/test_wgrad_exact_gpu.py into a duplicate of another."""
import ctypes

import pytest
import torch

import wgrad_cases as wc


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from frhip import _abi
    return _abi.lib()


def query(lib, args, taps9):
    plan = (ctypes.c_int * 8)(*([-7] * 8))
    old = lib.frhip_set_wgrad_taps9(taps9)
    try:
        rc = lib.frhip_wgrad_plan(*args, plan)
    finally:
        lib.frhip_set_wgrad_taps9(old)
    return rc, tuple(plan)


def test_every_case_gets_the_plan_it_claims(lib):
    assert len(wc.BY_NAME) == len(wc.CASES)
    wrong = []
    for case in wc.CASES:
        rc, plan = query(lib, wc.plan_args(case), case.taps9)
        if rc != 0 or plan != case.plan or (case.tree, case.short, case.mid) != wc.derived_claims(case):
            wrong.append((case.name, rc, plan, case.plan, wc.derived_claims(case)))
    assert not wrong, wrong
    assert lib.frhip_set_wgrad_taps9(-1) == 1


def test_no_two_cases_are_the_same_launch():
    keys = [(case.op, case.dtype, wc.plan_args(case), case.taps9) for case in wc.CASES]
    assert len(set(keys)) == len(keys)


def test_the_table_covers_every_branch_of_the_plan():
    fam = lambda *families: [case for case in wc.CASES if case.plan[0] in families]
    plain9 = [case for case in fam(wc.TAPS9) if case.op == "conv"]
    xform = [case for case in fam(wc.TAPS9) if case.op == "bnrelu"]
    assert {case.plan[0] for case in wc.CASES} == {wc.TAP128, wc.TAP256, wc.TAPS9, wc.ROWS}
    assert {case.plan[5] for case in wc.CASES} == {wc.OUT, wc.SLABS, wc.OVERWRITE}
    # clear-then-slabs with one reduce pass and through the two-level tree
    assert {case.tree for case in wc.CASES if wc.clears_output(case) and case.plan[5] == wc.SLABS} == {False, True}
    assert len(plain9) + len(xform) == len(fam(wc.TAPS9))
    for group in (fam(wc.TAP128), fam(wc.TAP256), plain9, xform, fam(wc.ROWS)):
        assert any(case.tree for case in group)
    for group in (fam(wc.TAP128, wc.TAP256), plain9):
        assert any(case.short for case in group)
    assert {case.plan[1] for case in fam(wc.TAPS9)} == {12, 13, 14, 102, 103}
    assert {case.plan[1] for case in wc.CASES if wc.table_capable(case)} == {12, 13, 14}
    assert {case.plan[1] for case in wc.CASES if case.mid} == {12, 13, 14}
    no_table = {(case.h, case.w) for case in plain9 if not wc.table_capable(case)}
    assert len(no_table) >= 2 and all(wc.period(h, w) > wc.MAX_TABLE_PERIOD for h, w in no_table)
    # one K step over several images, maps one pixel high / wide, both sides of each stage boundary and of the per-tap hand-over
    assert any(case.h * case.w < 64 for case in plain9) and any(case.h == 1 for case in plain9) and any(case.w == 1 for case in plain9)
    by_width = {case.w: case.plan[:2] for case in wc.CASES if case.op == "conv" and case.taps9 and (case.r, case.stride) == (3, 1)}
    assert [by_width[w] for w in (15, 16, 31, 32, 56, 57)] == [(2, 14), (2, 13), (2, 13), (2, 12), (2, 12), (0, 0)]
    # every M is ragged somewhere: a last K step that is not whole, in each kernel that steps through pixels
    for group in (fam(wc.TAP128), fam(wc.TAP256), plain9, xform):
        assert any(wc.gemm_rows(case) % 64 for case in group)
    assert any(case.ldp > case.kc for case in wc.CASES) and any(case.dtype == "fp32" for case in wc.CASES)
    assert any(not case.workspace for case in wc.CASES)


def test_the_child_process_list_fits_the_table_cache():
    cases = [wc.BY_NAME[name] for name in wc.CHILD_TABLE_CASES]
    geoms = {(case.h, case.w) for case in cases}
    assert all(wc.table_capable(case) for case in cases)
    assert len(geoms) == len(cases) <= wc.TABLE_GEOMETRIES == 8
    assert {case.plan[1] for case in cases} == {12, 13, 14}
    assert any(case.mid for case in cases)
    ninth = wc.BY_NAME[wc.CHILD_NINTH_CASE]
    assert wc.table_capable(ninth) and (ninth.h, ninth.w) not in geoms and len(geoms) == wc.TABLE_GEOMETRIES


def test_the_overwrite_cases_run_with_the_searched_split_count():
    """frhip_gemm_tn_overwrite has no splits argument: an overwrite case states splits = 0, and the one that goes through the tree gets
    there by its size"""
    from frhip import _abi
    params = {name: params for _, name, params in _abi.prototypes()}
    assert not any("splits" in p for p in params["frhip_gemm_tn_overwrite"]) and any("splits" in p for p in params["frhip_gemm_tn"])
    cases = [case for case in wc.CASES if wc.overwrite(case)]
    assert all(case.splits == 0 for case in cases)
    assert [(case.plan[2], case.tree) for case in cases if wc.clears_output(case)] == [(9, False), (34, True)]


@pytest.mark.parametrize("name", [case.name for case in wc.CASES])
def test_the_two_references_agree_and_every_sum_is_exact_in_fp32(name):
    case = wc.BY_NAME[name]
    data = wc.operands(name)
    assert int(data["x"].abs().max()) <= 4 and int(data["dy"].abs().max()) <= 4 and int(data["dw0"].abs().max()) <= 8
    assert int(data["dw0"].abs().max()) > 0
    if case.op == "bnrelu":
        assert set(data["scale"].tolist()) <= {-2, -1, 1, 2} and int(data["shift"].abs().max()) <= 3
        act = wc.activated(name)
        assert int(act.min()) == 0 and int(act.max()) <= 11 and torch.equal(act.bfloat16().long(), act)
    assert wc.bound(name) < 2 ** 24
    a, b = wc.reference_f64(name), wc.reference_i64(name)
    assert a.dtype == torch.float64 and b.dtype == torch.int64 and a.shape == b.shape == (case.kc, case.r, case.s, case.c)
    assert torch.equal(a, b.double()) and torch.equal(a.long(), b)
    assert int(b.abs().max()) > 0 and int(b.abs().max()) + 8 <= wc.bound(name)
    want = wc.expected(name)
    assert torch.equal(want.float().double(), want)


@pytest.mark.parametrize("name", [case.name for case in wc.CASES if wc.nine_tap(case)])
def test_a_wrong_padding_predicate_would_show_in_every_tap(name):
    """The nine-tap kernel reads tap (dy, dx) of pixel m at pixel m + dy W + dx of the flattened stream and replaces the lanes whose
    neighbour is padding by zeros.  Without that replacement -- the neighbour read from the next row or the next image -- each of the
    eight outer taps of every case must come out different from the reference, so the operands cannot hide a padding error."""
    case = wc.BY_NAME[name]
    m = wc.gemm_rows(case)
    flat = torch.nn.functional.pad(wc.activated(name).reshape(m, case.c), (0, 0, case.w + 1, case.w + 1))
    p = wc.operands(name)["dy"].reshape(m, case.kc).t().contiguous()
    ref = wc.reference_i64(name)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            start = case.w + 1 + dy * case.w + dx
            leaky = p @ flat[start:start + m]
            assert torch.equal(leaky, ref[:, dy + 1, dx + 1]) == (dy == 0 and dx == 0), (name, dy, dx)


def test_the_mask_table_hooks(lib):
    assert lib.frhip_set_wgrad_mask_table(-1) == 1          # the default, and a query changes nothing
    assert lib.frhip_set_wgrad_mask_table(0) == 1
    try:
        assert lib.frhip_set_wgrad_mask_table(-1) == 0
        assert lib.frhip_set_wgrad_mask_table(5) == 0       # any positive value enables
        assert lib.frhip_set_wgrad_mask_table(0) == 1
    finally:
        lib.frhip_set_wgrad_mask_table(1)
    assert lib.frhip_set_wgrad_mask_table(-1) == 1
    if not torch.cuda.is_available():
        # the query reads the cache of the current device: none here, so nothing is cached, whatever the geometry
        assert [lib.frhip_wgrad_mask_table_period(h, w) for h, w in ((8, 8), (28, 28), (9, 9), (0, 0))] == [0, 0, 0, 0]
