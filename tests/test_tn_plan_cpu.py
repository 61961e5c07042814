"""The launch plan of the weight gradients (csrc/tn_plan.h, read through frhip_wgrad_plan) against a committed table: which kernel a layer
runs on, its K split, whether the splits go through slabs and the reduce tree.  No GPU: the query touches no device.

tests/golden/tn_plan_table.json holds, per row, the query's arguments (dtype, n, h, w, c, kc, ldp, r, s, stride, pad, splits, have_workspace,
workspace_bytes, overwrite, transform), the frhip_set_wgrad_taps9 switch and either the expected plan or the expected error text.  The
expected values were produced by the host code of the commit BEFORE the plan was factored out (its split loops, slab rules, branch
conditions and reduce-tree arithmetic copied into a stand-alone program), so a row that fails says that a launch has changed, which on
the GPU would show only as a step-time or summation-order difference.  A deliberate change of the plan regenerates the rows it moves."""
import ast
import ctypes
import json
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "tn_plan_table.json")) as f:
    TABLE = json.load(f)
FIELDS = ("family", "instantiation", "splits", "ksteps", "ksteps_per_split", "store", "groups", "per_group")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from frhip import _abi
    return _abi.lib()


def query(lib, row):
    """-> (rc, plan, error text) of one table row, under the row's nine-tap switch"""
    plan = (ctypes.c_int * 8)(*([-7] * 8))
    old = lib.frhip_set_wgrad_taps9(row["taps9"])
    try:
        rc = lib.frhip_wgrad_plan(*row["args"], plan)
    finally:
        lib.frhip_set_wgrad_taps9(old)
    return rc, list(plan), lib.frhip_last_error().decode()


def test_every_row_of_the_table_gets_its_plan(lib):
    assert len(TABLE) >= 140 and len({row["name"] for row in TABLE}) == len(TABLE)
    wrong = []
    for row in TABLE:
        rc, plan, err = query(lib, row)
        if "error" in row:
            if rc != -1 or err != row["error"] or plan != [-7] * 8:
                wrong.append((row["name"], rc, err, plan))
        elif rc != 0 or plan != row["plan"]:
            wrong.append((row["name"], rc, dict(zip(FIELDS, plan)), dict(zip(FIELDS, row["plan"]))))
    assert not wrong, wrong
    assert lib.frhip_set_wgrad_taps9(-1) == 1


def test_the_table_has_every_family_and_every_nine_tap_instantiation():
    plans = [row["plan"] for row in TABLE if "plan" in row]
    assert {p[0] for p in plans} == {0, 1, 2, 3}
    # the table is wanted wherever there is no operand transform; the launch decides whether it can be had
    assert {p[1] for p in plans if p[0] == 2} == {102, 103, 12, 13, 14}
    assert {p[5] for p in plans} == {0, 1, 2}
    assert any(p[6] > 1 for p in plans if p[0] < 2) and any(p[6] > 1 for p in plans if p[0] == 2) and any(p[6] > 1 for p in plans if p[0] == 3)


def test_every_plan_covers_its_k_range_and_fits_its_workspace(lib):
    for row in TABLE:
        if "error" in row:
            continue
        rc, plan, _ = query(lib, row)
        assert rc == 0, row["name"]
        dt, n, h, w, c, kc, ldp, r, s, stride, pad, want_splits, have_ws, ws_bytes, overwrite, transform = row["args"]
        family, inst, splits, ksteps, per, store, groups, per_group = plan
        out_elems = kc * r * s * c
        assert splits >= 1, row["name"]
        assert per * (splits - 1) < ksteps <= per * splits, row["name"]
        m = n * ((h + 2 * pad - r) // stride + 1) * ((w + 2 * pad - s) // stride + 1)
        assert ksteps == (n if family == 3 else (m + 63) // 64), row["name"]
        if store == 1:
            assert have_ws and splits * out_elems * 4 <= ws_bytes and splits > 1, row["name"]
        elif store == 2:
            assert overwrite and splits == 1 and family < 2, row["name"]
        else:
            assert store == 0 and splits == 1, row["name"]
        assert (groups >= 1) == (store == 1), row["name"]
        if groups:
            assert per_group * (groups - 1) < splits <= per_group * groups, row["name"]
        if want_splits > 0:
            assert splits <= want_splits, row["name"]
        assert (inst != 0) == (family == 2) and (inst >= 100) == bool(transform), row["name"]


def test_the_table_covers_every_weight_gradient_of_the_recorded_networks():
    """every conv_wgrad and gemm_tn signature of SWIN34_LAUNCHES / ALTERNET50_LAUNCHES (tests/test_bench_launches_gpu.py) has its row: a
    network change that adds a weight-gradient shape must add its plan"""
    with open(os.path.join(HERE, "test_bench_launches_gpu.py")) as f:
        src = f.read()
    have = {tuple(row["args"]) for row in TABLE if "plan" in row and row["taps9"] == 1}
    ws = 160 << 20
    seen = 0
    for net in ("SWIN34", "ALTERNET50"):
        for sig in ast.literal_eval(re.search(r"^%s_LAUNCHES = (\{.*?^\})" % net, src, flags=re.S | re.M).group(1)):
            if sig[0] == "conv_wgrad":
                _, dt, n, h, w, c, k, r, s, stride, pad, splits = sig
                args = (0, n, h, w, c, k, k, r, s, stride, pad, splits, 1, ws, 0, 0)
            elif sig[0] == "gemm_tn":
                _, dt, m, kc, ldp, c, splits, overwrite = sig
                args = (0, m, 1, 1, c, kc, ldp, 1, 1, 1, 0, splits, 1, ws, int(overwrite), 0)
            else:
                continue
            assert dt == "bf16" and args in have, sig
            seen += 1
    assert seen >= 30


def test_ops_wrapper_reads_the_same_plan(lib):
    from frhip import ops
    assert ops.WORKSPACE_BYTES == 160 << 20
    row = next(r for r in TABLE if r["name"] == "resnet50 3x3/s1 14x14x256")
    assert ops.wgrad_plan(*row["args"][:11]) == tuple(row["plan"])
    assert ops.WGRAD_FAMILIES[row["plan"][0]] == "rows"
    row = next(r for r in TABLE if r["name"] == "no workspace, overwrite, many rows")
    assert ops.wgrad_plan(*row["args"][:12], workspace_bytes=None, overwrite=True) == tuple(row["plan"])
