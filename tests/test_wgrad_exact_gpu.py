"""Every branch of the weight gradients' launch plan (csrc/tn_plan.h) on the GPU, on operands whose sums fp32 holds exactly.

tests/wgrad_cases.py has the cases -- one per kernel family, nine-tap instantiation, store path, reduce-tree depth, short last split and
split that starts inside the lane-mask period; tests/test_wgrad_cases_cpu.py pins that each still gets that plan -- and the integer
reference.  Here each case runs through its public op and must EQUAL the reference (torch.equal, no tolerance), twice, so it is also the
same from run to run.  The nine-tap cases run on both twins of their instantiation: with frhip_set_wgrad_mask_table(0), which always
tracks the padding predicates per lane, and with the default, which takes the lane-mask table when the process-wide cache (8 geometries,
period <= 64) has or can take the geometry.  Which twin the default run took depends on what ran earlier in the process, so it is
reported (printed, and in the junit properties), not required; the fresh process of the last test is where the table twins MUST run."""
import os
import subprocess
import sys
import time

import pytest
import torch

import wgrad_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _lib():
    from frhip._abi import lib
    return lib()


def run_twice(name):
    want = wc.expected(name)
    for run in range(2):
        got = wc.launch(name)
        wrong = int((got != want).sum())
        assert torch.equal(got, want), (name, "run %d" % run, "%d of %d elements differ" % (wrong, want.numel()),
                                        "largest difference %r" % float((got - want).abs().nan_to_num(float("inf")).max()))


@pytest.mark.parametrize("name", [case.name for case in wc.CASES])
def test_weight_gradient_equals_the_integer_reference(name, record_property):
    case = wc.BY_NAME[name]
    lib = _lib()
    assert lib.frhip_set_wgrad_mask_table(-1) == 1
    if not wc.nine_tap(case):
        run_twice(name)
        return
    old = lib.frhip_set_wgrad_mask_table(0)
    try:
        before = lib.frhip_wgrad_mask_table_period(case.h, case.w)
        run_twice(name)
        assert lib.frhip_wgrad_mask_table_period(case.h, case.w) == before           # the twin without the table asks for none
    finally:
        lib.frhip_set_wgrad_mask_table(old)
    run_twice(name)
    cached = lib.frhip_wgrad_mask_table_period(case.h, case.w)
    period = wc.period(case.h, case.w)
    if period > wc.MAX_TABLE_PERIOD:
        assert cached == 0
    else:
        assert cached in (0, period)
    twin = "table" if wc.wants_table(case) and cached else "no table"
    record_property("nine_tap_twin", twin)
    print("nine-tap twin of the default run: %-9s inst %3d  %dx%d (period %d)  %s" % (twin, case.plan[1], case.h, case.w, period, name))


CHILD = r'''
import os, sys
import torch
sys.path[:0] = [%r, os.path.join(%r, "face-recognition-pytorch_amd"), os.path.join(%r, "tests")]
import wgrad_cases as wc
from frhip._abi import lib
assert lib().frhip_set_wgrad_mask_table(-1) == 1
for name in wc.CHILD_TABLE_CASES + [wc.CHILD_NINTH_CASE]:
    case = wc.BY_NAME[name]
    assert lib().frhip_wgrad_mask_table_period(case.h, case.w) == 0, name                # a fresh process: nothing cached yet
    got = wc.launch(name)
    cached = lib().frhip_wgrad_mask_table_period(case.h, case.w)
    assert cached == (0 if name == wc.CHILD_NINTH_CASE else wc.period(case.h, case.w)), (name, cached)
    assert torch.equal(got, wc.expected(name)), name
    print("child: inst %%d  %%dx%%d  table period %%d  %%s" %% (case.plan[1], case.h, case.w, cached, name), flush=True)
print("child: done")
''' % (ROOT, ROOT, ROOT)
CHILD_TIMEOUT = 7       # seconds: the child takes 1.9 - 2.2 s (interpreter and torch start, device start, nine launches), about 3 x that


def test_table_twins_in_a_fresh_process_then_a_ninth_geometry_without():
    """One fresh interpreter, one device, default settings: its table cache is empty, so the eight geometries of CHILD_TABLE_CASES
    (instantiations 12, 13 and 14) each get their table -- the query reports the period H W / gcd(H W, 64) after the launch -- and the
    ninth geometry finds the cache full and runs without.  All nine equal the integer reference."""
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-c", CHILD], env=dict(os.environ), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=CHILD_TIMEOUT)
    out = r.stdout.decode(errors="replace")
    print(out)
    print("the child took %.1f s of its %d s" % (time.perf_counter() - t0, CHILD_TIMEOUT))
    assert r.returncode == 0, out
    lines = [line for line in out.splitlines() if line.startswith("child: ")]
    assert len(lines) == len(wc.CHILD_TABLE_CASES) + 2 and lines[-1] == "child: done", out
