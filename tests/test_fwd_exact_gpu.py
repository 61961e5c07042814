"""Every route of the forward convolutions on the GPU, on operands whose results bf16 and fp32 hold exactly.

tests/fwd_cases.py has the cases -- one per kernel family, NT tile, store epilogue, strided filter and map edge, each with the variants it
runs (bare, with statistics, folded eval BatchNorm with and without ReLU and residual, operand transform with and without act_out and
statistics) -- and the integer reference; tests/test_fwd_cases_cpu.py pins that each run still takes the route it claims.  Here each run
goes through its C entry point under the case's switches, twice.  y (or the affine output), act_out and the partial rows each sit inside a
larger buffer, the interior filled with NaN beforehand, between guard rows that must come back untouched; x, w and the residual lie
between NaN guards, so that a read outside the tensor poisons the result.  y and act_out must EQUAL the reference (torch.equal, no
tolerance): one unwritten pixel, one dropped tap or K chunk, one tap gathered from the neighbouring row, one padding pixel that went through
the operand transform is at least an integer off.  The partial rows: as many as frhip_conv_fwd_route reports, every element finite, each
row equal to the reference's own sums over its block of output rows -- one launch and no parity offsets, so this holds per row on the
generic and the halo routes alike."""
import ctypes

import pytest
import torch

import fwd_cases as fc

pytestmark = pytest.mark.gpu


def _lib():
    from frhip._abi import lib
    return lib()


def _equal(got, want, what, where):
    want = want.double()
    wrong = got != want
    assert torch.equal(got, want), where + (
        what, "%d of %d elements differ, %d are NaN" % (int(wrong.sum()), got.numel(), int(got.isnan().sum())),
        "first at %r" % (wrong.nonzero()[0].tolist(),))


@pytest.mark.parametrize("name,variant", fc.RUNS, ids=["%s / %s" % run for run in fc.RUNS])
def test_forward_convolution_equals_the_integer_reference(name, variant):
    case = fc.BY_NAME[name]
    want = fc.expected(name, variant)
    lib = _lib()
    if "persistent" in name:
        # the lean kernel of the 256 x 256 tile launches at most one workgroup per compute unit, in whole eights
        tiles = (fc.rows(case) // 256) * (case.k // 256)
        workgroups = torch.cuda.get_device_properties(0).multi_processor_count & ~7
        assert 8 <= workgroups < tiles, "the persistent case is sized for a device of %d compute units" % fc.PERSISTENT_CUS
    with fc.switches(lib, case):
        route = (ctypes.c_int * 5)()
        assert lib.frhip_conv_fwd_route(*fc.shape_args(case), fc.VARIANTS[variant][0], route) == 0
        for run in range(2):
            where = (name, variant, "run %d" % run)
            y, act, part, clean = fc.launch(name, variant)
            assert clean, where + ("a guard row was written",)
            _equal(y, want["y"], "y", where)
            assert (act is None) == (want["act"] is None)
            if act is not None:
                _equal(act, want["act"], "act_out", where)
            assert (part is None) == (want["rows"] is None)
            if part is not None:
                assert part.shape[0] == route[4] == want["rows"].shape[0], where
                assert bool(part.isfinite().all()), where + ("%d elements of the partial rows are not finite" % int((~part.isfinite()).sum()),)
                _equal(part, want["rows"], "partial rows", where)


def test_the_switches_are_back_at_their_defaults():
    lib = _lib()
    tile, halo = lib.frhip_set_nt_tile(0), lib.frhip_set_conv_halo(1)
    lib.frhip_set_nt_tile(tile), lib.frhip_set_conv_halo(halo)
    assert (lib.frhip_set_halo_wide_dirs(-1), lib.frhip_set_epi_lean(-1), tile, halo) == (2, 1, 0, 1)
