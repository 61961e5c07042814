"""Every route of the data-gradient convolutions on the GPU, on operands whose results bf16 and fp32 hold exactly.

tests/dgrad_cases.py has the cases -- one per kernel family, NT tile, store epilogue, parity-class layout and map edge, each with the
epilogue variants it runs (bare, dense or compact residual, masked or unmasked BatchNorm-backward partials, stochastic depth) -- and the
integer reference; tests/test_dgrad_cases_cpu.py pins that each run still takes the route it claims.  Here each run goes through its C
entry point under the case's switches, twice.  dx sits inside a larger buffer, its interior filled with NaN beforehand, between guard rows
that must come back untouched, and must EQUAL the reference (torch.equal, no tolerance): one unwritten pixel, one dropped tap or K chunk,
one padding lane read from the neighbour is at least an integer off.  The partial rows sit in such a buffer too: frhip_dgrad_stat_rows of
them, every element finite afterwards, their sum over the rows equal to the reference's two per-channel sums, and on the halo routes (one
row per 256 output rows) each row equal to the reference's own 256-row sums."""
import pytest
import torch

import dgrad_cases as dc

pytestmark = pytest.mark.gpu


def _lib():
    from frhip._abi import lib
    return lib()


@pytest.mark.parametrize("name,variant", dc.RUNS, ids=["%s / %s" % run for run in dc.RUNS])
def test_data_gradient_equals_the_integer_reference(name, variant):
    case = dc.BY_NAME[name]
    want = dc.expected(name, variant)
    lib = _lib()
    if "persistent" in name:
        # the lean kernel of the 256 x 256 tile launches at most one workgroup per compute unit, in whole eights
        tiles = (dc.rows(case) // 256) * (case.c // 256)
        workgroups = torch.cuda.get_device_properties(0).multi_processor_count & ~7
        assert 8 <= workgroups < tiles, "the persistent case is sized for a device of %d compute units" % dc.PERSISTENT_CUS
    with dc.switches(lib, case):
        for run in range(2):
            dx, part, clean = dc.launch(name, variant)
            assert clean, (name, variant, "run %d" % run, "a guard row was written")
            wrong = dx != want["dx"].double()
            assert torch.equal(dx, want["dx"].double()), (
                name, variant, "run %d" % run, "%d of %d elements differ, %d are NaN" % (int(wrong.sum()), dx.numel(), int(dx.isnan().sum())),
                "first at (n, h, w, c) = %r" % (wrong.nonzero()[0].tolist(),))
            if "s1" not in want:
                assert part is None
                continue
            assert part.shape == (case.route[4], 2, case.c) and bool(part.isfinite().all()), (name, variant, "run %d" % run)
            sums = part.sum(0)
            assert torch.equal(sums[0], want["s1"]) and torch.equal(sums[1], want["s2"]), (
                name, variant, "run %d" % run, "largest difference %r / %r" % (float((sums[0] - want["s1"]).abs().max()),
                                                                              float((sums[1] - want["s2"]).abs().max())))
            if dc.is_halo(case):
                assert torch.equal(part, dc.tile_rows(name, variant)), (name, variant, "run %d" % run)


def test_the_switches_are_back_at_their_defaults():
    lib = _lib()
    tile, halo = lib.frhip_set_nt_tile(0), lib.frhip_set_conv_halo(1)
    lib.frhip_set_nt_tile(tile), lib.frhip_set_conv_halo(halo)
    assert (lib.frhip_set_halo_wide_dirs(-1), lib.frhip_set_epi_lean(-1), tile, halo) == (2, 1, 0, 1)
