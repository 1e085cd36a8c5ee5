"""tests/test_gpu_noise_runs.py on the CPU, through the SIMT emulation of tests/hip_emu (TEST INFRASTRUCTURE): the same checks
of noise_mfma65_kernel's runs of consecutive tiles, at shapes cut to the emulated chip - 4 CUs, 8 blocks at once - so that a
batch is cut into runs of several tiles and a row alone into single ones, as on the MI355X at the GPU module's shapes."""
import pytest

import test_gpu_noise_runs as G
from tests.hip_emu import emu_simt

ddsp = emu_simt.ddsp_fixture(G)

# (batch, frames, samples): two runs of three tiles per row (canonical; ragged with an odd N; frames of 192 samples) on 6 of the 8
# blocks; a row alone: 7 single tiles (tests/test_noise_mfma_plan.py holds both to that)
SHAPES = [(3, 180, 11520), (3, 180, 11520 - 17), (3, 60, 11520)]


@pytest.mark.parametrize('source', G.SOURCES)
@pytest.mark.parametrize('b,f,n', SHAPES)
def test_rows_in_runs_equal_rows_alone_and_the_oracle(ddsp, b, f, n, source):
  G.check_runs(ddsp, b, f, n, source)


def test_generated_2048_level_noise_equals_the_same_noise_supplied_in_runs(ddsp):
  G.check_gen11_equals_supplied11(ddsp, *SHAPES[0])
