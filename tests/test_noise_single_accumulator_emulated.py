"""tests/test_gpu_noise_single_accumulator.py on the CPU, through the SIMT emulation of tests/hip_emu (TEST INFRASTRUCTURE): the
same shapes, impulses and operand extremes through the same source - the DPP move of the fp32 accumulator included.  The
comparison with the three-accumulator pipeline's measured errors stays with the GPU module: those are an MI355X's figures."""
import pytest

import test_gpu_noise_runs as G
import test_gpu_noise_single_accumulator as S
import test_noise_runs_emulated as E
from tests.hip_emu import emu_simt

ddsp = emu_simt.ddsp_fixture(G)          # (S launches through G.run: G is the module that holds the device)


@pytest.mark.parametrize('source', S.SOURCES)
@pytest.mark.parametrize('b,f', S.SHAPES)
def test_small_shapes_against_the_oracle_and_rows_alone(ddsp, b, f, source):
  S.check_shape(ddsp, b, f, source)


@pytest.mark.parametrize('s', S.IMPULSES)
def test_impulse_gives_the_taps_in_place_and_exact_zeros_elsewhere(ddsp, s):
  S.check_impulse(ddsp, s)


def test_largest_taps_with_23_bit_noise(ddsp):
  S.check_largest_taps(ddsp)


@pytest.mark.parametrize('source', S.SOURCES)
def test_neighbouring_frames_seven_decades_apart(ddsp, source):
  S.check_unequal_frames(ddsp, source)


@pytest.mark.parametrize('exponent', [-20, 20])
def test_supplied_noise_at_any_scale(ddsp, exponent):
  S.check_noise_scale(ddsp, exponent)


@pytest.mark.parametrize('s', S.CONTINUED_IMPULSES)
def test_impulse_across_the_carry_into_a_continued_tile(ddsp, s):
  S.check_impulse(ddsp, s, *E.SHAPES[0][:2])       # (the emulated chip's batch that is cut into runs of several tiles)


def test_taps_at_the_floor(ddsp):
  S.check_taps_at_the_floor(ddsp)


def test_subnormal_lo_parts_reach_the_product(ddsp):
  S.check_subnormal_lo_parts(ddsp)
