"""noise_mfma65_kernel's FIR with ONE accumulator per pair of frames (csrc/filtered_noise_mfma.hip): the tap fragment stays where
it was read, the accumulator moves a column up between the k-steps (Horner's rule), and taps and noise are cut into fp16 parts
on one scale each (split_scaled: taps times 2^13, noise times 2^14), so that hi hi, hi lo and lo hi add up in one place.

What can go wrong with that and what holds it here:
  * a column shifted out of the tile, or one that should have received zeros and did not   -> impulses, exact zeros around them
  * the carry between pairs, wavefronts and tiles in a different order somewhere            -> rows in a batch == rows alone
  * scaled operands leaving fp16's range, or small ones losing their lo parts               -> largest, most unequal, smallest
  * accuracy given away against the three-accumulator pipeline this replaced                -> the parent's measured errors

Shapes: frames of 64 samples, 65 bands, window_size 0.  33 frames is one tile of the kernel plus a frame, 70 two tiles plus (all
four FIR wavefronts work, the carry crosses between them, and the last reaches past the end), 125 is odd.  At these sizes every tile
is a run of its own (noise_mfma_plan.h picks runs of one tile wherever the tiles fit the chip): the carry handed from a tile to
the tile that CONTINUES its run is reached by CONTINUED_* below - an impulse either side of such a boundary, in the batch of
tests/test_gpu_noise_runs.py that tests/test_noise_mfma_plan.py holds to runs longer than a tile - and by that module's own checks.
tests/test_noise_single_accumulator_emulated.py runs the same checks on the CPU emulation."""
import functools

import numpy as np
import pytest

from oracle import ddsp_oracle as O
import test_gpu_noise_runs as G

pytestmark = pytest.mark.gpu

ddsp = G.ddsp                            # the module-scoped fixture: the built library on the device

SOURCES = G.SOURCES
SHAPES = [(1, 1), (2, 33), (2, 70), (3, 125)]       # (batch, frames)
IMPULSES = [0, 63, 64, 127, 128 + 63, 2047, 2048]       # frame, pair and wavefront edges of a 70-frame clip (single tiles)
# a run's first tile ends with output frame 29, the tile that continues it starts at frame 30 with the carry from LDS
CONTINUED_SHAPE = G.SHAPES[0][:2]        # (batch, frames) that the run plan cuts into runs of several tiles on an MI355X
CONTINUED_IMPULSES = [64 * 30 - 1, 64 * 30, 64 * 30 + 63]
START = 62                               # crop_and_compensate_delay of 128 taps: out[n] = z[n + 62]

# (max, RMS) error against the fp64 oracle of every (batch, frames, source) of SHAPES, measured on an MI355X at the parent of the
# commit that introduced the single accumulator (78b39a6: three accumulators, hi + lo / 2048 operands) with errors() below
# (both columns of every row, before and after: profiles/r08_noise_fir_single_accumulator.txt)
PARENT = '78b39a6'
PARENT_ERRORS = {
    (1, 1, 'gen23'): (1.2853e-10, 4.6474e-11),
    (1, 1, 'gen11'): (1.1068e-10, 4.1294e-11),
    (1, 1, 'supplied'): (1.3275e-10, 4.3987e-11),
    (2, 33, 'gen23'): (7.8197e-10, 1.1755e-10),
    (2, 33, 'gen11'): (5.4699e-10, 1.0394e-10),
    (2, 33, 'supplied'): (7.5636e-10, 1.1430e-10),
    (2, 70, 'gen23'): (1.3069e-09, 1.5321e-10),
    (2, 70, 'gen11'): (1.7652e-09, 1.5792e-10),
    (2, 70, 'supplied'): (1.3245e-09, 1.4434e-10),
    (3, 125, 'gen23'): (2.2070e-09, 1.5755e-10),
    (3, 125, 'gen11'): (1.1746e-09, 1.4069e-10),
    (3, 125, 'supplied'): (1.4482e-09, 1.4319e-10),
}


@functools.lru_cache(maxsize=None)
def case(b, f, source):
  """(magnitudes, supplied noise, fp64 reference on the noise the source filters) of a shape: made once, never written."""
  n = 64 * f
  rng = np.random.default_rng(7000 + 131 * b + f)
  mags = rng.standard_normal((b, f, 65)).astype(np.float32)
  supplied = rng.uniform(-1, 1, (b, n)).astype(np.float32)
  x = supplied if source == 'supplied' else np.concatenate([G.device_noise(n, r, source) for r in range(b)])
  ref = O.filtered_noise(mags, x, 0, dtype=np.float64)
  for a in (mags, supplied, ref):
    a.setflags(write=False)
  return mags, supplied, ref


def errors(ddsp, b, f, source):
  """-> (kernel output, max |err|, RMS err) of a shape against the fp64 oracle."""
  mags, supplied, ref = case(b, f, source)
  out, _ = G.run(ddsp, mags, 64 * f, source, supplied)
  d = out.astype(np.float64) - ref
  return out, float(np.abs(d).max()), float(np.sqrt(np.mean(d * d)))


def check_shape(ddsp, b, f, source):
  mags, supplied, ref = case(b, f, source)
  out, err, rms = errors(ddsp, b, f, source)
  print('%s B=%d F=%d: max|err| %.3e rms %.3e (tol %.3e)' % (source, b, f, err, rms, G.noise_tol(ref)))
  assert np.isfinite(out).all()
  assert err <= G.noise_tol(ref)
  for r in sorted({0, b - 1}):
    alone, _ = G.run(ddsp, mags[r:r + 1], 64 * f, source, supplied[r:r + 1], batch_offset=r)
    np.testing.assert_array_equal(alone[0], out[r], err_msg='row %d' % r)


def check_impulse(ddsp, s, b=1, f=70):
  """An impulse at sample s of the LAST row of a batch of b clips of f frames (the other rows: silence in, exact silence out)."""
  n = 64 * f
  mags = np.full((b, f, 65), 30.0, np.float32)
  x = np.zeros((b, n), np.float32)
  x[-1, s] = 1.0
  out, _ = G.run(ddsp, mags, n, 'supplied', x)
  ref = O.filtered_noise(mags[-1:], x[-1:], 0, dtype=np.float64)
  err = np.abs(out[-1:] - ref).max()
  print('impulse at %d of %d x %d: max|err| %.3e (tol %.3e)' % (s, b, f, err, G.noise_tol(ref)))
  assert err <= G.noise_tol(ref)
  lo, hi = max(s - START, 0), min(s - START + 128, n)         # the frame's 128 taps placed at s
  outside = out.copy()
  outside[-1, lo:hi] = 0.0
  assert not outside.any(), 'non-zero outputs outside [%d, %d) of the last row at %s' % (lo, hi, np.argwhere(outside)[:8].tolist())
  assert np.abs(out[-1, lo:hi]).max() > 1.0                   # (the centre tap of an all-pass of gain 2 is there)


def check_against_oracle(ddsp, mags, source, supplied=None, tol=None):
  """-> the output; within `tol(ref)` (noise_tol) of the fp64 oracle on the noise the kernel filtered."""
  b, f, _ = mags.shape
  n = 64 * f
  x = supplied if source == 'supplied' else np.concatenate([G.device_noise(n, r, source) for r in range(b)])
  out, _ = G.run(ddsp, mags, n, source, supplied)
  ref = O.filtered_noise(mags, x, 0, dtype=np.float64)
  bound = (tol or G.noise_tol)(ref)
  err = np.abs(out - ref).max()
  print('%s: max|err| %.3e (bound %.3e, max|ref| %.3e)' % (source, err, bound, np.abs(ref).max()))
  assert np.isfinite(out).all()
  assert err <= bound
  return out


def check_largest_taps(ddsp):
  check_against_oracle(ddsp, np.full((2, 70, 65), 88.0, np.float32), 'gen23')


def check_unequal_frames(ddsp, source):
  mags = np.full((2, 70, 65), 30.0, np.float32)
  mags[:, 1::2] = -30.0
  rng = np.random.default_rng(5)
  check_against_oracle(ddsp, mags, source, rng.uniform(-1, 1, (2, 64 * 70)).astype(np.float32))


def check_noise_scale(ddsp, exponent):
  mags, supplied, _ = case(2, 70, 'supplied')
  check_against_oracle(ddsp, mags, 'supplied', np.ldexp(supplied, exponent).astype(np.float32))


def floor_tol(ref):
  return 1e-9 + 1e-5 * np.abs(ref).max()


def check_taps_at_the_floor(ddsp):
  mags = np.full((2, 70, 65), -30.0, np.float32)
  x = np.where(np.random.default_rng(9).integers(0, 2, (2, 64 * 70)) == 1, 1.0, -1.0).astype(np.float32)
  check_against_oracle(ddsp, mags, 'supplied', x, tol=floor_tol)


def cut_taps(ir, flush_subnormal_lo):
  """Exact taps as split_scaled hands them to the matrix cores (2^13 h = hi + lo in fp16), back as numbers: with the lo parts as
  they are, or with those below fp16's normal range (2^-14) taken as zero, as a matrix core that flushed its inputs would.
  -> (taps, share of the lo parts that are non-zero subnormals)."""
  t = ir * 8192.0
  hi = t.astype(np.float16).astype(np.float64)
  lo = (t - hi).astype(np.float16).astype(np.float64)
  subnormal = (np.abs(lo) < 2.0 ** -14) & (lo != 0.0)
  if flush_subnormal_lo:
    lo = np.where(subnormal, 0.0, lo)
  return (hi + lo) / 8192.0, float(subnormal.mean())


@functools.lru_cache(maxsize=None)
def subnormal_case():
  """Magnitudes of 7e-7 .. 6e-5 after exp_sigmoid - taps of up to 1.8e-5, scaled 0.14: four in five of their lo parts are
  non-zero fp16 subnormals, none is normal - and noise of +-1, which is its own hi part.
  -> (magnitudes, noise, fp64 reference, error of the exact FIR on taps cut with lo kept, the same with subnormal lo flushed)."""
  rng = np.random.default_rng(11)
  mags = rng.uniform(-1.5, 0.5, (2, 70, 65)).astype(np.float32)
  x = np.where(rng.integers(0, 2, (2, 64 * 70)) == 1, 1.0, -1.0).astype(np.float32)
  ctl = O.filtered_noise_get_controls(mags, dtype=np.float64)['magnitudes']
  ir = O.frequency_impulse_response(ctl, 0, dtype=np.float64)
  ref = O.fft_convolve(x, ir, 'same', dtype=np.float64)
  kept, share = cut_taps(ir, False)
  flushed, _ = cut_taps(ir, True)
  assert share > 0.5
  err_kept = np.abs(O.fft_convolve(x, kept, 'same', dtype=np.float64) - ref).max()
  err_flushed = np.abs(O.fft_convolve(x, flushed, 'same', dtype=np.float64) - ref).max()
  return mags, x, ref, float(err_kept), float(err_flushed)


def check_subnormal_lo_parts(ddsp):
  mags, x, ref, err_kept, err_flushed = subnormal_case()
  bound = floor_tol(ref)
  print('operands cut exactly: lo kept %.3e, subnormal lo flushed %.3e; bound %.3e' % (err_kept, err_flushed, bound))
  # the inputs tell the two apart: flushing misses the bound by a clear factor, keeping stays far inside it
  assert err_flushed >= 4 * bound and err_kept <= bound / 4
  check_against_oracle(ddsp, mags, 'supplied', x, tol=floor_tol)


@pytest.mark.parametrize('source', SOURCES)
@pytest.mark.parametrize('b,f', SHAPES)
def test_small_shapes_against_the_oracle_and_rows_alone(ddsp, b, f, source):
  check_shape(ddsp, b, f, source)


@pytest.mark.parametrize('s', IMPULSES)
def test_impulse_gives_the_taps_in_place_and_exact_zeros_elsewhere(ddsp, s):
  check_impulse(ddsp, s)


def test_largest_taps_with_23_bit_noise(ddsp):
  """Every magnitude at exp_sigmoid's maximum 2: the largest taps the kernel designs, 2^14 after scaling."""
  check_largest_taps(ddsp)


@pytest.mark.parametrize('source', SOURCES)
def test_neighbouring_frames_seven_decades_apart(ddsp, source):
  """Frames alternate between magnitudes 2 and 1e-7: the two halves of one tap fragment hold frames 2e7 apart in scale."""
  check_unequal_frames(ddsp, source)


@pytest.mark.parametrize('exponent', [-20, 20])
def test_supplied_noise_at_any_scale(ddsp, exponent):
  check_noise_scale(ddsp, exponent)


@pytest.mark.parametrize('s', CONTINUED_IMPULSES)
def test_impulse_across_the_carry_into_a_continued_tile(ddsp, s):
  check_impulse(ddsp, s, *CONTINUED_SHAPE)


def test_taps_at_the_floor(ddsp):
  """Every magnitude at exp_sigmoid's floor 1e-7, noise of +-1.  Bound: 1e-9 + 1e-5 max|ref| (max|ref| = 1.0e-7 here).  The oracle
  itself at fp32 against fp64 on these inputs: max|err| 4.4e-14; the kernel on an MI355X: 7.6e-13.  An accuracy check only: the
  filter is ONE tap of 1e-7 whose lo part (-6.2e-9 after scaling) lies below fp16's smallest subnormal and rounds to zero - the
  7.6e-13 are that lo part - so this case says nothing about subnormal operands; the next test does."""
  check_taps_at_the_floor(ddsp)


def test_subnormal_lo_parts_reach_the_product(ddsp):
  """Taps of up to 1.8e-5: 81 % of their lo parts are non-zero fp16 subnormals (none is normal).  Bound, as at the floor:
  1e-9 + 1e-5 max|ref| = 1.52e-9 (max|ref| 5.2e-5).  The exact FIR on operands cut as the kernel cuts them is 1.05e-10 off the fp64
  oracle with the lo parts kept and 1.42e-8 with the subnormal ones flushed - 9 x the bound - and the fp32 oracle 2.5e-11: the test
  passes only where the matrix cores take subnormal fp16 inputs as they are.  The kernel on an MI355X: 1.07e-10."""
  check_subnormal_lo_parts(ddsp)


@pytest.mark.parametrize('source', SOURCES)
@pytest.mark.parametrize('b,f', SHAPES)
def test_no_less_accurate_than_three_accumulators(ddsp, b, f, source):
  """Same 22 bits per operand, the same number of fp32 roundings per output to within the five shifted partial sums: the maximum
  over these few thousand samples may move by tens of percent with the order of the sum, the RMS may not."""
  parent_max, parent_rms = PARENT_ERRORS[(b, f, source)]
  _, err, rms = errors(ddsp, b, f, source)
  print('%s B=%d F=%d: max %.3e (parent %.3e) rms %.3e (parent %.3e)' % (source, b, f, err, parent_max, rms, parent_rms))
  assert err <= 1.5 * parent_max
  assert rms <= 1.1 * parent_rms
