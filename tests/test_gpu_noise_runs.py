"""noise_mfma65_kernel on runs of consecutive tiles (csrc/noise_mfma_plan.h): the carry that crosses from one tile of a run into
the next, and the promise that comes with it - what a sample is does not depend on how its row was cut.

A batch whose tiles outnumber the blocks the chip holds (2 per CU) is cut into runs longer than one tile; a row filtered ALONE
(batch 1, a few dozen tiles) is cut into single tiles, each recomputing its two frames of history.  Every shape below has
B * ceil(N / 2048) > 2 * 256, so the first happens on an MI355X, and the tests hold the two to bit equality: generated noise is
matched through `batch_offset`, which the Python class does not expose, hence the C ABI is called directly.

tests/test_noise_runs_emulated.py runs the same checks on the CPU at shapes cut to the emulated chip's 4 CUs."""
import functools

import numpy as np
import pytest
import torch

from oracle import ddsp_oracle as O

pytestmark = pytest.mark.gpu

DEV = 'cuda'      # the emulated module sets 'cpu'

SEED = 0x1234ABCD5
SOURCES = ['gen23', 'gen11', 'supplied']
# (batch, frames, samples): canonical frames of 64; ragged N (odd: the per-element stores); frames of 192 (several staged frames per tap row)
SHAPES = [(20, 1000, 64000), (20, 1000, 64000 - 17), (6, 1000, 192000)]


@pytest.fixture(scope='module')
def ddsp():
  if not torch.cuda.is_available():
    pytest.skip('gpu tests need a GPU (run with -m gpu on an MI355X)')
  from ddsp_amd import build
  build.build()
  import ddsp_amd
  from ddsp_amd import _lib
  _lib.load()
  return ddsp_amd


def noise_tol(ref):                      # test_gpu_parity's NOISE tolerance
  return 2e-6 + 1e-5 * np.abs(ref).max()


@functools.lru_cache(maxsize=None)
def inputs(b, f, n):
  """Magnitudes and supplied noise of a shape: made once, shared by every test of the shape, never written."""
  rng = np.random.default_rng(b * 1000003 + n)
  mags = rng.standard_normal((b, f, 65)).astype(np.float32)
  noise = rng.uniform(-1, 1, (b, n)).astype(np.float32)
  mags.setflags(write=False)
  noise.setflags(write=False)
  return mags, noise


def run(ddsp, mags, n, source, noise=None, batch_offset=0, seed=SEED):
  """ddsp_filtered_noise_f32 (window_size 0: the canonical 128 taps, exp_sigmoid fused) -> audio [B, n], controls [B, F, 65]."""
  from ddsp_amd import _lib, core
  lib = _lib.load()
  b, f, m = mags.shape
  # (copies, for this RAW C call only: ddsp_filtered_noise_f32 picks its kernel by the 16-byte alignment of the supplied noise, and
  # a row sliced out of a batch with an odd N is off it.  synths.FilteredNoise stages such a view itself - core.aligned16,
  # tests/test_gpu_layouts.py)
  tm = torch.as_tensor(np.array(mags), device=DEV)
  tn = torch.as_tensor(np.array(noise), device=DEV) if source == 'supplied' else None
  audio = torch.empty((b, n), dtype=torch.float32, device=DEV)
  ctl = torch.empty_like(tm)
  ws_bytes = lib.ddsp_filtered_noise_workspace_bytes(b, f, m, n, 0)
  ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=DEV)
  flags = _lib.NOISE_SCALE_EXP_SIGMOID | (_lib.NOISE_BITS_23 if source == 'gen23' else 0)
  rc = lib.ddsp_filtered_noise_f32(tm.data_ptr(), tn.data_ptr() if tn is not None else None, audio.data_ptr(), ctl.data_ptr(),
                                   ws.data_ptr(), ws.numel(), b, f, m, n, 0, -5.0, flags, seed, batch_offset, core._stream())
  _lib.check(rc, 'ddsp_filtered_noise_f32')
  if DEV == 'cuda':
    torch.cuda.synchronize()
  return audio.cpu().numpy(), ctl.cpu().numpy()


def device_noise(n, row, source):
  """Row `row` of the noise the kernel generates (the oracle takes the 64-bit seed as the C entry does: the Philox key)."""
  return O.device_uniform_noise(1, n, SEED, row, noise_bits=23 if source == 'gen23' else 11)


def check_runs(ddsp, b, f, n, source):
  mags, supplied = inputs(b, f, n)
  batch, ctl = run(ddsp, mags, n, source, supplied)
  assert np.isfinite(batch).all()
  # a row alone (one tile per run, history recomputed) == the row in the batch (runs of several tiles), bit for bit
  rows = sorted({0, b // 2, b - 1})
  for r in rows:
    alone, ctl_alone = run(ddsp, mags[r:r + 1], n, source, supplied[r:r + 1], batch_offset=r)
    np.testing.assert_array_equal(alone[0], batch[r], err_msg='row %d' % r)
    np.testing.assert_array_equal(ctl_alone[0], ctl[r], err_msg='controls of row %d' % r)
  # two rows against the fp64 oracle
  for r in (rows[0], rows[-1]):
    x = supplied[r:r + 1] if source == 'supplied' else device_noise(n, r, source)
    ref = O.filtered_noise(mags[r:r + 1], x, 0, dtype=np.float64)
    err = np.abs(batch[r:r + 1] - ref).max()
    print('%s B=%d N=%d row %d: max|err| %.3e (tol %.3e)' % (source, b, n, r, err, noise_tol(ref)))
    assert err <= noise_tol(ref)
  # the controls: every frame written, once (test_filtered_noise_fused_tile_edges' bound)
  np.testing.assert_allclose(ctl, O.filtered_noise_get_controls(mags)['magnitudes'], rtol=2e-5, atol=1e-9)
  # the same call again (the counter rewound: same seed): the same bits
  again, ctl_again = run(ddsp, mags, n, source, supplied)
  np.testing.assert_array_equal(again, batch)
  np.testing.assert_array_equal(ctl_again, ctl)
  return batch


def check_gen11_equals_supplied11(ddsp, b, f, n):
  """2048-level noise is ONE fp16 plane whether it is generated or supplied: the two instances must agree bit for bit."""
  mags, _ = inputs(b, f, n)
  gen, _ = run(ddsp, mags, n, 'gen11')
  same = np.concatenate([device_noise(n, r, 'gen11') for r in range(b)])
  inj, _ = run(ddsp, mags, n, 'supplied', same)
  np.testing.assert_array_equal(gen, inj)


@pytest.mark.parametrize('source', SOURCES)
@pytest.mark.parametrize('b,f,n', SHAPES)
def test_rows_in_runs_equal_rows_alone_and_the_oracle(ddsp, b, f, n, source):
  check_runs(ddsp, b, f, n, source)


def test_generated_2048_level_noise_equals_the_same_noise_supplied_in_runs(ddsp):
  check_gen11_equals_supplied11(ddsp, *SHAPES[0])
