"""The run plan of noise_mfma65_kernel (ddsp_amd/csrc/noise_mfma_plan.h) on the CPU: the header is plain host C++, compiled here
behind a three-function C shim.  Every output frame of every row must fall in exactly one tile, a run must stay inside its row,
every block's tiles must be what the kernel's own arithmetic gives it, and the headline shape (batch 128, 1000 frames of 64
samples, 512 blocks) must come to 8 tiles per block - it was 9 when every tile recomputed its history."""
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, 'ddsp_amd', 'csrc')

SHIM = r'''
#include "noise_mfma_plan.h"
using namespace ddsp;
extern "C" void plan(int B, int F, int fs, int start, int slots, long* out) {
  const MfRunPlan p = plan_noise_mfma_runs(B, F, fs, start, slots);
  out[0] = p.frames; out[1] = p.run_len; out[2] = p.run_frames; out[3] = p.runs_per_row; out[4] = p.n_runs; out[5] = p.n_whole;
  out[6] = p.grid; out[7] = p.ticks; out[8] = p.cost;
}
extern "C" void run_of(int B, int F, int fs, int start, int slots, int run, int* b, int* r) {
  const MfRunPlan p = plan_noise_mfma_runs(B, F, fs, start, slots);
  mf_plan_run(p, run, b, r);
}
extern "C" void tile_of(int B, int F, int fs, int start, int slots, int r, int j, int* out) {
  const MfRunPlan p = plan_noise_mfma_runs(B, F, fs, start, slots);
  const MfPlanTile t = mf_plan_tile(p, r, j);
  out[0] = t.staged; out[1] = t.first_out; out[2] = t.cont;
}
'''
FIELDS = ('frames', 'run_len', 'run_frames', 'runs_per_row', 'n_runs', 'n_whole', 'grid', 'ticks', 'cost')


@functools.lru_cache(maxsize=None)
def shim():
  cxx = next((c for c in ('/opt/rocm/lib/llvm/bin/clang++', shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'))
              if c and os.path.exists(c)), None)
  if cxx is None:
    pytest.skip('no C++ compiler on this machine')
  tmp = tempfile.mkdtemp(prefix='ddsp_plan_')
  src, out = os.path.join(tmp, 'shim.cpp'), os.path.join(tmp, 'libplan.so')
  with open(src, 'w') as f:
    f.write(SHIM)
  subprocess.run([cxx, '-std=c++17', '-O1', '-shared', '-fPIC', '-I' + HEADER_DIR, src, '-o', out], check=True)
  return ctypes.CDLL(out)


def plan(b, f, fs, start, slots):
  out = (ctypes.c_long * len(FIELDS))()
  shim().plan(b, f, fs, start, slots, out)
  return dict(zip(FIELDS, out))


def tiles_of_block(b, f, fs, start, slots, p, block):
  """(row, staged frame, first output frame, end of output, continues) of every tile of a block, in the kernel's order."""
  lib = shim()
  tiles = []
  for run in range(block, p['n_runs'], p['grid']):
    row, r = ctypes.c_int(), ctypes.c_int()
    lib.run_of(b, f, fs, start, slots, run, ctypes.byref(row), ctypes.byref(r))
    for j in range(p['run_len']):
      t = (ctypes.c_int * 3)()
      lib.tile_of(b, f, fs, start, slots, r.value, j, t)
      tiles.append((row.value, t[0], t[1], t[0] + 32, bool(t[2])))
  return tiles


SHAPES = [(128, 1000, 64, 62, 512), (32, 1000, 64, 62, 512), (1, 1000, 64, 62, 512), (20, 1000, 64, 62, 512),
          (6, 1000, 192, 62, 512), (3, 140, 64, 62, 8), (300, 90, 64, 62, 512), (1024, 1000, 64, 62, 512), (2, 1, 64, 62, 512),
          (7, 333, 128, 62, 16), (5, 40, 4096, 62, 8), (1, 1, 64, 62, 1)]


@pytest.mark.parametrize('b,f,fs,start,slots', SHAPES)
def test_every_frame_in_exactly_one_tile_and_runs_stay_in_their_rows(b, f, fs, start, slots):
  p = plan(b, f, fs, start, slots)
  assert p['frames'] == -(-(f * fs + start) // 64) and p['run_frames'] == 32 * p['run_len'] - 2
  assert p['grid'] == min(p['n_runs'], slots) and p['n_runs'] == b * p['runs_per_row']
  covered = [[0] * p['frames'] for _ in range(b)]
  most = 0
  for block in range(p['grid']):
    tiles = tiles_of_block(b, f, fs, start, slots, p, block)
    most = max(most, len(tiles))
    for k, (row, staged, first, end, cont) in enumerate(tiles):
      assert 0 <= row < b
      if cont:
        # the carry comes from the block's previous tile: same row, ending where this one starts
        assert k > 0 and tiles[k - 1][0] == row and tiles[k - 1][3] == staged == first
      else:
        assert first == staged + 2 and first % p['run_frames'] == 0
      for frame in range(first, min(end, p['frames'])):
        covered[row][frame] += 1
  assert all(c == 1 for row in covered for c in row)
  assert most == p['ticks']


def test_headline_shape_runs_eight_tiles_per_block():
  p = plan(128, 1000, 64, 62, 512)
  assert p['grid'] == 512 and p['ticks'] == 8 and p['run_len'] > 1
  assert all(len(tiles_of_block(128, 1000, 64, 62, 512, p, blk)) == 8 for blk in (0, 127, 128, 255, 256, 511))
  # every tile cut alone, as before: 34 per row, 4352 over 512 blocks - 9 for a quarter of them
  assert -(-(128 * -(-p['frames'] // 30)) // 512) == 9


def test_tiles_that_fit_the_chip_stay_one_per_block():
  for b, f in ((1, 1000), (8, 1000), (15, 1000), (3, 40), (2, 1)):
    p = plan(b, f, 64, 62, 512)
    assert p['run_len'] == 1 and p['ticks'] == 1 and p['grid'] == p['n_runs'] == b * -(-p['frames'] // 30)


def test_the_shapes_of_the_run_tests_do_run_runs():
  """tests/test_gpu_noise_runs.py (256 CUs) and tests/test_noise_runs_emulated.py (4 CUs): batches in runs, rows alone in single tiles."""
  import test_gpu_noise_runs as G
  import test_noise_runs_emulated as E
  for shapes, slots in ((G.SHAPES, 512), (E.SHAPES, 8)):
    for b, f, n in shapes:
      fs = -(-n // f)
      assert plan(b, f, fs, 62, slots)['run_len'] > 1, (b, f, n)
      assert plan(1, f, fs, 62, slots)['run_len'] == 1, (b, f, n)
