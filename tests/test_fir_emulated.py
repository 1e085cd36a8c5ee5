"""tests/test_gpu_fir.py on the CPU, through the SIMT emulation of tests/hip_emu (TEST INFRASTRUCTURE, see
tests/test_simt_emulated.py): kernel logic - the tiles and halos of the two correlations, the frame arithmetic, the crop, the
sinc design and its backward sums, the adjoint of the frequency-sampling design - checked without GPU time.  It does not
replace the `-m gpu` run.

Built the way tests/test_wasserstein_emulated.py builds its library: emu_simt's own list of sources plus fir_grad.hip, with
emu_simt's preprocessing and flags, under its own output path."""
import ctypes
import fcntl
import hashlib
import os
import subprocess

import pytest
import torch

import test_gpu_fir as G
from ddsp_amd import _lib, core
from tests.hip_emu import emu_simt

SOURCES = emu_simt.SOURCES + ['fir_grad.hip']
BUILD = os.path.join(emu_simt.HERE, '_build', 'simt_fir')
OUT = os.path.join(BUILD, 'libddsp_simt_fir_emu.so')


def _build():
  os.makedirs(BUILD, exist_ok=True)
  with open(os.path.join(BUILD, '.lock'), 'w') as lock:
    fcntl.flock(lock, fcntl.LOCK_EX)
    digest = hashlib.sha256((emu_simt._digest() + ' '.join(SOURCES)).encode()).hexdigest()
    stamp = OUT + '.stamp'
    if os.path.exists(OUT) and os.path.exists(stamp) and open(stamp).read().strip() == digest:
      return OUT
    staged = []
    for name in os.listdir(emu_simt.CSRC):
      with open(os.path.join(emu_simt.CSRC, name)) as f:
        text = f.read()
      dst = os.path.join(BUILD, name.replace('.hip', '.cpp'))
      with open(dst, 'w') as f:
        f.write(emu_simt._preprocess(text))
      if name in SOURCES:
        staged.append(dst)
    include = os.path.join(emu_simt.HERE, 'include_simt')
    cmd = [emu_simt.CLANG, '-std=c++17', '-O1', '-g0', '-ffp-contract=fast-honor-pragmas', '-mfma', '-shared', '-fPIC', '-w',
           '-I' + include, '-I' + os.path.join(emu_simt.ROOT, 'include'),
           '-include', os.path.join(include, 'hip', 'hip_runtime.h')] + staged + ['-o', OUT]
    subprocess.run(cmd, check=True)
    with open(stamp, 'w') as f:
      f.write(digest + '\n')
    return OUT


@pytest.fixture(scope='module')
def ddsp():
  import ddsp_amd
  os.environ.setdefault('DDSP_EMU_CUS', '4')
  if not os.path.exists(emu_simt.CLANG):
    pytest.skip('the SIMT emulation builds with the ROCm clang++ (%s), which this machine does not have' % emu_simt.CLANG)
  lib = ctypes.CDLL(_build())
  for name, (restype, argtypes) in _lib.SIGNATURES.items():
    if not hasattr(lib, name):
      continue
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = restype, argtypes
  saved = (_lib.load, core._device, core._stream, dict(core._ws_bytes_cache), G.DEV, dict(core._design_cache))
  _lib.load = lambda: lib
  core._device = lambda: torch.device('cpu')
  core._stream = lambda: None
  core._ws_bytes_cache.clear()
  core._design_cache.clear()
  G.DEV = 'cpu'
  yield ddsp_amd
  _lib.load, core._device, core._stream = saved[0], saved[1], saved[2]
  core._ws_bytes_cache.clear()
  core._ws_bytes_cache.update(saved[3])
  core._design_cache.clear()
  core._design_cache.update(saved[5])
  G.DEV = saved[4]


for _name in dir(G):
  if _name.startswith('test_') and callable(getattr(G, _name)):
    globals()[_name] = getattr(G, _name)

# left to the GPU run: the allocator statistic of the device
SLOW_UNDER_EMULATION = ('test_peak_memory',)
