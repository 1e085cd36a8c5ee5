"""TEST INFRASTRUCTURE ONLY: builds the gfx950 kernel sources of ddsp_amd/csrc for the HOST with the ROCm clang++
against the SIMT stand-in <hip/hip_runtime.h> of tests/hip_emu/include_simt (threads of a block as fibers,
wavefront operations evaluated when all live lanes have arrived, MFMA / DPP / swizzle modelled) and loads the
result with the argument types of ddsp_amd/_lib.py.  The sources are compiled as they are, with two textual
substitutions the host language needs:
  * `extern __shared__ <attrs> T name[];`   ->  a pointer to the emulated block's dynamic LDS;
  * the four `asm volatile(...)` statements of harmonic.hip (pairs of scalar row loads with their wait, one
    `s_waitcnt vmcnt(0)`) -> the same loads / a wavefront join in C++.
Nothing in ddsp_amd/ ever loads this; it exists so that kernel logic can be checked on the CPU when no GPU
(or no GPU budget) is at hand.

There is ONE emulated library, made of the very list of sources the product build compiles, and one harness that points the
Python layer of ddsp_amd at it: emulated() is the context manager, ddsp_fixture() wraps it as the `ddsp` fixture of the
tests/test_*_emulated.py modules, and reexport() hands such a module the test functions of the GPU modules it re-runs."""
import contextlib
import ctypes
import hashlib
import os
import re
import subprocess

import torch

from ddsp_amd import _lib, core
from ddsp_amd.build import SOURCES            # the product's own list: the two builds cannot disagree about what the library is

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, 'ddsp_amd', 'csrc')
BUILD = os.path.join(HERE, '_build', 'simt')
OUT = os.path.join(BUILD, 'libddsp_simt_emu.so')
CLANG = '/opt/rocm/lib/llvm/bin/clang++'

_DYN_LDS = re.compile(r'extern\s+__shared__\s+(?:__attribute__\(\(aligned\(\d+\)\)\)\s+)?([A-Za-z_][\w:]*)\s+(\w+)\[\];')

_emu = None


# the scalar loads of the direct-sum kernel: two rows of N dwords into SGPR vectors, then their wait
_SLOAD = re.compile(
    r'asm volatile\("s_load_dwordx(\d+) %0, %2, (?:0x0|%4)\\n\\ts_load_dwordx\d+ %1, %3, (?:0x0|%4)\\n\\ts_waitcnt lgkmcnt\(0\)"'
    r'\s*:\s*"=&s"\((\w+)\),\s*"=&s"\((\w+)\)\s*:\s*"s"\((\w+)\),\s*"s"\((\w+)\)(?:,\s*"i"\((\w+)\))?\s*:\s*"memory"\);')
_WAITCNT = re.compile(r'asm volatile\("s_waitcnt vmcnt\(0\)"\s*:::\s*"memory"\);')


def _preprocess(text):
  text = text.replace('"../../include/ddsp_amd.h"', '<ddsp_amd.h>')      # the staged copies live elsewhere
  text = _SLOAD.sub(lambda m: 'ddsp_emu_sload<%s>(%s, %s, %s, %s, %s);' % (
      m.group(1), m.group(2), m.group(3), m.group(4), m.group(5), m.group(6) or '0'), text)
  text = _WAITCNT.sub('ddsp_emu_wave_sync();', text)
  if 'asm volatile' in text:
    raise RuntimeError('inline assembly the emulation does not know')
  return _DYN_LDS.sub(r'DDSP_EMU_DYNAMIC_LDS(\1, \2);', text)


def _digest():
  h = hashlib.sha256(' '.join(SOURCES).encode())
  paths = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC))]
  paths += [os.path.join(HERE, 'include_simt', 'hip', 'hip_runtime.h'), os.path.join(ROOT, 'include', 'ddsp_amd.h'),
            os.path.abspath(__file__)]
  for path in paths:
    with open(path, 'rb') as f:
      h.update(f.read())
  return h.hexdigest()


def build(verbose=False):
  """Builds under an exclusive lock on the build directory: pytest-xdist workers that find the library stale at the same
  moment used to stage and compile into the same files at once (one of them then failed to load a half-written object)."""
  import fcntl
  os.makedirs(BUILD, exist_ok=True)
  with open(os.path.join(BUILD, '.lock'), 'w') as lock:
    fcntl.flock(lock, fcntl.LOCK_EX)
    return _build_locked(verbose)


def _build_locked(verbose):
  stamp = OUT + '.stamp'
  digest = _digest()
  if os.path.exists(OUT) and os.path.exists(stamp) and open(stamp).read().strip() == digest:
    return OUT
  staged = []
  for name in os.listdir(CSRC):                       # headers travel with the sources
    with open(os.path.join(CSRC, name)) as f:
      text = f.read()
    dst = os.path.join(BUILD, name.replace('.hip', '.cpp'))
    with open(dst, 'w') as f:
      f.write(_preprocess(text))
    if name in SOURCES:
      staged.append(dst)
  # -ffp-contract=fast -mfma: a*b+c contracts to an FMA as in hipcc's default mode (the FFT butterflies of the
  # SpectralLoss are measurably less accurate without); fast-honor-pragmas is hipcc's own default, so the rn_* helpers of common.h stay uncontracted here exactly as on the device
  cmd = [CLANG, '-std=c++17', '-O1', '-g0', '-ffp-contract=fast-honor-pragmas', '-mfma', '-shared', '-fPIC', '-w',
         '-I' + os.path.join(HERE, 'include_simt'), '-I' + os.path.join(ROOT, 'include'),
         '-include', os.path.join(HERE, 'include_simt', 'hip', 'hip_runtime.h')] + staged + ['-o', OUT]
  if verbose:
    print(' '.join(cmd))
  subprocess.run(cmd, check=True)
  with open(stamp, 'w') as f:
    f.write(digest + '\n')
  return OUT


def load():
  global _emu
  if _emu is None:
    lib = ctypes.CDLL(build())
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
      fn = getattr(lib, name)                             # every entry point of the header, as in _lib.load()
      fn.restype, fn.argtypes = restype, argtypes
    _emu = lib
  return _emu


@contextlib.contextmanager
def emulated(*gpu_modules):
  """Points ddsp_amd at the emulated library and at host memory, and the given GPU test modules at DEV = 'cpu'; puts
  everything back on the way out, also when the body raises.  The two caches of core hold what the DEVICE library answered
  (workspace sizes) or made (FIR designs, tensors on the device), so they are set aside and start empty here."""
  lib = load()
  saved = (_lib.load, core._device, core._stream, dict(core._ws_bytes_cache), dict(core._design_cache),
           [module.DEV for module in gpu_modules])
  try:
    _lib.load = lambda: lib
    core._device = lambda: torch.device('cpu')
    core._stream = lambda: None
    core._ws_bytes_cache.clear()
    core._design_cache.clear()
    for module in gpu_modules:
      module.DEV = 'cpu'
    yield lib
  finally:
    _lib.load, core._device, core._stream = saved[:3]
    for cache, was in ((core._ws_bytes_cache, saved[3]), (core._design_cache, saved[4])):
      cache.clear()
      cache.update(was)
    for module, dev in zip(gpu_modules, saved[5]):
      module.DEV = dev


def ddsp_fixture(*gpu_modules):
  """The module-scoped `ddsp` fixture of an emulated test module: ddsp_amd under emulated(*gpu_modules)."""
  import pytest

  @pytest.fixture(scope='module')
  def ddsp():
    import ddsp_amd
    os.environ.setdefault('DDSP_EMU_CUS', '4')        # the emulated chip's CU count (persistent kernels size their grid by it)
    if not os.path.exists(CLANG):
      pytest.skip('the SIMT emulation builds with the ROCm clang++ (%s), which this machine does not have' % CLANG)
    with emulated(*gpu_modules):
      yield ddsp_amd
  return ddsp


def reexport(namespace, *gpu_modules):
  """Every test function of the GPU modules into `namespace` (the emulated module's globals()) under its own name, so that its
  parametrisation comes along."""
  for module in gpu_modules:
    for name in dir(module):
      if name.startswith('test_') and callable(getattr(module, name)):
        namespace[name] = getattr(module, name)
