"""tests/nonfinite_table.py held to the kernels, and the float-to-integer helper of csrc/common.h held to gfx950's instruction.
Host tests: the rows run through the SIMT emulation, as tests/test_layouts_table.py runs them.

  * an excused row must in fact break the rule it is excused from (an excuse that has become unnecessary fails here);
  * an R2 excuse may only be a row of the Reverb family (batch rows transformed in pairs); outputs that reduce over the batch
    need none (Row.scalar) and may not be listed either;
  * every key names a row and an argument that exist, every reason is a sentence;
  * wt_floor_int / cvt_i32_saturating on the host give what v_cvt_flr_i32_f32 / v_cvt_i32_f32 give (the ISA manual's rule for the
    float-to-integer conversions: NaN -> 0, out of range and the infinities saturate) - the emulation can only carry a non-finite
    value to the same address as the device if it converts it the same way."""
import ctypes
import functools
import os
import subprocess
import tempfile

import pytest

import nonfinite_table as NF
import test_gpu_layouts as GL
import test_gpu_nonfinite as G
from tests.hip_emu import emu_simt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
REVERB_FAMILY = ('Reverb/', 'ExpDecayReverb', 'FilteredNoiseReverb', 'ProcessorGroup')     # (the group ends in a Reverb)

SHIM = r'''
#include "common.h"
extern "C" int floor_int(float x) { return ddsp::wt_floor_int(x); }
extern "C" int to_int(float x) { return ddsp::cvt_i32_saturating(x); }
'''


@functools.lru_cache(maxsize=None)
def shim():
  if not os.path.exists(emu_simt.CLANG):
    pytest.skip('the kernels\' headers build for the host with the ROCm clang++ (%s), which this machine does not have' % emu_simt.CLANG)
  tmp = tempfile.mkdtemp(prefix='ddsp_cvt_')
  src, out = os.path.join(tmp, 'shim.cpp'), os.path.join(tmp, 'libcvt.so')
  with open(src, 'w') as f:
    f.write(SHIM)
  include = os.path.join(ROOT, 'tests', 'hip_emu', 'include_simt')
  subprocess.run([emu_simt.CLANG, '-std=c++17', '-O1', '-shared', '-fPIC', '-w', '-I' + include, '-I' + os.path.join(ROOT, 'include'),
                  '-I' + os.path.join(ROOT, 'ddsp_amd', 'csrc'), '-include', os.path.join(include, 'hip', 'hip_runtime.h'), src, '-o', out],
                 check=True)
  lib = ctypes.CDLL(out)
  for fn in (lib.floor_int, lib.to_int):
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_float]
  return lib


@pytest.mark.parametrize('x, floor, trunc', [
    (float('nan'), 0, 0), (float('inf'), INT_MAX, INT_MAX), (float('-inf'), INT_MIN, INT_MIN), (3e9, INT_MAX, INT_MAX),
    (-3e9, INT_MIN, INT_MIN), (-0.5, -1, 0), (0.5, 0, 0), (-1.0, -1, -1), (255.75, 255, 255), (2147483520.0, 2147483520, 2147483520)])
def test_host_float_to_int_is_the_device_instruction(x, floor, trunc):
  assert shim().floor_int(x) == floor
  assert shim().to_int(x) == trunc


# ---- the two lists ---------------------------------------------------------------------------------------------------------
def test_the_lists_name_rows_and_arguments_that_exist():
  for name, reason in NF.EXEMPT_ROWS.items():
    assert name in NF.BY_NAME, name
    assert isinstance(reason, str) and len(reason) > 20, name
  for (name, arg), reason in NF.KEEPS_FINITE.items():
    assert name in NF.BY_NAME and arg in [a.name for a in NF.BY_NAME[name].args], (name, arg)
    assert isinstance(reason, str) and len(reason) > 20, (name, arg)
  for (name, arg) in NF.PLANT:
    assert name in NF.BY_NAME and arg in [a.name for a in NF.BY_NAME[name].args], (name, arg)


def test_only_the_reverb_family_is_excused_from_the_row_rule():
  for name in NF.EXEMPT_ROWS:
    assert name.startswith(REVERB_FAMILY), name + ': only rows whose kernel transforms batch rows in pairs may be excused from R2'
    assert not NF.BY_NAME[name].scalar, name + ': an output that reduces over the batch has no row 0 to hold and needs no excuse'


@pytest.fixture(scope='module')
def ddsp():
  import ddsp_amd
  os.environ.setdefault('DDSP_EMU_CUS', '4')
  if not os.path.exists(emu_simt.CLANG):
    pytest.skip('the SIMT emulation builds with the ROCm clang++ (%s), which this machine does not have' % emu_simt.CLANG)
  with emu_simt.emulated(G, GL):
    yield ddsp_amd


@pytest.mark.parametrize('name', sorted(NF.EXEMPT_ROWS))
def test_an_excused_row_does_break_the_row_rule(ddsp, name):
  row = NF.BY_NAME[name]
  broken = []
  for ai, arg in enumerate(row.args):
    result = G.run_poisoned(ddsp, row, ai, float('nan'))
    if result is not None:
      broken += G.row0_differences(row, ai, *result)
  assert broken, name + ': excused from R2, yet batch row 0 keeps its bits for a NaN in every argument - drop the excuse'
