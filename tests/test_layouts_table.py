"""tests/layout_table.py against ddsp_amd._lib.SIGNATURES: every C entry is reached by some row of the table (forward and
backward of the row on plain tensors, run through the SIMT emulation with the library's entry points counted) or is named in
layout_table.EXEMPT with a reason - so that a kernel added later cannot stay out of tests/test_gpu_layouts.py silently.  A host
test: it needs no GPU."""
import os

import pytest

import layout_table as L
import test_gpu_layouts as G
from ddsp_amd import _lib
from tests.hip_emu import emu_simt


class _Counting:
  """The library with every entry point looked up through it noted down."""

  def __init__(self, lib):
    self._lib, self.reached = lib, set()

  def __getattr__(self, name):
    self.reached.add(name)
    return getattr(self._lib, name)


@pytest.fixture(scope='module')
def reached():
  import ddsp_amd
  os.environ.setdefault('DDSP_EMU_CUS', '4')
  if not os.path.exists(emu_simt.CLANG):
    pytest.skip('the SIMT emulation builds with the ROCm clang++ (%s), which this machine does not have' % emu_simt.CLANG)
  by_row = {}
  with emu_simt.emulated(G) as lib:
    for row in L.ROWS:
      counting = _Counting(lib)
      _lib.load = lambda: counting                      # (emulated() puts the real one back on the way out)
      G._run(ddsp_amd, row, G._base_values(row), [i for i, a in enumerate(row.args) if a.grad])
      by_row[row.name] = counting.reached
  return by_row


def test_every_c_entry_is_reached_by_a_row_or_exempt_with_a_reason(reached):
  by_any = set().union(*reached.values())
  missing = sorted(set(_lib.SIGNATURES) - by_any - set(L.EXEMPT))
  assert not missing, 'C entries no row of tests/layout_table.py reaches and EXEMPT does not name: %s' % missing


def test_the_exemptions_are_real(reached):
  by_any = set().union(*reached.values())
  assert set(L.EXEMPT) <= set(_lib.SIGNATURES), sorted(set(L.EXEMPT) - set(_lib.SIGNATURES))
  assert all(isinstance(reason, str) and len(reason) > 10 for reason in L.EXEMPT.values())
  stale = sorted(set(L.EXEMPT) & by_any)
  assert not stale, 'exempt, yet reached by a row: %s' % stale


def test_every_row_reaches_the_library(reached):
  idle = sorted(name for name, entries in reached.items() if not entries and name not in L.FRAMEWORK_ONLY)
  assert not idle, 'rows that never call the kernel library: %s' % idle
