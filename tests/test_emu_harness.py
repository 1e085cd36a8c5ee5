"""The harness of tests/hip_emu/emu_simt.py (TEST INFRASTRUCTURE) leaves the process as it found it: what the `ddsp` fixture
of every tests/test_*_emulated.py module swaps - _lib.load, core._device, core._stream, the GPU module's DEV - and the two
caches of core that hold answers of the library (workspace sizes; FIR designs, which are tensors on the device) are back
exactly, whether the body returned or raised."""
import contextlib
import os

import numpy as np
import pytest
import torch

import test_gpu_fir as G
from ddsp_amd import _lib, core
from tests.hip_emu import emu_simt


def _state():
  return (_lib.load, core._device, core._stream, G.DEV, dict(core._ws_bytes_cache), dict(core._design_cache))


@pytest.mark.skipif(not os.path.exists(emu_simt.CLANG), reason='the SIMT emulation builds with the ROCm clang++')
@pytest.mark.parametrize('raises', [False, True])
def test_harness_restores_the_process(raises):
  name, b, _, n, f, l = G.SHAPES[0]
  assert name == 'in_frame'
  design = torch.zeros(1)
  core._ws_bytes_cache[('sentinel',)] = 7                  # what an earlier user of the device would have left
  core._design_cache[('sentinel',)] = design
  try:
    before = _state()
    with pytest.raises(ZeroDivisionError) if raises else contextlib.nullcontext():
      with emu_simt.emulated(G):
        assert G.DEV == 'cpu' and not core._ws_bytes_cache and not core._design_cache      # starts empty
        mags = torch.as_tensor(np.ones((b, f, (l + 1) // 2), np.float32), device=G.DEV).requires_grad_(True)
        core.frequency_impulse_response(mags, window_size=0).sum().backward()             # the backward makes a design
        core.cached_workspace_bytes('ddsp_harmonic_workspace_bytes', b, f, 4, n)
        assert len(core._design_cache) == 1 and len(core._ws_bytes_cache) == 1 and mags.grad is not None
        if raises:
          1 / 0
    after = _state()
    assert all(x is y for x, y in zip(before[:4], after[:4]))
    assert after[4] == before[4] and list(after[5]) == list(before[5]) and after[5][('sentinel',)] is design
  finally:
    del core._ws_bytes_cache[('sentinel',)], core._design_cache[('sentinel',)]

