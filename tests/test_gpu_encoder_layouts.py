"""The normalisations, the differentiable resampler and the z encoder on offset, strided and non-fp32 tensors: the one property of
tests/test_gpu_layouts.py - a call on tensors of any layout or dtype returns the bits of the same call on freshly allocated
contiguous fp32 copies of the same values, outputs and input gradients - for the public entries that reach csrc/group_norm.hip
and for core.resample with a gradient: normalize_op (one block per batch row, and split over blocks), Normalize, core.resample,
MfccTimeDistributedRnnEncoder.  The helpers are that module's; the rows are here because the C entries behind them sit in
ddsp_amd._lib.NORM_SIGNATURES, outside the table tests/layout_table.py is held to - so this file carries its own coverage check:
every name of NORM_SIGNATURES is reached by a row or EXEMPT with a reason.

A layer's weights are drawn by its initialisers under a fixed seed at every call, so the variant and its reference hold the same
weights.  tests/test_encoder_layouts_emulated.py runs this module through the SIMT emulation on the CPU."""
import pytest
import torch

import layout_table as L
import test_gpu_layouts as GL
from ddsp_amd import _lib
from ddsp_amd.training import encoders, nn

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B, T, W = 2, 5, 6


def _seeded(make):
  torch.manual_seed(20261019)
  return make()


def _encoder(d, audio, f0_scaled):
  enc = _seeded(lambda: encoders.MfccTimeDistributedRnnEncoder(rnn_channels=16, z_dims=4, z_time_steps=1000))
  return enc(dict(audio=audio, f0_scaled=f0_scaled))


ROWS = [
    L.Row('normalize_op', lambda d, x: nn.normalize_op(x, 'instance'), [L.N('x', B, T, 2, W, expand=0)]),
    L.Row('normalize_op_split', lambda d, x: nn.normalize_op(x, 'layer'), [L.N('x', B, 70, 1, 256, expand=0)]),
    L.Row('Normalize', lambda d, x: _seeded(lambda: nn.Normalize('layer'))(x), [L.N('x', B, T, W, expand=0)]),
    L.Row('resample', lambda d, x: d.core.resample(x, 12, method='cubic'), [L.N('x', B, T, W, expand=0)]),
    L.Row('upsample_with_windows', lambda d, x: d.core.upsample_with_windows(x, 20), [L.N('x', B, T, W, expand=0)]),
    L.Row('MfccTimeDistributedRnnEncoder', _encoder, [L.N('audio', B, 512, scale=0.3, grad=False, expand=0),
                                                      L.N('f0_scaled', B, 10, 1, grad=False, expand=0)]),
]
BY_NAME = {row.name: row for row in ROWS}
EXEMPT = {}        # C entry -> why no row reaches it


def _variant_cases():
  return [pytest.param(row.name, variant, id='%s-%s' % (row.name, variant)) for row in ROWS for variant in GL.VARIANTS
          if any(GL._applies(variant, a, row) for a in row.args)]


@pytest.mark.parametrize('name, variant', _variant_cases())
def test_layout_gives_the_bits_of_fresh_contiguous_fp32(ddsp, name, variant):
  row = BY_NAME[name]
  on = [i for i, a in enumerate(row.args) if GL._applies(variant, a, row)]
  for i in on:                                                   # each argument alone
    GL._check_case(ddsp, row, variant, [i])
  if len(on) > 1:                                                # all at once
    GL._check_case(ddsp, row, variant, on)


class _Counting:
  """The library with every entry point looked up through it noted down."""

  def __init__(self, lib):
    self._lib, self.reached = lib, set()

  def __getattr__(self, name):
    self.reached.add(name)
    return getattr(self._lib, name)


def test_every_norm_entry_is_reached_by_a_row_or_exempt_with_a_reason(ddsp):
  load = _lib.load
  counting = _Counting(load())
  try:
    _lib.load = lambda: counting
    for row in ROWS:
      GL._run(ddsp, row, GL._base_values(row), [i for i, a in enumerate(row.args) if a.grad])
  finally:
    _lib.load = load
  missing = sorted(set(_lib.NORM_SIGNATURES) - counting.reached - set(EXEMPT))
  assert not missing, 'norm entries no row reaches and EXEMPT does not name: %s' % missing
  assert set(EXEMPT) <= set(_lib.NORM_SIGNATURES) and not set(EXEMPT) & counting.reached
  assert all(isinstance(reason, str) and len(reason) > 10 for reason in EXEMPT.values())
  assert 'ddsp_resample_ex_backward_f32' in counting.reached            # core.resample's gradient runs its adjoint kernel


@pytest.fixture(scope='module')
def ddsp():
  import ddsp_amd
  assert GL.DEV == DEV, 'the helpers of tests/test_gpu_layouts.py must run on the device this module runs on'
  return ddsp_amd
