"""SpectralLoss(deterministic=True): the gradient whose overlapping frames are added by a store pass and a per-sample sum pass
(csrc/spectral_loss_det.hip) instead of fp32 atomics.  For every slab instance and every count of covering blocks: the same
bits twice, on a fresh instance and beside another stream's work; rows that do not see each other; the value of the default
path, to the bits; the right gradient (the analytic oracle where there is one, the default path's gradient everywhere);
backward() twice doubling the gradient exactly; and the torch-wide switch.

Nothing here tries to catch the ATOMIC path differing between runs: it may well not differ on a given run."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import ddsp_oracle as O
from test_gpu_parity import ddsp, npy  # noqa: F401  (the fixture builds and loads the library)

pytestmark = pytest.mark.gpu

DEV = 'cuda'      # tests/test_spectral_loss_deterministic_emulated.py re-runs this module on host memory with DEV = 'cpu'

ALL_TERMS = dict(mag_weight=1.0, delta_time_weight=1.0, delta_freq_weight=1.0, cumsum_freq_weight=1.0, logmag_weight=1.0)
# name: (batch, samples, fft_sizes or None for the default six, keywords, mask of shape [batch, 1, 1] or None)
CASES = {
    'g_1_2_64_256_ragged': (3, 5001, (4096, 2048, 64, 16), dict(mag_weight=1.0, logmag_weight=0.5), None),
    'clip_shorter_than_a_stretch': (2, 700, (2048, 256), dict(), None),
    'three_times_a_power_of_two': (2, 3000, (3072, 192, 96), dict(), None),
    'big_kernel_beside_the_grid': (1, 20000, (8192, 6144, 1024), dict(), None),
    'split_fused_and_plain': (2, 3000, (100, 1000, 64), dict(), None),
    'general_l2_all_terms': (2, 4000, (250, 1022), dict(loss_type='L2', **ALL_TERMS), None),
    'general_cosine': (2, 3000, (384,), dict(loss_type='COSINE'), None),
    'loudness_and_all_terms': (2, 8000, None, dict(loudness_weight=0.5, **ALL_TERMS), None),
    'loudness_only': (2, 8000, None, dict(mag_weight=0.0, loudness_weight=1.0), None),
    'general_mask': (2, 3000, (512,), dict(), (1.0, 0.5)),
}
NAMES = list(CASES)
# 'L1' with the magnitude and log-magnitude terms alone: O.spectral_loss_backward is their analytic gradient
ORACLE_L1 = ('g_1_2_64_256_ragged', 'clip_shorter_than_a_stretch', 'three_times_a_power_of_two', 'big_kernel_beside_the_grid',
             'split_fused_and_plain')


def _log(case, **figures):
  path = os.environ.get('DDSP_PARITY_LOG')
  if path:
    with open(path, 'a') as f:
      f.write(json.dumps(dict(case=case, **{k: float(v) for k, v in figures.items()})) + '\n')


@functools.lru_cache(maxsize=None)
def _signals(name):
  """Target and audio of a case, made once and never written to."""
  batch, n = CASES[name][:2]
  rng = np.random.default_rng(1000 * n + batch + len(name))
  t = (0.3 * rng.standard_normal((batch, n))).astype(np.float32)
  a = (0.8 * t + 0.05 * rng.standard_normal((batch, n))).astype(np.float32)
  t.setflags(write=False)
  a.setflags(write=False)
  return t, a


def _loss(ddsp, name, deterministic):
  sizes, kw = CASES[name][2:4]
  if sizes is not None:
    kw = dict(kw, fft_sizes=sizes)
  return ddsp.losses.SpectralLoss(deterministic=deterministic, **kw)


def _call(name, loss, rows=None):
  """-> (the loss, a [batch, samples] leaf with requires_grad) of one call; `rows`: the batch in that order of rows."""
  t, a = _signals(name)
  mask = CASES[name][4]
  if rows is not None:
    t, a = t[rows], a[rows]
  weights = None
  if mask is not None:
    mask = np.asarray(mask, np.float32)
    weights = torch.tensor((mask if rows is None else mask[rows]).reshape(-1, 1, 1), device=DEV)
  leaf = torch.tensor(a, device=DEV).requires_grad_(True)
  return loss(torch.tensor(t, device=DEV), leaf, weights=weights), leaf


def _value_and_grad(name, loss, rows=None):
  val, leaf = _call(name, loss, rows)
  val.backward()
  return val.detach(), leaf.grad


@functools.lru_cache(maxsize=None)
def _default_path_on(name, dev):
  import ddsp_amd
  assert dev == DEV
  val, grad = _value_and_grad(name, _loss(ddsp_amd, name, False))
  return np.float32(npy(val)), npy(grad).astype(np.float64)


def _default_path(name):
  """Value and gradient of deterministic=False (today's kernels), once per case and device - the module's fixture has loaded
  the library by now."""
  return _default_path_on(name, DEV)


def _deterministic(ddsp, name):
  val, grad = _value_and_grad(name, _loss(ddsp, name, True))
  return np.float32(npy(val)), npy(grad)


@pytest.mark.parametrize('name', NAMES)
def test_twice_on_a_fresh_instance_and_beside_another_stream_same_bits(ddsp, name):
  loss = _loss(ddsp, name, True)
  first = npy(_value_and_grad(name, loss)[1])
  assert np.isfinite(first).all() and np.abs(first).max() > 0
  assert np.array_equal(npy(_value_and_grad(name, loss)[1]), first), 'second call on one instance'
  assert np.array_equal(npy(_value_and_grad(name, _loss(ddsp, name, True))[1]), first), 'a fresh instance'
  if DEV != 'cuda' or not torch.cuda.is_available():
    return                                                      # (real streams: left to the GPU run)
  other = _loss(ddsp, name, True)
  streams = [torch.cuda.Stream(), torch.cuda.Stream()]
  for side in streams:
    side.wait_stream(torch.cuda.current_stream())
  results = []
  for which, side in enumerate(streams):
    with torch.cuda.stream(side):
      results.append(_value_and_grad(name, (loss, other)[which])[1])
  for side in streams:
    torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  for which, got in enumerate(results):
    assert np.array_equal(npy(got), first), 'stream %d' % which


@pytest.mark.parametrize('name', [n for n in NAMES if CASES[n][0] >= 2 and CASES[n][3].get('loss_type', 'L1') in ('L1', 'L2')])
def test_rows_do_not_see_each_other(ddsp, name):
  """The gradient of the row-permuted batch is the row-permuted gradient, to the bits."""
  batch = CASES[name][0]
  rows = np.roll(np.arange(batch), 1)
  loss = _loss(ddsp, name, True)
  straight = npy(_value_and_grad(name, loss)[1])
  permuted = npy(_value_and_grad(name, loss, rows)[1])
  assert np.array_equal(permuted, straight[rows])


@pytest.mark.parametrize('name', NAMES)
def test_value_is_the_default_paths_to_the_bits(ddsp, name):
  want = _default_path(name)[0]
  got = _deterministic(ddsp, name)[0]
  assert np.isfinite(got) and got.tobytes() == want.tobytes(), (float(got), float(want))
  # ... and without a gradient being asked for
  t, a = _signals(name)
  mask = CASES[name][4]
  weights = None if mask is None else torch.tensor(np.asarray(mask, np.float32).reshape(-1, 1, 1), device=DEV)
  values = [np.float32(npy(_loss(ddsp, name, flag)(torch.tensor(t, device=DEV), torch.tensor(a, device=DEV), weights=weights)))
            for flag in (True, False)]
  assert values[0].tobytes() == values[1].tobytes()


@pytest.mark.parametrize('name', NAMES)
def test_gradient_against_the_oracle_and_the_default_path(ddsp, name):
  """'L1' mag + logmag cases and the loudness term alone: the analytic oracle, under the rules of
  test_spectral_loss_with_frames_of_three_times_a_power_of_two and test_spectral_loss_loudness_term_golden_and_gradient.
  Every case: the default path's gradient of the same inputs.  Both paths are held to the truth at atol = 1e-9 + 2e-4 max|g|, so
  all but 0.1 % of the samples within twice that, all within twenty times (the two shares tests/test_gpu_backward_state.py uses
  for this gradient)."""
  t, a = _signals(name)
  sizes, kw = CASES[name][2:4]
  got = _deterministic(ddsp, name)[1].astype(np.float64)
  if name in ORACLE_L1:
    ref = O.spectral_loss_backward(t, a, sizes, kw.get('mag_weight', 1.0), kw.get('logmag_weight', 0.0))
    err = np.abs(got - ref)
    atol = 1e-9 + 2e-4 * np.abs(ref).max()
    _log('spectral_loss_det/%s/oracle' % name, median=np.median(err), q90=np.quantile(err, 0.9), atol=atol)
    print(name, 'oracle: median %.3e  q90 %.3e  atol %.3e' % (np.median(err), np.quantile(err, 0.9), atol))
    assert np.median(err) <= 0.2 * atol and np.quantile(err, 0.9) <= atol, (float(np.median(err)), float(np.quantile(err, 0.9)), atol)
  if name == 'loudness_only':
    lt, la = O.compute_loudness(t, dtype=np.float64), O.compute_loudness(a, dtype=np.float64)
    ref = O.compute_loudness_backward(a, -np.sign(lt - la) / lt.size)
    err = np.abs(got - ref)
    atol = 1e-9 + 2e-4 * np.abs(ref).max()
    _log('spectral_loss_det/%s/oracle' % name, q99=np.quantile(err, 0.99), max=err.max(), atol=atol)
    print(name, 'oracle: q99 %.3e  max %.3e  atol %.3e' % (np.quantile(err, 0.99), err.max(), atol))
    assert np.quantile(err, 0.99) <= atol and err.max() <= 20 * atol, (float(np.quantile(err, 0.99)), float(err.max()), atol)
  default = _default_path(name)[1]
  diff = np.abs(got - default)
  atol = 1e-9 + 2e-4 * np.abs(default).max()
  _log('spectral_loss_det/%s/default_path' % name, max=diff.max(), atol=atol, above=(diff > 2 * atol).mean())
  print(name, 'default path: max |difference| %.3e  atol %.3e  above 2 atol %.2e' % (diff.max(), atol, (diff > 2 * atol).mean()))
  assert (diff > 2 * atol).mean() <= 1e-3 and diff.max() <= 20 * atol, (float((diff > 2 * atol).mean()), float(diff.max()), atol)


@pytest.mark.parametrize('name', NAMES)
def test_backward_twice_with_retain_graph_doubles_the_gradient_exactly(ddsp, name):
  val, leaf = _call(name, _loss(ddsp, name, True))
  val.backward(retain_graph=True)
  single = leaf.grad.clone()
  val.backward()
  assert float(single.abs().max()) > 0
  assert torch.equal(leaf.grad, 2 * single)


@pytest.mark.parametrize('name', NAMES)
def test_torch_deterministic_algorithms_switch_selects_the_slab_path(ddsp, name):
  """deterministic=None follows torch.are_deterministic_algorithms_enabled() at the time of the call."""
  want = _deterministic(ddsp, name)[1]
  loss = _loss(ddsp, name, None)
  was, warn_only = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
  assert not was                                               # nothing in the tree turns it on
  assert not loss._slabs()
  try:
    torch.use_deterministic_algorithms(True, warn_only=True)
    assert loss._slabs()
    got = npy(_value_and_grad(name, loss)[1])
  finally:
    torch.use_deterministic_algorithms(was, warn_only=warn_only)
  assert np.array_equal(got, want)
  assert not loss._slabs()
