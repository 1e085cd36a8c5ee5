"""The rest of core.py on the MI355X - frequencies_critical_bands, harmonic_distribution_to_wavetable, the psychoacoustic and
scale functions, gradient_reversal - against tests/core_rest_truth.py (the reference's formulas in fp64 at the fp32 inputs)
and the fixtures tests/golden/make_golden_core_rest.py took from the reference's own code.
tests/test_core_rest_emulated.py runs this module through the SIMT emulation on the CPU.

Tolerances (computed by core_rest_truth, reasons there):
  critical bands   forward 5e-7 M per element, M the largest intermediate of the fp32 chain; gradient (2e-6 + 1.25e-7 M) R,
                   R the largest product of the factors that are not the sigmoids';
  wavetables       3e-6 (n_wavetable / L) max(1, max |truth|) forward, 3e-6 (n_wavetable / L) max(1, max |rfft g|) backward;
  elementwise      2e-6 |truth| + 2e-6 max |truth| over the grid, values and gradients.
Against a fixture the bound is the sum of the kernel's and the fixture's own (both are held to it against the truth).
Every comparison is printed, and appended to the file DDSP_PARITY_LOG names when it is set.

Shapes: tests/core_rest_cases.py - the smallest at which each path can go wrong (tile tails, a depth beyond a wavefront,
K = 1, both limits, one row, 257 rows, a depth in two chunks; a partial block of 4 and of 128 rows, the Nyquist harmonic,
the smallest and the largest transform, the two kinds of length the fused kernel does not take)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import core_rest_cases as C
import core_rest_truth as T
from ddsp_amd import core, synths

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@functools.lru_cache(maxsize=None)
def load_golden(name):
  with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', name + '.npz')) as z:
    return {k: z[k] for k in z.files}


def _log(case, **figures):
  print(case, figures)
  path = os.environ.get('DDSP_PARITY_LOG')
  if path:
    with open(path, 'a') as f:
      f.write(json.dumps(dict(case=case, **{k: float(v) for k, v in figures.items()})) + '\n')


def _dev(array, grad=False):
  return torch.as_tensor(np.array(array), device=DEV).requires_grad_(grad)


def _np(x):
  return x.detach().cpu().numpy().astype(np.float64)


def _check(case, got, truth, tol):
  """max |got - truth| <= tol (a number, or an array for an elementwise bound)."""
  got, truth = _np(got), np.asarray(truth, np.float64)
  assert got.shape == truth.shape, (case, got.shape, truth.shape)
  same = (got == truth) | (np.isnan(got) & np.isnan(truth))          # (equal infinities have no finite difference)
  err = np.where(same, 0.0, np.abs(got - truth))
  _log(case, err=float(np.max(err)), worst_share_of_tolerance=float(np.max(err / tol)), tolerance=float(np.max(tol)))
  assert np.all(err <= tol), (case, float(np.max(err)), float(np.max(tol)))


# ---- frequencies_critical_bands ---------------------------------------------------------------------------------------
def _bands(ddsp, name, x, **override):
  kwargs = dict(C.critical_band_kwargs(name), **override)
  return ddsp.core.frequencies_critical_bands(x, **kwargs)


@pytest.mark.parametrize('name', list(C.CRITICAL_BAND_CASES))
def test_critical_bands_forward_matches_the_truth(ddsp, name):
  k = C.CRITICAL_BAND_CASES[name][0]
  kwargs = C.critical_band_kwargs(name)
  x = C.critical_band_input(name)
  truth = T.critical_bands(x, k, **kwargs)
  tol = T.critical_bands_tolerance(k, **kwargs)
  if name == C.LIMITS_CASE:
    assert truth.min() == 20.0 and truth.max() == 8000.0             # both limits are reached
  with torch.no_grad():
    out = _bands(ddsp, name, _dev(x))
  assert out.shape == x.shape[:2] + (k,) and out.dtype == torch.float32
  _check('critical_bands/' + name, out, truth, tol)
  if name in C.CRITICAL_BAND_GOLDEN_CASES:
    _check('critical_bands/' + name + '/golden', out, load_golden('core_rest_critical_bands')[name + '/out'], 2.0 * tol)


@pytest.mark.parametrize('name', list(C.CRITICAL_BAND_CASES))
def test_critical_bands_gradient_matches_the_truth(ddsp, name):
  k = C.CRITICAL_BAND_CASES[name][0]
  kwargs = C.critical_band_kwargs(name)
  x_np, g_np = C.critical_band_input(name), C.critical_band_cotangent(name)
  x = _dev(x_np, grad=True)
  out = _bands(ddsp, name, x)
  grad, = torch.autograd.grad(out, x, _dev(g_np))
  assert torch.isfinite(grad).all()
  _check('critical_bands/' + name + '/grad', grad, T.critical_bands_grad(x_np, g_np, k, **kwargs),
         T.critical_bands_grad_tolerance(x_np, g_np, k, **kwargs))


def test_critical_bands_takes_the_four_dimensional_form(ddsp):
  name = 'k100_d4_mel'
  k, depth = C.CRITICAL_BAND_CASES[name][:2]
  x_np, g_np = C.critical_band_input(name), C.critical_band_cotangent(name)
  kwargs = dict(C.critical_band_kwargs(name), depth=1)               # (ignored: the depth is the last axis)
  flat, four = _dev(x_np, grad=True), _dev(x_np.reshape(x_np.shape[:2] + (k, depth)), grad=True)
  out_flat, out_four = _bands(ddsp, name, flat), ddsp.core.frequencies_critical_bands(four, **kwargs)
  assert torch.equal(out_flat, out_four)
  g_flat, = torch.autograd.grad(out_flat, flat, _dev(g_np))
  g_four, = torch.autograd.grad(out_four, four, _dev(g_np))
  assert g_four.shape == four.shape and torch.equal(g_flat.reshape(four.shape), g_four)


def test_critical_bands_any_other_scale_is_mel(ddsp):
  name = 'k100_d4_mel'
  x = _dev(C.critical_band_input(name))
  with torch.no_grad():
    assert torch.equal(_bands(ddsp, name, x), _bands(ddsp, name, x, scale='anything'))
    assert not torch.equal(_bands(ddsp, name, x), _bands(ddsp, name, x, scale='bark'))


def test_critical_bands_refuses_a_ragged_depth(ddsp):
  with pytest.raises(ValueError):
    ddsp.core.frequencies_critical_bands(_dev(np.zeros((1, 2, 7), np.float32)), depth=2)


@pytest.mark.parametrize('name', ['k7_d65_bark', 'k33_d3_bark_rows257', 'k2_d2500_mel'])
def test_critical_bands_same_bits_twice_and_for_a_row_alone(ddsp, name):
  x_np, g_np = C.critical_band_input(name), C.critical_band_cotangent(name)

  def run(x_arr, g_arr):
    x = _dev(x_arr, grad=True)
    out = _bands(ddsp, name, x)
    grad, = torch.autograd.grad(out, x, _dev(g_arr))
    return out.detach(), grad

  out, grad = run(x_np, g_np)
  again, grad_again = run(x_np, g_np)
  assert torch.equal(out, again) and torch.equal(grad, grad_again)
  b, t = x_np.shape[0] - 1, x_np.shape[1] // 2
  alone, grad_alone = run(x_np[b:b + 1, t:t + 1], g_np[b:b + 1, t:t + 1])
  assert torch.equal(alone, out[b:b + 1, t:t + 1]) and torch.equal(grad_alone, grad[b:b + 1, t:t + 1])


# ---- harmonic_distribution_to_wavetable -------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(C.WAVETABLE_CASES))
def test_wavetable_forward_matches_the_truth(ddsp, name):
  k, n_wavetable, _ = C.WAVETABLE_CASES[name]
  hd = C.wavetable_input(name)
  truth = T.wavetable(hd, n_wavetable)
  tol = T.wavetable_tolerance(truth, k, n_wavetable)
  with torch.no_grad():
    out = ddsp.core.harmonic_distribution_to_wavetable(_dev(hd), n_wavetable=n_wavetable)
  assert out.shape == hd.shape[:2] + (C.wavetable_length(k, n_wavetable),) and out.dtype == torch.float32
  _check('wavetable/' + name, out, truth, tol)
  if name in C.WAVETABLE_GOLDEN_CASES:
    _check('wavetable/' + name + '/golden', out, load_golden('core_rest_wavetable')[name + '/out'], 2.0 * tol)


@pytest.mark.parametrize('name', list(C.WAVETABLE_CASES))
def test_wavetable_gradient_matches_the_truth(ddsp, name):
  k, n_wavetable, _ = C.WAVETABLE_CASES[name]
  hd_np, g_np = C.wavetable_input(name), C.wavetable_cotangent(name)
  hd = _dev(hd_np, grad=True)
  out = ddsp.core.harmonic_distribution_to_wavetable(hd, n_wavetable=n_wavetable)
  grad, = torch.autograd.grad(out, hd, _dev(g_np))
  _check('wavetable/' + name + '/grad', grad, T.wavetable_grad(g_np, k, n_wavetable), T.wavetable_grad_tolerance(g_np, k, n_wavetable))


def test_wavetable_refuses_more_harmonics_than_half_the_table(ddsp):
  with pytest.raises(ValueError):
    ddsp.core.harmonic_distribution_to_wavetable(_dev(np.full((1, 2, 40), 0.025, np.float32)), n_wavetable=64)


@pytest.mark.parametrize('name', ['k100_w2048', 'k32_w64_nyquist'])
def test_wavetable_same_bits_twice_and_for_a_row_alone(ddsp, name):
  n_wavetable = C.WAVETABLE_CASES[name][1]
  hd_np, g_np = C.wavetable_input(name), C.wavetable_cotangent(name)

  def run(hd_arr, g_arr):
    hd = _dev(hd_arr, grad=True)
    out = ddsp.core.harmonic_distribution_to_wavetable(hd, n_wavetable=n_wavetable)
    grad, = torch.autograd.grad(out, hd, _dev(g_arr))
    return out.detach(), grad

  out, grad = run(hd_np, g_np)
  again, grad_again = run(hd_np, g_np)
  assert torch.equal(out, again) and torch.equal(grad, grad_again)
  b, t = hd_np.shape[0] - 1, hd_np.shape[1] // 2
  alone, grad_alone = run(hd_np[b:b + 1, t:t + 1], g_np[b:b + 1, t:t + 1])
  assert torch.equal(alone, out[b:b + 1, t:t + 1]) and torch.equal(grad_alone, grad[b:b + 1, t:t + 1])


def test_wavetable_synthesis_accepts_the_tables(ddsp):
  name = 'k60_w512'
  with torch.no_grad():
    tables = ddsp.core.harmonic_distribution_to_wavetable(_dev(C.wavetable_input(name)), n_wavetable=512)     # [2, 5, 512]
    f0 = torch.full((2, 5, 1), 220.0, device=DEV)
    amps = torch.full((2, 5, 1), 0.5, device=DEV)
    audio = ddsp.core.wavetable_synthesis(f0, amps, tables, n_samples=320, sample_rate=16000)
  assert audio.shape == (2, 320)


# ---- elementwise -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(C.ELEMENTWISE_CASES))
def test_elementwise_values_and_gradients(ddsp, name):
  fn_name, kwargs, _ = C.ELEMENTWISE_CASES[name]
  x_np, g_np = C.elementwise_input(name), C.elementwise_cotangent(name)
  truth = getattr(T, fn_name)(x_np, **kwargs)
  x = _dev(x_np, grad=True)
  out = getattr(ddsp.core, fn_name)(x, **kwargs)
  _check('elementwise/' + name, out, truth, T.elementwise_tolerance(truth))
  _check('elementwise/' + name + '/golden', out, load_golden('core_rest_elementwise')[name + '/out'], 2.0 * T.elementwise_tolerance(truth))
  grad, = torch.autograd.grad(out, x, _dev(g_np))
  grad_truth = g_np.astype(np.float64) * getattr(T, 'd_' + fn_name)(x_np, **kwargs)
  assert torch.isfinite(grad).all()
  _check('elementwise/' + name + '/grad', grad, grad_truth, T.elementwise_tolerance(grad_truth))


def test_the_poles_keep_their_ieee_results(ddsp):
  with torch.no_grad():
    assert float(ddsp.core.hz_to_bark(_dev(np.zeros(1, np.float32)))[0]) == np.float32(-0.53)
    assert float(ddsp.core.bark_to_hz(_dev(np.full(1, -0.53, np.float32)))[0]) == 0.0


def test_log10_is_logb_of_ten(ddsp):
  x_np = np.array([0.0, -1.0, 1e-6, 1.0, 10.0, 12345.0], np.float32)
  truth = np.log(np.where(x_np <= 0.0, 1e-5, x_np).astype(np.float64)) / np.log(10.0)
  with torch.no_grad():
    x = _dev(x_np)
    out = ddsp.core.log10(x)
    assert torch.equal(out, ddsp.core.logb(x, base=10.0))
  _check('elementwise/log10', out, truth, T.elementwise_tolerance(truth))
  with pytest.raises(NotImplementedError):
    ddsp.core.log10(_dev(x_np, grad=True))


def test_gradient_reversal(ddsp):
  x = _dev(C.elementwise_input('mel_to_hz'), grad=True)
  g = _dev(C.elementwise_cotangent('mel_to_hz'))
  out = ddsp.core.gradient_reversal(x)
  assert torch.equal(out, x)
  grad, = torch.autograd.grad(out, x, g)
  assert torch.equal(grad, -g)


# ---- captured graphs (GPU only) ----------------------------------------------------------------------------------------
def _replays_like_eager(fn, x_first, x_second, g):
  """Forward + backward of fn captured once on a side stream with torch.cuda.graph and replayed on new inputs written into the
  captured buffer: the same bits as the eager calls."""
  static_x = x_first.clone().requires_grad_(True)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    for _ in range(2):
      torch.autograd.grad(fn(static_x), static_x, g)
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):
    captured_out = fn(static_x)
    captured_grad, = torch.autograd.grad(captured_out, static_x, g)
  for x_new in (x_first, x_second):
    with torch.no_grad():
      static_x.copy_(x_new)
    graph.replay()
    torch.cuda.synchronize()
    x = x_new.clone().requires_grad_(True)
    out = fn(x)
    grad, = torch.autograd.grad(out, x, g)
    assert torch.equal(captured_out, out) and torch.equal(captured_grad, grad)
  assert not torch.equal(fn(x_first.clone()), fn(x_second.clone()))     # (the replay had something new to work on)


def test_both_kernels_replay_from_a_captured_graph(ddsp):
  if DEV != 'cuda' or not torch.cuda.is_available():
    pytest.skip('needs real streams and graphs: left to the GPU run')
  name = 'k7_d65_bark'
  x = C.critical_band_input(name)
  _replays_like_eager(lambda v: _bands(ddsp, name, v), _dev(x), _dev(np.ascontiguousarray(x[::-1])), _dev(C.critical_band_cotangent(name)))
  name = 'k100_w2048'
  hd = C.wavetable_input(name)
  _replays_like_eager(lambda v: ddsp.core.harmonic_distribution_to_wavetable(v, n_wavetable=2048), _dev(hd),
                      _dev(np.ascontiguousarray(hd[::-1])), _dev(C.wavetable_cotangent(name)))


# ---- synths.Sinusoidal(freq_scale_fn=core.frequencies_critical_bands) ---------------------------------------------------
def test_sinusoidal_runs_the_function_as_given_and_passes_its_gradient(ddsp):
  rng = np.random.default_rng(5)
  amps_np = rng.uniform(0.0, 0.2, (2, 10, 8)).astype(np.float32)
  freqs_np = rng.standard_normal((2, 10, 8)).astype(np.float32)
  synth = ddsp.synths.Sinusoidal(n_samples=640, sample_rate=16000, amp_scale_fn=None,
                                 freq_scale_fn=ddsp.core.frequencies_critical_bands)
  amps, freqs = _dev(amps_np), _dev(freqs_np, grad=True)
  audio = synth(amps, freqs)
  assert audio.shape == (2, 640)
  with torch.no_grad():
    ctl_freqs = ddsp.core.frequencies_critical_bands(_dev(freqs_np))
    ctl_amps = ddsp.core.remove_above_nyquist(ctl_freqs, _dev(amps_np), 16000)
    by_hand = synth.get_signal(ctl_amps, ctl_freqs)
  _check('sinusoidal/critical_bands/audio', audio, _np(by_hand), 1e-6)   # the same kernels on the same controls
  grad, = torch.autograd.grad(audio.square().sum(), freqs)
  assert grad.shape == freqs.shape and torch.isfinite(grad).all() and float(grad.abs().max()) > 0.0


@pytest.fixture(scope='module')
def ddsp():
  import ddsp_amd
  return ddsp_amd
