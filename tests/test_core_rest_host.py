"""The host side of the rest of core.py, no GPU and no kernels: the plumbing functions (pad_axis, center_crop, leaf_key,
map_shape, copy_if_tf_function), spectral_ops.pad_or_trim_to_expected_length (ddsp/spectral_ops_test.py:70-100 re-expressed),
the table builders of frequencies_critical_bands against tests/core_rest_truth.py, the length rule and the ValueErrors of
harmonic_distribution_to_wavetable, the truth's own closed form, the C ABI's registration, and the fixtures."""
import os

import numpy as np
import pytest
import torch

import core_rest_cases as C
import core_rest_truth as T
from ddsp_amd import _lib, build, core, spectral_ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _golden(name):
  with np.load(os.path.join(GOLDEN, name + '.npz')) as z:
    return {k: z[k] for k in z.files}


@pytest.fixture
def on_cpu(monkeypatch):
  """tf_float32 moves what it is given to the GPU; the plumbing under test here is torch on whatever device it gets."""
  monkeypatch.setattr(core, '_device', lambda: torch.device('cpu'))


# ---- plumbing --------------------------------------------------------------------------------------------------------
def test_leaf_key_map_shape_copy():
  assert core.leaf_key('a/b/c') == 'c' and core.leaf_key('a') == 'a' and core.leaf_key('a.b', delimiter='.') == 'b'
  nested = {'x': torch.zeros(2, 3), 'y': {'z': np.zeros((4, 1, 5)), 'w': torch.zeros(())}}
  assert core.map_shape(nested) == {'x': [2, 3], 'y': {'z': [4, 1, 5], 'w': []}}
  assert all(isinstance(d, int) for d in core.map_shape(nested)['y']['z'])
  thing = {'a': [1, 2]}
  assert core.copy_if_tf_function(thing) is thing


def test_pad_axis(on_cpu):
  x = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
  out = core.pad_axis(x, (1, 2), axis=1)
  assert out.shape == (2, 6, 4)
  assert torch.equal(out[:, 1:4], x) and float(out[:, 0].abs().max()) == 0.0 and float(out[:, 4:].abs().max()) == 0.0
  out = core.pad_axis(x, (0, 3), axis=2, constant_values=-1.5)
  assert out.shape == (2, 3, 7) and torch.equal(out[..., :4], x) and bool((out[..., 4:] == -1.5).all())
  assert core.pad_axis(x, (2, 0), axis=0).shape == (4, 3, 4)
  assert core.pad_axis(x, (2, 1), axis=-1).shape == (2, 3, 7)
  row = torch.tensor([[1.0, 2.0, 3.0, 4.0]])
  assert core.pad_axis(row, (2, 1), axis=1, mode='REFLECT').tolist() == [[3.0, 2.0, 1.0, 2.0, 3.0, 4.0, 3.0]]
  assert core.pad_axis(row, (2, 1), axis=1, mode='symmetric').tolist() == [[2.0, 1.0, 1.0, 2.0, 3.0, 4.0, 4.0]]
  assert torch.equal(core.pad_axis(row, (2, 1), axis=1, mode='REFLECT'),
                     spectral_ops.pad(torch.tensor([[1.0, 2.0, 3.0, 4.0]]), 4, 1, 'center', mode='REFLECT')[:, :7])
  leaf = torch.ones(2, 3, requires_grad=True)
  core.pad_axis(leaf, (1, 1), axis=1).sum().backward()
  assert torch.equal(leaf.grad, torch.ones(2, 3))
  with pytest.raises(ValueError):
    core.pad_axis(row, (1, 1), axis=2)
  with pytest.raises(ValueError):
    core.pad_axis(row, (-1, 1), axis=1)
  with pytest.raises(ValueError):
    core.pad_axis(row, (1, 1), axis=1, mode='EDGE')
  with pytest.raises(TypeError):
    core.pad_axis(row, (1, 1), axis=1, name='x')


def test_center_crop():
  audio = torch.arange(20, dtype=torch.float32).reshape(2, 10)
  assert torch.equal(core.center_crop(audio, 4), audio[:, 2:-2])
  assert torch.equal(core.center_crop(audio, 5), audio[:, 2:-2])
  frames = torch.zeros(2, 10, 3)
  assert core.center_crop(frames, 6).shape == (2, 4, 3)


@pytest.mark.parametrize('as_tensor', [False, True])
@pytest.mark.parametrize('num_dims', [1, 2])
def test_pad_or_trim_vector_to_expected_length(as_tensor, num_dims):
  vector_len, padded_len, trimmed_len = 10, 15, 4
  vector = np.ones(vector_len) + np.random.default_rng(0).uniform()
  target_padded = np.concatenate([vector, np.zeros(padded_len - vector_len)])
  target_trimmed = vector[:trimmed_len]
  if num_dims > 1:
    vector, target_padded, target_trimmed = (np.tile(v, (16, 1)) for v in (vector, target_padded, target_trimmed))
  given = torch.as_tensor(vector) if as_tensor else vector
  padded = spectral_ops.pad_or_trim_to_expected_length(given, padded_len, use_tf=as_tensor)
  trimmed = spectral_ops.pad_or_trim_to_expected_length(given, trimmed_len, use_tf=as_tensor)
  assert isinstance(padded, torch.Tensor if as_tensor else np.ndarray) and type(trimmed) is type(padded)
  np.testing.assert_allclose(np.asarray(padded), target_padded)
  np.testing.assert_allclose(np.asarray(trimmed), target_trimmed)
  same = spectral_ops.pad_or_trim_to_expected_length(given, vector_len)
  np.testing.assert_array_equal(np.asarray(same), vector)
  filled = spectral_ops.pad_or_trim_to_expected_length(given, 12, pad_value=-3.0)
  assert float(np.asarray(filled)[..., -1].max()) == -3.0


def test_pad_or_trim_refuses_a_length_beyond_the_tolerance():
  with pytest.raises(ValueError, match='Vector length: 10 differs from expected length: 31 beyond tolerance of : 20'):
    spectral_ops.pad_or_trim_to_expected_length(np.ones(10), 31)
  with pytest.raises(ValueError, match='beyond tolerance of : 2'):
    spectral_ops.pad_or_trim_to_expected_length(torch.ones(3, 10), 7, len_tolerance=2)
  assert spectral_ops.pad_or_trim_to_expected_length(np.ones(10), 30).shape == (30,)
  assert 'pad_or_trim_to_expected_length' not in spectral_ops.__doc__.split('Not offered')[1]


# ---- the tables of frequencies_critical_bands ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(C.CRITICAL_BAND_CASES))
def test_critical_band_tables_match_the_truth(name):
  k = C.CRITICAL_BAND_CASES[name][0]
  kwargs = C.critical_band_kwargs(name)
  kwargs.pop('bandwidth_scale')
  f_center, bw, dm = core.critical_band_tables(k, **kwargs)
  t_center, t_bw, t_dm = T.critical_band_tables(k, **kwargs)
  assert f_center.dtype == bw.dtype == dm.dtype == np.float32
  assert f_center.shape == bw.shape == (k,) and dm.shape == (kwargs['depth'],)
  np.testing.assert_array_equal(f_center, t_center.astype(np.float32))          # float64 on the host, rounded once
  np.testing.assert_array_equal(bw, t_bw.astype(np.float32))
  np.testing.assert_allclose(dm, t_dm, rtol=1e-6 * max(1, kwargs['depth']) ** 0.5 + 3e-7 * kwargs['depth'], atol=1e-37)
  assert dm[0] == 1.0 and abs(f_center[0] - 20.0) < 1e-4
  if k > 1:
    assert abs(f_center[-1] - 8000.0) < 1e-2 and np.all(np.diff(f_center) > 0)


def test_critical_band_tables_scales():
  bark = core.critical_band_tables(5, scale='bark')[0]
  mel = core.critical_band_tables(5, scale='mel')[0]
  other = core.critical_band_tables(5, scale='anything')[0]
  np.testing.assert_array_equal(mel, other)
  assert not np.array_equal(bark, mel)
  assert core.critical_band_tables(1)[0].tolist() == [np.float32(T.bark_to_hz(T.hz_to_bark(20.0)))]
  np.testing.assert_allclose(core.critical_band_tables(3, depth=4, depth_scale=2.0)[2], [1.0, 0.5, 0.25, 0.125])


def test_the_limits_case_reaches_both_limits_in_the_truth():
  name = C.LIMITS_CASE
  truth = T.critical_bands(C.critical_band_input(name), C.CRITICAL_BAND_CASES[name][0], **C.critical_band_kwargs(name))
  assert truth.min() == 20.0 and truth.max() == 8000.0


def test_truth_gradients_are_the_slopes_of_the_truth():
  """Central differences in fp64 on the truth's own functions: the analytic gradients are the derivatives of what they claim."""
  name = 'k7_d65_bark'
  k, kwargs = C.CRITICAL_BAND_CASES[name][0], C.critical_band_kwargs(name)
  x = C.critical_band_input(name).astype(np.float64)[:1, :2]
  g = C.critical_band_cotangent(name).astype(np.float64)[:1, :2]
  grad = T.critical_bands_grad(x, g, k, **kwargs)
  for index in [(0, 0, 0), (0, 1, 66), (0, 0, 454)]:
    h = np.zeros_like(x)
    h[index] = 1e-5
    slope = np.sum(g * (T.critical_bands(x + h, k, **kwargs) - T.critical_bands(x - h, k, **kwargs))) / 2e-5
    assert abs(slope - grad[index]) <= 1e-6 * max(1.0, abs(slope))
  for name, (fn_name, fn_kwargs, _) in C.ELEMENTWISE_CASES.items():
    if fn_name == 'nan_to_num':
      continue
    x = C.elementwise_input(name).astype(np.float64)
    x = x[(np.abs(x) > 1e-3) & (np.abs(x + 700.0) > 1.0) & (x > -700.0) & (np.abs(x + 0.53) > 1e-3)]     # away from kinks and poles
    h = 1e-6 * np.maximum(1.0, np.abs(x))
    fn = getattr(T, fn_name)
    slope = (fn(x + h, **fn_kwargs) - fn(x - h, **fn_kwargs)) / (2.0 * h)
    np.testing.assert_allclose(getattr(T, 'd_' + fn_name)(x, **fn_kwargs), slope, rtol=1e-5, atol=1e-9)


# ---- harmonic_distribution_to_wavetable -----------------------------------------------------------------------------------
def test_wavetable_length_rule_and_errors():
  assert core.harmonic_wavetable_length(100, 2048) == 2048
  assert core.harmonic_wavetable_length(3, 7) == 6                   # odd: n_wavetable - 1
  assert core.harmonic_wavetable_length(32, 64) == 64
  assert core.harmonic_wavetable_length(100, 1000) == 1000
  for k, n in ((40, 64), (4, 7), (33, 64)):
    with pytest.raises(ValueError):
      core.harmonic_wavetable_length(k, n)
  for name, (k, n_wavetable, _) in C.WAVETABLE_CASES.items():
    assert core.harmonic_wavetable_length(k, n_wavetable) == T.wavetable_length(k, n_wavetable) == C.wavetable_length(k, n_wavetable)
  fused = {name: core._harmonic_wavetable_fused(C.wavetable_length(k, n)) for name, (k, n, _) in C.WAVETABLE_CASES.items()}
  assert fused == {'k100_w2048': True, 'k32_w64_nyquist': True, 'k60_w512': True, 'k5_w64_one_row': True, 'k3_w7_odd': False,
                   'k100_w1000': False, 'k100_w8192': True}
  assert not core._harmonic_wavetable_fused(32) and not core._harmonic_wavetable_fused(16384)


@pytest.mark.parametrize('name', list(C.WAVETABLE_CASES))
def test_truth_closed_form_is_the_reference_chain(name):
  k, n_wavetable, _ = C.WAVETABLE_CASES[name]
  hd = C.wavetable_input(name)
  chain, closed = T.wavetable(hd, n_wavetable), T.wavetable_closed_form(hd, n_wavetable)
  assert chain.shape == closed.shape == hd.shape[:2] + (T.wavetable_length(k, n_wavetable),)
  assert float(np.abs(chain - closed).max()) <= 1e-13 * n_wavetable
  g = C.wavetable_cotangent(name).astype(np.float64)
  basis_grad = np.stack([np.sum(g * T.wavetable_closed_form(np.eye(k)[j][None, None], n_wavetable), axis=-1) for j in range(0, k, max(1, k // 4))], -1)
  np.testing.assert_allclose(T.wavetable_grad(g, k, n_wavetable)[..., ::max(1, k // 4)], basis_grad, rtol=0, atol=1e-9 * n_wavetable)


def test_the_general_path_is_the_reference_chain_on_torch(on_cpu):
  """Lengths the fused kernel does not take never reach the library: torch.fft.irfft, differentiable by torch."""
  for name in ('k3_w7_odd', 'k100_w1000'):
    k, n_wavetable, _ = C.WAVETABLE_CASES[name]
    hd = torch.as_tensor(np.array(C.wavetable_input(name))).requires_grad_(True)
    out = core.harmonic_distribution_to_wavetable(hd, n_wavetable=n_wavetable)
    truth = T.wavetable(C.wavetable_input(name), n_wavetable)
    assert float(np.abs(out.detach().numpy() - truth).max()) <= T.wavetable_tolerance(truth, k, n_wavetable)
    g = torch.as_tensor(np.array(C.wavetable_cotangent(name)))
    grad, = torch.autograd.grad(out, hd, g)
    assert float(np.abs(grad.numpy() - T.wavetable_grad(g.numpy(), k, n_wavetable)).max()) <= T.wavetable_grad_tolerance(g.numpy(), k, n_wavetable)
  with pytest.raises(ValueError):
    core.harmonic_distribution_to_wavetable(torch.full((1, 2, 40), 0.025), n_wavetable=64)


def test_log_scale_refuses_bounds_that_have_no_logarithm(on_cpu):
  with pytest.raises(ValueError):
    core.log_scale(torch.zeros(3), 0.0, 10.0)


# ---- the C ABI and the fixtures ----------------------------------------------------------------------------------------------
def test_the_new_entry_points_are_declared_registered_and_built():
  with open(os.path.join(os.path.dirname(GOLDEN), os.pardir, 'include', 'ddsp_amd.h')) as f:
    header = f.read()
  for name in ('ddsp_critical_bands_f32', 'ddsp_critical_bands_backward_f32', 'ddsp_harmonic_wavetable_f32',
               'ddsp_harmonic_wavetable_backward_f32', 'ddsp_scale_convert_f32', 'ddsp_scale_convert_backward_f32'):
    assert name in _lib.SIGNATURES and ('int %s(' % name) in header
  for op, code in _lib.SCALE_OPS.items():
    assert ('#define DDSP_SCALE_%s %d\n' % (op.upper(), code)) in header
  for source in ('scale_fns.hip', 'critical_bands.hip', 'harmonic_wavetable.hip'):
    assert source in build.SOURCES
  for name in ('hz_to_bark', 'bark_to_hz', 'hz_to_mel', 'mel_to_hz', 'hz_to_erb', 'sym_exp_sigmoid', 'soft_limit', 'log_scale', 'log10',
               'nan_to_num', 'gradient_reversal', 'pad_axis', 'center_crop', 'leaf_key', 'map_shape', 'copy_if_tf_function',
               'frequencies_critical_bands', 'harmonic_distribution_to_wavetable'):
    assert callable(getattr(core, name))


def test_the_fixtures_carry_what_the_gpu_tests_read():
  bands = _golden('core_rest_critical_bands')
  for name in C.CRITICAL_BAND_GOLDEN_CASES:
    k, _, _, _, (b, t) = C.CRITICAL_BAND_CASES[name]
    np.testing.assert_array_equal(bands[name + '/x'], C.critical_band_input(name))
    assert bands[name + '/out'].shape == (b, t, k) and bands[name + '/out'].dtype == np.float32
    for key, value in C.critical_band_kwargs(name).items():
      assert bands[name + '/' + key].item() == value
  tables = _golden('core_rest_wavetable')
  for name in C.WAVETABLE_GOLDEN_CASES:
    k, n_wavetable, (b, t) = C.WAVETABLE_CASES[name]
    np.testing.assert_array_equal(tables[name + '/harmonic_distribution'], C.wavetable_input(name))
    assert tables[name + '/out'].shape == (b, t, C.wavetable_length(k, n_wavetable)) and int(tables[name + '/n_wavetable']) == n_wavetable
  values = _golden('core_rest_elementwise')
  for name, (fn_name, kwargs, _) in C.ELEMENTWISE_CASES.items():
    np.testing.assert_array_equal(values[name + '/x'], C.elementwise_input(name))
    assert values[name + '/out'].shape == values[name + '/x'].shape and str(values[name + '/function']) == fn_name
    for key, value in kwargs.items():
      assert values[name + '/' + key].item() == value
