"""The consistency losses and core.sinusoidal_to_harmonic on the MI355X against tests/consistency_truth.py (fp64 at the fp32
inputs).  tests/test_consistency_emulated.py runs the small cases of this module through the SIMT emulation on the CPU.

Tolerances: scalars 5e-5 relative (the SpectralLoss figure); gradients 2e-4 max|gradient| (every synth's);
per-frame tensors: the kernel's error against the fp64 truth may be up to 4 x that of the truth helper's fp32 mode on the same
case (which stands for the reference's arithmetic), with a floor of a few fp32 ulp of the tensor's scale for cases where the
fp32 mode happens to land on the truth.  Every comparison is appended to profiles/consistency_parity_errors.jsonl when
DDSP_PARITY_LOG is set.

Goldens (tests/golden/consistency_*.npz, made by the reference's own losses.py / core.py on the numpy TF stand-in) are held to
the scalar ceiling, relative to the fixture's largest value."""
import json
import os
import zlib

import numpy as np
import pytest
import torch

import consistency_truth as T
from ddsp_amd import core, losses

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SCALAR_RTOL = 5e-5
GRAD_RTOL = 2e-4
TENSOR_RATIO = 4.0
TENSOR_FLOOR = 8 * 2.0 ** -24          # eight fp32 ulp of the tensor's largest magnitude


def _log(case, **figures):
  print(case, figures)
  path = os.environ.get('DDSP_PARITY_LOG')
  if path:
    with open(path, 'a') as f:
      f.write(json.dumps(dict(case=case, **{k: float(v) for k, v in figures.items()})) + '\n')


def _dev(*arrays, grad=False):
  return [torch.as_tensor(a, device=DEV).requires_grad_(grad) for a in arrays]


def _np(x):
  return x.detach().cpu().numpy().astype(np.float64)


def _check_tensor(case, got, truth, faithful):
  truth, faithful = truth.numpy(), faithful.numpy().astype(np.float64)
  finite = np.isfinite(truth)
  scale = np.max(np.abs(truth[finite])) if finite.any() else 1.0
  scale = scale if scale > 0.0 else 1.0              # a tensor of zeros: the error is absolute
  err = np.max(np.abs(got - truth)[finite]) / scale if finite.any() else 0.0
  ref_err = np.max(np.abs(faithful - truth)[finite]) / scale if finite.any() else 0.0
  _log(case, kernel_err=err, reference_fp32_err=ref_err, scale=scale)
  assert np.array_equal(np.isnan(got), np.isnan(truth))
  assert err <= max(TENSOR_RATIO * ref_err, TENSOR_FLOOR), (case, err, ref_err)


def _check_scalar(case, got, truth):
  err = abs(float(got) - float(truth)) / max(abs(float(truth)), 1e-30)
  _log(case, scalar_rel_err=err)
  assert err <= SCALAR_RTOL, (case, float(got), float(truth))


def _check_grads(case, got, truth, inputs, degenerate=False, out_mag=0.0, floors=None):
  """2e-4 of the largest gradient element, per input: the plain bound.

  degenerate (cases of ONE sinusoid only): an input whose gradient vanishes analytically - the normalised weight of a single
  sinusoid is 1 whatever its amplitude - is left with the rounding of terms that cancel; those terms are as large as the
  other inputs' sensitivities, so the scale of input i is then at least max_j max|x_j dL/dx_j| / max|x_i|, and where the loss
  does not depend on its inputs at all (one sinusoid that is its own candidate: the ratio is 1) the cancelling terms are of
  the size of the contracted output itself: out_mag = |cotangent . output| enters that maximum at a thousandth.
  floors: where autograd adds two gradients that may cancel (the sinusoids as their own candidates), the larger addend."""
  sens = max(float(np.max(np.abs(np.asarray(x, np.float64) * t))) for x, t in zip(inputs, truth))
  sens = max(sens, 1e-3 * float(out_mag))
  for i, (g, t, x) in enumerate(zip(got, truth, inputs)):
    g = _np(g)
    scale = max(np.max(np.abs(t)), 1e-30, floors[i] if floors else 0.0)
    if degenerate:
      scale = max(scale, sens / max(float(np.max(np.abs(x))), 1e-30))
    err = np.max(np.abs(g - t)) / scale
    _log('%s/grad%d' % (case, i), grad_err=err, scale=scale, plain_scale=np.max(np.abs(t)))
    assert np.isfinite(g).all()
    assert err <= GRAD_RTOL, (case, i, err)


# (name, B, T, K, C or H, sample_rate): the small ones also run under the emulation.  The fp64 truth materialises
# [B, T, C, K, G], so forward AND gradients of the shipped shape (100 sinusoids, 100 candidates, 30 gaussians, 10 points) are
# compared on 48 frames; test_shipped_1000_frames compares the forward of a whole row of 1000 frames, the truth in chunks
SHAPES = [('k1', 2, 3, 1, 1, 16000), ('k7', 2, 5, 7, 7, 16000), ('k100', 1, 4, 100, 100, 16000), ('k257', 1, 2, 257, 257, 16000),
          ('k1024', 1, 1, 1024, 1024, 16000), ('k20_48k', 2, 4, 20, 9, 48000), ('shipped_k100_c100', 2, 24, 100, 100, 16000)]
SCALES = [0.02, 0.1, 0.5, 5.0]


def _case(name, b, t, k, c, sr, seed=0, zeros=False, wide=False):
  rng = np.random.default_rng(zlib.crc32(('%s/%d' % (name, seed)).encode()))
  amps, freqs = T.make_sinusoids(rng, b, t, k, sr, zeros=zeros, wide=wide)
  f0c = np.exp(rng.uniform(np.log(60.0), np.log(1500.0), (b, t, c))).astype(np.float32)
  return amps, freqs, f0c, rng


def _s2h(name, b, t, k, h, sr, normalize, width):
  amps, freqs, f0c, rng = _case(name, b, t, k, 1, sr, wide=True, zeros=True)
  if width != 0.1 and k > 1:
    # sinusoids near harmonics of f0, as the function is used: at width 0.02 random frequencies leave nothing to compare
    freqs = (f0c * rng.integers(1, h + 2, freqs.shape) * rng.uniform(1.0 - 2.0 * width, 1.0 + 2.0 * width, freqs.shape)).astype(np.float32)
  kw = dict(harmonic_width=width, n_harmonics=h, sample_rate=sr, normalize=normalize)
  da, df, d0 = _dev(amps, freqs, f0c, grad=True)
  harm_amp, harm_dist = core.sinusoidal_to_harmonic(da, df, d0, **kw)
  assert harm_amp.shape == (b, t, 1) and harm_dist.shape == (b, t, h)
  truth = T.sinusoidal_to_harmonic(amps, freqs, f0c, **kw)
  faithful = T.sinusoidal_to_harmonic(amps, freqs, f0c, dtype=torch.float32, **kw)
  case = 's2h/%s/norm%d/width%g' % (name, normalize, width)
  _check_tensor(case + '/amp', _np(harm_amp), truth[0], faithful[0])
  _check_tensor(case + '/dist', _np(harm_dist), truth[1], faithful[1])
  for cot_scale in (1e-6, 1.0, 1e6):
    ca = (rng.standard_normal((b, t, 1)) * cot_scale).astype(np.float32)
    cd = (rng.standard_normal((b, t, h)) * cot_scale).astype(np.float32)
    got = torch.autograd.grad([harm_amp, harm_dist], [da, df, d0], _dev(ca, cd), retain_graph=True)
    want = T.grads(lambda a, f, f0: T.sinusoidal_to_harmonic(a, f, f0, **kw), (amps, freqs, f0c), (ca, cd))
    _check_grads('%s/cot%g' % (case, cot_scale), got, want, (amps, freqs, f0c), degenerate=(k == 1))


@pytest.mark.parametrize('shape', SHAPES, ids=[s[0] for s in SHAPES])
@pytest.mark.parametrize('normalize', [False, True])
def test_sinusoidal_to_harmonic(ddsp, shape, normalize):
  _s2h(*shape, normalize, 0.1)


@pytest.mark.parametrize('width', SCALES)
@pytest.mark.parametrize('normalize', [False, True])
def test_sinusoidal_to_harmonic_widths(ddsp, width, normalize):
  _s2h('widths', 2, 6, 20, 12, 16000, normalize, width)


@pytest.mark.parametrize('shape', SHAPES, ids=[s[0] for s in SHAPES])
@pytest.mark.parametrize('mode', ['candidates', 'sinusoids', 'c1'])
def test_twm(ddsp, shape, mode):
  name, b, t, k, c, sr = shape
  amps, freqs, f0c, rng = _case(name, b, t, k, c, sr, zeros=(mode == 'c1'), wide=(mode == 'candidates'))
  if mode == 'c1':
    f0c = f0c[:, :, :1].copy()
  kw = dict(sinusoids_scale=0.5, harmonics_scale=0.2, n_harmonic_points=10, n_harmonic_gaussians=30, sample_rate=sr)
  loss = losses.TWMLoss(**kw)
  da, df = _dev(amps, freqs, grad=True)
  if mode == 'sinusoids':
    d0, f0c = df, freqs
  else:
    d0, = _dev(f0c, grad=True)
  s, h = loss.get_loss_tensors(d0, df, da)
  truth = T.twm_loss_tensors(f0c, freqs, amps, **kw)
  faithful = T.twm_loss_tensors(f0c, freqs, amps, dtype=torch.float32, **kw)
  case = 'twm/%s/%s' % (name, mode)
  _check_tensor(case + '/sinusoids_loss', _np(s), truth[0], faithful[0])
  _check_tensor(case + '/harmonics_loss', _np(h), truth[1], faithful[1])
  scalar = loss(d0, df, da)
  _check_scalar(case + '/scalar', scalar, T.twm_loss(f0c, freqs, amps, **kw))
  inputs = [df, da] if mode == 'sinusoids' else [d0, df, da]
  if mode == 'sinusoids':
    want_fn, want_in = (lambda f, a: T.twm_loss(f, f, a, **kw)), (freqs, amps)
    # autograd adds dL/d candidates and dL/d freqs, which may cancel (one sinusoid that is its own candidate: the loss is a
    # constant): the sum is held to 2e-4 of the larger addend
    sep = T.grads(lambda f0, f, a: T.twm_loss(f0, f, a, **kw), (freqs, freqs, amps))
    addend = max(np.max(np.abs(sep[0])), np.max(np.abs(sep[1])))
  else:
    want_fn, want_in = (lambda f0, f, a: T.twm_loss(f0, f, a, **kw)), (f0c, freqs, amps)
  for cot_scale in (1e-6, 1.0, 1e6):
    got = torch.autograd.grad(scalar, inputs, torch.tensor(cot_scale, device=DEV), retain_graph=True)
    want = T.grads(want_fn, want_in, [np.float64(np.float32(cot_scale))])
    _check_grads('%s/cot%g' % (case, cot_scale), got, want, want_in, degenerate=(k == 1), out_mag=cot_scale * abs(float(scalar)),
                 floors=[cot_scale * addend, 0.0] if mode == 'sinusoids' else None)
  # predict_f0: the truth's loss at the chosen candidate is the truth's minimum, to the forward tolerance, in every frame
  f0 = loss.predict_f0(d0.detach(), df.detach(), da.detach())
  assert isinstance(f0, np.ndarray) and f0.shape == (b, t, 1)
  L = (truth[0] + truth[1]).numpy()
  idx = np.argmin(np.abs(f0c.astype(np.float64) - f0), axis=-1)
  chosen = np.take_along_axis(L, idx[..., None], -1)[..., 0]
  assert np.all(np.take_along_axis(f0c, idx[..., None], -1) == f0)
  gap = np.max((chosen - np.nanmin(L, -1)) / np.maximum(np.abs(np.nanmin(L, -1)), 1e-30))
  _log(case + '/predict_f0', worst_gap=gap)
  assert gap <= SCALAR_RTOL


@pytest.mark.parametrize('scale', SCALES)
def test_twm_scales(ddsp, scale):
  amps, freqs, f0c, rng = _case('scales', 2, 6, 20, 8, 16000)
  kw = dict(sinusoids_scale=scale, harmonics_scale=scale, n_harmonic_points=7, n_harmonic_gaussians=33, sample_rate=16000)
  loss = losses.TWMLoss(**kw)
  d0, df, da = _dev(f0c, freqs, amps, grad=True)
  s, h = loss.get_loss_tensors(d0, df, da)
  truth = T.twm_loss_tensors(f0c, freqs, amps, **kw)
  faithful = T.twm_loss_tensors(f0c, freqs, amps, dtype=torch.float32, **kw)
  _check_tensor('twm/scale%g/sinusoids_loss' % scale, _np(s), truth[0], faithful[0])
  _check_tensor('twm/scale%g/harmonics_loss' % scale, _np(h), truth[1], faithful[1])
  cs, ch = (rng.standard_normal(s.shape).astype(np.float32) for _ in range(2))
  got = torch.autograd.grad([s, h], [d0, df, da], _dev(cs, ch))
  want = T.grads(lambda f0, f, a: T.twm_loss_tensors(f0, f, a, **kw), (f0c, freqs, amps), (cs, ch))
  _check_grads('twm/scale%g' % scale, got, want, (f0c, freqs, amps))


def test_twm_stays_finite_far_from_the_grid(ddsp):
  """Ratios of 100 against centres 1 .. 30: the log-sum-exp is max-subtracted, as TFP's is."""
  freqs = np.full((1, 2, 4), 5000.0, np.float32)
  amps = np.full((1, 2, 4), 0.5, np.float32)
  f0c = np.full((1, 2, 1), 50.0, np.float32)
  s, h = losses.TWMLoss().get_loss_tensors(*_dev(f0c, freqs, amps))
  truth = T.twm_loss_tensors(f0c, freqs, amps)
  assert np.isfinite(_np(s)).all()
  np.testing.assert_allclose(_np(s), truth[0].numpy(), rtol=1e-5)


def test_twm_nyquist_equality_is_masked(ddsp):
  """800 Hz x 10 = 8000 Hz = Nyquist: both sides of the comparison are the same function of the same number: masked."""
  freqs = np.array([[[800.0, 1600.0, 2400.0]]], np.float32)
  amps = np.ones((1, 1, 3), np.float32)
  f0c = np.array([[[800.0, 9000.0]]], np.float32)
  s, h = losses.TWMLoss().get_loss_tensors(*_dev(f0c, freqs, amps))
  truth = T.twm_loss_tensors(f0c, freqs, amps)
  np.testing.assert_allclose(_np(h), truth[1].numpy(), rtol=1e-5, atol=1e-6)
  assert _np(h)[0, 0, 1] == 0.0                     # every harmonic above Nyquist: safe_divide(mask, mean(mask)) = 0


def test_predict_f0_all_nan_raises(ddsp):
  freqs = np.full((1, 2, 3), np.nan, np.float32)
  amps = np.ones((1, 2, 3), np.float32)
  with pytest.raises(ValueError):
    losses.TWMLoss().predict_f0(*_dev(freqs, freqs, amps))


KDE_WEIGHTS = [dict(), dict(weight_a=1.0, weight_b=1.0, weight_mean_amp=0.0, scale_a=0.5, scale_b=0.5),
               dict(weight_a=0.0, weight_b=2.0, weight_mean_amp=3.0, scale_a=0.02, scale_b=5.0)]


@pytest.mark.parametrize('shape', SHAPES, ids=[s[0] for s in SHAPES])
@pytest.mark.parametrize('weights', range(len(KDE_WEIGHTS)))
def test_kde(ddsp, shape, weights):
  name, b, t, k, kb, sr = shape
  kw = KDE_WEIGHTS[weights]
  amps_a, freqs_a, _, rng = _case(name, b, t, k, 1, sr, zeros=True, wide=True)
  amps_b, freqs_b = T.make_sinusoids(rng, b, t, kb, sr)
  loss = losses.KDEConsistencyLoss(**kw)
  dev = _dev(amps_a, freqs_a, amps_b, freqs_b, grad=True)
  case = 'kde/%s/w%d' % (name, weights)
  nll = loss.nll(dev[0], dev[1], dev[2], dev[3], 0.1)
  assert nll.shape == (b, t)
  _check_tensor(case + '/nll', _np(nll), T.kde_nll(amps_a, freqs_a, amps_b, freqs_b, 0.1),
                T.kde_nll(amps_a, freqs_a, amps_b, freqs_b, 0.1, dtype=torch.float32))
  scalar = loss(*dev)
  _check_scalar(case + '/scalar', scalar, T.kde_loss(amps_a, freqs_a, amps_b, freqs_b, **kw))
  for cot_scale in (1e-6, 1.0, 1e6):
    got = torch.autograd.grad(scalar, dev, torch.tensor(cot_scale, device=DEV), retain_graph=True)
    want = T.grads(lambda *xs: T.kde_loss(*xs, **kw), (amps_a, freqs_a, amps_b, freqs_b), [np.float64(np.float32(cot_scale))])
    _check_grads('%s/cot%g' % (case, cot_scale), got, want, (amps_a, freqs_a, amps_b, freqs_b), degenerate=(k == 1 or kb == 1))


@pytest.mark.parametrize('scale', SCALES)
def test_kde_nll_scales(ddsp, scale):
  amps_a, freqs_a, _, rng = _case('kde_scales', 2, 6, 20, 1, 16000, zeros=True)
  amps_b, freqs_b = T.make_sinusoids(rng, 2, 6, 13)
  dev = _dev(amps_a, freqs_a, amps_b, freqs_b, grad=True)
  nll = losses.KDEConsistencyLoss().nll(*dev, scale)
  _check_tensor('kde/scale%g/nll' % scale, _np(nll), T.kde_nll(amps_a, freqs_a, amps_b, freqs_b, scale),
                T.kde_nll(amps_a, freqs_a, amps_b, freqs_b, scale, dtype=torch.float32))
  cot = rng.standard_normal(nll.shape).astype(np.float32)
  got = torch.autograd.grad(nll, dev, _dev(cot)[0])
  want = T.grads(lambda *xs: T.kde_nll(*xs, scale), (amps_a, freqs_a, amps_b, freqs_b), (cot,))
  _check_grads('kde/scale%g' % scale, got, want, (amps_a, freqs_a, amps_b, freqs_b))


def test_shipped_1000_frames(ddsp):
  """The shipped shape as it ships: one row of 1000 frames, 100 sinusoids, 100 candidates (the sinusoids), 30 gaussians, 10
  points, 100 harmonics.  Forward values of every function against the fp64 truth, which is evaluated 25 frames at a time."""
  t, k, step = 1000, 100, 25
  amps, freqs, f0c, rng = _case('t1000', 1, t, k, 1, 16000)
  amps_b, freqs_b = T.make_sinusoids(rng, 1, t, k)
  da, df, d0, dab, dfb = _dev(amps, freqs, f0c, amps_b, freqs_b)
  s, h = losses.TWMLoss().get_loss_tensors(df, df, da)
  nll = losses.KDEConsistencyLoss().nll(da, df, dab, dfb, 0.1)
  ha, hd = core.sinusoidal_to_harmonic(da, df, d0)
  def chunks(fn, dtype):
    outs = [fn(slice(i, i + step), dtype) for i in range(0, t, step)]
    return [torch.cat([o[j] for o in outs], 1) for j in range(len(outs[0]))]
  for dtype, store in ((torch.float64, 'truth'), (torch.float32, 'faithful')):
    twm_ = chunks(lambda sl, dt: T.twm_loss_tensors(freqs[:, sl], freqs[:, sl], amps[:, sl], dtype=dt), dtype)
    kde_ = chunks(lambda sl, dt: (T.kde_nll(amps[:, sl], freqs[:, sl], amps_b[:, sl], freqs_b[:, sl], 0.1, dtype=dt),), dtype)
    s2h_ = chunks(lambda sl, dt: T.sinusoidal_to_harmonic(amps[:, sl], freqs[:, sl], f0c[:, sl], dtype=dt), dtype)
    if store == 'truth':
      truth = twm_ + kde_ + s2h_
    else:
      faithful = twm_ + kde_ + s2h_
  names = ('sinusoids_loss', 'harmonics_loss', 'kde_nll', 'harm_amp', 'harm_dist')
  for name, got, tr, fa in zip(names, (s, h, nll, ha, hd), truth, faithful):
    _check_tensor('shipped_t1000/' + name, _np(got), tr, fa)
  L = (truth[0] + truth[1]).numpy()
  f0 = losses.TWMLoss().predict_f0(df, df, da)
  idx = np.argmin(np.abs(freqs.astype(np.float64) - f0), axis=-1)
  gap = np.max((np.take_along_axis(L, idx[..., None], -1)[..., 0] - L.min(-1)) / np.abs(L.min(-1)))
  _log('shipped_t1000/predict_f0', worst_gap=gap)
  assert gap <= SCALAR_RTOL


def test_known_answer_predict_f0_of_a_harmonic_series(ddsp):
  """The case of tests/test_consistency_host.py (chosen there with the truth helper): f0, 2 f0, ... and f0 among the candidates."""
  f0 = 220.0
  freqs = (f0 * np.arange(1, 13, dtype=np.float32))[None, None]
  amps = (1.0 / np.arange(1, 13, dtype=np.float32))[None, None]
  cands = np.array([[[110.0, 146.7, 220.0, 330.0, 440.0, 660.0]]], np.float32)
  got = losses.TWMLoss().predict_f0(*_dev(cands, freqs, amps))
  assert got.shape == (1, 1, 1) and got[0, 0, 0] == np.float32(220.0)


def test_known_answer_harmonic_round_trip(ddsp):
  """sinusoidal_to_harmonic(harmonic_to_sinusoidal(...)) returns the harmonic controls for the harmonics below Nyquist."""
  f0 = np.array([[[400.0]]], np.float32)
  dist = np.array([[[0.4, 0.3, 0.2, 0.1] + [0.0] * 26]], np.float32)
  amp = np.array([[[0.7]]], np.float32)
  sin_amps, sin_freqs = core.harmonic_to_sinusoidal(*_dev(amp, dist, f0))
  harm_amp, harm_dist = core.sinusoidal_to_harmonic(sin_amps, sin_freqs, _dev(f0)[0], n_harmonics=30)
  np.testing.assert_allclose(_np(harm_amp), amp, rtol=1e-6)
  np.testing.assert_allclose(_np(harm_dist), dist, atol=1e-7)


def test_thin_losses(ddsp):
  rng = np.random.default_rng(5)
  b, t, h = 2, 12, 8
  amp, amp_t = (rng.uniform(0.0, 3e-4, (b, t, 1)).astype(np.float32) for _ in range(2))
  dist, dist_t = (rng.uniform(0.0, 1.0, (b, t, h)).astype(np.float32) for _ in range(2))
  f0, f0_t = (rng.uniform(50.0, 900.0, (b, t, 1)).astype(np.float32) for _ in range(2))
  f0[0, 0] = 0.0
  dev = _dev(amp, amp_t, dist, dist_t, f0, f0_t, grad=True)
  got = losses.HarmonicConsistencyLoss(amp_weight=2.0, dist_weight=0.5, f0_weight=3.0)(*dev)
  want = T.harmonic_consistency(amp, amp_t, dist, dist_t, f0, f0_t, amp_weight=2.0, dist_weight=0.5, f0_weight=3.0)
  assert sorted(got) == ['f0_hz_loss', 'harm_amp_loss', 'harm_dist_loss']
  for key in got:
    _check_scalar('harmonic_consistency/' + key, got[key], want[key])
  total = sum(got.values())
  grads = torch.autograd.grad(total, dev, allow_unused=True)
  wg = T.grads(lambda *xs: sum(T.harmonic_consistency(*xs, amp_weight=2.0, dist_weight=0.5, f0_weight=3.0).values()),
               (amp, amp_t, dist, dist_t, f0, f0_t))
  _check_grads('harmonic_consistency', grads, wg, (amp, amp_t, dist, dist_t, f0, f0_t))
  x, y = (rng.uniform(0.0, 1.0, (b, t, h)).astype(np.float32) for _ in range(2))
  x[0, 0] = 0.0
  dx, dy = _dev(x, y, grad=True)
  got = losses.amp_loss(dx, dy, log=True, amin=1e-3)
  _check_scalar('amp_loss_log', got, T.amp_loss(x, y, log=True, amin=1e-3))
  _check_grads('amp_loss_log', torch.autograd.grad(got, [dx, dy]), T.grads(lambda a, c: T.amp_loss(a, c, log=True, amin=1e-3), (x, y)), (x, y))
  got = losses.freq_loss(_dev(x * np.float32(1000.0))[0], _dev(y * np.float32(1000.0))[0], loss_type='L2')
  _check_scalar('freq_loss_l2', got, T.freq_loss(x * np.float32(1000.0), y * np.float32(1000.0), 'L2'))
  _check_scalar('param_loss_l2', losses.ParamLoss(weight=0.25, loss_type='L2')(dx, dy), 0.25 * T.mean_difference(torch.as_tensor(x, dtype=torch.float64), torch.as_tensor(y, dtype=torch.float64), 'L2'))
  _check_scalar('filtered_noise_consistency', losses.FilteredNoiseConsistencyLoss(weight=2.0)(dx, dy), 2.0 * T.amp_loss(x, y))


def test_loss_group_with_consistency_losses(ddsp):
  amps, freqs, f0c, rng = _case('group', 2, 6, 12, 1, 16000)
  amps_b, freqs_b = T.make_sinusoids(rng, 2, 6, 9)
  twm, kde = losses.TWMLoss(name='twm'), losses.KDEConsistencyLoss(name='kde')
  group = losses.LossGroup(dag=[(twm, ['f0', 'freqs', 'amps']), (kde, ['amps', 'freqs', 'amps_b', 'freqs_b'])])
  dev = _dev(f0c, freqs, amps, amps_b, freqs_b, grad=True)
  out = group(dict(zip(['f0', 'freqs', 'amps', 'amps_b', 'freqs_b'], dev)))
  assert sorted(out) == ['kde', 'twm']
  _check_scalar('group/twm', out['twm'], T.twm_loss(f0c, freqs, amps))
  _check_scalar('group/kde', out['kde'], T.kde_loss(amps, freqs, amps_b, freqs_b))
  got = torch.autograd.grad(out['twm'] + out['kde'], dev)
  want = T.grads(lambda f0, f, a, ab, fb: T.twm_loss(f0, f, a) + T.kde_loss(a, f, ab, fb), (f0c, freqs, amps, amps_b, freqs_b))
  _check_grads('group', got, want, (f0c, freqs, amps, amps_b, freqs_b))


def _everything(f0c, freqs, amps, amps_b, freqs_b):
  dev = _dev(f0c, freqs, amps, amps_b, freqs_b, grad=True)
  s, h = losses.TWMLoss().get_loss_tensors(dev[0], dev[1], dev[2])
  nll = losses.KDEConsistencyLoss().nll(dev[2], dev[1], dev[3], dev[4], 0.1)
  ha, hd = core.sinusoidal_to_harmonic(dev[2], dev[1], dev[0][:, :, :1].contiguous(), n_harmonics=11)
  outs = [s, h, nll, ha, hd]
  # a cotangent that depends on the position inside a row alone
  total = sum((o * torch.linspace(0.5, 1.5, o[0].numel(), device=DEV).reshape(o.shape[1:])).sum() for o in outs)
  return [o.detach() for o in outs] + list(torch.autograd.grad(total, dev))


def test_same_bits_twice_row_alone_and_sub_batch(ddsp):
  amps, freqs, f0c, rng = _case('bits', 4, 9, 33, 5, 16000, zeros=True)
  amps_b, freqs_b = T.make_sinusoids(rng, 4, 9, 17)
  args = (f0c, freqs, amps, amps_b, freqs_b)
  first, second = _everything(*args), _everything(*args)
  for a, b in zip(first, second):
    assert torch.equal(a, b)
  row = _everything(*[v[2:3] for v in args])
  sub = _everything(*[v[1:3] for v in args])
  for a, r, s in zip(first, row, sub):
    assert torch.equal(a[2:3], r) and torch.equal(a[1:3], s)


def test_peak_memory_shipped_shape_batch_8(ddsp):
  """Forward + backward of TWMLoss and of sinusoidal_to_harmonic at 1000 frames, 100 / 100 / 30 / 10, batch 8, allocate less
  than ONE [B, T, C, K] fp32 tensor (320 MB)."""
  b, t, k = 8, 1000, 100
  amps, freqs, f0c, rng = _case('peak', b, t, k, 1, 16000)
  da, df, d0 = _dev(amps, freqs, f0c, grad=True)
  limit = b * t * k * k * 4
  for name, fn in (('twm', lambda: losses.TWMLoss()(df, df, da)),
                   ('s2h', lambda: sum(o.sum() for o in core.sinusoidal_to_harmonic(da, df, d0)))):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    out.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    _log('peak_memory/' + name, peak_bytes=peak, limit_bytes=limit)
    assert peak < limit


def _golden_close(case, got, want):
  want = np.asarray(want, np.float64)
  err = float(np.max(np.abs(_np(got).reshape(want.shape) - want))) / max(float(np.max(np.abs(want))), 1e-30)
  _log('golden/' + case, rel_err=err)
  assert err <= SCALAR_RTOL, (case, err)


def test_goldens(ddsp, golden):
  for name in ('consistency_s2h', 'consistency_s2h_normalize'):
    g = golden(name)
    harm_amp, harm_dist = core.sinusoidal_to_harmonic(*_dev(g['sin_amps'], g['sin_freqs'], g['f0_hz']), n_harmonics=g['harm_dist'].shape[-1],
                                                      normalize=bool(g['normalize']))
    _golden_close(name + '/harm_amp', harm_amp, g['harm_amp'])
    _golden_close(name + '/harm_dist', harm_dist, g['harm_dist'])
  for name in ('consistency_twm_own_candidates', 'consistency_twm_c1'):
    g = golden(name)
    loss = losses.TWMLoss()
    args = _dev(g['f0_candidates'], g['freqs'], g['amps'])
    s, h = loss.get_loss_tensors(*args)
    _golden_close(name + '/sinusoids_loss', s, g['sinusoids_loss'])
    _golden_close(name + '/harmonics_loss', h, g['harmonics_loss'])
    _golden_close(name + '/loss', loss(*args), g['loss'])
    # near-ties: the reference's own loss at the candidate chosen here is its minimum to the forward tolerance
    f0 = loss.predict_f0(*args)
    L = (g['sinusoids_loss'] + g['harmonics_loss']).astype(np.float64)
    idx = np.argmin(np.abs(g['f0_candidates'].astype(np.float64) - f0), axis=-1)
    chosen = np.take_along_axis(L, idx[..., None], -1)[..., 0]
    assert np.all((chosen - L.min(-1)) <= SCALAR_RTOL * np.abs(L.min(-1)))
  for name in ('consistency_kde_default', 'consistency_kde_zero_frame', 'consistency_kde_finetune'):
    g = golden(name)
    kw = {k: float(g[k]) for k in ('weight_a', 'weight_b', 'weight_mean_amp', 'scale_a', 'scale_b') if k in g}
    loss = losses.KDEConsistencyLoss(**kw)
    args = _dev(g['amps_a'], g['freqs_a'], g['amps_b'], g['freqs_b'])
    _golden_close(name + '/nll', loss.nll(*args, loss.scale_b), g['nll'])
    _golden_close(name + '/loss', loss(*args), g['loss'])
  g = golden('consistency_thin_losses')
  args = _dev(*[g[k] for k in ('harm_amp', 'harm_amp_target', 'harm_dist', 'harm_dist_target', 'f0_hz', 'f0_hz_target')])
  out = losses.HarmonicConsistencyLoss()(*args)
  for key in ('harm_amp_loss', 'harm_dist_loss', 'f0_hz_loss'):
    _golden_close('thin/' + key, out[key], g[key])
  _golden_close('thin/amp_loss_log', losses.amp_loss(args[2], args[3], log=True), g['amp_loss_log'])
  _golden_close('thin/freq_loss', losses.freq_loss(args[4], args[5]), g['freq_loss'])
  _golden_close('thin/param_loss_l2', losses.ParamLoss(loss_type='L2')(args[2], args[3]), g['param_loss_l2'])


@pytest.fixture(scope='module')
def ddsp():
  import ddsp_amd
  return ddsp_amd
