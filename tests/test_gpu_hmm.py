"""losses.HmmTranscriber on the MI355X against tests/hmm_truth.py (the dense model in fp64 at the fp32 inputs).
tests/test_hmm_emulated.py runs this module through the SIMT emulation on the CPU.

Tolerances (as tests/test_gpu_wasserstein.py applies them): the scalar nll 5e-5 relative; gradients 2e-4
of the largest element of each gradient; per-row log-probabilities: the kernel's error against the fp64 truth may be up to
4 x that of the truth helper's fp32 mode on the same case, with a floor of eight fp32 ulp of the largest magnitude.  The
decoded path must equal the truth's at every step, and its fp64 score must lie within eight fp32 ulp of the optimum.  Every
comparison is appended to the file DDSP_PARITY_LOG names, when it is set.

Shapes (n_pitches, steps) at batch 2, the smallest at which each part of the kernels can go wrong: no transition at all; the
smallest model with transitions; small odd sizes; one wavefront of states exactly; one state past it; the shipped state
count; the shipped shape (the fp64 scale accumulation over a full clip, 16 chunks of observations, 32 words of back-trace
bits); past the 256 states of the one-wavefront kernel; the bound.

Measured on the MI355X (profiles/hmm_parity_errors.jsonl): log_prob at 128 x 1000 off by 5.6e-8 relative, the dense fp32
recursion by 5.2e-6; largest over all cases: rows 1.1e-7, scalars 7.6e-8, gradients 2.1e-7; no path mismatch."""
import functools
import json
import os
import zlib

import numpy as np
import pytest
import torch

import hmm_truth as T
from ddsp_amd import losses

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SCALAR_RTOL = 5e-5
GRAD_RTOL = 2e-4
TENSOR_RATIO = 4.0
TENSOR_FLOOR = 8 * 2.0 ** -24          # eight fp32 ulp of the tensor's largest magnitude
BATCH = 2

# (n_pitches, steps)
SHAPES = [(2, 1), (2, 6), (5, 7), (64, 33), (65, 9), (128, 64), (128, 1000), (257, 12), (1024, 4)]
IDS = ['n%d_t%d' % s for s in SHAPES]
# The cases are seeded by name; where seed 0 of a short case gives a row whose most likely path (the TRUTH's) never changes
# state - a single note, or silence throughout - the first seed that makes both rows change is named here.
SEEDS = {(2, 6): 3, (5, 7): 1}
OTHER_MODEL = dict(avg_length=20, midi_std=1.0, amps_on_center=1.2, amps_on_scale=0.4, amps_off_center=0.1, amps_off_scale=0.2)


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


@functools.lru_cache(maxsize=None)
def _case(n_pitches, steps, model=(), far=False):
  """The inputs of a case and everything the truth says about them, computed once and never changed."""
  kwargs = dict(model)
  name = 'hmm/n%d_t%d/%s%s' % (n_pitches, steps, 'other' if kwargs else 'default', '/far' if far else '')
  rng = np.random.default_rng(zlib.crc32(('%s/%d' % (name, SEEDS.get((n_pitches, steps), 0))).encode()))
  pitch, amps = T.make_notes(rng, BATCH, steps, n_pitches)
  if far:
    amps[0, 5], pitch[0, 20], pitch[1, 40] = 50.0, -300.0, 1000.0
  cot = rng.standard_normal(BATCH).astype(np.float32)
  case = dict(name=name, pitch=pitch, amps=amps, cot=cot, kwargs=kwargs)
  case['log_prob'] = T.log_prob(pitch, amps, n_pitches, **kwargs).numpy()
  case['log_prob_fp32'] = T.log_prob(pitch, amps, n_pitches, dtype=torch.float32, **kwargs).numpy().astype(np.float64)
  case['nll'] = float(T.nll(pitch, amps, n_pitches, weight=0.7, **kwargs))
  fn = lambda p, a: T.nll(p, a, n_pitches, weight=0.7, per_example_loss=True, **kwargs)
  case['grads'] = T.grads(fn, (pitch, amps), (cot,))
  case['grads_scalar'] = T.grads(lambda p, a: T.nll(p, a, n_pitches, weight=0.7, **kwargs), (pitch, amps))
  path, score = T.viterbi(pitch, amps, n_pitches, **kwargs)
  case['path'], case['score'] = path.numpy(), score.numpy()
  return case


def _hmm(n_pitches, steps, kwargs, weight=0.7):
  return losses.HmmTranscriber(n_timesteps=steps, n_pitches=n_pitches, weight=weight, **kwargs)


def _check_rows(case, got, truth, faithful):
  scale = float(np.max(np.abs(truth)))
  scale = scale if scale > 0.0 else 1.0
  err = float(np.max(np.abs(got - truth))) / scale
  ref_err = float(np.max(np.abs(faithful - truth))) / scale
  _log(case, kernel_err=err, reference_fp32_err=ref_err, scale=scale)
  assert got.shape == truth.shape and np.isfinite(got).all()
  assert err <= max(TENSOR_RATIO * ref_err, TENSOR_FLOOR), (case, err, ref_err)


def _check_scalar(case, got, truth):
  got = float(got.detach())
  err = abs(got - float(truth)) / max(abs(float(truth)), 1e-30)
  _log(case, scalar_rel_err=err)
  assert np.isfinite(got) and err <= SCALAR_RTOL, (case, got, float(truth))


def _check_grads(case, got, truth):
  """2e-4 of the largest element of each gradient."""
  for i, (g, t) in enumerate(zip(got, truth)):
    g = _np(g)
    scale = max(float(np.max(np.abs(t))), 1e-30)
    err = float(np.max(np.abs(g - t))) / scale
    _log('%s/grad%d' % (case, i), grad_err=err, scale=scale)
    assert g.shape == t.shape and np.isfinite(g).all()
    assert err <= GRAD_RTOL, (case, i, err)


def _check_values_and_grads(c, n_pitches, steps):
  hmm = _hmm(n_pitches, steps, c['kwargs'])
  pitch, amps = _dev(c['pitch'], c['amps'], grad=True)
  with torch.no_grad():
    plain = hmm.nll(pitch, amps, per_example_loss=True)                  # the forward-only route
  rows = hmm.nll(pitch, amps, per_example_loss=True)
  assert rows.shape == (BATCH,) and rows.requires_grad and not plain.requires_grad and torch.equal(rows.detach(), plain)
  to_log_prob = -steps / 0.7
  _check_rows(c['name'] + '/log_prob', _np(rows) * to_log_prob, c['log_prob'], c['log_prob_fp32'])
  scalar = hmm(pitch, amps)
  assert scalar.shape == ()
  _check_scalar(c['name'] + '/nll', scalar, c['nll'])
  _check_grads(c['name'] + '/rows', torch.autograd.grad(rows, (pitch, amps), _dev(c['cot'])[0]), c['grads'])
  _check_grads(c['name'] + '/scalar', torch.autograd.grad(scalar, (pitch, amps)), c['grads_scalar'])


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_log_prob_and_gradients(ddsp, shape):
  _check_values_and_grads(_case(*shape), *shape)


def test_log_prob_and_gradients_other_model(ddsp):
  _check_values_and_grads(_case(128, 64, tuple(sorted(OTHER_MODEL.items()))), 128, 64)


def test_far_inputs_are_finite_and_accurate(ddsp):
  """amps = 50, pitch = -300 and pitch = 1000 on three steps: no state is near, nothing underflows, nothing is NaN."""
  c = _case(128, 64, far=True)
  assert c['amps'][0, 5] == 50.0 and c['pitch'][0, 20] == -300.0 and c['pitch'][1, 40] == 1000.0
  assert np.isfinite(c['log_prob']).all() and all(np.isfinite(g).all() for g in c['grads'])
  _check_values_and_grads(c, 128, 64)


def _check_viterbi(c, n_pitches, steps):
  hmm = _hmm(n_pitches, steps, c['kwargs'])
  pitch, amps = _dev(c['pitch'], c['amps'])
  got = hmm.predict_midi(pitch, amps, channel_dim=False, dtype=torch.int64).cpu().numpy()
  assert got.shape == (BATCH, steps) and got.min() >= 0 and got.max() < n_pitches
  if steps >= 6:
    assert all((np.diff(row) != 0).any() for row in c['path']), 'the case must make the decoded path change state'
  score = T.path_score(got, c['pitch'], c['amps'], n_pitches, **c['kwargs']).numpy()
  deficit = float(np.max((c['score'] - score) / np.abs(c['score'])))
  mismatches = int((got != c['path']).sum())
  _log(c['name'] + '/viterbi', score_deficit=deficit, mismatches=mismatches)
  assert deficit <= TENSOR_FLOOR, (c['name'], deficit)
  assert mismatches == 0, (c['name'], mismatches)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_viterbi(ddsp, shape):
  _check_viterbi(_case(*shape), *shape)


def test_viterbi_other_model(ddsp):
  _check_viterbi(_case(128, 64, tuple(sorted(OTHER_MODEL.items()))), 128, 64)


def test_silence_decodes_to_state_zero(ddsp):
  """A stretch of silent steps (amps 0, any pitch) between two notes is state 0; the notes are their pitches."""
  steps = 48
  rng = np.random.default_rng(31)
  pitch, amps = np.zeros((1, steps, 1), np.float32), np.zeros((1, steps, 1), np.float32)
  pitch[0, :16, 0], amps[0, :16, 0] = 60.0 + rng.uniform(-0.2, 0.2, 16), 1.5
  pitch[0, 16:32, 0], amps[0, 16:32, 0] = rng.uniform(0.0, 128.0, 16), rng.normal(0.0, 0.02, 16)
  pitch[0, 32:, 0], amps[0, 32:, 0] = 72.0 + rng.uniform(-0.2, 0.2, 16), 1.5
  got = _hmm(128, steps, {}).predict_midi(*_dev(pitch, amps), channel_dim=False, dtype=torch.int32).cpu().numpy()[0]
  assert (got[:16] == 60).all() and (got[16:32] == 0).all() and (got[32:] == 72).all()
  assert np.array_equal(got, T.viterbi(pitch, amps, 128)[0].numpy()[0])


def test_predict_midi_shape_dtype_and_no_grad(ddsp):
  c = _case(5, 7)
  hmm = _hmm(5, 7, {})
  pitch, amps = _dev(c['pitch'], c['amps'], grad=True)
  for channel_dim, dtype in ((True, torch.float32), (False, torch.float32), (True, torch.int32), (False, torch.float64)):
    out = hmm.predict_midi(pitch, amps, channel_dim=channel_dim, dtype=dtype)
    assert out.shape == ((BATCH, 7, 1) if channel_dim else (BATCH, 7)) and out.dtype is dtype and not out.requires_grad
    assert np.array_equal(out.reshape(BATCH, 7).cpu().numpy().astype(np.int64), c['path'])
  assert hmm.predict_midi(pitch, amps).dtype is torch.float32 and hmm.predict_midi(pitch, amps).shape == (BATCH, 7, 1)
  # numpy and float64 inputs, as tf_float32 takes them
  out = hmm.predict_midi(c['pitch'].astype(np.float64), torch.as_tensor(c['amps'], dtype=torch.float64), channel_dim=False)
  assert np.array_equal(out.cpu().numpy().astype(np.int64), c['path'])
  _check_scalar('inputs/numpy_float64', hmm.nll(c['pitch'].astype(np.float64), c['amps']), c['nll'])
  # the straight-through estimate: the decoded values, the gradient of the pitch
  quant = hmm.predict_midi(pitch, amps)
  through = losses.HmmTranscriber.straight_through(pitch, quant)
  assert torch.allclose(through, quant, rtol=0.0, atol=1e-5)
  assert torch.equal(torch.autograd.grad(through.sum(), pitch)[0], torch.ones_like(pitch))


def _everything(hmm, pitch, amps):
  pitch, amps = _dev(pitch, amps, grad=True)
  rows = hmm.nll(pitch, amps, per_example_loss=True)
  cot = torch.linspace(0.5, 1.5, 3, device=DEV)[:rows.shape[0]]
  return [rows.detach()] + list(torch.autograd.grad(rows, (pitch, amps), cot)) + [hmm.predict_midi(pitch, amps, dtype=torch.int32)]


@pytest.mark.parametrize('shape', [(65, 9), (128, 64), (257, 12)], ids=['n65_t9', 'n128_t64', 'n257_t12'])
def test_same_bits_twice_row_alone_and_in_the_batch(ddsp, shape):
  n_pitches, steps = shape
  rng = np.random.default_rng(zlib.crc32(('hmm/bits/n%d_t%d' % shape).encode()))
  pitch, amps = T.make_notes(rng, 3, steps, n_pitches)
  hmm = _hmm(n_pitches, steps, {})
  first, second = _everything(hmm, pitch, amps), _everything(hmm, pitch, amps)
  for a, b in zip(first, second):
    assert torch.equal(a, b)
  alone = _everything(hmm, pitch[:1], amps[:1])
  for a, r in zip(first, alone):
    assert torch.equal(a[:1], r)


@pytest.fixture(scope='module')
def ddsp():
  import ddsp_amd
  return ddsp_amd
