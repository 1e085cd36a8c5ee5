"""spectral_ops.compute_mel / compute_logmel / compute_mfcc / compute_rms_energy / compute_power and the decibel conversions of
core on the MI355X, against the fp64 truth of tests/features_truth.py, the reference's own fp32 chain (tests/golden/mel_*.npz,
written by tests/golden/make_golden_mel.py) and the reference's unit tests, re-expressed (ddsp/spectral_ops_test.py:141-251).

Tolerances: features_truth.py's docstring - all derived from the 3e-6 max(1, max |X|) compute_mag is held to; rms energy
2e-6 max(1, max rms); power 2e-3 dB.  No element is left out of a comparison; every parity case first asserts, on the truth
alone, that its input keeps the wide log-mel tolerances rare (features_truth.usable).  Determinism: equal bits.
tests/test_features_emulated.py runs the small cases of this file on the CPU emulation of the kernels."""
import numpy as np
import pytest
import torch

import features_truth as T
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = 'cuda'
LOG_FLOOR = float(np.log(1e-5))


@pytest.fixture(scope='module')
def ddsp():
  if DEV == 'cuda':
    if not torch.cuda.is_available():
      pytest.skip('gpu tests need a GPU (run with -m gpu on an MI355X)')
    from ddsp_amd import build
    build.build()
  import ddsp_amd
  return ddsp_amd


def dev(x):
  return torch.as_tensor(np.asarray(x, np.float32), device=DEV)


def npy(t):
  return t.detach().cpu().numpy()


def held(what, ours, truth, tol):
  """max |ours - truth| / tol over EVERY element, printed before it is asserted (a tolerance of 0 asks for equality)."""
  ours = np.asarray(ours, np.float64)
  assert ours.shape == truth.shape, (what, ours.shape, truth.shape)
  assert np.isfinite(ours).all(), what
  err, tol = np.abs(ours - truth), np.broadcast_to(np.asarray(tol, np.float64), truth.shape)
  exact = tol == 0.0                                                  # (an empty mel band: the truth is 0, and so is its tolerance)
  assert np.all(err[exact] == 0.0), '%s: %d elements with a tolerance of 0 are not exact' % (what, int((err[exact] != 0.0).sum()))
  used = float((err[~exact] / tol[~exact]).max()) if (~exact).any() else 0.0
  print('%s: error / tolerance = %.4f' % (what, used))
  assert used <= 1.0, '%s: error is %.3f of the tolerance' % (what, used)


def check_mel_chain(ddsp, audio, lo_hz, hi_hz, bins, fft_size, overlap=0.75, pad_end=True, mfcc_bins=None, what=''):
  """mel, log-mel (and MFCC) of one geometry against the truth."""
  so = ddsp.spectral_ops
  t = T.features(audio, lo_hz, hi_hz, bins, fft_size, overlap, pad_end, mfcc_bins=mfcc_bins)
  print('%s: wide log-mel share %.4f, MFCC tolerance ratio %.4f' % ((what,) + T.usable(t)))
  x = dev(audio)
  held(what + ' mel', npy(so.compute_mel(x, lo_hz, hi_hz, bins, fft_size, overlap, pad_end)), t['mel'], t['tol_mel'])
  held(what + ' logmel', npy(so.compute_logmel(x, lo_hz, hi_hz, bins, fft_size, overlap, pad_end)), t['logmel'], t['tol_log'])
  if mfcc_bins is not None:
    held(what + ' mfcc', npy(so.compute_mfcc(x, lo_hz, hi_hz, fft_size, bins, mfcc_bins, overlap, pad_end)), t['mfcc'],
         t['tol_mfcc'])
  return t


# ---- 1. parity against the fp64 truth ------------------------------------------------------------------------------------
# the z encoder's four geometries (ddsp/training/encoders.py:85-118): fft size and overlap per number of time steps
ENCODER = {'steps250': (1024, 0.75), 'steps500': (512, 0.75), 'steps1000': (256, 0.75), 'steps125': (1024, 0.5)}


@pytest.mark.parametrize('steps', sorted(ENCODER))
def test_encoder_mfcc_geometries(ddsp, steps):
  fft_size, overlap = ENCODER[steps]
  check_mel_chain(ddsp, T.sample_audio(16000, 2, seed=0), 20.0, 8000.0, 128, fft_size, overlap, mfcc_bins=30, what=steps)


def test_pretrain_logmel_229(ddsp):                                  # gin/papers/icml2020/pretrain_model.gin:24-30
  check_mel_chain(ddsp, T.sample_audio(16000, 2, seed=0), 0.0, 8000.0, 229, 2048, what='logmel229')


def test_defaults_of_the_three_functions(ddsp):
  so = ddsp.spectral_ops
  # 31 hops of 512 samples: at 16 000 samples the last zero-padded frame of 2048 holds 128 samples under the foot of the
  # window, all 64 of its bands have a wide tolerance and the share sits AT the 2 % limit (2.00 % at this seed)
  audio = T.sample_audio(15872, 2, seed=1)
  x = dev(audio)
  t = T.features(audio, 0.0, 8000.0, 64, 2048)
  T.usable(t)
  held('compute_mel()', npy(so.compute_mel(x)), t['mel'], t['tol_mel'])
  t = T.features(audio, 80.0, 7600.0, 64, 2048)
  T.usable(t)
  held('compute_logmel()', npy(so.compute_logmel(x)), t['logmel'], t['tol_log'])
  t = T.features(audio, 20.0, 8000.0, 128, 1024, mfcc_bins=13)
  T.usable(t)
  out = so.compute_mfcc(x)
  assert list(out.shape) == [2, 62, 13]
  held('compute_mfcc()', npy(out), t['mfcc'], t['tol_mfcc'])


def test_pad_end_false(ddsp):
  t = check_mel_chain(ddsp, T.sample_audio(16000, 2, seed=2), 20.0, 8000.0, 128, 1024, pad_end=False, mfcc_bins=30, what='valid')
  assert t['mfcc'].shape[1] == 1 + (16000 - 1024) // 256


def test_odd_length_clip(ddsp):
  check_mel_chain(ddsp, T.sample_audio(12345, 2, seed=3), 20.0, 8000.0, 128, 512, mfcc_bins=30, what='n12345')


def test_frame_size_192(ddsp):                                       # not a power of two: a 256-point transform, 129 bins
  check_mel_chain(ddsp, T.sample_audio(8000, 2, seed=4), 80.0, 7600.0, 40, 192, mfcc_bins=13, what='frame192')


def test_input_forms(ddsp):
  so = ddsp.spectral_ops
  audio = T.sample_audio(4000, 2, seed=5)
  full = npy(so.compute_mfcc(dev(audio)))
  assert np.array_equal(npy(so.compute_mfcc(dev(audio)[..., None])), full)
  assert np.array_equal(npy(so.compute_mfcc(audio.astype(np.float64))), full)
  one = so.compute_mfcc(dev(audio[0]))
  assert list(one.shape) == [16, 13] and np.array_equal(npy(one), full[0])
  with pytest.raises(NotImplementedError):
    so.compute_mfcc(dev(audio).requires_grad_(True))
  with pytest.raises(ValueError):
    so.compute_mel(dev(audio), hi_hz=9000.0)


# ---- 2. the reference's own fp32 chain -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['mel_mfcc_fft1024', 'mel_mfcc_fft256', 'mel_logmel_229', 'mel_mel_default', 'mel_logmel_frame192'])
def test_goldens(ddsp, name):
  g = load_golden(name)
  fn = str(g['fn'])
  kw = {k[3:]: v.item() for k, v in g.items() if k.startswith('kw_')}
  ours = npy(getattr(ddsp.spectral_ops, fn)(dev(g['audio']), **kw))
  tkw = dict(kw)
  if fn == 'compute_mfcc':
    t = T.features(g['audio'], tkw['lo_hz'], tkw['hi_hz'], tkw['mel_bins'], tkw['fft_size'], tkw['overlap'], mfcc_bins=tkw['mfcc_bins'])
    key, tol = 'mfcc', t['tol_mfcc']
  else:
    lo, hi = (0.0, 8000.0) if fn == 'compute_mel' else (80.0, 7600.0)
    t = T.features(g['audio'], tkw.get('lo_hz', lo), tkw.get('hi_hz', hi), tkw.get('bins', 64), tkw.get('fft_size', 2048))
    key, tol = ('mel', t['tol_mel']) if fn == 'compute_mel' else ('logmel', t['tol_log'])
  held(name + ' vs truth', ours, t[key], tol)
  held(name + ' vs the reference', ours, g['out'].astype(np.float64), tol)


def test_golden_energy(ddsp):
  so = ddsp.spectral_ops
  g = load_golden('mel_energy')
  for tag, kw in (('default', dict()), ('same', dict(padding='same')), ('valid192', dict(frame_size=192, padding='valid'))):
    rms, pw = npy(so.compute_rms_energy(dev(g['audio']), **kw)), npy(so.compute_power(dev(g['audio']), **kw))
    held('rms ' + tag, rms, g['rms_' + tag].astype(np.float64), T.RMS_C * max(1.0, float(g['rms_' + tag].max())))
    held('power ' + tag, pw, g['power_' + tag].astype(np.float64), T.POWER_TOL_DB)


# ---- 3. rms energy, power and the decibel conversions --------------------------------------------------------------------
@pytest.mark.parametrize('frame_size,padding', [(512, 'center'), (512, 'same'), (512, 'valid'), (192, 'center'), (333, 'same'),
                                                (64, 'valid')])
def test_energy_against_truth(ddsp, frame_size, padding):
  so = ddsp.spectral_ops
  audio = T.sample_audio(16000, 2, seed=6)
  audio[1, 3000:9000] = 0.0                                           # a silent stretch: the floor of the dB scale
  rt = T.rms_energy(audio, frame_size=frame_size, padding=padding)
  held('rms', npy(so.compute_rms_energy(dev(audio), frame_size=frame_size, padding=padding)), rt, T.RMS_C * max(1.0, float(rt.max())))
  pt = T.power(audio, frame_size=frame_size, padding=padding)
  assert pt.min() == -80.0
  held('power', npy(so.compute_power(dev(audio), frame_size=frame_size, padding=padding)), pt, T.POWER_TOL_DB)
  held('power ref 20 range 60', npy(so.compute_power(dev(audio), frame_size=frame_size, ref_db=20.0, range_db=60.0, padding=padding)),
       T.power(audio, frame_size=frame_size, ref_db=20.0, range_db=60.0, padding=padding), T.POWER_TOL_DB)


def sinusoid(sample_rate, seconds, frequency=440.0, amp=0.75):       # spectral_ops_test.py: gen_np_sinusoid
  return (amp * np.sin(2.0 * np.pi * frequency * np.arange(int(sample_rate * seconds)) / sample_rate)).astype(np.float32)


def expected_db_length(ddsp, audio, sample_rate, padding, frame_rate=250, frame_size=512):
  return ddsp.spectral_ops.get_framed_lengths(audio.shape[-1], frame_size, sample_rate // frame_rate, padding)[0]


@pytest.mark.parametrize('sample_rate', [16000, 24000, 44100])
@pytest.mark.parametrize('seconds', [0.21, 0.4])
def test_compute_rms_energy(ddsp, sample_rate, seconds):              # spectral_ops_test.py:215-233
  audio = sinusoid(sample_rate, seconds)
  rms = ddsp.spectral_ops.compute_rms_energy(dev(audio), sample_rate, 250, 512, padding='center')
  assert list(rms.shape) == [expected_db_length(ddsp, audio, sample_rate, 'center')]
  assert np.isfinite(npy(rms)).all()
  rt = T.rms_energy(audio, sample_rate, 250, 512, 'center')[0]
  held('rms of a sinusoid', npy(rms), rt, T.RMS_C * max(1.0, float(rt.max())))


@pytest.mark.parametrize('padding', ['same', 'valid', 'center'])
def test_compute_power_padding(ddsp, padding):                        # spectral_ops_test.py:235-251
  audio = sinusoid(16000, 0.21)
  power = ddsp.spectral_ops.compute_power(dev(audio), 16000, 250, 512, padding=padding)
  assert list(power.shape) == [expected_db_length(ddsp, audio, 16000, padding)]
  assert np.isfinite(npy(power)).all()
  held('power of a sinusoid', npy(power), T.power(audio, 16000, 250, 512, padding=padding)[0], T.POWER_TOL_DB)


def test_batch_compute_power(ddsp):                                   # spectral_ops_test.py:141-162, the compute_power half
  audio = sinusoid(16000, 0.21)
  batch = ddsp.spectral_ops.compute_power(dev(np.tile(audio[None, :], [2, 1])), 16000, 250, 512, padding='same')
  assert list(batch.shape) == [2, expected_db_length(ddsp, audio, 16000, 'same')]
  # a batch and its rows alone agree, at different levels too
  audio = T.sample_audio(16000, 3, seed=8) * np.array([[1.0], [1e-2], [1e-5]], np.float32)
  batch = npy(ddsp.spectral_ops.compute_power(dev(audio), 16000, 250, 512))
  for i in range(3):
    assert np.array_equal(npy(ddsp.spectral_ops.compute_power(dev(audio[i]), 16000, 250, 512)), batch[i])
  assert batch.min() >= -80.0 and batch[2].max() < batch[0].min()


def test_power_is_amplitude_to_db_of_rms(ddsp):
  audio = dev(T.sample_audio(8000, 2, seed=9))
  so, core = ddsp.spectral_ops, ddsp.core
  assert torch.equal(so.compute_power(audio, ref_db=3.0, range_db=70.0), core.amplitude_to_db(so.compute_rms_energy(audio), 3.0, 70.0))


def test_db_conversions(ddsp):                                        # ddsp/core.py:247-277
  core = ddsp.core
  p = np.concatenate([[0.0, 1e-12, 1e-8, 1.0], np.logspace(-9, 3, 200)]).astype(np.float32)
  np.testing.assert_allclose(npy(core.power_to_db(dev(p))), T.power_to_db(p.astype(np.float64)), atol=1e-4)
  np.testing.assert_allclose(npy(core.power_to_db(dev(p), ref_db=20.7, range_db=100.0)),
                             T.power_to_db(p.astype(np.float64), 20.7, 100.0), atol=1e-4)
  np.testing.assert_allclose(npy(core.amplitude_to_db(dev(p))), T.power_to_db(p.astype(np.float64) ** 2), atol=1e-4)
  db = np.linspace(-100.0, 30.0, 261).astype(np.float32)
  np.testing.assert_allclose(npy(core.db_to_power(dev(db))), 10.0 ** (db.astype(np.float64) / 10.0), rtol=2e-6)
  np.testing.assert_allclose(npy(core.db_to_amplitude(dev(db))), 10.0 ** (db.astype(np.float64) / 20.0), rtol=2e-6)
  assert list(core.power_to_db(dev(np.ones((2, 3, 4)))).shape) == [2, 3, 4]
  with pytest.raises(NotImplementedError):
    core.power_to_db(dev(p).requires_grad_(True))


# ---- 4. silence and empty bands ------------------------------------------------------------------------------------------
def test_silence(ddsp):
  so = ddsp.spectral_ops
  x = torch.zeros((2, 4000), device=DEV)
  logmel = npy(so.compute_logmel(x, 20.0, 8000.0, 128, 1024))
  assert np.all(logmel == logmel.flat[0]) and abs(float(logmel.flat[0]) - LOG_FLOOR) <= 2e-6 * abs(LOG_FLOOR)
  assert np.all(npy(so.compute_mel(x)) == 0.0)
  mfcc = npy(so.compute_mfcc(x, mel_bins=128, mfcc_bins=30)).astype(np.float64)
  d = np.abs(T.dct_matrix(128, 30))
  tol = 2.0 * 2e-6 * abs(LOG_FLOOR) * d.sum(axis=1)                    # tol_log = 2e-6 |L| and the DCT's own 2e-6 sum |D| |L|
  expected = np.zeros(30)
  expected[0] = np.sqrt(2.0 * 128) * LOG_FLOOR
  held('silent mfcc', mfcc, np.broadcast_to(expected, mfcc.shape), np.broadcast_to(tol, mfcc.shape))
  assert np.all(npy(so.compute_rms_energy(x)) == 0.0) and np.all(npy(so.compute_power(x)) == -80.0)


def test_empty_mel_columns_sit_on_the_floor(ddsp):
  """fft 256, 128 bins from 20 Hz: 13 bands are narrower than a bin - all-zero columns - and give exactly safe_log's floor in
  noisy audio too, the value core.safe_log itself gives for 0."""
  so = ddsp.spectral_ops
  audio = T.sample_audio(4000, 2, seed=10)
  empty = ~T.mel_matrix(128, 129, 16000, 20.0, 8000.0).any(axis=0)
  assert empty.sum() == 13
  assert np.all(npy(so.compute_mel(dev(audio), 20.0, 8000.0, 128, 256))[..., empty] == 0.0)
  logmel = npy(so.compute_logmel(dev(audio), 20.0, 8000.0, 128, 256))
  floor = npy(ddsp.core.safe_log(torch.zeros(1, device=DEV)))[0]
  assert np.all(logmel[..., empty] == floor) and np.all(logmel[..., ~empty] > floor)


# ---- 5. determinism ------------------------------------------------------------------------------------------------------
def test_determinism(ddsp):
  so = ddsp.spectral_ops
  x = dev(T.sample_audio(16000, 3, seed=11))
  for fn, kw in ((so.compute_mfcc, dict(mfcc_bins=30)), (so.compute_logmel, dict(bins=229, lo_hz=0.0, hi_hz=8000.0)),
                 (so.compute_mel, dict()), (so.compute_rms_energy, dict()), (so.compute_power, dict())):
    first = fn(x, **kw)
    assert torch.equal(fn(x, **kw), first)
    assert torch.equal(fn(x[1:2].contiguous(), **kw)[0], first[1])


# ---- 6. nothing of the size of the magnitudes ----------------------------------------------------------------------------
def test_peak_memory(ddsp):
  """Batch 32 x 64 000 samples, fft 1024: across compute_mfcc the allocator's peak grows by less than the [32, 250, 513]
  magnitudes the composed path builds."""
  so = ddsp.spectral_ops
  x = dev(T.sample_audio(64000, 32, seed=12))
  so.compute_mfcc(x, mfcc_bins=30)                                    # (tables made and cached)
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  before = torch.cuda.max_memory_allocated()
  out = so.compute_mfcc(x, mfcc_bins=30)
  torch.cuda.synchronize()
  growth = torch.cuda.max_memory_allocated() - before
  mag_bytes = 32 * 250 * 513 * 4
  print('peak growth %d bytes, magnitudes %d bytes, output %d bytes' % (growth, mag_bytes, out.numel() * 4))
  assert list(out.shape) == [32, 250, 30]
  assert growth < mag_bytes
  assert growth <= 2 * out.numel() * 4


def test_full_length_batch(ddsp):
  """The encoder's own shape, 64 000 samples (batch 4): rows agree with the same rows alone, and with the truth."""
  audio = T.sample_audio(64000, 4, seed=13)
  out = ddsp.spectral_ops.compute_mfcc(dev(audio), mfcc_bins=30)
  assert list(out.shape) == [4, 250, 30]
  t = T.features(audio[:1], 20.0, 8000.0, 128, 1024, mfcc_bins=30)
  T.usable(t)
  held('64000 samples', npy(out[:1]), t['mfcc'], t['tol_mfcc'])


# ---- 7. beyond the fused limits: the general chain -----------------------------------------------------------------------
def test_fallback_beyond_the_limits(ddsp):
  so = ddsp.spectral_ops
  audio = T.sample_audio(4000, 2, seed=14)
  # more MFCCs than mel bins: mfccs[..., :mfcc_bins] keeps what there is
  assert not so.mel_fused_limits(1024, 40, 60) and so.mel_fused_limits(1024, 40, 40)
  t = T.features(audio, 20.0, 8000.0, 40, 1024, mfcc_bins=60)
  T.usable(t)
  out = so.compute_mfcc(dev(audio), mel_bins=40, mfcc_bins=60)
  assert list(out.shape) == [2, 16, 40]
  held('mfcc_bins > mel_bins', npy(out), t['mfcc'], t['tol_mfcc'])
  # more mel bins than the transform has points (most of them empty): held to the same tolerances, element by element
  assert not so.mel_fused_limits(64, 80) and so.mel_fused_limits(64, 64)
  t = T.features(audio, 0.0, 8000.0, 80, 64)
  held('bins > fft size, mel', npy(so.compute_mel(dev(audio), 0.0, 8000.0, 80, 64)), t['mel'], t['tol_mel'])
  held('bins > fft size, logmel', npy(so.compute_logmel(dev(audio), 0.0, 8000.0, 80, 64)), t['logmel'], t['tol_log'])
  # and the fused kernel at its limit agrees with the truth as well
  t = T.features(audio, 0.0, 8000.0, 64, 64)
  held('bins == fft size', npy(so.compute_logmel(dev(audio), 0.0, 8000.0, 64, 64)), t['logmel'], t['tol_log'])
