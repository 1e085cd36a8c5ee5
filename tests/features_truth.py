"""fp64 truth for the mel / log-mel / MFCC / rms-energy / power functions of ddsp_amd/spectral_ops.py, and the tolerances the
tests hold them to (tests/test_gpu_features.py, tests/golden/make_golden_mel.py).

Framing and |STFT| are the oracle's (oracle.ddsp_oracle.compute_mag at dtype float64).  The two TensorFlow functions are
restated from TensorFlow's published source:
  * tf.signal.linear_to_mel_weight_matrix: HTK mel scale 1127 ln(1 + f / 700); spectrogram bins linspace(0, sr / 2, n)[1:] (the
    DC bin is dropped and returns as a row of zeros); bins + 2 band edges equally spaced in mel; weight
    max(0, min((mel_k - lo) / (centre - lo), (hi - mel_k) / (hi - centre))); computed in float64, CAST TO FLOAT32 (the matrix
    the reference multiplies by), then used here in fp64;
  * tf.signal.mfccs_from_log_mel_spectrograms: 2 sum_n x[n] cos(pi k (2 n + 1) / (2 N)) / sqrt(2 N).

Tolerances, all from the figure compute_mag is held to, 3e-6 max(1, max |X|) (tests/test_gpu_reference_tests.py):
  s = max(1, max mag_truth)
  mel      tol_mel[m] = 3e-6 s sum_k W[k, m] + 1e-6 mel_truth[m]
  log-mel  tol_log[m] = log1p(tol_mel[m] / max(mel_truth[m] - tol_mel[m], 1e-5)) + 2e-6 max(1, |logmel_truth[m]|)
  MFCC     tol[k]     = sum_m |D[k, m]| tol_log[m] + 2e-6 sum_m |D[k, m]| |logmel_truth[m]|
  rms      2e-6 max(1, max rms);  power 2e-3 dB.
The log-mel tolerance is wide where a band holds almost no energy, so the inputs must keep that rare: usable() asserts, on
the truth alone, that at most 2 % of the log-mel elements have tol_log > 1e-2 and that the largest MFCC tolerance is at most
1 % of max |mfcc_truth|."""
import numpy as np

from oracle import ddsp_oracle as O

POWER_TOL_DB = 2e-3
RMS_C = 2e-6


def hz_to_mel(hz):
  return 1127.0 * np.log(1.0 + np.asarray(hz, np.float64) / 700.0)


def mel_matrix(bins, n_spectrogram_bins, sample_rate, lo_hz, hi_hz):
  """[n_spectrogram_bins, bins] float32."""
  spec = hz_to_mel(np.linspace(0.0, sample_rate / 2.0, n_spectrogram_bins)[1:])[:, None]
  edges = np.linspace(hz_to_mel(lo_hz), hz_to_mel(hi_hz), bins + 2)
  lo, centre, hi = edges[None, :-2], edges[None, 1:-1], edges[None, 2:]
  w = np.maximum(0.0, np.minimum((spec - lo) / (centre - lo), (hi - spec) / (hi - centre)))
  return np.concatenate([np.zeros((1, bins)), w], axis=0).astype(np.float32)


def dct_matrix(mel_bins, mfcc_bins):
  """[mfcc_bins, mel_bins] float64."""
  k = np.arange(mfcc_bins, dtype=np.float64)[:, None]
  n = np.arange(mel_bins, dtype=np.float64)[None, :]
  return 2.0 * np.cos(np.pi * k * (2.0 * n + 1.0) / (2.0 * mel_bins)) / np.sqrt(2.0 * mel_bins)


def sample_audio(n=16000, batch=2, seed=0, sample_rate=16000):
  """Broadband noise over a tone, 0.3 randn + 0.4 sin(2 pi 440 t): every mel band holds energy."""
  rng = np.random.default_rng(seed)
  t = np.arange(n) / float(sample_rate)
  return (0.3 * rng.standard_normal((batch, n)) + 0.4 * np.sin(2.0 * np.pi * 440.0 * t)[None, :]).astype(np.float32)


def features(audio, lo_hz, hi_hz, bins, fft_size, overlap=0.75, pad_end=True, sample_rate=16000, mfcc_bins=None):
  """dict: mag, mel, logmel (and mfcc) in fp64 with tol_mel, tol_log (and tol_mfcc), W (float32) and D."""
  audio = np.asarray(audio, np.float32)
  if audio.ndim == 1:
    audio = audio[None, :]
  mag = O.compute_mag(audio, fft_size, overlap, pad_end, dtype=np.float64)
  w = mel_matrix(bins, mag.shape[-1], sample_rate, lo_hz, hi_hz)
  mel = mag @ w.astype(np.float64)
  logmel = O.safe_log(mel)
  s = max(1.0, float(mag.max())) if mag.size else 1.0
  tol_mel = 3e-6 * s * w.astype(np.float64).sum(axis=0) + 1e-6 * mel
  tol_log = np.log1p(tol_mel / np.maximum(mel - tol_mel, 1e-5)) + 2e-6 * np.maximum(1.0, np.abs(logmel))
  out = dict(mag=mag, W=w, mel=mel, logmel=logmel, tol_mel=tol_mel, tol_log=tol_log)
  if mfcc_bins is not None:
    d = dct_matrix(bins, min(mfcc_bins, bins))
    out['D'] = d
    out['mfcc'] = logmel @ d.T
    out['tol_mfcc'] = tol_log @ np.abs(d).T + 2e-6 * (np.abs(logmel) @ np.abs(d).T)
  return out


def usable(t):
  """The two conditions on the truth that keep the wide tolerances rare; returns the two figures."""
  share = float(np.mean(t['tol_log'] > 1e-2))
  assert share <= 0.02, 'a share of %.4f of the log-mel elements has a tolerance above 1e-2: not a usable input' % share
  ratio = 0.0
  if 'mfcc' in t:
    ratio = float(t['tol_mfcc'].max() / np.abs(t['mfcc']).max())
    assert ratio <= 0.01, 'the largest MFCC tolerance is %.4f of max |mfcc|: not a usable input' % ratio
  return share, ratio


def _framed(audio, frame_size, hop, padding):
  audio = np.asarray(audio, np.float64)
  if audio.ndim == 1:
    audio = audio[None, :]
  n = audio.shape[1]
  if padding == 'center':
    audio = np.pad(audio, ((0, 0), (frame_size // 2, frame_size // 2)))
  elif padding == 'same':
    n_frames = -(-n // hop)
    audio = np.pad(audio, ((0, 0), (0, (n_frames - 1) * hop + frame_size - n)))
  elif padding != 'valid':
    raise ValueError(padding)
  length = audio.shape[1]
  n_frames = 1 + (length - frame_size) // hop if length >= frame_size else 0
  idx = np.arange(n_frames)[:, None] * hop + np.arange(frame_size)[None, :]
  return audio[:, idx]


def rms_energy(audio, sample_rate=16000, frame_rate=250, frame_size=512, padding='center'):
  frames = _framed(audio, frame_size, sample_rate // frame_rate, padding)
  return np.sqrt(np.mean(frames ** 2, axis=-1))


def power_to_db(power, ref_db=0.0, range_db=80.0):
  pmin = 10.0 ** -(range_db / 10.0)
  return np.maximum(10.0 * np.log10(np.maximum(pmin, power)) - ref_db, -range_db)


def power(audio, sample_rate=16000, frame_rate=250, frame_size=512, ref_db=0.0, range_db=80.0, padding='center'):
  return power_to_db(rms_energy(audio, sample_rate, frame_rate, frame_size, padding) ** 2, ref_db, range_db)
