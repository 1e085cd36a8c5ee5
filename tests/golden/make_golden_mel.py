"""Generate tests/golden/mel_*.npz by running the REFERENCE'S OWN spectral_ops.py / core.py on the numpy TensorFlow stand-in of
tf_numpy_shim.py (see make_golden.py).

    python tests/golden/make_golden_mel.py          (needs the reference checkout; DDSP_REFERENCE_ROOT)
    python tests/golden/make_golden_mel.py --tf     (where `import tensorflow` works: the same cases under the real
                                                     tf.signal functions, compared with the committed fixtures, nothing written)

The stand-in has no tf.signal.linear_to_mel_weight_matrix, no tf.signal.mfccs_from_log_mel_spectrograms, no tf.tensordot and no
TensorShape.concatenate: they are supplied here at run time, on the module the reference imports.  The two tf.signal functions
are restated from TensorFlow's published source (python/ops/signal/mel_ops.py, mfcc_ops.py), step by step in the order and the
dtype of that source: the mel matrix in float64 and cast to float32 at the end, the DCT as tf.signal.dct type 2 (float32)
times rsqrt(2 N).  TensorFlow is not needed - and cannot be run - where these fixtures are made; --tf pins the restatement
wherever it exists.

Clips of 4000 samples, batch 2, broadband (tests/features_truth.py::sample_audio).  Every fixture is checked against the fp64
truth before it is written: one that the reference's fp32 chain does not hold to the tolerances of features_truth.py with a
factor of 2.8 to spare is refused."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import features_truth as T  # noqa: E402

ROOM = 2.8
N = 4000

MEL_CASES = {
    # name: (function, keyword arguments)
    'mel_mfcc_fft1024': ('compute_mfcc', dict(lo_hz=20.0, hi_hz=8000.0, fft_size=1024, mel_bins=128, mfcc_bins=30, overlap=0.75)),
    'mel_mfcc_fft256': ('compute_mfcc', dict(lo_hz=20.0, hi_hz=8000.0, fft_size=256, mel_bins=128, mfcc_bins=30, overlap=0.75)),
    'mel_logmel_229': ('compute_logmel', dict(lo_hz=0.0, hi_hz=8000.0, bins=229, fft_size=2048)),
    'mel_mel_default': ('compute_mel', dict()),
    'mel_logmel_frame192': ('compute_logmel', dict(bins=40, fft_size=192)),
}
TABLES = {
    'mel': [(128, 513, 16000, 20.0, 8000.0), (128, 129, 16000, 20.0, 8000.0), (229, 1025, 16000, 0.0, 8000.0),
            (64, 1025, 16000, 80.0, 7600.0)],
    'dct': [(128, 30), (128, 13), (64, 64)],
}


def a(x):
  return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


def truth_of(fn, audio, kw):
  kw = dict(kw)
  if fn == 'compute_mfcc':
    return T.features(audio, kw.pop('lo_hz', 20.0), kw.pop('hi_hz', 8000.0), kw.pop('mel_bins', 128), kw.pop('fft_size', 1024),
                      kw.pop('overlap', 0.75), mfcc_bins=kw.pop('mfcc_bins', 13))
  lo, hi = (0.0, 8000.0) if fn == 'compute_mel' else (80.0, 7600.0)
  return T.features(audio, kw.pop('lo_hz', lo), kw.pop('hi_hz', hi), kw.pop('bins', 64), kw.pop('fft_size', 2048),
                    kw.pop('overlap', 0.75))


def held(fn, out, t, room):
  key = {'compute_mel': 'mel', 'compute_logmel': 'logmel', 'compute_mfcc': 'mfcc'}[fn]
  tol = t['tol_' + ('log' if key == 'logmel' else key)]
  return float((np.abs(np.asarray(out, np.float64) - t[key]) / tol).max()) * room


def install_shim():
  import tf_numpy_shim
  if os.environ.get('DDSP_REFERENCE_ROOT'):
    tf_numpy_shim.install(os.environ['DDSP_REFERENCE_ROOT'])
  else:
    tf_numpy_shim.install()
  v2 = sys.modules['tensorflow.compat.v2']
  shape_cls, tensor_cls = tf_numpy_shim.TensorShape, tf_numpy_shim.Tensor

  def _t(x):
    return np.asarray(x).view(tensor_cls)

  # mag.shape[:-1].concatenate(matrix.shape[-1:]) and mel.set_shape(...)
  plain_getitem = tuple.__getitem__
  shape_cls.__getitem__ = lambda self, i: shape_cls(plain_getitem(self, i)) if isinstance(i, slice) else plain_getitem(self, i)
  shape_cls.concatenate = lambda self, other: shape_cls(tuple(self) + tuple(other))
  tensor_cls.set_shape = lambda self, shape: None

  def linear_to_mel_weight_matrix(num_mel_bins=20, num_spectrogram_bins=129, sample_rate=8000, lower_edge_hertz=125.0,
                                  upper_edge_hertz=3800.0, dtype=np.float32):
    # mel_ops.py: everything in float64, the result cast to `dtype`
    def hz_to_mel(f):
      return 1127.0 * np.log(1.0 + f / 700.0)
    nyquist = np.float64(sample_rate) / 2.0
    linear = np.linspace(0.0, nyquist, num_spectrogram_bins, dtype=np.float64)[1:]          # bands_to_zero = 1
    spec_mel = hz_to_mel(linear)[:, None]
    edges = np.linspace(hz_to_mel(np.float64(lower_edge_hertz)), hz_to_mel(np.float64(upper_edge_hertz)), num_mel_bins + 2)
    triples = np.stack([edges[i:i + 3] for i in range(num_mel_bins)])                         # shape_ops.frame(edges, 3, 1)
    lower, center, upper = (triples[:, i][None, :] for i in range(3))
    lower_slopes = (spec_mel - lower) / (center - lower)
    upper_slopes = (upper - spec_mel) / (upper - center)
    weights = np.maximum(0.0, np.minimum(lower_slopes, upper_slopes))
    return _t(np.pad(weights, [[1, 0], [0, 0]]).astype(dtype))

  def mfccs_from_log_mel_spectrograms(log_mel_spectrograms):
    # mfcc_ops.py: dct(x, type=2) * rsqrt(num_mel_bins * 2.0); tf.signal.dct type 2, norm=None: 2 sum_n x[n] cos(pi k (2n + 1) / 2N)
    x = np.asarray(log_mel_spectrograms, np.float32)
    n_bins = x.shape[-1]
    k = np.arange(n_bins, dtype=np.float64)[:, None]
    n = np.arange(n_bins, dtype=np.float64)[None, :]
    basis = (2.0 * np.cos(np.pi * k * (2.0 * n + 1.0) / (2.0 * n_bins))).astype(np.float32)
    dct2 = np.matmul(x, basis.T)
    return _t(dct2 * np.float32(1.0 / np.sqrt(np.float32(n_bins * 2.0))))

  v2.signal.linear_to_mel_weight_matrix = linear_to_mel_weight_matrix
  v2.signal.mfccs_from_log_mel_spectrograms = mfccs_from_log_mel_spectrograms
  v2.tensordot = lambda x, y, axes: _t(np.tensordot(np.asarray(x), np.asarray(y), axes))
  return v2


def run_shim():
  v2 = install_shim()
  from ddsp import spectral_ops  # noqa: E402  (the reference's file)
  audio = T.sample_audio(N, 2, seed=0)
  for name, (fn, kw) in MEL_CASES.items():
    out = a(getattr(spectral_ops, fn)(audio, **kw))
    t = truth_of(fn, audio, kw)
    share, ratio = T.usable(t)
    used = held(fn, out, t, ROOM)
    print('%-24s %-15s %s reference / tolerance x %.1f = %.3f (wide log-mel share %.4f, MFCC tol ratio %.4f)'
          % (name, fn, out.shape, ROOM, used, share, ratio))
    assert used <= 1.0, 'the reference itself does not hold the tolerance with room: not a usable fixture'
    np.savez_compressed(os.path.join(HERE, name + '.npz'), audio=audio, out=out, fn=fn,
                        **{'kw_' + k: v for k, v in kw.items()})
  # rms energy and power (spectral_ops_test.py's shapes: frame 512 at 250 frames per second; and a frame of 192)
  arrays = {'audio': audio}
  for tag, kw in (('default', dict()), ('same', dict(padding='same')), ('valid192', dict(frame_size=192, padding='valid'))):
    rms = a(spectral_ops.compute_rms_energy(audio, **kw))
    pw = a(spectral_ops.compute_power(audio, **kw))
    rt, pt = T.rms_energy(audio, **kw), T.power(audio, **kw)
    e_rms = float(np.abs(rms - rt).max()) / (T.RMS_C * max(1.0, float(rt.max())))
    e_pw = float(np.abs(pw - pt).max()) / T.POWER_TOL_DB
    print('mel_energy %-10s rms %s reference / tolerance x %.1f = %.3f, power %.3f' % (tag, rms.shape, ROOM, e_rms * ROOM, e_pw * ROOM))
    assert e_rms * ROOM <= 1.0 and e_pw * ROOM <= 1.0
    arrays['rms_' + tag], arrays['power_' + tag] = rms, pw
  np.savez_compressed(os.path.join(HERE, 'mel_energy.npz'), **arrays)
  # the tables themselves
  arrays = {}
  for key in TABLES['mel']:
    arrays['mel_%d_%d_%d_%g_%g' % key] = a(v2.signal.linear_to_mel_weight_matrix(*key))
  for mel_bins, mfcc_bins in TABLES['dct']:
    eye = np.eye(mel_bins, dtype=np.float32)
    arrays['dct_%d_%d' % (mel_bins, mfcc_bins)] = a(v2.signal.mfccs_from_log_mel_spectrograms(eye)).T[:mfcc_bins]
  np.savez_compressed(os.path.join(HERE, 'mel_tables.npz'), **arrays)


def run_tf():
  """The same cases under the real tf.signal functions, against the committed fixtures."""
  import tensorflow as tf

  def chain(fn, audio, kw):
    kw = dict(kw)
    mfcc = fn == 'compute_mfcc'
    lo, hi = (20.0, 8000.0) if mfcc else ((0.0, 8000.0) if fn == 'compute_mel' else (80.0, 7600.0))
    lo, hi = kw.get('lo_hz', lo), kw.get('hi_hz', hi)
    bins = kw.get('mel_bins', 128) if mfcc else kw.get('bins', 64)
    size = kw.get('fft_size', 1024 if mfcc else 2048)
    overlap = kw.get('overlap', 0.75)
    mag = tf.abs(tf.signal.stft(audio, int(size), int(size * (1.0 - overlap)), fft_length=None, pad_end=True))
    mel = tf.tensordot(mag, tf.signal.linear_to_mel_weight_matrix(bins, int(mag.shape[-1]), 16000, lo, hi), 1)
    if fn == 'compute_mel':
      return mel.numpy()
    logmel = tf.math.log(tf.where(mel <= 0.0, 1e-5, mel))
    return tf.signal.mfccs_from_log_mel_spectrograms(logmel)[..., :kw.get('mfcc_bins', 13)].numpy() if mfcc else logmel.numpy()

  for name, (fn, kw) in MEL_CASES.items():
    with np.load(os.path.join(HERE, name + '.npz')) as z:
      audio, out = z['audio'], z['out']
    t = truth_of(fn, audio, kw)
    print('%-24s TensorFlow / tolerance = %.3f; fixture vs TensorFlow max %.3e'
          % (name, held(fn, chain(fn, audio, kw), t, 1.0), float(np.abs(chain(fn, audio, kw) - out).max())))
  with np.load(os.path.join(HERE, 'mel_tables.npz')) as z:
    for key in TABLES['mel']:
      w = tf.signal.linear_to_mel_weight_matrix(*key).numpy()
      print('mel matrix %s: fixture == TensorFlow: %s' % (key, np.array_equal(w, z['mel_%d_%d_%d_%g_%g' % key])))
    for mel_bins, mfcc_bins in TABLES['dct']:
      d = tf.signal.mfccs_from_log_mel_spectrograms(tf.eye(mel_bins)).numpy().T[:mfcc_bins]
      print('dct %d x %d: fixture vs TensorFlow max %.3e' % (mfcc_bins, mel_bins, float(np.abs(d - z['dct_%d_%d' % (mel_bins, mfcc_bins)]).max())))


if __name__ == '__main__':
  if '--tf' in sys.argv:
    run_tf()
  else:
    run_shim()
