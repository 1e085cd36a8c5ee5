"""Mirror of ddsp/spectral_ops.py: compute_mag / compute_logmag (:67-70, 95-97), compute_mel / compute_logmel / compute_mfcc
(:73-133), compute_rms_energy / compute_power (:223-249), compute_loudness (:253-324), pad and get_framed_lengths (:136-220).

Forward only (the differentiable entry is losses.SpectralLoss); magnitudes come from the plain STFT kernels under a frame
geometry given at run time (ddsp_stft_frames_mag_f32: csrc/spectral_loss.hip), so any `overlap` whose hop is a whole number of
samples and both settings of `pad_end` run.

The mel features run in ONE kernel (ddsp_mel_features_f32): the STFT block keeps its magnitudes in LDS, projects them on the mel
bands, takes the safe log and the DCT there and writes only [batch, n_frames, bins or mfcc_bins]; compute_mag's
[batch, n_frames, fft_size / 2 + 1] tensor is never built.  The two TensorFlow functions under them are restated on the host in
fp64 from TensorFlow's published source (tf.signal.linear_to_mel_weight_matrix, tf.signal.mfccs_from_log_mel_spectrograms;
DESIGN.md section 2) and cached per argument tuple.  Beyond the kernel's limits (more mel bins than the transform has points,
more MFCCs than mel bins) the same functions run as compute_mag followed by the table products with torch.

pad_or_trim_to_expected_length (:367-423) is host plumbing: numpy in, numpy out; tensor in, tensor out.

Not offered: compute_f0 / PretrainedCREPE (a pretrained network)."""
import numpy as np
import torch

from ddsp_amd import _lib
from ddsp_amd import core
from ddsp_amd import losses

DB_RANGE = core.DB_RANGE


def _audio_2d(audio):
  audio = core.tf_float32(audio)
  core.require_no_grad('spectral_ops (losses.SpectralLoss is the differentiable entry)', audio)
  if audio.dim() == 3:
    audio = audio[..., 0]
  squeeze = audio.dim() == 1
  if squeeze:
    audio = audio[None, :]
  if audio.dim() != 2:
    raise ValueError('audio must be [batch, n_samples], [batch, n_samples, 1] or [n_samples], got {}'.format(tuple(audio.shape)))
  return audio.contiguous(), squeeze


def _frames_mag(audio, frame_size, hop, pad_left, n_frames):
  """|tf.signal.stft| under a frame geometry: frames of frame_size samples every hop, the first pad_left samples before sample 0,
  the enclosing power of two transformed (fft_length=None, spectral_ops.py:40-45)."""
  b, n = audio.shape
  fft_size = 1 << max(int(frame_size) - 1, 1).bit_length()
  if frame_size & 1 or not 64 <= fft_size <= 8192:
    raise NotImplementedError('frame sizes on the MI355X path: even, in [34, 8192], got {}'.format(frame_size))
  if n_frames <= 0:
    return torch.empty((b, 0, fft_size // 2 + 1), dtype=torch.float32, device=audio.device)
  mag = torch.empty((b, n_frames, fft_size // 2 + 1), dtype=torch.float32, device=audio.device)
  lib = _lib.load()
  rc = lib.ddsp_stft_frames_mag_ex_f32(audio.data_ptr(), mag.data_ptr(), b, n, fft_size, int(frame_size), int(hop), int(pad_left),
                                       int(n_frames), core._stream())
  _lib.check(rc, 'ddsp_stft_frames_mag_ex_f32')
  return mag


def get_framed_lengths(input_length, frame_size, hop_size, padding='center'):
  """(n_frames, padded_length) of a strided framing (spectral_ops.py:130-168)."""
  def get_n_frames(length):
    return int(np.floor((length - frame_size) // hop_size)) + 1
  if padding == 'valid':
    padded_length = input_length
    n_frames = get_n_frames(input_length)
  elif padding == 'center':
    padded_length = input_length + frame_size
    n_frames = get_n_frames(padded_length)
  elif padding == 'same':
    n_frames = int(np.ceil(input_length / hop_size))
    padded_length = (n_frames - 1) * hop_size + frame_size
  else:
    raise ValueError('`padding` must be one of [\'center\', \'same\', \'valid\'], received ({}).'.format(padding))
  return n_frames, padded_length


def stft(audio, frame_size=2048, overlap=0.75, pad_end=True):
  """The complex spectrogram [batch, n_frames, bins] (complex64) of spectral_ops.stft (spectral_ops.py:34-47): tf.signal.stft with
  fft_length=None - frames of frame_size samples every int(frame_size * (1 - overlap)) under a periodic Hann window, zero-padded
  to the enclosing power of two.  Forward only (losses.SpectralLoss is the differentiable entry)."""
  audio, squeeze = _audio_2d(audio)
  b, n = audio.shape
  frame_size = int(frame_size)
  hop = int(frame_size * (1.0 - overlap))
  if hop <= 0:
    raise ValueError('overlap {} leaves no hop for frames of {}'.format(overlap, frame_size))
  fft_size = 1 << max(frame_size - 1, 1).bit_length()
  if frame_size & 1 or not 64 <= fft_size <= 8192:
    raise NotImplementedError('stft on the MI355X path: even frame sizes in [34, 8192], got {}'.format(frame_size))
  n_frames = -(-n // hop) if pad_end else (1 + (n - frame_size) // hop if n >= frame_size else 0)
  spectrum = torch.empty((b, max(n_frames, 0), fft_size // 2 + 1, 2), dtype=torch.float32, device=audio.device)
  if n_frames > 0:
    rc = _lib.load().ddsp_stft_frames_f32(audio.data_ptr(), spectrum.data_ptr(), b, n, fft_size, frame_size, hop, 0, n_frames,
                                          core._stream())
    _lib.check(rc, 'ddsp_stft_frames_f32')
  spectrum = torch.view_as_complex(spectrum)
  return spectrum[0] if squeeze else spectrum


def compute_mag(audio, size=2048, overlap=0.75, pad_end=True):
  """|STFT| [batch, n_frames, bins] (spectral_ops.py:67-70): frames of `size` every size * (1 - overlap) samples under a periodic
  Hann window; pad_end: zero-padded frames up to the last sample (tf.signal.frame)."""
  audio, squeeze = _audio_2d(audio)
  n = audio.shape[1]
  hop = int(size * (1.0 - overlap))
  if hop <= 0:
    raise ValueError('overlap {} leaves no hop for frames of {}'.format(overlap, size))
  n_frames = -(-n // hop) if pad_end else (1 + (n - size) // hop if n >= size else 0)
  mag = _frames_mag(audio, int(size), hop, 0, n_frames)
  return mag[0] if squeeze else mag


def compute_logmag(audio, size=2048, overlap=0.75, pad_end=True):
  """core.safe_log of compute_mag (spectral_ops.py:95-97)."""
  return core.safe_log(compute_mag(audio, size, overlap, pad_end))


def compute_loudness(audio, sample_rate=16000, frame_rate=250, n_fft=512, range_db=DB_RANGE, ref_db=0.0, use_tf=True,
                     padding='center'):
  """Perceptual loudness in dB [batch, n_frames] (spectral_ops.py:253-324): A-weighted mean power per frame of n_fft samples every
  sample_rate // frame_rate, floored at -range_db.  `use_tf` is accepted and ignored (one implementation)."""
  del use_tf
  audio, squeeze = _audio_2d(audio)
  b, n = audio.shape
  hop = sample_rate // frame_rate
  if padding not in ('center', 'same', 'valid'):
    raise ValueError('`padding` must be one of [\'center\', \'same\', \'valid\'], received ({}).'.format(padding))
  if padding != 'valid' and hop > n_fft:
    raise ValueError('During padding, frame_size ({}) must be greater than hop_size ({}).'.format(n_fft, hop))
  if n_fft < 2 or n_fft & (n_fft - 1):
    # tf.signal.stft transforms the enclosing power of two (fft_size // 2 + 1 bins) while the A-weighting curve has n_fft // 2 + 1
    # entries (spectral_ops.py:296-311): the reference's `power_db + a_weighting` fails to broadcast for any other n_fft.  (ADVICE
    # r5: this used to read the curve past its end on the device.)
    raise ValueError('compute_loudness: n_fft must be a power of two (the A-weighting curve has n_fft // 2 + 1 entries, the '
                     'spectrogram {} bins), got {}'.format((1 << max(int(n_fft) - 1, 1).bit_length()) // 2 + 1, n_fft))
  n_frames, _ = get_framed_lengths(n, n_fft, hop, padding)
  pad_left = n_fft // 2 if padding == 'center' else 0
  mag = _frames_mag(audio, int(n_fft), hop, pad_left, max(n_frames, 0))
  frames, bins = mag.shape[1], mag.shape[2]
  loud = torch.empty((b, frames), dtype=torch.float32, device=audio.device)
  if frames:
    wt = _a_weighting(sample_rate, n_fft, audio.device)
    _lib.check(_lib.load().ddsp_loudness_from_mag_f32(mag.data_ptr(), wt.data_ptr(), loud.data_ptr(), b, frames, bins,
                                                      float(range_db), float(ref_db), core._stream()),
               'ddsp_loudness_from_mag_f32')
  return loud[0] if squeeze else loud


_weighting_cache = {}


def _a_weighting(sample_rate, n_fft, device):
  key = (int(sample_rate), int(n_fft), str(device))
  if key not in _weighting_cache:
    _weighting_cache[key] = torch.as_tensor(losses.a_weighting_linear(sample_rate, n_fft), device=device)
  return _weighting_cache[key]


# --------------------------------------------------------------------------------------
# mel / log-mel / MFCC (ddsp/spectral_ops.py:73-133)
# --------------------------------------------------------------------------------------
_MEL_BREAK_HZ, _MEL_HIGH_Q = 700.0, 1127.0


def _hz_to_mel(hz):
  return _MEL_HIGH_Q * np.log(1.0 + np.asarray(hz, np.float64) / _MEL_BREAK_HZ)


_mel_matrix_cache = {}


def linear_to_mel_weight_matrix(num_mel_bins=20, num_spectrogram_bins=129, sample_rate=8000, lower_edge_hertz=125.0,
                                upper_edge_hertz=3800.0):
  """tf.signal.linear_to_mel_weight_matrix, restated: [num_spectrogram_bins, num_mel_bins] float32 (numpy), computed in float64.
  HTK mel scale; num_mel_bins + 2 band edges equally spaced in mel; triangular weights over the spectrogram bins
  linspace(0, sample_rate / 2, num_spectrogram_bins) without the DC bin, which comes back as a row of zeros."""
  if num_mel_bins <= 0:
    raise ValueError('num_mel_bins must be positive. Got: %s' % num_mel_bins)
  if lower_edge_hertz < 0.0:
    raise ValueError('lower_edge_hertz must be non-negative. Got: %s' % lower_edge_hertz)
  if lower_edge_hertz >= upper_edge_hertz:
    raise ValueError('lower_edge_hertz %.1f >= upper_edge_hertz %.1f' % (lower_edge_hertz, upper_edge_hertz))
  if sample_rate <= 0.0:
    raise ValueError('sample_rate must be positive. Got: %s' % sample_rate)
  if upper_edge_hertz > sample_rate / 2:
    raise ValueError('upper_edge_hertz must not be larger than the Nyquist frequency (sample_rate / 2). Got %s for sample_rate: %s'
                     % (upper_edge_hertz, sample_rate))
  key = (int(num_mel_bins), int(num_spectrogram_bins), float(sample_rate), float(lower_edge_hertz), float(upper_edge_hertz))
  if key not in _mel_matrix_cache:
    bins_mel = _hz_to_mel(np.linspace(0.0, key[2] / 2.0, key[1])[1:])[:, None]
    edges = np.linspace(_hz_to_mel(key[3]), _hz_to_mel(key[4]), key[0] + 2)
    lower, center, upper = edges[None, :-2], edges[None, 1:-1], edges[None, 2:]
    weights = np.maximum(0.0, np.minimum((bins_mel - lower) / (center - lower), (upper - bins_mel) / (upper - center)))
    matrix = np.concatenate([np.zeros((1, key[0])), weights], axis=0).astype(np.float32)
    matrix.setflags(write=False)
    _mel_matrix_cache[key] = matrix
  return _mel_matrix_cache[key]


_dct_cache = {}


def mfcc_dct_matrix(mel_bins, mfcc_bins):
  """The rows tf.signal.mfccs_from_log_mel_spectrograms keeps, [mfcc_bins, mel_bins] float32 (numpy):
  D[k, n] = 2 cos(pi k (2 n + 1) / (2 N)) / sqrt(2 N), the unnormalised DCT-II times rsqrt(2 N), N = mel_bins."""
  key = (int(mel_bins), int(mfcc_bins))
  if key not in _dct_cache:
    k = np.arange(key[1], dtype=np.float64)[:, None]
    n = np.arange(key[0], dtype=np.float64)[None, :]
    table = (2.0 * np.cos(np.pi * k * (2.0 * n + 1.0) / (2.0 * key[0])) / np.sqrt(2.0 * key[0])).astype(np.float32)
    table.setflags(write=False)
    _dct_cache[key] = table
  return _dct_cache[key]


def mel_band_tables(matrix):
  """The banded form of a mel matrix the kernel reads: bands [3, bins] int32 (first bin, number of bins, index of the band's
  first packed weight) and the packed weights.  A column without a non-zero entry (a band narrower than one bin) has count 0."""
  n_bins = matrix.shape[1]
  bands = np.zeros((3, n_bins), np.int32)
  packed = []
  total = 0
  for m in range(n_bins):
    nz = np.flatnonzero(matrix[:, m])
    if nz.size:
      k0, count = int(nz[0]), int(nz[-1] - nz[0] + 1)
      bands[:, m] = (k0, count, total)
      packed.append(matrix[k0:k0 + count, m])
      total += count
    else:
      bands[:, m] = (0, 0, total)
  weights = np.concatenate(packed).astype(np.float32) if packed else np.zeros((0,), np.float32)
  return bands, weights


_device_table_cache = {}


def _mel_device_tables(key, device):
  """(bands, weights, n_weights, matrix) on `device` for a mel-matrix key."""
  ck = ('mel',) + key + (str(device),)
  if ck not in _device_table_cache:
    matrix = linear_to_mel_weight_matrix(*key)
    bands, weights = mel_band_tables(matrix)
    n_weights = int(weights.size)
    if n_weights == 0:
      weights = np.zeros((1,), np.float32)          # (a pointer to pass; nothing reads it)
    _device_table_cache[ck] = (torch.as_tensor(bands, device=device).contiguous(), torch.as_tensor(weights, device=device),
                               n_weights, torch.as_tensor(matrix.copy(), device=device))
  return _device_table_cache[ck]


def _dct_device_tables(mel_bins, mfcc_bins, device):
  """(the DCT table transposed, [mel_bins, mfcc_bins], and as it is) on `device`."""
  ck = ('dct', int(mel_bins), int(mfcc_bins), str(device))
  if ck not in _device_table_cache:
    table = mfcc_dct_matrix(mel_bins, mfcc_bins)
    _device_table_cache[ck] = (torch.as_tensor(np.ascontiguousarray(table.T), device=device), torch.as_tensor(table.copy(), device=device))
  return _device_table_cache[ck]


def mel_fused_limits(fft_size, bins, mfcc_bins=None):
  """True where ddsp_mel_features_f32 takes the shape: the [G, bins] tile of a block's G = 8192 / S frames lies in the 8192
  floats of the S-point transform's LDS array (bins <= S, S the enclosing power of two of fft_size), and mfcc_bins <= bins."""
  transform = 1 << max(int(fft_size) - 1, 1).bit_length()
  return bins <= transform and (mfcc_bins is None or mfcc_bins <= bins)


def _mel_features(mode, audio, lo_hz, hi_hz, bins, fft_size, overlap, pad_end, sample_rate, mfcc_bins=None):
  audio, squeeze = _audio_2d(audio)
  b, n = audio.shape
  fft_size, bins = int(fft_size), int(bins)
  hop = int(fft_size * (1.0 - overlap))
  if hop <= 0:
    raise ValueError('overlap {} leaves no hop for frames of {}'.format(overlap, fft_size))
  transform = 1 << max(fft_size - 1, 1).bit_length()
  key = (bins, transform // 2 + 1, float(sample_rate), float(lo_hz), float(hi_hz))
  linear_to_mel_weight_matrix(*key)                             # (its ValueErrors before anything runs)
  if mfcc_bins is not None:
    mfcc_bins = int(mfcc_bins)
    if mfcc_bins <= 0:
      raise ValueError('mfcc_bins must be positive, got {}'.format(mfcc_bins))
  if fft_size & 1 or not 64 <= transform <= 8192:
    raise NotImplementedError('frame sizes on the MI355X path: even, in [34, 8192], got {}'.format(fft_size))
  n_frames = max(-(-n // hop) if pad_end else (1 + (n - fft_size) // hop if n >= fft_size else 0), 0)
  bands, weights, n_weights, matrix = _mel_device_tables(key, audio.device)
  if not mel_fused_limits(fft_size, bins, mfcc_bins):
    # the general chain: compute_mag, then the table products (the reference's own order of operations)
    out = torch.matmul(_frames_mag(audio, fft_size, hop, 0, n_frames), matrix)
    if mode != 'mel':
      out = core.safe_log(out)
    if mode == 'mfcc':
      kept = min(mfcc_bins, bins)                               # (mfccs[..., :mfcc_bins] of `bins` coefficients)
      out = torch.matmul(out, _dct_device_tables(bins, kept, audio.device)[1].t())
    return out[0] if squeeze else out
  width = mfcc_bins if mode == 'mfcc' else bins
  out = torch.empty((b, n_frames, width), dtype=torch.float32, device=audio.device)
  if n_frames:
    dct_t = _dct_device_tables(bins, mfcc_bins, audio.device)[0] if mode == 'mfcc' else None
    rc = _lib.load().ddsp_mel_features_f32(audio.data_ptr(), bands.data_ptr(), weights.data_ptr(),
                                           dct_t.data_ptr() if dct_t is not None else None, out.data_ptr(), b, n, transform,
                                           fft_size, hop, 0, n_frames, bins, mfcc_bins or 0, n_weights, _lib.MEL_MODES[mode], 1e-5,
                                           core._stream())
    _lib.check(rc, 'ddsp_mel_features_f32')
  return out[0] if squeeze else out


def compute_mel(audio, lo_hz=0.0, hi_hz=8000.0, bins=64, fft_size=2048, overlap=0.75, pad_end=True, sample_rate=16000):
  """Mel spectrogram [batch, n_frames, bins] (spectral_ops.py:73-89): compute_mag projected on
  linear_to_mel_weight_matrix(bins, fft bins, sample_rate, lo_hz, hi_hz), in one kernel."""
  return _mel_features('mel', audio, lo_hz, hi_hz, bins, fft_size, overlap, pad_end, sample_rate)


def compute_logmel(audio, lo_hz=80.0, hi_hz=7600.0, bins=64, fft_size=2048, overlap=0.75, pad_end=True, sample_rate=16000):
  """core.safe_log of compute_mel (spectral_ops.py:97-109)."""
  return _mel_features('logmel', audio, lo_hz, hi_hz, bins, fft_size, overlap, pad_end, sample_rate)


def compute_mfcc(audio, lo_hz=20.0, hi_hz=8000.0, fft_size=1024, mel_bins=128, mfcc_bins=13, overlap=0.75, pad_end=True,
                 sample_rate=16000):
  """Mel-frequency cepstral coefficients [batch, n_frames, mfcc_bins] (spectral_ops.py:112-133): the first mfcc_bins
  coefficients of tf.signal.mfccs_from_log_mel_spectrograms(compute_logmel(...))."""
  return _mel_features('mfcc', audio, lo_hz, hi_hz, mel_bins, fft_size, overlap, pad_end, sample_rate, mfcc_bins)


# --------------------------------------------------------------------------------------
# pad, rms energy, power (ddsp/spectral_ops.py:171-249)
# --------------------------------------------------------------------------------------
def pad(x, frame_size, hop_size, padding='center', axis=1, mode='CONSTANT', constant_values=0):
  """Pads a tensor for strided framing (spectral_ops.py:171-220): 'valid' nothing, 'same' at the end up to
  (ceil(n / hop) - 1) hop + frame_size, 'center' frame_size // 2 on both sides.  Host plumbing (torch)."""
  x = core.tf_float32(x)
  if padding == 'valid':
    return x
  if hop_size > frame_size:
    raise ValueError('During padding, frame_size ({}) must be greater than hop_size ({}).'.format(frame_size, hop_size))
  if padding not in ('same', 'center'):
    raise ValueError('`padding` must be one of [\'center\', \'same\', \'valid\'], received ({}).'.format(padding))
  if x.dim() <= 1:
    axis = 0
  n_t = x.shape[axis]
  if padding == 'same':
    _, n_t_padded = get_framed_lengths(n_t, frame_size, hop_size, padding)
    before, after = 0, int(n_t_padded - n_t)
  else:
    before = after = int(frame_size // 2)
  x = x.movedim(axis, -1)
  mode = mode.upper()
  if mode == 'CONSTANT':
    out = torch.nn.functional.pad(x, (before, after), value=float(constant_values))
  elif mode in ('REFLECT', 'SYMMETRIC'):
    skip = 1 if mode == 'REFLECT' else 0                        # REFLECT leaves the edge sample out, SYMMETRIC repeats it
    if max(before, after) + skip > n_t:
      raise ValueError('{} padding of {} needs at least {} samples, got {}'.format(mode, max(before, after), max(before, after) + skip,
                                                                                 n_t))
    left = x[..., skip:skip + before].flip(-1)
    right = x[..., n_t - skip - after:n_t - skip].flip(-1)
    out = torch.cat([left, x, right], dim=-1)
  else:
    raise ValueError('`mode` must be one of CONSTANT, REFLECT, SYMMETRIC, received ({}).'.format(mode))
  return out.movedim(-1, axis).contiguous()


def _frame_energy(audio, sample_rate, frame_rate, frame_size, padding, db, ref_db=0.0, range_db=DB_RANGE):
  audio, squeeze = _audio_2d(audio)
  b, n = audio.shape
  frame_size, hop = int(frame_size), int(sample_rate // frame_rate)
  if padding not in ('center', 'same', 'valid'):
    raise ValueError('`padding` must be one of [\'center\', \'same\', \'valid\'], received ({}).'.format(padding))
  if padding != 'valid' and hop > frame_size:
    raise ValueError('During padding, frame_size ({}) must be greater than hop_size ({}).'.format(frame_size, hop))
  if frame_size <= 0 or hop <= 0:
    raise ValueError('frame_size and hop must be positive, got {} and {}'.format(frame_size, hop))
  # tf.signal.frame(pad(audio), frame_size, hop, pad_end=False): the frames that lie inside the padded clip
  pad_left = frame_size // 2 if padding == 'center' else 0
  if padding == 'center':
    padded = n + 2 * pad_left
  elif padding == 'same':
    padded = get_framed_lengths(n, frame_size, hop, padding)[1]
  else:
    padded = n
  n_frames = 1 + (padded - frame_size) // hop if padded >= frame_size else 0
  out = torch.empty((b, n_frames), dtype=torch.float32, device=audio.device)
  if n_frames:
    rc = _lib.load().ddsp_frame_energy_f32(audio.data_ptr(), out.data_ptr(), b, n, frame_size, hop, pad_left, n_frames,
                                           float(ref_db), float(range_db), _lib.ENERGY_DB if db else 0, core._stream())
    _lib.check(rc, 'ddsp_frame_energy_f32')
  return out[0] if squeeze else out


def compute_rms_energy(audio, sample_rate=16000, frame_rate=250, frame_size=512, padding='center'):
  """Root mean squared energy [batch, n_frames] (spectral_ops.py:223-234) of frames of frame_size samples every
  sample_rate // frame_rate; any frame size."""
  return _frame_energy(audio, sample_rate, frame_rate, frame_size, padding, False)


def compute_power(audio, sample_rate=16000, frame_rate=250, frame_size=512, ref_db=0.0, range_db=DB_RANGE, padding='center'):
  """Power in dB [batch, n_frames] (spectral_ops.py:237-249): core.amplitude_to_db(compute_rms_energy(...), ref_db, range_db),
  in the energy kernel (the same bits as the two calls)."""
  return _frame_energy(audio, sample_rate, frame_rate, frame_size, padding, True, ref_db, range_db)


def pad_or_trim_to_expected_length(vector, expected_len, pad_value=0, len_tolerance=20, use_tf=False):
  """Make the last axis of a 1-D or 2-D vector `expected_len` long (spectral_ops.py:367-423): padded at the end with
  pad_value or trimmed; ValueError when the lengths differ by more than len_tolerance to begin with.  A numpy array comes
  back as a numpy array, a tensor as a tensor (differentiable); `use_tf` is accepted and has nothing to choose."""
  del use_tf
  expected_len = int(expected_len)
  vector_len = int(vector.shape[-1])
  if abs(vector_len - expected_len) > len_tolerance:
    raise ValueError('Vector length: {} differs from expected length: {} '
                     'beyond tolerance of : {}'.format(vector_len, expected_len, len_tolerance))
  is_tensor = isinstance(vector, torch.Tensor)
  if not is_tensor:
    vector = np.asarray(vector)
  is_1d = len(vector.shape) == 1
  vector = vector[None, :] if is_1d else vector
  if vector_len < expected_len:
    n_padding = expected_len - vector_len
    if is_tensor:
      vector = torch.nn.functional.pad(vector, (0, n_padding), value=float(pad_value))
    else:
      vector = np.pad(vector, ((0, 0), (0, n_padding)), mode='constant', constant_values=pad_value)
  elif vector_len > expected_len:
    vector = vector[..., :expected_len]
  return vector[0] if is_1d else vector
