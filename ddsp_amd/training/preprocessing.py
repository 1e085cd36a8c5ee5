"""ddsp/training/preprocessing.py on the MI355X: the scalings and F0LoudnessPreprocessor, on core.resample, core.hz_to_midi and
spectral_ops.compute_loudness.  The scalings themselves are single framework multiplies."""
from ddsp_amd import core
from ddsp_amd import spectral_ops
from ddsp_amd.training import nn

F0_RANGE = 127.0  # MIDI.
DB_RANGE = spectral_ops.DB_RANGE  # dB (80.0).


# ---------------------- Preprocess Helpers ------------------------------------
def at_least_3d(x):
  """Optionally adds time, batch, then channel dimension."""
  x = core.tf_float32(x)
  x = x[None] if x.dim() == 0 else x
  x = x[None, :] if x.dim() == 1 else x
  x = x[:, :, None] if x.dim() == 2 else x
  return x


def scale_db(db):
  """Scales [-DB_RANGE, 0] to [0, 1]."""
  return (core.tf_float32(db) / DB_RANGE) + 1.0


def inv_scale_db(db_scaled):
  """Scales [0, 1] to [-DB_RANGE, 0]."""
  return (core.tf_float32(db_scaled) - 1.0) * DB_RANGE


def scale_f0_hz(f0_hz):
  """Scales [0, Nyquist] Hz to [0, 1.0] MIDI-scaled."""
  return core.hz_to_midi(f0_hz) / F0_RANGE


def inv_scale_f0_hz(f0_scaled):
  """Scales [0, 1.0] MIDI-scaled to [0, Nyquist] Hz."""
  return core.midi_to_hz(core.tf_float32(f0_scaled) * F0_RANGE)


# ---------------------- Preprocess objects ------------------------------------
class F0LoudnessPreprocessor(nn.DictLayer):
  """Resamples and scales 'f0_hz' and 'loudness_db' features (ddsp/training/preprocessing.py:59-101)."""

  def __init__(self, time_steps=1000, frame_rate=250, sample_rate=16000, compute_loudness=True, **kwargs):
    super().__init__(**kwargs)
    self.time_steps = time_steps
    self.frame_rate = frame_rate
    self.sample_rate = sample_rate
    self.compute_loudness = compute_loudness

  def call(self, loudness_db, f0_hz, audio=None) -> ['f0_hz', 'loudness_db', 'f0_scaled', 'ld_scaled']:
    # Compute loudness fresh (it's fast).
    if self.compute_loudness:
      loudness_db = spectral_ops.compute_loudness(audio, sample_rate=self.sample_rate, frame_rate=self.frame_rate)
    # Resample features to the frame_rate.
    f0_hz = self.resample(f0_hz)
    loudness_db = self.resample(loudness_db)
    # For NN training, scale frequency and loudness to the range [0, 1].
    f0_scaled = scale_f0_hz(f0_hz)
    ld_scaled = scale_db(loudness_db)
    return f0_hz, loudness_db, f0_scaled, ld_scaled

  @staticmethod
  def invert_scaling(f0_scaled, ld_scaled):
    """Takes in scaled f0 and loudness, and puts them back to hz & db scales."""
    return inv_scale_f0_hz(f0_scaled), inv_scale_db(ld_scaled)

  def resample(self, x):
    return core.resample(at_least_3d(x), self.time_steps)
