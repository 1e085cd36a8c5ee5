"""ddsp/training/encoders.py on the MI355X: the encoders that make the latent `z` (ddsp/training/encoders.py:27-334).

ZEncoder (the base: compute_z, then expand_z to the conditioning's frame count), MfccTimeDistributedRnnEncoder (the z encoder of
the shipped configurations: MFCCs -> instance norm -> GRU -> Dense), MfccEncoder, AggregateFeaturesEncoder and OneHotEncoder.
The kernels: the fused MFCC kernel (csrc/features.hip, forward only - audio is data), the normalisation (csrc/group_norm.hip),
the GRU (csrc/decoder.hip) and the resampler with its adjoint (csrc/general.hip); Dense is the framework's matrix product.
Every weight is a torch.nn.Parameter under the reference's (Keras) name and layout, and z is differentiable in all of them.
The transcribing front end of gin/papers/icml2020/pretrain_model.gin: ResnetSinusoidalEncoder (log-mel -> nn.ResNet on
csrc/conv2d.hip -> one Dense per split) and SinusoidalToHarmonicEncoder (a network over the sinusoids -> harmonic controls).
NOT BUILT: MfccRnnEncoder (its default branch concatenates over the batch: a reference bug to be settled on its own), the
MIDI and expression encoders; rnn_type='lstm' raises ValueError as nn.Rnn does."""
import torch

from ddsp_amd import core
from ddsp_amd import spectral_ops
from ddsp_amd.training import nn


# ------------------ Encoders --------------------------------------------------
class ZEncoder(nn.DictLayer):
  """Base class to implement an encoder that creates a latent z vector.

  Users should override compute_z() to define the actual encoder structure.
  Input_keys from compute_z() instead of call(), output_keys are always ['z'].
  """

  def __init__(self, input_keys=None, **kwargs):
    """Constructor."""
    input_keys = input_keys or self.get_argument_names('compute_z')
    super().__init__(input_keys, output_keys=['z'], **kwargs)
    self.input_keys.append('f0_scaled')  # Input to get n_timesteps dynamically.

  def call(self, *args, **unused_kwargs):
    """Takes in input tensors and returns a latent tensor z."""
    time_steps = int(args[-1].shape[1])
    inputs = args[:-1]  # Last input just used for time_steps.
    z = self.compute_z(*inputs)
    return self.expand_z(z, time_steps)

  def expand_z(self, z, time_steps):
    """Make sure z has same temporal resolution as other conditioning (core.resample carries the gradient)."""
    # Add time dim of z if necessary.
    if len(z.shape) == 2:
      z = z[:, None, :]
    # Expand time dim of z if necessary.
    z_time_steps = int(z.shape[1])
    if z_time_steps != time_steps:
      z = core.resample(z, time_steps)
    return z

  def compute_z(self, *inputs):
    """Takes in input tensors and returns a latent tensor z."""
    raise NotImplementedError


class MfccTimeDistributedRnnEncoder(ZEncoder):
  """Use MFCCs as latent variables, distribute across timesteps."""

  def __init__(self,
               rnn_channels=512,
               rnn_type='gru',
               z_dims=32,
               z_time_steps=250,
               **kwargs):
    super().__init__(**kwargs)
    if z_time_steps not in [63, 125, 250, 500, 1000]:
      raise ValueError(
          '`z_time_steps` currently limited to 63,125,250,500 and 1000')
    self.z_audio_spec = {
        '63': {
            'fft_size': 2048,
            'overlap': 0.5
        },
        '125': {
            'fft_size': 1024,
            'overlap': 0.5
        },
        '250': {
            'fft_size': 1024,
            'overlap': 0.75
        },
        '500': {
            'fft_size': 512,
            'overlap': 0.75
        },
        '1000': {
            'fft_size': 256,
            'overlap': 0.75
        }
    }
    self.fft_size = self.z_audio_spec[str(z_time_steps)]['fft_size']
    self.overlap = self.z_audio_spec[str(z_time_steps)]['overlap']

    # Layers.
    self.z_norm = nn.Normalize('instance')
    self.rnn = nn.Rnn(rnn_channels, rnn_type)
    self.dense_out = nn.Dense(z_dims)

  def compute_mfccs(self, audio):
    """[batch, n_samples] -> [batch, n_frames, 30]; no gradient flows into the audio."""
    return spectral_ops.compute_mfcc(
        audio,
        lo_hz=20.0,
        hi_hz=8000.0,
        fft_size=self.fft_size,
        mel_bins=128,
        mfcc_bins=30,
        overlap=self.overlap,
        pad_end=True)

  def compute_z_from_mfccs(self, mfccs):
    # Normalize.
    z = self.z_norm(mfccs[:, :, None, :])[:, :, 0, :]
    # Run an RNN over the latents.
    z = self.rnn(z)
    # Bounce down to compressed z dimensions.
    z = self.dense_out(z)
    return z

  def compute_z(self, audio):
    return self.compute_z_from_mfccs(self.compute_mfccs(audio))


class OneHotEncoder(ZEncoder):
  """Get an embedding from the instrument one-hot."""

  def __init__(self,
               one_hot_key='instrument',
               vocab_size=1024,
               n_dims=256,
               skip_expand=True,
               **kwargs):
    super().__init__(input_keys=[one_hot_key], **kwargs)
    self.one_hot_key = one_hot_key
    self.vocab_size = vocab_size
    self.n_dims = n_dims
    self.skip_expand = skip_expand
    self.embedding = nn.get_embedding(vocab_size=self.vocab_size, n_dims=self.n_dims)

  def compute_z(self, one_hot):
    return self.embedding(one_hot)

  def expand_z(self, z, time_steps):
    if self.skip_expand:
      # Don't expand z here, rely on broadcasting instead
      return z
    else:
      return super().expand_z(z, time_steps)


class AggregateFeaturesEncoder(ZEncoder):
  """Take mean of feature embeddings in time."""

  def __init__(self, ch=512, **kwargs):
    super().__init__(**kwargs)
    self.fc = nn.Dense(ch)

  def compute_z(self, f0_scaled, ld_scaled):
    x = torch.cat([core.tf_float32(f0_scaled), core.tf_float32(ld_scaled)], dim=-1)
    z = self.fc(x)
    return z.mean(dim=1, keepdim=True)


class MfccEncoder(ZEncoder):
  """Use MFCCs as latent variables.

  The reference's compute_z ends in `self.nom_out(...)`, a typo for the `norm_out` layer its constructor makes, and raises
  AttributeError; here it calls norm_out, which is what it evidently means."""

  def __init__(self,
               fft_sizes=(1024,),
               mel_bins=(128,),
               mfcc_bins=(30,),
               time_steps=250,
               **kwargs):
    super().__init__(**kwargs)
    self.fft_sizes = core.make_iterable(fft_sizes)
    self.mel_bins = core.make_iterable(mel_bins)
    self.mfcc_bins = core.make_iterable(mfcc_bins)
    self.time_steps = time_steps

    # Layers.
    self.norm_out = nn.Normalize('instance')

  def compute_mfccs(self, audio):
    """The MFCCs of every (fft_size, mel_bins, mfcc_bins), each resampled to time_steps, concatenated over the channels."""
    mfccs = []
    for fft_size, mel_bin, mfcc_bin in zip(self.fft_sizes, self.mel_bins,
                                           self.mfcc_bins):
      mfcc = spectral_ops.compute_mfcc(
          audio,
          lo_hz=20.0,
          hi_hz=8000.0,
          fft_size=fft_size,
          mel_bins=mel_bin,
          mfcc_bins=mfcc_bin)
      mfccs.append(core.resample(mfcc, self.time_steps))
    return torch.cat(mfccs, dim=-1)

  def compute_z_from_mfccs(self, mfccs):
    return self.norm_out(mfccs[:, :, None, :])[:, :, 0, :]

  def compute_z(self, audio):
    return self.compute_z_from_mfccs(self.compute_mfccs(audio))


# Transcribing Autoencoder Encoders --------------------------------------------
class ResnetSinusoidalEncoder(nn.DictLayer):
  """This encoder maps directly from audio to synthesizer parameters (ddsp/training/encoders.py:130-173).

  EXPERIMENTAL

  It is equivalent of a base Encoder and Decoder together: spectral_fn (the fused log-mel kernel of csrc/features.hip) ->
  nn.ResNet (csrc/conv2d.hip, csrc/group_norm.hip) -> one Dense per output split over the collapsed frequency axis.  The default
  size='tiny' is not in nn.ResNet's table and raises its KeyError, as in the reference: pass 'small', 'medium' or 'large'.
  """

  def __init__(self,
               output_splits=(('frequencies', 100 * 64),
                              ('amplitudes', 100),
                              ('noise_magnitudes', 60)),
               spectral_fn=spectral_ops.compute_logmel,
               size='tiny',
               **kwargs):
    super().__init__(output_keys=[key for key, dim in output_splits], **kwargs)
    self.output_splits = output_splits
    self.spectral_fn = spectral_fn

    # Layers.
    self.resnet = nn.ResNet(size=size)
    self.dense_outs = torch.nn.ModuleList([nn.Dense(v[1]) for v in output_splits])

  def call(self, audio):
    """Updates conditioning with z and (optionally) f0."""
    outputs = {}

    # [batch, 64000, 1]
    mag = self.spectral_fn(audio)

    # [batch, 125, 229]
    mag = mag[:, :, :, None]
    x = self.resnet(mag)

    # [batch, 125, 8, 1024]
    # # Collapse the frequency dimension.
    x = x.reshape(int(x.shape[0]), int(x.shape[1]), -1)

    # [batch, 125, 8192]
    for layer, key in zip(self.dense_outs, self.output_keys):
      outputs[key] = layer(x)

    return outputs


class SinusoidalToHarmonicEncoder(nn.DictLayer):
  """Predicts harmonic controls from sinusoidal controls (ddsp/training/encoders.py:176-251).

  EXPERIMENTAL

  Differentiable in its weights and in sin_amps.  sin_freqs is data: core.hz_to_unit carries no backward and raises
  NotImplementedError for an input that requires grad (InverseSynthesis feeds both behind a stop-gradient by default).
  """

  def __init__(self,
               net=None,
               n_harmonics=100,
               f0_depth=64,
               amp_scale_fn=core.exp_sigmoid,
               # pylint: disable=g-long-lambda
               freq_scale_fn=lambda x: core.frequencies_softmax(
                   x, depth=64, hz_min=20.0, hz_max=1200.0),
               # pylint: enable=g-long-lambda
               sample_rate=16000,
               **kwargs):
    """Constructor."""
    super().__init__(**kwargs)
    self.n_harmonics = n_harmonics
    self.amp_scale_fn = amp_scale_fn
    self.freq_scale_fn = freq_scale_fn
    self.sample_rate = sample_rate

    # Layers.
    self.net = net
    self.amp_out = nn.Dense(1)
    self.hd_out = nn.Dense(n_harmonics)
    self.f0_out = nn.Dense(f0_depth)

  def call(self, sin_freqs, sin_amps) -> ['harm_amp', 'harm_dist', 'f0_hz']:
    """Converts (sin_freqs, sin_amps) to (f0, amp, hd).

    Args:
      sin_freqs: Sinusoidal frequencies in Hertz, of shape
        [batch, time, n_sinusoids].
      sin_amps: Sinusoidal amplitudes, linear scale, greater than 0, of shape
        [batch, time, n_sinusoids].

    Returns:
      f0: Fundamental frequency in Hertz, of shape [batch, time, 1].
      amp: Amplitude, linear scale, greater than 0, of shape [batch, time, 1].
      hd: Harmonic distribution, linear scale, greater than 0, of shape
        [batch, time, n_harmonics].
    """
    # Scale the inputs.
    nyquist = self.sample_rate / 2.0
    sin_freqs_unit = core.hz_to_unit(sin_freqs, hz_min=0.0, hz_max=nyquist)

    # Combine.
    x = torch.cat([core.tf_float32(sin_freqs_unit), core.tf_float32(sin_amps)], dim=-1)

    # Run it through the network.
    x = self.net(x)
    x = x['out'] if isinstance(x, dict) else x

    # Output layers.
    harm_amp = self.amp_out(x)
    harm_dist = self.hd_out(x)
    f0 = self.f0_out(x)

    # Output scaling.
    harm_amp = self.amp_scale_fn(harm_amp)
    harm_dist = self.amp_scale_fn(harm_dist)
    f0_hz = self.freq_scale_fn(f0)

    # Filter harmonic distribution for nyquist.  The harmonics' frequencies only pick the mask (no gradient reaches f0_hz
    # through a comparison, here or in the reference); core.remove_above_nyquist and core.safe_divide carry no backward, so the
    # select and the divide are their definitions as framework ops: the gradient flows through harm_dist.
    harm_freqs = core.get_harmonic_frequencies(f0_hz.detach(), self.n_harmonics)
    harm_dist = torch.where(harm_freqs >= self.sample_rate / 2.0, torch.zeros_like(harm_dist), harm_dist)
    total = harm_dist.sum(dim=-1, keepdim=True)
    harm_dist = harm_dist / torch.where(total == 0, torch.full_like(total, 1e-7), total)

    return (harm_amp, harm_dist, f0_hz)
