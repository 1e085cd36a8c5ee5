"""ddsp/training/encoders.py on the MI355X: the encoders that make the latent `z` (ddsp/training/encoders.py:27-334).

ZEncoder (the base: compute_z, then expand_z to the conditioning's frame count), MfccTimeDistributedRnnEncoder (the z encoder of
the shipped configurations: MFCCs -> instance norm -> GRU -> Dense), MfccEncoder, AggregateFeaturesEncoder and OneHotEncoder.
The kernels: the fused MFCC kernel (csrc/features.hip, forward only - audio is data), the normalisation (csrc/group_norm.hip),
the GRU (csrc/decoder.hip) and the resampler with its adjoint (csrc/general.hip); Dense is the framework's matrix product.
Every weight is a torch.nn.Parameter under the reference's (Keras) name and layout, and z is differentiable in all of them.
NOT BUILT: MfccRnnEncoder (its default branch concatenates over the batch: a reference bug to be settled on its own), the
ResNet, MIDI and expression encoders; rnn_type='lstm' raises ValueError as nn.Rnn does."""
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
