"""ddsp/training/decoders.py on the MI355X: RnnFcDecoder, the decoder of every shipped solo-instrument configuration, and
DilatedConvDecoder, the synth coder of the MIDI autoencoders (gin/models/midiae/*.gin).

RnnFcDecoder: one FcStack per input, a GRU over the concatenated stacks, a further FcStack over (stacks, GRU), a final Dense split
into the synthesiser controls.  DilatedConvDecoder: a DilatedConvStack over the concatenated inputs, conditioned on z through
FiLM, then the same final Dense.  The layers are those of ddsp_amd.training.nn (kernels: csrc/decoder.hip, csrc/dilated_conv.hip,
csrc/group_norm.hip)."""
import torch

from ddsp_amd import core
from ddsp_amd.training import nn


class RnnFcDecoder(nn.DictLayer):
  """RNN and FC stacks for f0 and loudness (ddsp/training/decoders.py:27-109)."""

  def __init__(self,
               rnn_channels=512,
               rnn_type='gru',
               ch=512,
               layers_per_stack=3,
               stateless=False,
               input_keys=('ld_scaled', 'f0_scaled', 'z'),
               output_splits=(('amps', 1), ('harmonic_distribution', 40)),
               **kwargs):
    """Constructor.

    Args:
      rnn_channels: Dims for the RNN layer.
      rnn_type: 'gru' ('lstm' is not built: ValueError).
      ch: Dims of the fully connected layers.
      layers_per_stack: Fully connected layers per a stack.
      stateless: Change api to explicitly pass in and out RNN state. Uses nn.StatelessRnn.
      input_keys: Create a fully connected stack for each input.
      output_splits: Splits the outputs into these dimensions.
      **kwargs: name.

    Returns:
      Dictionary with keys from output_splits. Also has 'state' key if `stateless=True`, for manually handling state.
    """
    # Always put state as the last input and output.
    output_keys = [v[0] for v in output_splits]
    if stateless:
      input_keys = list(input_keys) + ['state']
      output_keys = list(output_keys) + ['state']
    super().__init__(input_keys=input_keys, output_keys=output_keys, **kwargs)
    self.stateless = stateless
    self.output_splits = output_splits

    # Don't create a stack for manual RNN state.
    n_stacks = len(self.input_keys) - (1 if stateless else 0)
    rnn_cls = nn.StatelessRnn if stateless else nn.Rnn
    self.input_stacks = torch.nn.ModuleList([nn.FcStack(ch, layers_per_stack) for _ in range(n_stacks)])
    self.rnn = rnn_cls(rnn_channels, rnn_type)
    self.out_stack = nn.FcStack(ch, layers_per_stack)
    self.dense_out = nn.Dense(sum([v[1] for v in output_splits]))

  def call(self, *inputs, **unused_kwargs):
    # Last input is always carried state for stateless RNN.
    inputs = list(inputs)
    if self.stateless:
      state = inputs.pop()
    inputs = [stack(x) for stack, x in zip(self.input_stacks, inputs)]
    x = torch.cat(inputs, dim=-1)
    if self.stateless:
      x, new_state = self.rnn(x, state)
    else:
      x = self.rnn(x)
    x = torch.cat(inputs + [x], dim=-1)
    x = self.dense_out(self.out_stack(x))
    output_dict = nn.split_to_dict(x, self.output_splits)
    if self.stateless:
      output_dict['state'] = new_state
    return output_dict


class DilatedConvDecoder(nn.OutputSplitsLayer):
  """WaveNet style 1-D dilated convolution with optional conditioning (ddsp/training/decoders.py:221-285)."""

  def __init__(self,
               ch=256,
               kernel_size=3,
               layers_per_stack=5,
               stacks=2,
               dilation=2,
               norm_type='layer',
               resample_stride=1,
               stacks_per_resample=1,
               resample_after_convolve=True,
               input_keys=('ld_scaled', 'f0_scaled'),
               output_splits=(('amps', 1), ('harmonic_distribution', 60)),
               conditioning_keys=('z'),
               precondition_stack=None,
               spectral_norm=False,
               ortho_init=False,
               **kwargs):
    """Constructor, combines input_keys and conditioning_keys.  The default conditioning_keys is the STRING 'z', as in the
    reference: list('z') == ['z'].  spectral_norm=True is not built (ValueError)."""
    self.conditioning_keys = ([] if conditioning_keys is None else
                              list(conditioning_keys))
    input_keys = list(input_keys) + self.conditioning_keys
    super().__init__(input_keys, output_splits, **kwargs)

    # Conditioning.
    self.n_conditioning = len(self.conditioning_keys)
    self.conditional = bool(self.conditioning_keys)
    if not self.conditional and precondition_stack is not None:
      raise ValueError('You must specify conditioning keys if you specify'
                       'a precondition stack.')

    # Layers.
    self.precondition_stack = precondition_stack
    self.dilated_conv_stack = nn.DilatedConvStack(
        ch=ch,
        kernel_size=kernel_size,
        layers_per_stack=layers_per_stack,
        stacks=stacks,
        dilation=dilation,
        norm_type=norm_type,
        resample_type='upsample' if resample_stride > 1 else None,
        resample_stride=resample_stride,
        stacks_per_resample=stacks_per_resample,
        resample_after_convolve=resample_after_convolve,
        conditional=self.conditional,
        spectral_norm=spectral_norm,
        ortho_init=ortho_init)

  def _parse_inputs(self, inputs):
    """Split x and z inputs and run preconditioning."""
    inputs = [core.tf_float32(v) for v in inputs]
    if self.conditional:
      x = torch.cat(inputs[:-self.n_conditioning], dim=-1)
      z = torch.cat(inputs[-self.n_conditioning:], dim=-1)
      if self.precondition_stack is not None:
        z = self.precondition_stack(z)
      return [x, z]
    else:
      return torch.cat(inputs, dim=-1)

  def compute_output(self, *inputs):
    stack_inputs = self._parse_inputs(inputs)
    return self.dilated_conv_stack(stack_inputs)
