"""ddsp/training/decoders.py on the MI355X: RnnFcDecoder, the decoder of every shipped model configuration.

One FcStack per input, a GRU over the concatenated stacks, a further FcStack over (stacks, GRU), a final Dense split into the
synthesiser controls.  The layers are those of ddsp_amd.training.nn (kernels: csrc/decoder.hip)."""
import torch

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
