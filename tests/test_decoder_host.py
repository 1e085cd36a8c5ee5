"""Host tests of the decoder layers (no GPU): tests/decoder_truth.py against an independent implementation in fp64
(torch.nn.GRU with the gate blocks reordered (z, r, h) -> (r, z, n) and the matrices transposed, F.layer_norm(eps=1e-3),
F.leaky_relu(0.2)) to 1e-12 in values and gradients; DictLayer's key handling case by case (ddsp/training/nn.py:111-215); the
small helpers; the unsupported forms; the preprocessing scalings; the C ABI of csrc/decoder_abi.h against
ddsp_amd._lib.DECODER_SIGNATURES and the built library; its error codes."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import decoder_truth as T
from ddsp_amd import _lib
from ddsp_amd import build as build_mod
from ddsp_amd.training import decoders, nn, preprocessing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


def _close(a, b):
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  assert a.shape == b.shape
  assert float(np.max(np.abs(a - b))) <= TOL * max(1.0, float(np.max(np.abs(b)))), float(np.max(np.abs(a - b)))


# ---- the truth against an independent implementation ---------------------------------------------------------------------
def _torch_gru(hidden, kernel, recurrent_kernel, bias):
  """torch.nn.GRU holding Keras weights: rows (r, z, n) of weight_ih = columns (z, r, h) of kernel, transposed."""
  order = np.concatenate([np.arange(hidden, 2 * hidden), np.arange(hidden), np.arange(2 * hidden, 3 * hidden)])
  gru = torch.nn.GRU(kernel.shape[0], hidden, batch_first=True).double()
  with torch.no_grad():
    gru.weight_ih_l0.copy_(torch.as_tensor(kernel.T[order]))
    gru.weight_hh_l0.copy_(torch.as_tensor(recurrent_kernel.T[order]))
    gru.bias_ih_l0.copy_(torch.as_tensor(bias[0][order]))
    gru.bias_hh_l0.copy_(torch.as_tensor(bias[1][order]))
  return gru, order


@pytest.mark.parametrize('with_state', [False, True])
def test_truth_gru_is_torch_gru_with_reordered_gates(with_state):
  rng = np.random.default_rng(1)
  batch, steps, width, hidden = 3, 9, 5, 7
  x, kernel = rng.standard_normal((batch, steps, width)), 0.4 * rng.standard_normal((width, 3 * hidden))
  rk, bias = 0.4 * rng.standard_normal((hidden, 3 * hidden)), 0.3 * rng.standard_normal((2, 3 * hidden))
  h0 = 0.5 * rng.standard_normal((batch, hidden))
  cot = rng.standard_normal((batch, steps, hidden))
  ins = (x, kernel, rk, bias) + ((h0,) if with_state else ())
  gru, order = _torch_gru(hidden, kernel, rk, bias)
  xt = torch.tensor(x, requires_grad=True)
  ht = torch.tensor(h0[None], requires_grad=True)
  y, _ = gru(xt, ht if with_state else None)
  _close(T.gru(*ins).numpy(), y.detach().numpy())
  assert T.gru(*ins, dtype=torch.float32).dtype is torch.float32
  leaves = [xt, gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0] + ([ht] if with_state else [])
  want = torch.autograd.grad(y, leaves, torch.tensor(cot))
  got = T.grads(T.gru, ins, [cot])
  _close(got[0], want[0].numpy())
  _close(got[1][:, order], want[1].numpy().T)
  _close(got[2][:, order], want[2].numpy().T)
  _close(got[3][0][order], want[3].numpy())
  _close(got[3][1][order], want[4].numpy())
  if with_state:
    _close(got[4], want[5].numpy()[0])


@pytest.mark.parametrize('act', ['leaky_relu', 'relu', 'sigmoid', 'tanh', 'linear'])
def test_truth_fc_is_layer_norm_and_activation_of_torch(act):
  rng = np.random.default_rng(2)
  x, kernel, bias = rng.standard_normal((4, 3, 6)), rng.standard_normal((6, 5)), rng.standard_normal(5)
  gamma, beta, cot = 1.0 + 0.3 * rng.standard_normal(5), rng.standard_normal(5), rng.standard_normal((4, 3, 5))
  fn = {'leaky_relu': lambda v: F.leaky_relu(v, 0.2), 'relu': F.relu, 'sigmoid': torch.sigmoid, 'tanh': torch.tanh, 'linear': lambda v: v}[act]
  leaves = [torch.tensor(v, requires_grad=True) for v in (x, kernel, bias, gamma, beta)]
  y = fn(F.layer_norm(F.linear(leaves[0], leaves[1].t(), leaves[2]), (5,), leaves[3], leaves[4], eps=1e-3))
  _close(T.fc(x, (kernel, bias, gamma, beta), act).numpy(), y.detach().numpy())
  _close(T.bias_norm_act(x @ kernel, bias, gamma, beta, act).numpy(), y.detach().numpy())
  truth = lambda x_, k_, b_, g_, be_: T.fc(x_, (k_, b_, g_, be_), act)
  for got, want in zip(T.grads(truth, (x, kernel, bias, gamma, beta), [cot]), torch.autograd.grad(y, leaves, torch.tensor(cot))):
    _close(got, want.numpy())
  stacked = T.fc_stack(x, [(kernel, bias, gamma, beta)] * 1, act)
  _close(stacked.numpy(), y.detach().numpy())


def test_truth_decoder_is_its_parts():
  rng = np.random.default_rng(3)
  n = lambda *s: 0.4 * rng.standard_normal(s)
  fcw = lambda i, o: (n(i, o), n(o), 1.0 + n(o), n(o))
  weights = dict(input_stacks=[[fcw(1, 2)], [fcw(1, 2)]], gru=(n(4, 9), n(3, 9), n(2, 9)), out_stack=[fcw(7, 2)], dense_out=(n(2, 11), n(11)))
  a, b, state = n(2, 4, 1), n(2, 4, 1), n(2, 3)
  outs = T.rnn_fc_decoder([a, b], weights, (('amps', 1), ('hd', 10)), state=state)
  assert [tuple(o.shape) for o in outs] == [(2, 4, 1), (2, 4, 10), (2, 3)]
  sa, sb = T.fc(a, weights['input_stacks'][0][0]), T.fc(b, weights['input_stacks'][1][0])
  y = T.gru(torch.cat([sa, sb], -1), *weights['gru'], h0=state)
  full = T.dense(T.fc(torch.cat([sa, sb, y], -1), weights['out_stack'][0]), *weights['dense_out'])
  _close(torch.cat(outs[:2], -1).numpy(), full.numpy())
  _close(outs[2].numpy(), y[:, -1].numpy())
  assert len(T.rnn_fc_decoder([a, b], weights, (('amps', 1), ('hd', 10)))) == 2


# ---- DictLayer (ddsp/training/nn.py:111-215) -----------------------------------------------------------------------------
class _Layer(nn.DictLayer):
  def call(self, a, b, c=3) -> ['x', 'y', 'z']:
    return a, b, c


class _DictOut(nn.DictLayer):
  def call(self, a) -> ['ignored']:
    return {'out': a}


class _OneOut(nn.DictLayer):
  def call(self, a, b) -> ['x', 'y']:
    return a


def test_dict_layer_infers_its_keys():
  layer = _Layer()
  assert layer.input_keys == ['a', 'b'] and layer.default_input_keys == ['c'] and layer.default_input_values == [3]
  assert layer.output_keys == ['x', 'y', 'z'] and layer.all_input_keys == ['a', 'b', 'c'] and layer.n_inputs == 3
  given = _Layer(input_keys=['p', 'q', 'r'], output_keys=['u', 'v', 'w'])       # given keys overwrite the defaults
  assert given.input_keys == ['p', 'q', 'r'] and given.default_input_keys == [] and given.output_keys == ['u', 'v', 'w']
  assert given({'p': 1, 'q': 2, 'r': 5}) == {'u': 1, 'v': 2, 'w': 5}


def test_dict_layer_dict_positional_kwargs_and_defaults():
  layer = _Layer()
  assert layer({'a': 1, 'b': 2}) == {'x': 1, 'y': 2, 'z': 3}                  # dict input, default used
  assert layer({'a': 1, 'b': 2, 'c': 4, 'unused': 9}) == {'x': 1, 'y': 2, 'z': 4}
  assert layer(1, 2) == {'x': 1, 'y': 2, 'z': 3}                              # positional
  assert layer(1, 2, 7) == {'x': 1, 'y': 2, 'z': 7}
  assert layer({'a': 1}, {'b': 2}) == {'x': 1, 'y': 2, 'z': 3}                # dicts are merged
  assert layer({'a': 1, 'b': 0}, {'b': 2}) == {'x': 1, 'y': 2, 'z': 3}        # the later one wins
  assert layer(1, {'b': 2}) == {'x': 1, 'y': 2, 'z': 3}                       # tensors first, then looked-up keys
  assert layer(a=1, b=2) == {'x': 1, 'y': 2, 'z': 3}                          # kwargs
  assert layer({'a': 1}, b=2, c=5) == {'x': 1, 'y': 2, 'z': 5}
  assert layer({'a': 0, 'b': 2}, a=1) == {'x': 1, 'y': 2, 'z': 3}             # a kwarg overrides the dict


def test_dict_layer_nested_keys_and_dict_outputs():
  layer = _Layer(input_keys=['outer/a', 'outer/inner/b', 'c'])
  assert layer({'outer': {'a': 1, 'inner': {'b': 2}}, 'c': 3}) == {'x': 1, 'y': 2, 'z': 3}
  assert _DictOut()({'a': 5}) == {'out': 5}                                   # a dict from call() is returned directly


def test_dict_layer_errors():
  layer = _Layer()
  with pytest.raises(TypeError, match=r'2 input tensors extracted from inputs\(including default args\) but the layer expects 3 tensors'):
    layer({'a': 1})                                                           # b missing: a and the default
  with pytest.raises(TypeError, match='Input keys'):
    layer(1, 2, 3, 4)
  with pytest.raises(ValueError, match=r"Output keys \(\['x', 'y'\]\) must have the samelength as outputs"):
    _OneOut()(1, 2)


def test_output_splits_layer():
  class Splits(nn.OutputSplitsLayer):
    def compute_output(self, f0, ld):
      return torch.cat([f0, ld], -1)
  layer = Splits(output_splits=(('amps', 1), ('hd', 4)))
  assert layer.input_keys == ['f0', 'ld'] and layer.output_keys == ['amps', 'hd'] and layer.n_out == 5
  with pytest.raises(NotImplementedError):
    nn.OutputSplitsLayer().compute_output()


# ---- helpers -------------------------------------------------------------------------------------------------------------
def test_split_to_dict_and_ensure_4d():
  x = torch.arange(2 * 3 * 6, dtype=torch.float32).reshape(2, 3, 6)
  parts = nn.split_to_dict(x, (('a', 1), ('b', 3), ('c', 2)))
  assert list(parts) == ['a', 'b', 'c'] and [p.shape[-1] for p in parts.values()] == [1, 3, 2]
  assert torch.equal(torch.cat(list(parts.values()), -1), x)
  for n_dims, shape in ((2, (2, 1, 1, 6)), (3, (2, 3, 1, 6)), (4, (2, 3, 1, 6))):
    v = x[:, 0] if n_dims == 2 else (x if n_dims == 3 else x[:, :, None])
    assert nn.ensure_4d(v).shape == shape and torch.equal(nn.inv_ensure_4d(nn.ensure_4d(v), n_dims), v)


def test_get_nonlinearity():
  x = torch.tensor([-2.0, 0.0, 3.0])
  assert torch.equal(nn.get_nonlinearity('leaky_relu')(x), torch.tensor([-0.4, 0.0, 3.0]))
  assert torch.equal(nn.get_nonlinearity('relu')(x), torch.tensor([0.0, 0.0, 3.0]))
  assert torch.equal(nn.get_nonlinearity('linear')(x), x)
  assert torch.equal(nn.get_nonlinearity('sigmoid')(x), torch.sigmoid(x)) and torch.equal(nn.get_nonlinearity('tanh')(x), torch.tanh(x))
  for bad in ('swish', 'gelu', None):
    with pytest.raises(ValueError, match=r"supported: \['leaky_relu', 'linear', 'relu', 'sigmoid', 'tanh'\]"):
      nn.get_nonlinearity(bad)
  with pytest.raises(ValueError, match='supported'):
    nn.Fc(8, nonlinearity='swish')


def test_unsupported_rnn_forms_raise():
  with pytest.raises(ValueError, match='lstm.*not built'):
    nn.Rnn(8, 'lstm')
  with pytest.raises(ValueError, match='bidir=True is not built'):
    nn.Rnn(8, 'gru', bidir=True)
  with pytest.raises(ValueError, match='not built'):
    nn.StatelessRnn(8, 'lstm')
  with pytest.raises(ValueError, match='not built'):
    nn.RnnFc(8, 4)                                                            # the reference's default rnn_type is 'lstm'
  with pytest.raises(ValueError, match='not built'):
    decoders.RnnFcDecoder(rnn_type='lstm')
  with pytest.raises(ValueError, match="'gru' or 'lstm'"):
    nn.Rnn(8, 'rnn')


def test_layers_construct_without_a_gpu_and_fail_loudly_when_called():
  dec = decoders.RnnFcDecoder(stateless=True)
  assert dec.input_keys == ['ld_scaled', 'f0_scaled', 'z', 'state'] and dec.output_keys == ['amps', 'harmonic_distribution', 'state']
  assert len(dec.input_stacks) == 3 and isinstance(dec.rnn, nn.StatelessRnn)
  assert isinstance(nn.RnnSandwich().layers[1], nn.Rnn) and isinstance(nn.FcStackOut(4, 2, 3).dense_out, nn.Dense)
  assert isinstance(nn.RnnFc(8, 4, rnn_type='gru', n_rnn=2).layers[2], nn.Fc)
  if not torch.cuda.is_available():
    with pytest.raises(_lib.DdspLibraryError):
      nn.Fc(4)(torch.zeros(2, 3))
    with pytest.raises(_lib.DdspLibraryError):
      nn.Rnn(4, 'gru')(torch.zeros(1, 2, 3))


def test_preprocessing_scalings_invert_each_other():
  """The scalings run kernels (core.hz_to_midi, core.midi_to_hz): here through the SIMT emulation, on host memory."""
  from tests.hip_emu import emu_simt
  assert preprocessing.F0_RANGE == 127.0 and preprocessing.DB_RANGE == 80.0
  assert 'preprocessing' in dir(__import__('ddsp_amd').training)
  if not torch.cuda.is_available():
    with pytest.raises(_lib.DdspLibraryError):
      preprocessing.scale_db(np.zeros(3))
  with emu_simt.emulated():
    db = torch.linspace(-80.0, 0.0, 9)
    scaled = preprocessing.scale_db(db)
    assert float(scaled[0]) == 0.0 and float(scaled[-1]) == 1.0
    assert torch.allclose(preprocessing.inv_scale_db(scaled), db, atol=1e-5)
    hz = torch.tensor([55.0, 220.0, 440.0, 4000.0])
    scaled = preprocessing.scale_f0_hz(hz)
    assert abs(float(scaled[2]) - 69.0 / 127.0) < 1e-6
    assert torch.allclose(preprocessing.inv_scale_f0_hz(scaled), hz, rtol=1e-5)
    f0, db_back = preprocessing.F0LoudnessPreprocessor.invert_scaling(scaled, preprocessing.scale_db(db))
    assert torch.allclose(f0, hz, rtol=1e-5) and torch.allclose(db_back, db, atol=1e-5)
    assert preprocessing.at_least_3d(torch.tensor(1.0)).shape == (1, 1, 1) and preprocessing.at_least_3d(torch.zeros(3)).shape == (1, 3, 1)
    assert preprocessing.at_least_3d(torch.zeros(2, 3)).shape == (2, 3, 1) and preprocessing.at_least_3d(torch.zeros(2, 3, 4)).shape == (2, 3, 4)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
  build_mod.build()
  return _lib.load()


def test_every_decoder_signature_is_declared_and_exported(lib):
  header = open(os.path.join(ROOT, 'ddsp_amd', 'csrc', 'decoder_abi.h')).read()
  header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
  declared = set(re.findall(r'\b(ddsp_[a-z0-9_]+)\s*\(', header))
  assert declared and declared == set(_lib.DECODER_SIGNATURES), declared ^ set(_lib.DECODER_SIGNATURES)
  assert not set(_lib.DECODER_SIGNATURES) & set(_lib.SIGNATURES)
  public = open(os.path.join(ROOT, 'include', 'ddsp_amd.h')).read()
  for name in declared:
    assert hasattr(lib, name) and name not in public, name
    fn = _lib.decoder_entry(lib, name)                    # idempotent
    assert fn.argtypes == _lib.DECODER_SIGNATURES[name][1] and _lib.decoder_entry(lib, name).restype is _lib.DECODER_SIGNATURES[name][0]
  for code, value in re.findall(r'#define DDSP_ACT_([A-Z_]+) (\d+)', header):
    assert _lib.ACTIVATIONS[code.lower()] == int(value)
  assert int(re.search(r'#define DDSP_GRU_MAX_HIDDEN (\d+)', header).group(1)) == _lib.GRU_MAX_HIDDEN


def test_workspace_queries(lib):
  assert lib.ddsp_gru_forward_workspace_bytes(2, 3) == 512                     # no packed matrix off the MFMA path
  assert lib.ddsp_gru_forward_workspace_bytes(32, 512) == 512 + 3 * 32 * 16 * 2 * 64 * 16
  assert lib.ddsp_gru_forward_workspace_bytes(2, 48) == 512 + 3 * 3 * 2 * 2 * 64 * 16       # K tail: two 32-deep steps for 48
  assert lib.ddsp_gru_backward_workspace_bytes(32, 512) == lib.ddsp_gru_forward_workspace_bytes(32, 512) + 2 * 32 * 512 * 4
  assert lib.ddsp_gru_forward_workspace_bytes(1, 4096) == 0
  assert lib.ddsp_bias_norm_act_backward_workspace_bytes(5, 64) == 2 * 4 * 3 * 64 * 4
  assert lib.ddsp_bias_norm_act_backward_workspace_bytes(10 ** 6, 512) == 256 * 4 * 3 * 512 * 4
  assert lib.ddsp_bias_norm_act_backward_workspace_bytes(0, 512) == 0


def test_null_pointers_bad_shapes_and_limits_return_codes(lib):
  p = 64                                                                       # any non-null value: nothing is launched
  assert lib.ddsp_bias_norm_act_f32(None, p, p, p, p, None, None, 1, 1, 0, 1e-3, None) == -1
  assert lib.ddsp_bias_norm_act_f32(p, p, p, p, p, p, None, 1, 1, 0, 1e-3, None) == -1      # xhat without rstd
  assert lib.ddsp_bias_norm_act_f32(p, p, p, p, p, None, None, 1, 0, 0, 1e-3, None) == -2
  assert lib.ddsp_bias_norm_act_f32(p, p, p, p, p, None, None, 1, 4, 5, 1e-3, None) == -2   # no such activation
  assert lib.ddsp_bias_norm_act_f32(p, p, p, p, p, None, None, 1, 1 << 24, 0, 1e-3, None) == -3
  assert lib.ddsp_bias_norm_act_f32(p, p, p, p, p, None, None, 0, 4, 0, 1e-3, None) == 0    # no rows: nothing to do
  assert lib.ddsp_bias_norm_act_backward_f32(p, p, p, p, p, p, None, p, 1 << 20, 1, 4, 0, None) == -1
  assert lib.ddsp_bias_norm_act_backward_f32(p, p, p, p, p, p, p, p, 16, 5, 64, 0, None) == -4
  assert lib.ddsp_bias_norm_act_backward_f32(p, p, p, p, p, p, p, None, 0, 5, 64, 0, None) == -1
  assert lib.ddsp_gru_forward_f32(None, p, p, p, p, None, p, 1 << 20, 1, 1, 16, None) == -1
  assert lib.ddsp_gru_forward_f32(p, p, p, p, p, None, p, 1 << 20, 1, 0, 16, None) == -2
  assert lib.ddsp_gru_forward_f32(p, p, p, p, p, None, p, 1 << 20, 1, 1, 0, None) == -2
  assert lib.ddsp_gru_forward_f32(p, p, p, p, p, None, p, 1 << 20, 1, 1, 2049, None) == -3
  assert lib.ddsp_gru_forward_f32(p, p, p, p, p, None, p, 1 << 20, 1 << 30, 1, 16, None) == -3
  assert lib.ddsp_gru_forward_f32(p, p, p, p, p, None, p, 16, 1, 1, 16, None) == -4
  assert lib.ddsp_gru_forward_f32(p, p, p, p, p, None, None, 0, 1, 1, 16, None) == -1
  assert lib.ddsp_gru_forward_f32(p, p, p, p, p, None, None, 0, 0, 1, 16, None) == 0        # no rows
  assert lib.ddsp_gru_backward_f32(p, p, p, None, p, p, p, p, p, 1 << 20, 1, 1, 16, None) == -1
  assert lib.ddsp_gru_backward_f32(p, p, p, p, p, p, p, p, p, 1 << 20, 1, 0, 16, None) == -2
  assert lib.ddsp_gru_backward_f32(p, p, p, p, p, p, p, p, p, 1 << 20, 1, 1, 4096, None) == -3
  assert lib.ddsp_gru_backward_f32(p, p, p, p, p, p, p, p, p, 16, 1, 1, 3, None) == -4
