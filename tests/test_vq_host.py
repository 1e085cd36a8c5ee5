"""What needs no GPU of ddsp_amd.training.nn's vector quantizer and of the small layers that came with it: the C ABI of
csrc/vq_abi.h against ddsp_amd._lib.VQ_SIGNATURES and the built library, and its error codes; every ValueError and limit of the
Python layer with no device present; the buffer names of VectorQuantization (through the SIMT emulation, on host memory);
polyphase_resample, straight_through_softmax and straight_through_choice on host tensors."""
import os
import re

import numpy as np
import pytest
import torch

from ddsp_amd import _lib
from ddsp_amd import build as build_mod
from ddsp_amd.training import nn
from tests.hip_emu import emu_simt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ddsp = emu_simt.ddsp_fixture()


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
  build_mod.build()
  return _lib.load()


def test_every_vq_signature_is_declared_and_exported(lib):
  header = open(os.path.join(ROOT, 'ddsp_amd', 'csrc', 'vq_abi.h')).read()
  limits = dict((name, int(value, 0)) for name, value in re.findall(r'#define DDSP_(VQ_[A-Z_]+) (\w+)', header))
  header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
  declared = set(re.findall(r'\b(ddsp_[a-z0-9_]+)\s*\(', header))
  assert declared and declared == set(_lib.VQ_SIGNATURES), declared ^ set(_lib.VQ_SIGNATURES)
  for other in (_lib.SIGNATURES, _lib.DECODER_SIGNATURES, _lib.NORM_SIGNATURES, _lib.CONV_SIGNATURES, _lib.CONV2D_SIGNATURES):
    assert not set(_lib.VQ_SIGNATURES) & set(other)
  public = open(os.path.join(ROOT, 'include', 'ddsp_amd.h')).read()
  for name in declared:
    assert hasattr(lib, name) and name not in public, name
    fn = _lib.vq_entry(lib, name)                         # idempotent
    assert fn.argtypes == _lib.VQ_SIGNATURES[name][1] and _lib.vq_entry(lib, name).restype is _lib.VQ_SIGNATURES[name][0]
  assert 'vq.hip' in build_mod.SOURCES
  assert limits == {'VQ_MAX_CENTROIDS': _lib.VQ_MAX_CENTROIDS, 'VQ_MAX_DIMS': _lib.VQ_MAX_DIMS}


def test_workspace_query(lib):
  ws = lib.ddsp_vq_workspace_bytes
  assert ws(3, 3) == 512 + 256                                                  # the plain kernel: the header and |e|^2 / 2
  assert ws(16, 8) == 512 + 256 + 1 * 1 * 128 * 16                              # one (step, tile) of fragments hi / lo
  assert ws(1024, 64) == 512 + 4096 + 2 * 64 * 128 * 16
  assert ws(4096, 512) == 512 + 16384 + 16 * 256 * 128 * 16
  assert ws(0, 4) == 0 and ws(4, 0) == 0 and ws(4097, 4) == 0 and ws(4, 513) == 0


def test_null_pointers_bad_shapes_and_limits_return_codes(lib):
  p = 64                                                                        # any non-null value: nothing is launched
  ok = dict(x=p, e=p, c=p, z=p, ws=p, ws_bytes=1 << 20, rows=4, heads=2, k=16, dims=8, stream=None)
  assign = lambda **kw: lib.ddsp_vq_assign_f32(*dict(ok, **kw).values())
  for name in ('x', 'e', 'c', 'z', 'ws'):
    assert assign(**{name: None}) == -1, name
  for bad in (dict(rows=-1), dict(heads=0), dict(k=0), dict(dims=0)):
    assert assign(**bad) == -2, bad
  for beyond in (dict(k=4097), dict(dims=513), dict(rows=1 << 30, heads=2)):
    assert assign(**beyond) == -3, beyond
  assert assign(ws_bytes=16) == -4
  assert assign(rows=0, ws=None) == 0                                           # an empty batch: a no-op
  ok = dict(x=p, c=p, counts=p, sums=p, rows=4, heads=2, k=16, dims=8, stream=None)
  stats = lambda **kw: lib.ddsp_vq_statistics_f32(*dict(ok, **kw).values())
  for name in ('x', 'c', 'counts', 'sums'):
    assert stats(**{name: None}) == -1, name
  for bad in (dict(rows=-1), dict(heads=0), dict(k=0), dict(dims=0)):
    assert stats(**bad) == -2, bad
  for beyond in (dict(k=4097), dict(dims=513), dict(rows=1 << 30, heads=2)):
    assert stats(**beyond) == -3, beyond


# ---- the Python layer's errors: raised before anything touches a device ---------------------------------------------------
def test_shape_errors():
  x, e = torch.zeros(3, 8), torch.zeros(5, 4)
  with pytest.raises(ValueError, match=r'Input depth must be a multiple of the number of heads\.'):
    nn.vq_assign(x, e, num_heads=3)
  with pytest.raises(ValueError, match=r'e must be \[k, depth / num_heads\] = \[k, 4\], got \(5, 8\)'):
    nn.vq_assign(x, torch.zeros(5, 8), num_heads=2)
  with pytest.raises(ValueError, match=r'e must be \[k, depth / num_heads\], got \(5,\)'):
    nn.vq_assign(x, torch.zeros(5), num_heads=2)
  with pytest.raises(ValueError, match=r'x must be \[\.\.\., depth\] with depth >= 1, got \(\)'):
    nn.vq_assign(torch.zeros(()), e)
  with pytest.raises(ValueError, match=r'k and num_heads must be at least 1, got k = 5, num_heads = 0'):
    nn.vq_assign(x, e, num_heads=0)
  with pytest.raises(ValueError, match=r'k and num_heads must be at least 1, got k = 0, num_heads = 2'):
    nn.vq_statistics(x, torch.zeros(3, 2, dtype=torch.int64), 0, num_heads=2)
  with pytest.raises(ValueError, match=r'c must hold integers of shape \(3, 2\), got torch.int64 of \(3, 1\)'):
    nn.vq_statistics(x, torch.zeros(3, 1, dtype=torch.int64), 5, num_heads=2)
  with pytest.raises(ValueError, match=r'c must hold integers of shape \(3, 2\), got torch.float32 of \(3, 2\)'):
    nn.vq_statistics(x, torch.zeros(3, 2), 5, num_heads=2)
  with pytest.raises(ValueError, match=r'Input depth must be a multiple of the number of heads\.'):
    nn.VectorQuantization(8, num_heads=3).build(8)


def test_limits_one_past():
  many = torch.zeros(1, 1).expand(2 ** 31, 1)                                    # stride 0: no memory behind it
  with pytest.raises(NotImplementedError, match=r'at most 4096 centroids of 512 dims per head on the MI355X path, got k = 4097, depth / num_heads = 4'):
    nn.vq_assign(torch.zeros(2, 8), torch.zeros(4097, 4), num_heads=2)
  with pytest.raises(NotImplementedError, match=r'at most 4096 centroids of 512 dims per head on the MI355X path, got k = 2, depth / num_heads = 513'):
    nn.vq_assign(torch.zeros(2, 1026), torch.zeros(2, 513), num_heads=2)
  with pytest.raises(NotImplementedError, match=r'rows \* num_heads must stay below 2 \*\* 31, got rows = 2147483648, num_heads = 1'):
    nn.vq_assign(many, torch.zeros(2, 1))
  with pytest.raises(NotImplementedError, match=r'vq_statistics: at most 4096 centroids .* got k = 4097, depth / num_heads = 4'):
    nn.vq_statistics(torch.zeros(2, 8), torch.zeros(2, 2, dtype=torch.int64), 4097, num_heads=2)
  with pytest.raises(NotImplementedError, match=r'vq_statistics: rows \* num_heads must stay below 2 \*\* 31, got rows = 1073741824, num_heads = 2'):
    nn.vq_statistics(torch.zeros(1, 2).expand(2 ** 30, 2), torch.zeros(1, 2, dtype=torch.int64).expand(2 ** 30, 2), 4, num_heads=2)
  with pytest.raises(NotImplementedError, match=r'VectorQuantization: at most 4096 centroids .* got k = 4097, depth / num_heads = 8'):
    nn.VectorQuantization(4097).build(8)
  with pytest.raises(NotImplementedError, match=r'VectorQuantization: at most 4096 centroids .* got k = 4, depth / num_heads = 513'):
    nn.VectorQuantization(4, num_heads=2).build(1026)


def test_state_dict_holds_the_reference_variable_names(ddsp):
  layer = nn.VectorQuantization(6, num_heads=2)
  assert not layer.state_dict() and layer.name == 'vector_quantization'
  layer.build(10)
  state = layer.state_dict()
  assert list(state) == ['counts', 'sums'] and tuple(state['counts'].shape) == (6,) and tuple(state['sums'].shape) == (6, 5)
  assert not state['counts'].any() and not state['sums'].any() and not list(layer.parameters())
  other = nn.VectorQuantization(6, num_heads=2, name='vq2')
  other.build(10)
  other.load_state_dict({'counts': torch.arange(6.0), 'sums': torch.ones(6, 5)})
  assert torch.equal(other.centroids()[0], torch.zeros(5)) and torch.equal(other.centroids()[2], torch.full((5,), 0.5))
  z = torch.zeros(2, 10)
  assert list(other.get_losses_dict(z, z)) == ['vq2_commitment_loss']


# ---- polyphase_resample ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_t, stride', [(4, 2), (5, 5), (4, 1)])
def test_reconstructions_are_lossless(n_t, stride):
  """The reference's PolyphaseResampleTest, case by case."""
  x = torch.arange(n_t).reshape(1, n_t, 1).repeat(2, 1, 3)
  x_down = nn.polyphase_resample(x, stride, 'down', trim_or_pad='pad')
  assert tuple(x_down.shape) == (2, n_t // stride, 3 * stride)
  x_recon = nn.polyphase_resample(x_down, stride, 'up', trim_or_pad='pad')
  assert torch.equal(x, x_recon)


def test_polyphase_pads_trims_and_keeps_the_rank():
  x = torch.arange(2 * 5 * 3, dtype=torch.float32).reshape(2, 5, 3)
  down = nn.polyphase_resample(x, 2, 'down')                                    # time 5 -> 6 -> 3
  assert tuple(down.shape) == (2, 3, 6) and torch.equal(down[:, :2].reshape(2, 4, 3), x[:, :4]) and not down[:, 2, 3:].any()
  assert torch.equal(nn.polyphase_resample(down, 2, 'up')[:, :5], x)             # reconstructs x up to the padding
  trimmed = nn.polyphase_resample(x, 2, 'down', trim_or_pad='trim')             # time 5 -> 4 -> 2
  assert tuple(trimmed.shape) == (2, 2, 6) and torch.equal(trimmed.reshape(2, 4, 3), x[:, :4])
  up = nn.polyphase_resample(x, 2, 'up')                                        # ch 3 -> 4 -> 2
  assert tuple(up.shape) == (2, 10, 2) and torch.equal(up.reshape(2, 5, 4)[:, :, :3], x) and not up.reshape(2, 5, 4)[:, :, 3].any()
  up_trimmed = nn.polyphase_resample(x, 2, 'up', trim_or_pad='trim')            # ch 3 -> 2 -> 1
  assert tuple(up_trimmed.shape) == (2, 10, 1) and torch.equal(up_trimmed.reshape(2, 5, 2), x[:, :, :2])
  assert torch.equal(nn.polyphase_resample(x, 2, 'down', trim_or_pad='anything'), trimmed)        # the reference's quirk: not 'pad' is 'trim'
  x4 = x[:, :, None, :]
  for kind in ('down', 'up'):
    out = nn.polyphase_resample(x4, 2, kind)
    assert out.dim() == 4 and out.shape[2] == 1 and torch.equal(out[:, :, 0, :], nn.polyphase_resample(x, 2, kind))
    assert torch.equal(nn.PolyphaseResample(2, kind, 'trim')(x), nn.polyphase_resample(x, 2, kind, 'trim'))
  with pytest.raises(ValueError, match='`resample_type` must be either "up" or "down"'):
    nn.polyphase_resample(x, 2, 'sideways')


def test_polyphase_gradient():
  x = torch.randn(2, 5, 3, dtype=torch.float64, requires_grad=True)
  for kind in ('down', 'up'):
    y = nn.polyphase_resample(x, 2, kind)
    w = torch.randn_like(y)
    grad, = torch.autograd.grad((y * w).sum(), x)
    back = nn.polyphase_resample(w, 2, 'up' if kind == 'down' else 'down')      # the adjoint of pad + reshape: reshape back, drop the padding
    assert torch.equal(grad, back[:, :5, :3])


# ---- the straight-through estimators ---------------------------------------------------------------------------------------
def test_straight_through_softmax():
  torch.manual_seed(5)
  logits = torch.randn(4, 6, 5, requires_grad=True)
  sample, probs = nn.straight_through_softmax(logits)
  onehot = sample.detach().round()
  assert tuple(sample.shape) == (4, 6, 5) and float((sample.detach() - onehot).abs().max()) <= 1e-6
  assert torch.equal(onehot.sum(-1), torch.ones(4, 6)) and set(onehot.unique().tolist()) == {0.0, 1.0}
  assert torch.allclose(probs, torch.softmax(logits, -1), rtol=0, atol=1e-7)
  w = torch.randn(4, 6, 5)
  grad, = torch.autograd.grad((sample * w).sum(), logits, retain_graph=True)
  want, = torch.autograd.grad((torch.softmax(logits, -1) * onehot * w).sum(), logits)
  assert torch.allclose(grad, want, rtol=0, atol=1e-7)
  draws = torch.stack([nn.straight_through_softmax(torch.tensor([0.0, 50.0, 0.0]))[0] for _ in range(20)])
  assert torch.equal(draws.round(), torch.tensor([0.0, 1.0, 0.0]).expand(20, 3))          # the draw follows the probabilities


def test_straight_through_choice():
  torch.manual_seed(6)
  logits, values = torch.randn(3, 7, 4), torch.randn(3, 7, 4)
  choice = nn.straight_through_choice(logits, values)
  assert tuple(choice.shape) == (3, 7, 1)
  assert bool(((choice - values).abs() <= 1e-5 * values.abs().max()).any(-1).all())     # one of the values, up to the estimator's rounding
  sure = nn.straight_through_choice(torch.tensor([[0.0, 60.0]]), torch.tensor([[1.5, -2.5]]))
  assert tuple(sure.shape) == (1, 1) and abs(float(sure) + 2.5) <= 1e-6
