"""Host tests of the dilated convolution stack (no GPU): tests/dilated_conv_truth.py's explicit shifted sums against an
independent statement in fp64 - F.conv1d(padding=..., dilation=...) / F.conv_transpose1d on the permuted tensor - to 1e-12 in
values and gradients, for even and odd K and every stride the GPU tests use, and the upsampler against the adjoint of the
downsampler; constructor defaults and argument order against values typed in from the reference; weight names and shapes and the
output lengths of resampling stacks (the kernels through the SIMT emulation, on host memory); every ValueError; the C ABI of
csrc/conv_abi.h against ddsp_amd._lib.CONV_SIGNATURES and the built library, and its error codes."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dilated_conv_truth as T
from ddsp_amd import _lib
from ddsp_amd import build as build_mod
from ddsp_amd.training import decoders, nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


def _close(a, b):
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  assert a.shape == b.shape
  assert float(np.max(np.abs(a - b))) <= TOL * max(1.0, float(np.max(np.abs(b)))), float(np.max(np.abs(a - b)))


# ---- the truth against an independent implementation ---------------------------------------------------------------------
@pytest.mark.parametrize('relu', [False, True], ids=['linear', 'relu'])
@pytest.mark.parametrize('steps, ch_in, ch_out, taps, dilation', [(1, 1, 1, 1, 1), (20, 2, 4, 3, 1), (20, 4, 4, 3, 4), (5, 3, 2, 3, 8), (9, 3, 5, 2, 1),
                                                                  (9, 2, 3, 4, 3), (11, 2, 2, 5, 2), (7, 1, 2, 16, 1)])
def test_truth_conv_is_conv1d_of_torch_with_tf_same_padding(steps, ch_in, ch_out, taps, dilation, relu):
  rng = np.random.default_rng(21)
  x, kernel, bias = rng.standard_normal((2, steps, ch_in)), rng.standard_normal((taps, ch_in, ch_out)), rng.standard_normal(ch_out)
  cot = rng.standard_normal((2, steps, ch_out))
  leaves = [torch.tensor(v, requires_grad=True) for v in (x, kernel, bias)]
  total = (taps - 1) * dilation
  a = F.relu(leaves[0]) if relu else leaves[0]
  padded = F.pad(a.permute(0, 2, 1), (total // 2, total - total // 2))            # TF 'same': the odd one goes right
  want = F.conv1d(padded, leaves[1].permute(2, 1, 0), leaves[2], dilation=dilation).permute(0, 2, 1)
  fn = lambda *args: T.conv(*args, dilation=dilation, relu_input=relu)
  _close(fn(x, kernel, bias).numpy(), want.detach().numpy())
  _close(T.conv(x[:, :, None, :], kernel[:, None], bias, dilation, relu)[:, :, 0].numpy(), want.detach().numpy())
  assert T.conv(x, kernel, bias, dilation, relu, dtype=torch.float32).dtype is torch.float32
  for got, ref in zip(T.grads(fn, (x, kernel, bias), [cot]), torch.autograd.grad(want, leaves, torch.tensor(cot))):
    _close(got, ref.numpy())


def test_truth_relu_gradient_at_zero_is_zero():
  x = np.array([[[0.0, -1.0], [2.0, 0.0], [-0.0, 3.0]]])
  kernel = np.ones((1, 2, 1))
  got, = T.grads(lambda x_: T.conv(x_, kernel, None, 1, True), [x], [np.ones((1, 3, 1))])
  assert np.array_equal(got, (x > 0).astype(np.float64))


@pytest.mark.parametrize('steps, stride', [(8, 2), (9, 2), (1, 2), (10, 3), (7, 4)])
def test_truth_downsample_is_strided_conv1d_with_tf_same_padding(steps, stride):
  rng = np.random.default_rng(22)
  x, kernel, bias = rng.standard_normal((2, steps, 3)), rng.standard_normal((stride, 3, 4)), rng.standard_normal(4)
  out = -(-steps // stride)
  total = max((out - 1) * stride + stride - steps, 0)
  leaves = [torch.tensor(v, requires_grad=True) for v in (x, kernel, bias)]
  padded = F.pad(leaves[0].permute(0, 2, 1), (total // 2, total - total // 2))
  want = F.conv1d(padded, leaves[1].permute(2, 1, 0), leaves[2], stride=stride).permute(0, 2, 1)
  assert want.shape == (2, out, 4)
  fn = lambda *args: T.downsample(*args, stride)
  _close(fn(x, kernel, bias).numpy(), want.detach().numpy())
  cot = rng.standard_normal((2, out, 4))
  for got, ref in zip(T.grads(fn, (x, kernel, bias), [cot]), torch.autograd.grad(want, leaves, torch.tensor(cot))):
    _close(got, ref.numpy())


@pytest.mark.parametrize('steps, stride', [(5, 2), (1, 2), (4, 3), (3, 4)])
def test_truth_upsample_is_conv_transpose1d_cropped_and_the_adjoint_of_the_same_convolution(steps, stride):
  rng = np.random.default_rng(23)
  taps = 2 * stride
  x, kernel, bias = rng.standard_normal((2, steps, 3)), rng.standard_normal((taps, 4, 3)), rng.standard_normal(4)
  leaves = [torch.tensor(v, requires_grad=True) for v in (x, kernel, bias)]
  full = F.conv_transpose1d(leaves[0].permute(0, 2, 1), leaves[1].permute(2, 1, 0), leaves[2], stride=stride)
  want = full[:, :, stride // 2:stride // 2 + steps * stride].permute(0, 2, 1)
  assert want.shape == (2, steps * stride, 4)
  fn = lambda *args: T.upsample(*args, stride)
  _close(fn(x, kernel, bias).numpy(), want.detach().numpy())
  cot = rng.standard_normal((2, steps * stride, 4))
  for got, ref in zip(T.grads(fn, (x, kernel, bias), [cot]), torch.autograd.grad(want, leaves, torch.tensor(cot))):
    _close(got, ref.numpy())
  # TF defines conv2d_transpose as the input gradient of the 'same' convolution that maps steps * stride rows to steps: <down(u), x> = <u, up(x)>
  u, zero3, zero4 = rng.standard_normal((2, steps * stride, 4)), np.zeros(3), np.zeros(4)
  down = T.downsample(u, kernel, zero3, stride)                                    # the same array read as [k, ci = 4, co = 3]
  assert down.shape == (2, steps, 3)
  lhs = float((down * torch.tensor(x)).sum())
  rhs = float((torch.tensor(u) * T.upsample(x, kernel, zero4, stride)).sum())
  assert abs(lhs - rhs) <= 1e-11 * max(1.0, abs(lhs))


# ---- the reference's interface --------------------------------------------------------------------------------------------
def _signature(cls):
  return [(p.name, p.default) for p in list(inspect.signature(cls.__init__).parameters.values())[1:] if p.kind is not p.VAR_KEYWORD]


def test_constructor_arguments_order_and_defaults_are_the_references():
  # typed in from ddsp/training/nn.py:1156-1171 and ddsp/training/decoders.py:225-241
  assert _signature(nn.DilatedConvStack) == [
      ('ch', 256), ('layers_per_stack', 5), ('stacks', 2), ('kernel_size', 3), ('dilation', 2), ('norm_type', None), ('resample_type', None),
      ('resample_stride', 1), ('stacks_per_resample', 1), ('resample_after_convolve', True), ('spectral_norm', False), ('ortho_init', False),
      ('shift_only', False), ('conditional', False)]
  assert _signature(decoders.DilatedConvDecoder) == [
      ('ch', 256), ('kernel_size', 3), ('layers_per_stack', 5), ('stacks', 2), ('dilation', 2), ('norm_type', 'layer'), ('resample_stride', 1),
      ('stacks_per_resample', 1), ('resample_after_convolve', True), ('input_keys', ('ld_scaled', 'f0_scaled')),
      ('output_splits', (('amps', 1), ('harmonic_distribution', 60))), ('conditioning_keys', 'z'), ('precondition_stack', None),
      ('spectral_norm', False), ('ortho_init', False)]
  assert [(p.name, p.default) for p in inspect.signature(nn.dilated_conv).parameters.values()] == [
      ('x', inspect.Parameter.empty), ('kernel', inspect.Parameter.empty), ('bias', None), ('dilation', 1), ('relu_input', False)]


def test_decoder_keys_and_conditioning():
  dec = decoders.DilatedConvDecoder()
  assert dec.conditioning_keys == ['z'] and dec.input_keys == ['ld_scaled', 'f0_scaled', 'z'] and dec.conditional and dec.n_conditioning == 1
  assert dec.output_keys == ['amps', 'harmonic_distribution'] and dec.n_out == 61 and dec.dilated_conv_stack.conditional
  dec = decoders.DilatedConvDecoder(conditioning_keys=None)
  assert dec.input_keys == ['ld_scaled', 'f0_scaled'] and not dec.conditional and not dec.dilated_conv_stack.conditional
  dec = decoders.DilatedConvDecoder(conditioning_keys=('z', 'q_pitch'), precondition_stack=nn.Identity(), resample_stride=2)
  assert dec.input_keys[-2:] == ['z', 'q_pitch'] and len(dec.dilated_conv_stack.resample_layers) == 2
  assert all(isinstance(layer, nn.Conv2DTranspose) for layer in dec.dilated_conv_stack.resample_layers)


def test_stack_layer_lists_and_dilation_rates():
  stack = nn.DilatedConvStack(ch=8, layers_per_stack=3, stacks=2, dilation=2)
  assert len(stack.layers) == len(stack.norms) == 6 and len(stack.resample_layers) == 0 and stack.layers_per_resample == 0
  assert [layer.conv.dilation_rate for layer in stack.layers] == [1, 2, 4, 1, 2, 4] == T.dilations(3, 2, 2)
  assert stack.conv_in.dilation_rate == 1 and stack.conv_in.kernel_size == 3 and all(isinstance(n, nn.Normalize) for n in stack.norms)
  down = nn.DilatedConvStack(ch=8, layers_per_stack=3, stacks=2, dilation=-2, conditional=True, norm_type='layer')
  assert [layer.conv.dilation_rate for layer in down.layers] == [4, 2, 1, 4, 2, 1] == T.dilations(3, 2, -2)
  assert all(isinstance(n, nn.ConditionalNorm) and n.norm_type == 'layer' for n in down.norms)
  assert T.dilations(3, 1, 1.5) == [1, 1, 2]                                       # int() truncates, as the reference's does
  assert [layer.conv.dilation_rate for layer in nn.DilatedConvStack(layers_per_stack=3, stacks=1, dilation=1.5).layers] == [1, 1, 2]
  for after in (True, False):
    stack = nn.DilatedConvStack(ch=8, layers_per_stack=2, stacks=4, resample_type='downsample', resample_stride=3, stacks_per_resample=2,
                                resample_after_convolve=after)
    assert len(stack.resample_layers) == 2 and stack.layers_per_resample == 4
    assert all(isinstance(r, nn.Conv2D) and r.strides == 3 and r.kernel_size == 3 for r in stack.resample_layers)
  up = nn.DilatedConvStack(ch=8, resample_type='upsample', resample_stride=2, ortho_init=True)
  assert all(isinstance(r, nn.Conv2DTranspose) and r.strides == 2 and r.kernel_size == 4 and r.kernel_initializer == 'orthogonal'
             for r in up.resample_layers)


def test_every_value_error():
  with pytest.raises(ValueError, match='not built on the MI355X path'):
    nn.DilatedConvStack(spectral_norm=True)
  with pytest.raises(ValueError, match='not built on the MI355X path'):
    decoders.DilatedConvDecoder(spectral_norm=True)
  with pytest.raises(ValueError, match=re.escape('invalid resample type: sideways, must be either `upsample` or `downsample`.')):
    nn.DilatedConvStack(resample_type='sideways')
  with pytest.raises(ValueError, match=re.escape('You must specify conditioning keys if you specifya precondition stack.')):
    decoders.DilatedConvDecoder(conditioning_keys=None, precondition_stack=nn.Identity())
  with pytest.raises(ValueError, match='kernel_initializer'):
    nn.Conv2D(4, 3, kernel_initializer='he_normal')
  with pytest.raises(ValueError, match='over time only'):
    nn.Conv2D(4, (3, 3))
  with pytest.raises(ValueError, match='kernel_size'):
    nn.Conv2DTranspose(4, 2, 3)
  x, kernel = torch.zeros(1, 4, 2), torch.zeros(3, 2, 4)
  for bad_x, bad_kernel, bias, dilation, match in [
      (torch.zeros(4, 2), kernel, None, 1, 'x must be'), (torch.zeros(1, 4, 2, 2), kernel, None, 1, 'x must be'),
      (x, torch.zeros(2, 4), None, 1, 'kernel must be'), (x, torch.zeros(3, 2, 2, 4), None, 1, 'kernel must be'),
      (x, torch.zeros(3, 3, 4), None, 1, 'agree in ch_in'), (torch.zeros(1, 0, 2), kernel, None, 1, 'at least 1'),
      (x, kernel, torch.zeros(3), 1, 'bias must be'), (x, kernel, None, 0, 'dilation must be at least 1'),
      (torch.zeros(1, 1, 1040), torch.zeros(1, 1040, 16), None, 1, '1024'), (x, torch.zeros(17, 2, 4), None, 1, '16 taps'),
      (x, kernel, None, 2 ** 30, '2 \\*\\* 31'), (torch.zeros(1, 1, 2).expand(1 << 16, 1 << 14, 2), kernel, None, 1, '2 \\*\\* 31')]:
    with pytest.raises(ValueError, match=match):                                  # before anything touches the device: none is here
      nn.dilated_conv(bad_x, bad_kernel, bias, dilation)


# ---- weights and lengths (the kernels through the SIMT emulation, on host memory) -----------------------------------------
@pytest.fixture
def emulated():
  from tests.hip_emu import emu_simt
  if not os.path.exists(emu_simt.CLANG):
    pytest.skip('the SIMT emulation builds with the ROCm clang++, which this machine does not have')
  with emu_simt.emulated():
    yield


def test_weight_names_shapes_and_initialisers(emulated):
  torch.manual_seed(3)
  dec = decoders.DilatedConvDecoder(ch=4, layers_per_stack=2, stacks=1, input_keys=('ld_scaled', 'f0_scaled'), conditioning_keys=('z',),
                                    output_splits=(('amps', 1), ('harmonic_distribution', 3)), resample_stride=2)
  out = dec(dict(ld_scaled=torch.zeros(2, 5, 1), f0_scaled=torch.zeros(2, 5, 1), z=torch.ones(2, 5, 6)))
  assert list(out) == ['amps', 'harmonic_distribution'] and out['harmonic_distribution'].shape == (2, 10, 3)
  shapes = {name: tuple(p.shape) for name, p in dec.named_parameters()}
  assert shapes == {
      'dense_out.kernel': (4, 4), 'dense_out.bias': (4,),
      'dilated_conv_stack.conv_in.kernel': (3, 1, 2, 4), 'dilated_conv_stack.conv_in.bias': (4,),
      'dilated_conv_stack.layers.0.conv.kernel': (3, 1, 4, 4), 'dilated_conv_stack.layers.0.conv.bias': (4,),
      'dilated_conv_stack.layers.1.conv.kernel': (3, 1, 4, 4), 'dilated_conv_stack.layers.1.conv.bias': (4,),
      'dilated_conv_stack.norms.0.conditional_scale_and_shift.dense.kernel': (6, 8),
      'dilated_conv_stack.norms.0.conditional_scale_and_shift.dense.bias': (8,),
      'dilated_conv_stack.norms.1.conditional_scale_and_shift.dense.kernel': (6, 8),
      'dilated_conv_stack.norms.1.conditional_scale_and_shift.dense.bias': (8,),
      'dilated_conv_stack.resample_layers.0.kernel': (4, 1, 4, 4), 'dilated_conv_stack.resample_layers.0.bias': (4,)}
  conv = nn.Conv2D(6, 3)
  conv.build(10)
  assert tuple(conv.kernel.shape) == (3, 1, 10, 6) and float(conv.kernel.detach().abs().max()) <= (6.0 / (3 * 10 + 3 * 6)) ** 0.5 and not conv.bias.any()
  ortho = nn.Conv2D(6, 3, kernel_initializer='orthogonal')
  ortho.build(10)
  flat = ortho.kernel.detach().reshape(30, 6).double()
  assert torch.allclose(flat.t() @ flat, torch.eye(6, dtype=torch.float64), atol=1e-5)
  up = nn.Conv2DTranspose(6, 4, 2, kernel_initializer='orthogonal')
  up.build(3)
  flat = up.kernel.detach().reshape(24, 3).double()
  assert tuple(up.kernel.shape) == (4, 1, 6, 3) and torch.allclose(flat.t() @ flat, torch.eye(3, dtype=torch.float64), atol=1e-5)


@pytest.mark.parametrize('after', [True, False], ids=['resample_after', 'resample_before'])
@pytest.mark.parametrize('resample_type, stride, stacks, per', [('upsample', 2, 2, 1), ('downsample', 2, 2, 1), ('upsample', 3, 4, 2), ('downsample', 3, 4, 2)])
def test_output_lengths_of_resampling_stacks(emulated, resample_type, stride, stacks, per, after):
  steps = 36
  stack = nn.DilatedConvStack(ch=4, layers_per_stack=1, stacks=stacks, resample_type=resample_type, resample_stride=stride, stacks_per_resample=per,
                              resample_after_convolve=after)
  factor = stride ** (stacks // per)
  assert len(stack.resample_layers) == stacks // per
  y = stack(torch.ones(2, steps, 3))
  assert y.shape == (2, steps * factor if resample_type == 'upsample' else steps // factor, 4) and bool(torch.isfinite(y).all())


def test_layers_construct_without_a_gpu_and_fail_loudly_when_called():
  stack = nn.DilatedConvStack(ch=16)
  assert not stack.conv_in.built
  if not torch.cuda.is_available():
    with pytest.raises(_lib.DdspLibraryError):
      stack(torch.zeros(1, 4, 2))
    with pytest.raises(_lib.DdspLibraryError):
      nn.dilated_conv(torch.zeros(1, 4, 2), torch.zeros(3, 2, 16))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
  build_mod.build()
  return _lib.load()


def test_every_conv_signature_is_declared_and_exported(lib):
  header = open(os.path.join(ROOT, 'ddsp_amd', 'csrc', 'conv_abi.h')).read()
  flags = dict((name, int(value.rstrip('u'), 0)) for name, value in re.findall(r'#define DDSP_(CONVD_[A-Z_]+) (\w+)', header))
  header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
  declared = set(re.findall(r'\b(ddsp_[a-z0-9_]+)\s*\(', header))
  assert declared and declared == set(_lib.CONV_SIGNATURES), declared ^ set(_lib.CONV_SIGNATURES)
  for other in (_lib.SIGNATURES, _lib.DECODER_SIGNATURES, _lib.NORM_SIGNATURES):
    assert not set(_lib.CONV_SIGNATURES) & set(other)
  public = open(os.path.join(ROOT, 'include', 'ddsp_amd.h')).read()
  for name in declared:
    assert hasattr(lib, name) and name not in public, name
    fn = _lib.conv_entry(lib, name)                       # idempotent
    assert fn.argtypes == _lib.CONV_SIGNATURES[name][1] and _lib.conv_entry(lib, name).restype is _lib.CONV_SIGNATURES[name][0]
  assert 'dilated_conv.hip' in build_mod.SOURCES
  assert flags == {name: getattr(_lib, name) for name in ('CONVD_MAX_CHANNELS', 'CONVD_MAX_TAPS', 'CONVD_RELU_INPUT', 'CONVD_TRANSPOSE_W',
                                                            'CONVD_MASK_OUTPUT')}


def test_workspace_queries(lib):
  ws = lib.ddsp_dilated_conv_workspace_bytes
  assert ws(2, 20, 2, 4, 3) == 0                                                # the plain kernel needs none
  assert ws(3, 70, 128, 128, 3) == 512 + 256 + 3 * 4 * 8 * 128 * 16           # header, room for 3 x 16 row partials, (tap, step, tile) fragments hi / lo
  assert ws(32, 1000, 2, 128, 3) == 512 + 32 * 16 * 4 + 3 * 1 * 8 * 128 * 16
  assert ws(2, 20, 32, 272, 3) == 512 + 256 + 3 * 1 * 17 * 128 * 16
  assert ws(0, 5, 16, 16, 3) == 0 and ws(1, 5, 1040, 16, 3) == 0 and ws(1, 5, 16, 16, 17) == 0 and ws(1 << 11, 1 << 10, 16, 1 << 10, 1) == 0


def test_null_pointers_bad_shapes_and_limits_return_codes(lib):
  p = 64                                                                       # any non-null value: nothing is launched
  conv = lib.ddsp_dilated_conv_f32
  ok = dict(x=p, w=p, bias=None, addend=None, mask=None, y=p, ws=None, ws_bytes=0, batch=1, time=4, ch_in=2, ch_out=16, taps=3, dilation=1,
            pad_left=1, flags=0, stream=None)
  call = lambda **kw: conv(*dict(ok, **kw).values())
  assert call(x=None) == -1 and call(w=None) == -1 and call(y=None) == -1
  assert call(flags=_lib.CONVD_MASK_OUTPUT) == -1                                # a mask without its source
  assert call() == -1                                                            # the matrix-core path without a workspace
  assert call(ws=p, ws_bytes=16) == -4
  for bad in (dict(batch=-1), dict(time=0), dict(ch_in=0), dict(ch_out=0), dict(taps=0), dict(dilation=0), dict(pad_left=-1), dict(pad_left=3),
              dict(flags=0x8)):
    assert call(**bad) == -2, bad
  for beyond in (dict(ch_in=1040), dict(ch_out=1040), dict(taps=17), dict(batch=1 << 11, time=1 << 10, ch_in=1 << 10),
                 dict(batch=1 << 11, time=1 << 10, ch_out=1 << 10), dict(dilation=1 << 30, pad_left=0)):
    assert call(**beyond) == -3, beyond
  assert call(batch=0) == 0                                                      # no rows: nothing to do
