"""Host tests of the normalisations and the encoders (no GPU): tests/encoder_truth.py against an independent implementation in
fp64 (torch.nn.functional.group_norm on the permuted tensor) to 1e-12 in values and gradients; why the x = 100 + N(0, 1) case of
tests/test_gpu_encoder.py tells a one-pass variance from a two-pass one; the C ABI of csrc/norm_abi.h against
ddsp_amd._lib.NORM_SIGNATURES and the built library, and its error codes; the reference's error texts; ZEncoder's keys; the frame
counts of the five z_time_steps specs."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import encoder_truth as T
from ddsp_amd import _lib
from ddsp_amd import build as build_mod
from ddsp_amd.training import encoders, nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


def _close(a, b):
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  assert a.shape == b.shape
  assert float(np.max(np.abs(a - b))) <= TOL * max(1.0, float(np.max(np.abs(b)))), float(np.max(np.abs(a - b)))


# ---- the truth against an independent implementation ---------------------------------------------------------------------
@pytest.mark.parametrize('shape, norm_type', [((2, 5, 3, 6), 'instance'), ((3, 4, 1, 7), 'layer'), ((2, 3, 2, 64), 'group'),
                                              ((2, 1, 1, 96), 'group')])
def test_truth_normalize_op_is_group_norm_of_torch(shape, norm_type):
  rng = np.random.default_rng(11)
  x, cot = rng.standard_normal(shape), rng.standard_normal(shape)
  groups = T.N_GROUPS[norm_type](shape[-1])
  leaf = torch.tensor(x, requires_grad=True)
  want = F.group_norm(leaf.permute(0, 3, 1, 2), groups, eps=1e-5).permute(0, 2, 3, 1)
  _close(T.normalize_op(x, norm_type).numpy(), want.detach().numpy())
  assert T.normalize_op(x, norm_type, dtype=torch.float32).dtype is torch.float32
  fn = lambda x_: T.normalize_op(x_, norm_type)
  _close(T.grads(fn, [x], [cot])[0], torch.autograd.grad(want, [leaf], torch.tensor(cot))[0].numpy())
  assert T.normalize_op(x, None).numpy().shape == shape


def test_truth_normalize_is_group_norm_with_weights():
  rng = np.random.default_rng(12)
  x, cot = rng.standard_normal((2, 7, 8)), rng.standard_normal((2, 7, 8))
  scale, shift = 1.0 + 0.3 * rng.standard_normal((1, 1, 1, 8)), rng.standard_normal((1, 1, 1, 8))
  leaves = [torch.tensor(v, requires_grad=True) for v in (x, scale, shift)]
  want = F.group_norm(leaves[0][:, :, None, :].permute(0, 3, 1, 2), 8, leaves[1].reshape(-1), leaves[2].reshape(-1), eps=1e-5)
  want = want.permute(0, 2, 3, 1)[:, :, 0, :]
  fn = lambda *a: T.normalize(*a, 'instance')
  _close(fn(x, scale, shift).numpy(), want.detach().numpy())
  for got, ref in zip(T.grads(fn, (x, scale, shift), [cot]), torch.autograd.grad(want, leaves, torch.tensor(cot))):
    _close(got, ref.numpy())


def test_truth_resample_matrix_is_the_oracles_resample():
  from oracle import ddsp_oracle as O
  rng = np.random.default_rng(13)
  x = rng.standard_normal((2, 9, 3))
  for n, method, add_endpoint in ((36, 'linear', True), (5, 'linear', True), (36, 'cubic', False), (36, 'window', True)):
    _close(T.resample(x, n, method, add_endpoint).numpy(), O.resample(x, n, method=method, add_endpoint=add_endpoint, dtype=np.float64))
  assert T.expand_z(torch.zeros(2, 4), 1).shape == (2, 1, 4) and T.expand_z(torch.zeros(2, 1, 4), 6).shape == (2, 6, 4)


def test_one_pass_variance_fails_the_4x_rule_at_a_large_mean_and_two_passes_do_not():
  """The case (2, 40, 8, instance) with x = 100 + N(0, 1) of tests/test_gpu_encoder.py: in fp32, E[x^2] - mean^2 is wrong in
  the variance's third digit (x^2 ~ 1e4 carries 1e-3 of rounding, the variance is ~1), the truth's own fp32 mode is not."""
  rng = np.random.default_rng(14)
  x = (100.0 + rng.standard_normal((2, 40, 1, 8))).astype(np.float32)
  truth = T.normalize_op(x, 'instance').numpy()
  fp32 = T.normalize_op(x, 'instance', dtype=torch.float32).numpy().astype(np.float64)
  x32 = torch.as_tensor(x)
  mean = x32.mean(dim=(1, 2), keepdim=True)
  var = (x32 * x32).mean(dim=(1, 2), keepdim=True) - mean * mean
  one_pass = ((x32 - mean) / torch.sqrt(var + 1e-5)).numpy().astype(np.float64)
  scale = np.abs(truth).max()
  ref_err, one_pass_err = np.abs(fp32 - truth).max() / scale, np.abs(one_pass - truth).max() / scale
  bound = max(4.0 * ref_err, 8 * 2.0 ** -24)
  assert ref_err <= bound < one_pass_err, (ref_err, one_pass_err)
  assert one_pass_err > 10 * bound


# ---- the Python layer without a GPU --------------------------------------------------------------------------------------
class _AudioEncoder(encoders.ZEncoder):
  def compute_z(self, audio):
    return audio


def test_z_encoder_keys():
  enc = _AudioEncoder()
  assert enc.input_keys == ['audio', 'f0_scaled'] and enc.output_keys == ['z']
  assert encoders.MfccTimeDistributedRnnEncoder().input_keys == ['audio', 'f0_scaled']
  assert encoders.MfccEncoder().input_keys == ['audio', 'f0_scaled']
  assert encoders.AggregateFeaturesEncoder().input_keys == ['f0_scaled', 'ld_scaled', 'f0_scaled']
  assert encoders.OneHotEncoder().input_keys == ['instrument', 'f0_scaled'] and encoders.OneHotEncoder(one_hot_key='id').input_keys[0] == 'id'
  with pytest.raises(NotImplementedError):
    encoders.ZEncoder(input_keys=['audio']).compute_z()
  z = torch.zeros(2, 4)
  assert enc.expand_z(z, 1).shape == (2, 1, 4)           # a time axis is added; one step needs no resampling


def test_error_texts():
  for bad in (64, 0, 249, '250'):
    with pytest.raises(ValueError, match='`z_time_steps` currently limited to 63,125,250,500 and 1000'):
      encoders.MfccTimeDistributedRnnEncoder(z_time_steps=bad)
  with pytest.raises(ValueError, match='lstm.*not built'):
    encoders.MfccTimeDistributedRnnEncoder(rnn_type='lstm')
  x = torch.zeros(2, 3, 1, 48)
  with pytest.raises(KeyError, match='batch'):
    nn.normalize_op(x, 'batch')
  with pytest.raises(ValueError, match="norm_type='group' takes channels in multiples of 32, got 48"):
    nn.normalize_op(x, 'group')
  assert nn.normalize_op(x, None) is x
  assert not hasattr(encoders, 'MfccRnnEncoder')
  enc = encoders.MfccEncoder()
  assert isinstance(enc.norm_out, nn.Normalize) and not hasattr(enc, 'nom_out') and 'nom_out' in encoders.MfccEncoder.__doc__


def test_specs_of_the_five_z_time_steps():
  specs = {63: (2048, 0.5), 125: (1024, 0.5), 250: (1024, 0.75), 500: (512, 0.75), 1000: (256, 0.75)}
  for steps, (fft_size, overlap) in specs.items():
    enc = encoders.MfccTimeDistributedRnnEncoder(z_time_steps=steps)
    assert (enc.fft_size, enc.overlap) == (fft_size, overlap)
    assert isinstance(enc.z_norm, nn.Normalize) and enc.z_norm.norm_type == 'instance'
    assert isinstance(enc.rnn, nn.Rnn) and isinstance(enc.dense_out, nn.Dense) and enc.dense_out.units == 32


def test_frame_counts_of_the_five_specs_on_16000_samples():
  """One second of audio through each spec's MFCCs (the kernels through the SIMT emulation, on host memory)."""
  from tests.hip_emu import emu_simt
  if not os.path.exists(emu_simt.CLANG):
    pytest.skip('the SIMT emulation builds with the ROCm clang++, which this machine does not have')
  audio = (0.1 * np.random.default_rng(15).standard_normal((1, 16000))).astype(np.float32)
  with emu_simt.emulated():
    frames = [encoders.MfccTimeDistributedRnnEncoder(z_time_steps=steps).compute_mfccs(audio).shape for steps in (63, 125, 250, 500, 1000)]
  assert frames == [(1, n, 30) for n in (16, 32, 63, 125, 250)]


def test_layers_construct_without_a_gpu_and_fail_loudly_when_called():
  layer = nn.Normalize('group')
  assert not layer.built and nn.get_embedding(8, 2).input_dim == 8
  assert isinstance(nn.ConditionalNorm().conditional_scale_and_shift, nn.ConditionalScaleAndShift)
  if not torch.cuda.is_available():
    with pytest.raises(_lib.DdspLibraryError):
      layer(torch.zeros(2, 3, 64))
    with pytest.raises(_lib.DdspLibraryError):
      nn.normalize_op(torch.zeros(2, 3, 1, 4))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
  build_mod.build()
  return _lib.load()


def test_every_norm_signature_is_declared_and_exported(lib):
  header = open(os.path.join(ROOT, 'ddsp_amd', 'csrc', 'norm_abi.h')).read()
  header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
  declared = set(re.findall(r'\b(ddsp_[a-z0-9_]+)\s*\(', header))
  assert declared and declared == set(_lib.NORM_SIGNATURES), declared ^ set(_lib.NORM_SIGNATURES)
  assert not set(_lib.NORM_SIGNATURES) & set(_lib.SIGNATURES) and not set(_lib.NORM_SIGNATURES) & set(_lib.DECODER_SIGNATURES)
  public = open(os.path.join(ROOT, 'include', 'ddsp_amd.h')).read()
  for name in declared:
    assert hasattr(lib, name) and name not in public, name
    fn = _lib.norm_entry(lib, name)                       # idempotent
    assert fn.argtypes == _lib.NORM_SIGNATURES[name][1] and _lib.norm_entry(lib, name).restype is _lib.NORM_SIGNATURES[name][0]
  assert 'group_norm.hip' in build_mod.SOURCES


def test_workspace_queries(lib):
  fwd, bwd = lib.ddsp_group_norm_workspace_bytes, lib.ddsp_group_norm_backward_workspace_bytes
  assert fwd(32, 250, 30, 30) == 0                                             # one block per batch row: nothing to hand over
  assert bwd(32, 250, 30, 30) == 32 * 2 * 30 * 4                                # the partial rows of dshift, dscale
  assert fwd(2, 64, 256, 1) == 0 and fwd(2, 65, 256, 1) == (2 * 2 * 2 * 256 + 2 * 2 * 1) * 4      # the split threshold: 16384 floats
  assert fwd(32, 1000, 256, 1) == (32 * 16 * 2 * 256 + 2 * 32) * 4 == bwd(32, 1000, 256, 1)
  assert fwd(32, 1000, 256, 32) == (32 * 16 * 2 * 256 + 2 * 32 * 32) * 4
  assert fwd(2, 4, 4096, 4096) == (2 * 1 * 2 * 4096 + 2 * 2 * 4096) * 4        # one chunk, but more channels than LDS holds
  assert fwd(0, 5, 4, 1) == 0 and fwd(2, 5, 4, 3) == 0 and fwd(1 << 20, 1 << 10, 2, 1) == 0


def test_null_pointers_bad_shapes_and_limits_return_codes(lib):
  p = 64                                                                       # any non-null value: nothing is launched
  fwd, bwd = lib.ddsp_group_norm_f32, lib.ddsp_group_norm_backward_f32
  assert fwd(None, None, None, p, None, None, None, 0, 1, 1, 1, 1, 1e-5, None) == -1
  assert fwd(p, p, None, p, None, None, None, 0, 1, 1, 1, 1, 1e-5, None) == -1            # scale without shift
  assert fwd(p, None, None, p, p, None, None, 0, 1, 1, 1, 1, 1e-5, None) == -1            # mean without rstd
  assert fwd(p, None, None, p, None, None, None, 0, 1, 1, 6, 4, 1e-5, None) == -2         # 4 groups do not divide 6 channels
  assert fwd(p, None, None, p, None, None, None, 0, 1, 0, 4, 1, 1e-5, None) == -2
  assert fwd(p, None, None, p, None, None, None, 0, 1, 1, 4, 0, 1e-5, None) == -2
  assert fwd(p, None, None, p, None, None, None, 0, 1, 1, 4, 1, -1.0, None) == -2
  assert fwd(p, None, None, p, None, None, None, 0, 1 << 11, 1 << 10, 1 << 10, 1, 1e-5, None) == -3    # 2^31 elements
  assert fwd(p, None, None, p, None, None, None, 0, 0, 5, 4, 1, 1e-5, None) == 0          # no rows: nothing to do
  assert fwd(p, None, None, p, None, None, None, 0, 2, 65, 256, 1, 1e-5, None) == -1      # split, no workspace
  assert fwd(p, None, None, p, None, None, p, 16, 2, 65, 256, 1, 1e-5, None) == -4
  assert bwd(p, p, p, None, None, p, None, None, None, 0, 1, 1, 1, 1, None) == -1
  assert bwd(p, p, p, p, None, p, p, p, None, 0, 1, 1, 1, 1, None) == -1                  # dscale without scale
  assert bwd(p, p, p, p, p, p, p, None, None, 0, 1, 1, 1, 1, None) == -1                  # dscale without dshift
  assert bwd(p, p, p, p, None, p, None, None, None, 0, 1, 1, 6, 4, None) == -2
  assert bwd(p, p, p, p, None, p, None, None, None, 0, 1 << 11, 1 << 10, 1 << 10, 1, None) == -3
  assert bwd(p, p, p, p, None, p, None, None, None, 0, 0, 5, 4, 1, None) == 0
  assert bwd(p, p, p, p, p, p, p, p, None, 0, 2, 5, 4, 1, None) == -1                     # partial rows need the workspace
  assert bwd(p, p, p, p, p, p, p, p, p, 16, 2, 5, 4, 1, None) == -4
  assert bwd(p, p, p, p, None, p, None, None, p, 16, 2, 65, 256, 1, None) == -4
