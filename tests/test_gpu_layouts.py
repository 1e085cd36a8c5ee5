"""Every entry point on offset, strided and non-fp32 tensors.

THE ONE PROPERTY: a call on tensors of any layout or dtype returns the bits of the same call on freshly allocated contiguous
fp32 copies of the same values - outputs and every gradient.  No tolerance: the reference is the library itself on the layout
the rest of the suite holds to the fp64 truths.  Gradients are compared by logical index (torch.equal on the tensors, not on
storage), and each has the shape and the dtype of its leaf (a float64 leaf gets the fp32 gradient cast).  One exception, the
README's own: the SpectralLoss gradient without deterministic=True is overlap-added with fp32 atomics, so those rows
(Row.atomic_grad) hold their VALUE to bits and their gradient to the suite's bound for the atomics' order, 1e-5 of its largest
element; the deterministic rows hold the same gradient to bits.

tests/layout_table.py is the table of entries (name, call, argument builders) and says why the shapes are what they are;
tests/test_layouts_emulated.py runs this module through the SIMT emulation on the CPU; tests/test_layouts_table.py holds the
table to ddsp_amd._lib.SIGNATURES.

Per entry every variant is put on each tensor argument alone and then on all of them at once:
  offset1 / offset2 / offset3   a contiguous view that starts 1, 2, 3 floats past a 16-byte boundary (2: 8-byte aligned, the other
                                side of the `& 7` conditions of csrc/)
  transposed                    the last two axes swapped in memory (where both are longer than 1)
  stepped                       buf[..., ::2] of a buffer twice as wide
  expanded                      stride 0 along the axis the entry broadcasts
  cpu, numpy                    a host tensor, a numpy array
  float64, float16, bfloat16    compared with the call on x.to(float32); the output is fp32
  float64_leaf                  a requires_grad leaf of dtype float64
and per differentiable entry the gradient seeds: the stride-0 seed of out.sum().backward() against backward(ones_like(out)),
a seed at offset 1, a transposed one, a float64 one.

Then the rows-alone property on VIEWS (x[r:r + 1] of a batch whose rows are an odd number of floats long is a pointer off every
16-byte boundary) and the raw C call of ddsp_add_f32's contract."""
import zlib

import numpy as np
import pytest
import torch

import layout_table as L

pytestmark = pytest.mark.gpu
DEV = 'cuda'

LAYOUTS = ('offset1', 'offset2', 'offset3', 'transposed', 'stepped', 'expanded', 'cpu', 'numpy')
DTYPES = ('float64', 'float16', 'bfloat16', 'float64_leaf')
VARIANTS = LAYOUTS + DTYPES
SEEDS = ('sum', 'offset1', 'transposed', 'float64')
_KEEPS_VALUES = ('offset1', 'offset2', 'offset3', 'transposed', 'stepped', 'cpu', 'numpy', 'float64', 'float64_leaf')


# ---- the helpers ---------------------------------------------------------------------------------------------------------
def offset_view(x, k):
  """A contiguous view holding x that starts k floats past a 16-byte boundary."""
  assert x.dtype == torch.float32 and k in (1, 2, 3)
  buf = torch.empty(x.numel() + 8, dtype=x.dtype, device=x.device)
  base = (-(buf.data_ptr() // 4)) % 4                              # floats up to the next 16-byte boundary
  view = buf[base + k: base + k + x.numel()].view(x.shape)
  view.copy_(x)
  assert view.is_contiguous() and view.data_ptr() % 16 == 4 * k
  return view


def transposed_storage(x):
  """The same logical values, the last two axes swapped in memory."""
  assert x.dim() >= 2 and x.shape[-1] > 1 and x.shape[-2] > 1
  view = x.transpose(-1, -2).contiguous().transpose(-1, -2)
  assert not view.is_contiguous() and view.shape == x.shape
  return view


def stepped(x):
  """buf[..., ::2] of a buffer twice as wide (a 0-dim tensor: one element of a vector of two)."""
  if x.dim() == 0:
    buf = torch.zeros(2, dtype=x.dtype, device=x.device)
    buf[1] = x
    return buf[1]
  buf = torch.zeros(tuple(x.shape[:-1]) + (2 * x.shape[-1],), dtype=x.dtype, device=x.device)
  view = buf[..., ::2]
  view.copy_(x)
  assert view.shape == x.shape and (x.shape[-1] == 1 or not view.is_contiguous())
  return view


def expanded(x, axis):
  """Row 0 along `axis`, held with stride 0 there."""
  view = x.narrow(axis, 0, 1).clone().expand(x.shape)
  assert view.stride(axis) == 0 or x.shape[axis] == 1
  return view


def _can_transpose(shape):
  return len(shape) >= 2 and shape[-1] > 1 and shape[-2] > 1


def _applies(variant, arg, row):
  if variant == 'transposed':
    return _can_transpose(arg.shape)
  if variant == 'expanded':
    return arg.expand is not None and arg.shape[arg.expand] > 1
  if variant == 'numpy':
    return row.numpy
  if variant == 'float64_leaf':
    return arg.grad
  return True


def _vary(x, variant, arg):
  """x: contiguous fp32 on DEV."""
  if variant.startswith('offset'):
    return offset_view(x, int(variant[-1]))
  if variant == 'transposed':
    return transposed_storage(x)
  if variant == 'stepped':
    return stepped(x)
  if variant == 'expanded':
    return expanded(x, arg.expand)
  if variant == 'cpu':
    return x.cpu()
  if variant == 'numpy':
    return x.cpu().numpy()
  if variant in ('float64', 'float64_leaf'):
    return x.double()
  return x.to(getattr(torch, variant))


# ---- running a row -------------------------------------------------------------------------------------------------------
def _base_values(row):
  rng = np.random.default_rng(zlib.crc32(row.name.encode()))
  return [torch.as_tensor(arg.values(rng), device=DEV) for arg in row.args]


def _outputs(result):
  if isinstance(result, dict):
    result = [result[key] for key in sorted(result)]
  if isinstance(result, torch.Tensor):
    result = [result]
  return [t for t in result if isinstance(t, torch.Tensor)]


def _cotangents(row, outs):
  rng = np.random.default_rng(zlib.crc32(row.name.encode()) ^ 0x5eed)
  return [torch.as_tensor(rng.standard_normal(tuple(o.shape)).astype(np.float32), device=DEV) for o in outs]


def _run(ddsp, row, tensors, leaves, seed=None):
  """The call on `tensors`; gradients for the indices in `leaves` (those tensors are made leaves).  seed(g, out) re-lays a
  cotangent.  -> (outputs, {index: gradient})."""
  args = list(tensors)
  for i in leaves:
    args[i] = args[i].detach().requires_grad_(True)
  outs = _outputs(row.call(ddsp, *args))
  grads = {}
  if leaves:
    gs = _cotangents(row, outs)
    pairs = [(o, g if seed is None else seed(g)) for o, g in zip(outs, gs) if o.requires_grad]
    assert pairs, row.name + ': no output carries a gradient'
    got = torch.autograd.grad([o for o, _ in pairs], [args[i] for i in leaves], [g for _, g in pairs], allow_unused=True)
    grads = dict(zip(leaves, got))
  return [o.detach() for o in outs], grads, args


_reference_cache = {}


def _fresh(values):
  """Freshly allocated contiguous fp32 copies of the same values on DEV."""
  out = []
  for v in values:
    t = torch.as_tensor(v).detach().to(DEV).to(torch.float32)
    out.append(t.contiguous().clone())
  return out


def _reference(ddsp, row, values=None):
  """Outputs and gradients of the row on fresh contiguous fp32 tensors: of its own values (computed once, shared), or of
  `values`."""
  leaves = [i for i, a in enumerate(row.args) if a.grad]
  if values is None:
    key = (row.name, DEV)
    if key not in _reference_cache:
      outs, grads, _ = _run(ddsp, row, _base_values(row), leaves)
      _reference_cache[key] = (outs, grads)
    return _reference_cache[key]
  outs, grads, _ = _run(ddsp, row, _fresh(values), leaves)
  return outs, grads


def _same_bits(case, got, want):
  assert got.dtype == want.dtype and got.shape == want.shape, (case, got.dtype, want.dtype, got.shape, want.shape)
  same = torch.equal(got, want) or bool(((got == want) | (torch.isnan(got) & torch.isnan(want))).all())
  if not same:
    diff = (got.double() - want.double()).abs()
    raise AssertionError('%s: %d of %d elements differ, by up to %g' % (case, int((got != want).sum()), got.numel(), float(diff.max())))


ATOMICS_ORDER = 1e-5     # of the largest gradient: the suite's bound for "same kernel, atomics order only" (tests/test_gpu_parity.py)


def _same_gradient(row, case, got, want):
  """Bits - except where the row's gradient is overlap-added with fp32 atomics (Row.atomic_grad: the README's exception)."""
  if not row.atomic_grad:
    return _same_bits(case, got, want)
  assert got.dtype == want.dtype and got.shape == want.shape, (case, got.dtype, want.dtype, got.shape, want.shape)
  err, scale = float((got.double() - want.double()).abs().max()), float(want.double().abs().max())
  print(case, dict(err=err, bound=ATOMICS_ORDER * scale))
  assert err <= ATOMICS_ORDER * scale, (case, err, ATOMICS_ORDER * scale)


def _check_case(ddsp, row, variant, which):
  """The variant on the arguments `which`; everything else plain.  Outputs and every gradient against the reference."""
  base = _base_values(row)
  tensors = [(_vary(x, variant, row.args[i]) if i in which else x) for i, x in enumerate(base)]
  as_numpy = [isinstance(t, np.ndarray) for t in tensors]
  keeps = variant in _KEEPS_VALUES
  ref_outs, ref_grads = _reference(ddsp, row, None if keeps else tensors)
  # a dtype variant is a value passing through (an activation); the layout variants and float64_leaf are leaves themselves
  no_leaf = ('float64', 'float16', 'bfloat16')
  leaves = [i for i, a in enumerate(row.args) if a.grad and not as_numpy[i] and not (i in which and variant in no_leaf)]
  outs, grads, args = _run(ddsp, row, tensors, leaves)
  case = '%s[%s on %s]' % (row.name, variant, ','.join(row.args[i].name for i in which))
  assert len(outs) == len(ref_outs), case
  for n, (o, r) in enumerate(zip(outs, ref_outs)):
    _same_bits('%s output %d' % (case, n), o, r)
  for i in leaves:
    g, r = grads[i], ref_grads[i]
    name = '%s gradient of %s' % (case, row.args[i].name)
    assert (g is None) == (r is None), name
    if g is None:
      continue
    leaf = args[i]
    assert g.shape == leaf.shape and g.dtype == leaf.dtype and g.device == leaf.device, (name, g.shape, g.dtype, g.device)
    _same_gradient(row, name, g.to(DEV), r.to(leaf.dtype))


def _variant_cases():
  cases = []
  for row in L.ROWS:
    for variant in VARIANTS:
      if any(_applies(variant, a, row) for a in row.args):
        cases.append(pytest.param(row.name, variant, id='%s-%s' % (row.name, variant)))
  return cases


@pytest.mark.parametrize('name, variant', _variant_cases())
def test_layout_gives_the_bits_of_fresh_contiguous_fp32(ddsp, name, variant):
  row = L.BY_NAME[name]
  on = [i for i, a in enumerate(row.args) if _applies(variant, a, row)]
  for i in on:                                                   # each argument alone
    _check_case(ddsp, row, variant, [i])
  if len(on) > 1:                                                # all at once
    _check_case(ddsp, row, variant, on)


# ---- gradient seeds ------------------------------------------------------------------------------------------------------
def _seed_cases():
  return [pytest.param(row.name, seed, id='%s-%s' % (row.name, seed)) for row in L.ROWS if row.differentiable
          for seed in SEEDS if not (seed == 'transposed' and row.scalar)]


@pytest.mark.parametrize('name, seed', _seed_cases())
def test_gradient_seed_layout_gives_the_same_gradients(ddsp, name, seed):
  row = L.BY_NAME[name]
  leaves = [i for i, a in enumerate(row.args) if a.grad]
  if seed == 'sum':
    # what out.sum().backward() hands to backward(): a 0-dim one expanded to the output's shape, every stride 0
    args = [x.requires_grad_(i in leaves) for i, x in enumerate(_base_values(row))]
    outs = [o for o in _outputs(row.call(ddsp, *args)) if o.requires_grad]
    sum(o.sum() for o in outs).backward()
    again = [x.requires_grad_(i in leaves) for i, x in enumerate(_base_values(row))]
    outs = [o for o in _outputs(row.call(ddsp, *again)) if o.requires_grad]
    want = torch.autograd.grad(outs, [again[i] for i in leaves], [torch.ones_like(o) for o in outs], allow_unused=True)
    for i, r in zip(leaves, want):
      assert (args[i].grad is None) == (r is None)
      if r is not None:
        _same_gradient(row, '%s[sum seed] gradient of %s' % (name, row.args[i].name), args[i].grad, r)
    return
  _, ref_grads = _reference(ddsp, row)
  used = []

  def lay(g):
    if seed == 'offset1':
      used.append(g)
      return offset_view(g, 1)
    if seed == 'float64':
      used.append(g)
      return g.double()
    if _can_transpose(g.shape):
      used.append(g)
      return transposed_storage(g)
    return g
  _, grads, _ = _run(ddsp, row, _base_values(row), leaves, seed=lay)
  assert used, name + ': no output took the seed layout'
  for i in leaves:
    g, r = grads[i], ref_grads[i]
    assert (g is None) == (r is None)
    if g is not None:
      _same_gradient(row, '%s[%s seed] gradient of %s' % (name, seed, row.args[i].name), g, r)


# ---- rows alone, as views ------------------------------------------------------------------------------------------------
N_ODD = 2543          # rows an odd number of floats long: x[1:2] starts off every 8- and 16-byte boundary


def _rows_equal_alone(ddsp, fn, tensors, leaves, batch_axis_free=()):
  """fn(*tensors) -> [B, ...]; row r of the batch result == the call on the VIEWS x[r:r + 1] (arguments in `batch_axis_free` are
  shared by the rows), outputs and gradients."""
  def run(args, g):
    args = [a.detach().requires_grad_(i in leaves) for i, a in enumerate(args)]
    out = fn(*args)
    grads = torch.autograd.grad(out, [args[i] for i in leaves], g) if leaves else ()
    return out.detach(), grads
  b = tensors[0].shape[0]
  first = fn(*tensors)
  g = torch.as_tensor(np.random.default_rng(7).standard_normal(tuple(first.shape)).astype(np.float32), device=DEV)
  out, grads = run(tensors, g)
  for r in range(b):
    views = [t if i in batch_axis_free else t[r:r + 1] for i, t in enumerate(tensors)]
    for v in views:
      assert v.is_contiguous()
    alone, grads_alone = run(views, g[r:r + 1])
    _same_bits('row %d alone: output' % r, alone, out[r:r + 1])
    for i, ga, gb in zip(leaves, grads_alone, grads):
      if i not in batch_axis_free:
        _same_bits('row %d alone: gradient %d' % (r, i), ga, gb[r:r + 1])


def _rng_tensor(seed, *shape, scale=1.0, lo=None, hi=None):
  rng = np.random.default_rng(seed)
  values = rng.uniform(lo, hi, shape) if lo is not None else scale * rng.standard_normal(shape)
  return torch.as_tensor(values.astype(np.float32), device=DEV)


@pytest.mark.parametrize('bands, frames', [(65, 40), (65, 11), (64, 11)])
def test_filtered_noise_rows_alone_on_views_of_supplied_noise(ddsp, bands, frames):
  """README: "a row alone, a sub-batch and the full batch give the same bits".  noise[r:r + 1] of a batch with N % 4 != 0 is off
  the 16-byte boundary by which ddsp_filtered_noise_f32 picks its kernel."""
  # 40 frames of 64 samples (the last ragged): the canonical filter's own kernels; 11 frames of 232: the general ones
  mags = _rng_tensor(1, 3, frames, bands)
  noise = _rng_tensor(2, 3, N_ODD, lo=-1.0, hi=1.0)
  assert noise[1:2].data_ptr() % 16 != 0

  def fn(m, z):
    return ddsp.synths.FilteredNoise(n_samples=N_ODD, window_size=0)(m, noise=z)
  _rows_equal_alone(ddsp, fn, [mags, noise], leaves=[0])


def test_harmonic_rows_alone_on_views_with_an_odd_row_length(ddsp):
  frames, k = 7, 9                 # F K = 63 floats per row of the distribution, F = 7 per row of amplitudes and f0
  n = frames * 64
  tensors = [_rng_tensor(3, 3, frames, 1), _rng_tensor(4, 3, frames, k), _rng_tensor(5, 3, frames, 1, lo=180.0, hi=260.0)]
  assert tensors[1][1:2].data_ptr() % 16 != 0
  _rows_equal_alone(ddsp, lambda a, h, f: ddsp.synths.Harmonic(n_samples=n)(a, h, f), tensors, leaves=[0, 1, 2])


def test_reverb_rows_alone_on_views_with_an_odd_row_length(ddsp):
  """An impulse response per row.  (With one for the batch, two rows share a transform and a row alone is no pair: the exception
  the README names.)"""
  audio, ir = _rng_tensor(6, 3, N_ODD, scale=0.3), _rng_tensor(7, 3, 255, scale=0.05)
  _rows_equal_alone(ddsp, lambda a, i: ddsp.effects.Reverb(reverb_length=255)(a, i), [audio, ir], leaves=[0, 1])


@pytest.mark.parametrize('deterministic', [False, True])
def test_spectral_loss_rows_alone_on_views_with_an_odd_row_length(ddsp, deterministic):
  """The loss is a mean over the batch, so a row alone is compared as a batch of one taken as a VIEW with the same row as a fresh
  copy: value and gradient."""
  target, audio = _rng_tensor(8, 3, N_ODD, scale=0.3), _rng_tensor(9, 3, N_ODD, scale=0.3)
  loss = ddsp.losses.SpectralLoss(fft_sizes=(128, 64), logmag_weight=1.0, deterministic=deterministic)
  for r in range(3):
    view = audio[r:r + 1].requires_grad_(True)
    copy = audio[r:r + 1].clone().requires_grad_(True)
    assert r != 1 or view.data_ptr() % 8 != 0
    value_view, value_copy = loss(target[r:r + 1], view), loss(target[r:r + 1].clone(), copy)
    _same_bits('SpectralLoss row %d value' % r, value_view.detach(), value_copy.detach())
    if deterministic:               # (the atomics of the default gradient promise no bits)
      g_view, = torch.autograd.grad(value_view, view)
      g_copy, = torch.autograd.grad(value_copy, copy)
      _same_bits('SpectralLoss row %d gradient' % r, g_view, g_copy)


# ---- Add -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 2, 3])
def test_add_on_offset_views_is_the_sum(ddsp, k):
  """a + b bit-exactly (one rounding per element, as torch's own), forward and through the autograd node, from views at every
  offset and from the output of an earlier Add."""
  a, b = _rng_tensor(10, 2, 509), _rng_tensor(11, 2, 509)
  add = ddsp.processors.Add()
  want = a + b
  for va, vb in ((offset_view(a, k), b), (a, offset_view(b, k)), (offset_view(a, k), offset_view(b, 4 - k))):
    _same_bits('Add forward', add(va, vb), want)
    _same_bits('Add of an Add', add(add(va, vb)[1:2], vb[1:2]), want[1:2] + b[1:2])
    la, lb = va.detach().requires_grad_(True), vb.detach().requires_grad_(True)
    out = add(la, lb)
    _same_bits('Add recorded', out.detach(), want)
    g = offset_view(_rng_tensor(12, 2, 509), k)
    ga, gb = torch.autograd.grad(out, [la, lb], g)
    _same_bits('Add gradient a', ga, g)
    _same_bits('Add gradient b', gb, g)


@pytest.fixture(scope='module')
def ddsp():
  import ddsp_amd
  import ddsp_amd.training.nn  # noqa: F401
  return ddsp_amd
