"""Generate tests/golden/wasserstein_*.npz by running the REFERENCE'S OWN losses.py (wasserstein_distance and
WassersteinConsistencyLoss, ddsp/losses.py:584-686) on the numpy TensorFlow stand-in of tf_numpy_shim.py.

    python tests/golden/make_golden_wasserstein.py        (needs the reference checkout; DDSP_REFERENCE_ROOT)

The stand-in is set up by make_golden_consistency.py (imported, not run); the ops this function calls and the stand-in lacks -
argsort, sort, searchsorted and gather with batch_dims - are supplied here at run time, in fp32, with TensorFlow's stable
orders.  Every fixture is checked against the fp64 truth of tests/wasserstein_truth.py before it is written, at the bound
make_golden_consistency.py refuses at."""
import numpy as np

import make_golden_consistency as base            # installs the stand-in and imports the reference's core / losses
import wasserstein_truth as W  # noqa: E402

v2, losses, F32 = base.v2, base.losses, np.float32


def _f32(x):
  """Floating-point values are fp32, as every tensor of the reference is (the stand-in's hz_to_midi hands back a wider type)."""
  x = np.asarray(x)
  return x.astype(F32) if x.dtype.kind == 'f' else x


def _gather(params, indices, axis=-1, batch_dims=0):
  params, indices = _f32(params), np.asarray(indices)
  assert axis == -1 and batch_dims == params.ndim - 1 == indices.ndim - 1
  return np.take_along_axis(params, indices, axis=-1).view(base._TENSOR)


def _searchsorted(sorted_sequence, values, side='left'):
  seq, values = _f32(sorted_sequence), _f32(values)
  out = np.empty(values.shape, np.int32)
  for idx in np.ndindex(*seq.shape[:-1]):
    out[idx] = np.searchsorted(seq[idx], values[idx], side=side)
  return out.view(base._TENSOR)


base._supply(v2, 'argsort', lambda x, axis=-1: np.argsort(_f32(x), axis=axis, kind='stable').astype(np.int32).view(base._TENSOR))
base._supply(v2, 'sort', lambda x, axis=-1: base._t(np.sort(np.asarray(x, F32), axis=axis, kind='stable')))
base._supply(v2, 'searchsorted', _searchsorted)
base._supply(v2, 'gather', _gather)


def _pairs(seed, zeros=False):
  rng, amps_a, freqs_a = base.sinusoids(seed, k=8, zeros=zeros)
  amps_b, freqs_b = W.make_sinusoids(rng, 2, 12, 6, zeros=zeros)
  return rng, amps_a, freqs_a, amps_b, freqs_b


def distance_case(name, seed, p, weights=True):
  rng, wu, u, wv, v = _pairs(seed)
  u, v = np.log(u).astype(F32), np.log(v).astype(F32)           # any values do: the function is not about Hz
  wu, wv = (wu, wv) if weights else (None, None)
  ref = np.asarray(losses.wasserstein_distance(u, v, wu, wv, p=p), np.float64)
  base._held(name, 'distance', ref, W.wasserstein_distance(u, v, wu, wv, p=p))
  arrays = dict(u_values=u, v_values=v, p=np.float64(p), distance=base.a(ref))
  if weights:
    arrays.update(u_weights=wu, v_weights=wv)
  base.save(name, **arrays)


def class_case(name, seed, zeros=False, **kw):
  rng, amps_a, freqs_a, amps_b, freqs_b = _pairs(seed, zeros=zeros)
  if zeros:
    freqs_a[rng.uniform(size=freqs_a.shape) < 0.2] = 0.0
    freqs_b[rng.uniform(size=freqs_b.shape) < 0.2] = 0.0
    assert (freqs_a == 0.0).any() and (amps_a == 0.0).any() and (freqs_b == 0.0).any()
  ref = losses.WassersteinConsistencyLoss(**kw)(amps_a, freqs_a, amps_b, freqs_b)
  truth = W.wasserstein_loss(amps_a, freqs_a, amps_b, freqs_b, **kw)
  if kw.get('midi', True):
    base._held(name, 'loss', ref, truth)
  else:
    assert ref == 0.0 and truth == 0.0
  base.save(name, amps_a=amps_a, freqs_a=freqs_a, amps_b=amps_b, freqs_b=freqs_b, loss=base.a(ref),
            **{k: np.float64(v) for k, v in kw.items()})


if __name__ == '__main__':
  distance_case('wasserstein_distance_p1', 11, 1.0)
  distance_case('wasserstein_distance_p2', 12, 2.0)
  distance_case('wasserstein_distance_no_weights', 13, 1.0, weights=False)
  class_case('wasserstein_class_default', 14)
  class_case('wasserstein_class_midi_false', 15, midi=False)
  class_case('wasserstein_class_zero_freqs', 16, zeros=True)
