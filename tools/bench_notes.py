"""The note pooling of ddsp_amd.training.nn on its own: get_note_mask, pool_over_notes forward, and forward + backward, on the
fused path (csrc/notes.hip) at batch 32 x 1000 steps x 100 regions x 128 dims (what gin/models/midiae/z_midiae.gin ships) and
at 16 dims, and beside each the reference's chain (ddsp/training/nn.py:375-547) written in torch ops - with the
[batch, time, notes, dims] tensors it materialises; the thing compared against, not product code - on the same GPU in the
same session.  If the chain runs out of memory its batch is halved until it fits, and the batch it ran at is recorded.

    python tools/bench_notes.py [out.json]

Warm clocks, medians of five timed loops (host wall clock around synchronised loops); one JSON line at the end.  Beside
each measurement: the HBM floor, the time x, the mask and the outputs (and, backward, the cotangents and the gradient) take
at 8 TB/s."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import ddsp_amd as ddsp
from ddsp_amd import build
from ddsp_amd.training import nn
build.build()

BATCH, STEPS, REGIONS = 32, 1000, 100
HBM_BYTES_PER_US = 8e6


def timed(fn, steps, repeats=5):
  for _ in range(2): fn()
  t_settle = time.perf_counter()
  while time.perf_counter() - t_settle < 0.05:    # the GPU needs ~20 ms of load to reach its sustained clock
    fn()
    torch.cuda.synchronize()
  out = []
  for _ in range(repeats):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(steps): fn()
    torch.cuda.synchronize()
    out.append((time.perf_counter() - t0) / steps)
  return [statistics.median(out) * 1e6, min(out) * 1e6, max(out) * 1e6]


def pitches(seed, mean_length=12):
  """Integer pitches in segments of 1 .. 2 mean_length - 1 steps, three in ten silent."""
  rng = np.random.default_rng(seed)
  q = np.zeros((BATCH, STEPS), np.float32)
  for b in range(BATCH):
    t = 0
    while t < STEPS:
      n = min(int(rng.integers(1, 2 * mean_length)), STEPS - t)
      q[b, t:t + n] = 0.0 if rng.uniform() < 0.3 else float(rng.integers(30, 91))
      t += n
  return ddsp.core.tf_float32(q)


# ---- the reference's chain in torch ops ---------------------------------------------------------------------------------------
def safe_divide(num, den, eps=1e-7):
  return num / torch.where(den == 0.0, torch.full_like(den, eps), den)


def chain_moments(x, mask):
  mask_d = mask[..., None]
  lengths = mask_d.sum(1)
  x_masked = x[:, :, None, :] * mask_d                                 # [b, t, n, d]
  mean = safe_divide(x_masked.sum(1), lengths)
  numerator = (x[:, :, None, :] - mean[:, None]) * mask_d              # [b, t, n, d]
  numerator = (numerator ** 2.0).sum(1)
  var = safe_divide(numerator, lengths)
  positive = var > 0.0                                                 # the sqrt with zero gradient at 0, as the fused path's contract
  return mean, torch.where(positive, torch.sqrt(torch.where(positive, var, torch.ones_like(var))), torch.zeros_like(var))


def chain_mask(q, max_regions=REGIONS):
  edges = (torch.abs(q[:, 1:] - q[:, :-1]) > 0)[:, :-1]
  edges = torch.nn.functional.pad(edges, (1, 0), value=True)
  edges = torch.nn.functional.pad(edges, (0, 1), value=False)
  idx = torch.cumsum(edges.to(torch.int32), dim=1) - 1
  mask = (idx[..., None] == torch.arange(max_regions, device=q.device)[None, None, :]).to(torch.float32)
  note_pitches = chain_moments(q[:, :, None], mask)[0][:, :, 0]
  return mask * (note_pitches > 0.0).to(torch.float32)[:, None, :]


def chain_pool(x, mask):
  mean, std = chain_moments(x, mask)
  return (mean[:, None] * mask[..., None]).sum(2), (std[:, None] * mask[..., None]).sum(2)   # [b, t, n, d] twice


def largest_batch_that_fits(fn, batch):
  while batch >= 1:
    try:
      fn(batch)
      torch.cuda.synchronize()
      return batch
    except torch.cuda.OutOfMemoryError:
      torch.cuda.empty_cache()
      batch //= 2
  raise RuntimeError('the torch chain does not fit at batch 1')


q = pitches(0)
with torch.no_grad():
  mask = nn.get_note_mask(q)
  assert torch.equal(mask, chain_mask(q))
result = {'workload': 'training.nn note pooling: get_note_mask, pool_over_notes forward, forward + backward',
          'note': 'timings are [median, min, max] in microseconds per call, host wall clock around synchronised loops; '
                  'hbm_floor_us: the bytes of x, mask, outputs (backward: + cotangents, x and mask again, the gradient) at 8 TB/s',
          'shapes': {}}
row = {'batch': BATCH, 'steps': STEPS, 'regions': REGIONS,
       'hbm_floor_us': (q.numel() + mask.numel()) * 4 / HBM_BYTES_PER_US}
with torch.no_grad():
  row['us_fused'] = timed(lambda: nn.get_note_mask(q), 50)
  row['us_torch_chain'] = timed(lambda: chain_mask(q), 5)
row['speedup'] = row['us_torch_chain'][0] / row['us_fused'][0]
result['shapes']['get_note_mask_32x1000x100'] = row

for dims in (128, 16):
  x = torch.randn(BATCH, STEPS, dims, device=q.device)
  cots = [torch.randn(BATCH, STEPS, dims, device=q.device) for _ in range(2)]
  forward_bytes = (3 * x.numel() + mask.numel()) * 4
  row = {'batch': BATCH, 'steps': STEPS, 'regions': REGIONS, 'dims': dims,
         'hbm_floor_us_forward': forward_bytes / HBM_BYTES_PER_US,
         'hbm_floor_us_forward_backward': (forward_bytes + (4 * x.numel() + mask.numel()) * 4) / HBM_BYTES_PER_US}

  def forward_backward(pool, batch):
    leaf = x[:batch].clone().requires_grad_(True)
    m, c = mask[:batch], [v[:batch] for v in cots]
    def step():
      leaf.grad = None
      torch.autograd.backward(pool(leaf, m), c)
    return step, leaf

  chain_batch = largest_batch_that_fits(lambda b: forward_backward(chain_pool, b)[0](), BATCH)
  row['torch_chain_batch'] = chain_batch
  with torch.no_grad():
    ours, theirs = nn.pool_over_notes(x[:chain_batch], mask[:chain_batch]), chain_pool(x[:chain_batch], mask[:chain_batch])
    row['max_abs_difference_forward'] = max(float((a - b).abs().max()) for a, b in zip(ours, theirs))
    del ours, theirs
  step, leaf = forward_backward(nn.pool_over_notes, chain_batch)
  step(); fused_grad = leaf.grad.clone()
  step, leaf = forward_backward(chain_pool, chain_batch)
  step(); row['max_abs_difference_gradient'] = float((fused_grad - leaf.grad).abs().max())
  del step, leaf, fused_grad
  torch.cuda.empty_cache()
  for label, pool, batch, steps in (('fused', nn.pool_over_notes, BATCH, 50), ('torch_chain', chain_pool, chain_batch, 3)):
    with torch.no_grad():
      row['us_forward_' + label] = timed(lambda: pool(x[:batch], mask[:batch]), steps)
    row['us_forward_backward_' + label] = timed(forward_backward(pool, batch)[0], steps)
    torch.cuda.empty_cache()
  scale = BATCH / chain_batch                    # the chain's time is proportional to its batch: brought to the full batch
  for what in ('forward', 'forward_backward'):
    row[what + '_speedup'] = scale * row['us_%s_torch_chain' % what][0] / row['us_%s_fused' % what][0]
  result['shapes']['pool_over_notes_32x1000x100x%d' % dims] = row

if len(sys.argv) > 1:
  with open(sys.argv[1], 'w') as fh:
    fh.write(json.dumps(result, indent=1) + '\n')
print(json.dumps(result))
