"""The vector quantizer of ddsp_amd.training.nn on its own: the eval call, the training call without restarts, and vq_assign and
vq_statistics alone, on the fused path (csrc/vq.hip) at batch 32 x 1000 frames x depth 64 with k = 512 and 1024 centroids and 1
and 4 heads, and with k = 1000 (not a multiple of 16: the vector-ALU kernel), and beside each the reference's chain
(ddsp/training/nn.py:1380-1448) written in torch ops - with the [n, k] distance and one-hot matrices it materialises; the thing
compared against, not product code - on the same GPU in the same session.  The chain's training call leaves the restart rule
out (nothing restarts in either); the fused layer still evaluates it.

    python tools/bench_vq.py [out.json]

Warm clocks, medians of five timed loops (host wall clock around synchronised loops); one JSON line at the end.  Beside each
shape: the bytes of the two [n, k] matrices the chain writes, and the share of indices on which the two paths agree (they may
differ where two centroids are closer than fp32 tells apart)."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import ddsp_amd as ddsp
from ddsp_amd import build
from ddsp_amd.training import nn
build.build()

BATCH, FRAMES, DEPTH = 32, 1000, 64
SHAPES = [(512, 1), (1024, 1), (512, 4), (1024, 4), (1000, 1)]
GAMMA = 0.99


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


# ---- the reference's chain in torch ops ---------------------------------------------------------------------------------------
def chain_flat(x, heads):
  flat = x.reshape(-1, x.shape[-1])
  return torch.cat(torch.split(flat, x.shape[-1] // heads, dim=1), 0)


def chain_assign(x, e, heads):
  flat = chain_flat(x, heads)
  distances = (flat ** 2).sum(1)[:, None] - 2 * torch.matmul(flat, e.T) + (e ** 2).sum(1)[None, :]      # [n, k]
  c = torch.argmin(distances, 1)
  z = torch.cat(torch.split(e[c], flat.shape[0] // heads, 0), 1).reshape(x.shape)
  z = x + (z - x)
  return z, torch.stack(torch.split(c, flat.shape[0] // heads, 0), 1).reshape(x.shape[:-1] + (heads,)), c, flat


def chain_statistics(flat, c, k):
  oh = torch.nn.functional.one_hot(c, k).to(torch.float32)                                               # [n, k]
  return oh.sum(0), torch.matmul(oh.T, flat)


def chain_centroids(counts, sums):
  return torch.where(counts[:, None] == 0, torch.zeros_like(sums), sums / counts[:, None])


def chain_call(state, x, heads, training):
  counts, sums = state
  z, c, c_flat, flat = chain_assign(x, chain_centroids(counts, sums), heads)
  if training:
    batch_counts, batch_sums = chain_statistics(flat, c_flat, counts.shape[0])
    counts.sub_((1 - GAMMA) * (counts - batch_counts))
    sums.sub_((1 - GAMMA) * (sums - batch_sums))
  return z, c


result = {'workload': 'training.nn VectorQuantization: eval call, training call without restarts, vq_assign, vq_statistics',
          'note': 'timings are [median, min, max] in microseconds per call, host wall clock around synchronised loops; '
                  'speedup = the torch chain\'s median over the fused path\'s', 'shapes': {}}
torch.manual_seed(0)
dev = ddsp.core._device()
x = torch.randn(BATCH, FRAMES, DEPTH, device=dev)
for k, heads in SHAPES:
  dims, n = DEPTH // heads, BATCH * FRAMES * heads
  counts = 1.0 + 5.0 * torch.rand(k, device=dev)
  sums = torch.randn(k, dims, device=dev) * counts[:, None]
  layer = nn.VectorQuantization(k, gamma=GAMMA, restart_threshold=-1.0, num_heads=heads)
  layer.build(DEPTH)
  state = (counts.clone(), sums.clone())
  layer.counts.copy_(counts); layer.sums.copy_(sums)
  e = layer.centroids()
  row = {'batch': BATCH, 'frames': FRAMES, 'depth': DEPTH, 'k': k, 'heads': heads, 'vectors': n,
         'path': 'matrix cores' if k % 16 == 0 else 'vector ALU', 'chain_nk_matrix_bytes_each': n * k * 4}
  with torch.no_grad():
    z, c = nn.vq_assign(x, e, heads)
    z_chain, c_chain, c_flat, flat = chain_assign(x, e, heads)
    row['indices_agree_share'] = float((c == c_chain).to(torch.float32).mean())
    ours, theirs = nn.vq_statistics(x, c_chain, k, heads), chain_statistics(flat, c_flat, k)
    row['counts_equal'] = bool(torch.equal(ours[0], theirs[0]))
    row['sums_max_abs_difference'] = float((ours[1] - theirs[1]).abs().max())
    del z, z_chain, ours, theirs
    measurements = {
        'assign': (lambda: nn.vq_assign(x, e, heads), lambda: chain_assign(x, e, heads)),
        'statistics': (lambda: nn.vq_statistics(x, c, k, heads), lambda: chain_statistics(flat, c_flat, k)),
        'eval_call': (lambda: layer(x), lambda: chain_call(state, x, heads, False)),
        'training_call': (lambda: layer(x, training=True), lambda: chain_call(state, x, heads, True)),
    }
    for what, (fused, chain) in measurements.items():
      row['us_%s_fused' % what] = timed(fused, 20)
      row['us_%s_torch_chain' % what] = timed(chain, 5)
      row['%s_speedup' % what] = row['us_%s_torch_chain' % what][0] / row['us_%s_fused' % what][0]
      torch.cuda.empty_cache()
  result['shapes']['%dx%dx%d_k%d_heads%d' % (BATCH, FRAMES, DEPTH, k, heads)] = row

if len(sys.argv) > 1:
  with open(sys.argv[1], 'w') as fh:
    fh.write(json.dumps(result, indent=1) + '\n')
print(json.dumps(result))
