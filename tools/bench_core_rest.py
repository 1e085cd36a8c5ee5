"""core.frequencies_critical_bands and core.harmonic_distribution_to_wavetable on their own, forward and forward + backward,
on the fused kernels (csrc/critical_bands.hip, csrc/harmonic_wavetable.hip), and beside each the reference's chain
(ddsp/core.py:510-569, 1217-1235) written in torch ops - the thing compared against, not product code - on the same GPU in
the same session.  There is no earlier implementation in this library to compare with.

    python tools/bench_core_rest.py [out.json]

Critical bands at 32 x 1000 frames x 100 sinusoids with depth 1, 4 and 64; wavetables at 32 x 1000 frames, 100 harmonics ->
2048 points and 60 harmonics -> 512 points.  Warm clocks, medians of five timed loops (host wall clock around synchronised
loops); one JSON line at the end.  Beside each measurement: the HBM floor, the time the inputs and outputs (backward: the
input again, the cotangents and the gradient as well) take at 8 TB/s."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import ddsp_amd as ddsp
from ddsp_amd import build, core
build.build()

BATCH, FRAMES = 32, 1000
HBM_BYTES_PER_US = 8e6
DEV = 'cuda'


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


# ---- the reference's chains in torch ops ----------------------------------------------------------------------------------------
def chain_critical_bands(x, k, depth, tables, bandwidth_scale=1.0, hz_min=20.0, hz_max=8000.0):
  f_center, bw, depth_modifier = tables
  modifier = torch.tanh(x.reshape(x.shape[0], x.shape[1], k, depth))
  modifier = torch.sum(modifier * depth_modifier[None, None, None, :], dim=-1)
  f = f_center + bandwidth_scale * bw[None, None, :] * modifier
  return torch.nn.functional.softplus(f) + hz_min - torch.nn.functional.softplus(f - (hz_max - hz_min))


def chain_wavetable(hd, n_wavetable):
  n_pad = int(n_wavetable / 2 - hd.shape[-1])
  fft_in = torch.nn.functional.pad(hd, (1, n_pad))
  fft_in = torch.complex(fft_in, torch.zeros_like(fft_in))
  return torch.fft.irfft(fft_in) * (n_wavetable / 2)


def forward_backward(fn, x, cot):
  leaf = x.clone().requires_grad_(True)
  def step():
    leaf.grad = None
    torch.autograd.backward(fn(leaf), cot)
  return step, leaf


def measure(row, fused, chain, x, cot, steps):
  with torch.no_grad():
    ours, theirs = fused(x), chain(x)
    row['max_abs_difference_forward'] = float((ours - theirs).abs().max())
    del ours, theirs
  step, leaf = forward_backward(fused, x, cot)
  step(); fused_grad = leaf.grad.clone()
  step, leaf = forward_backward(chain, x, cot)
  step(); row['max_abs_difference_gradient'] = float((fused_grad - leaf.grad).abs().max())
  del step, leaf, fused_grad
  for label, fn in (('fused', fused), ('torch_chain', chain)):
    with torch.no_grad():
      row['us_forward_' + label] = timed(lambda: fn(x), steps)
    row['us_forward_backward_' + label] = timed(forward_backward(fn, x, cot)[0], steps)
    torch.cuda.empty_cache()
  for what in ('forward', 'forward_backward'):
    row[what + '_speedup'] = row['us_%s_torch_chain' % what][0] / row['us_%s_fused' % what][0]


result = {'workload': 'core.frequencies_critical_bands and core.harmonic_distribution_to_wavetable, forward and forward + backward',
          'note': 'timings are [median, min, max] in microseconds per call, host wall clock around synchronised loops; '
                  'hbm_floor_us: the bytes of input and output (backward: + input, cotangents, gradient) at 8 TB/s',
          'shapes': {}}

K = 100
for depth in (1, 4, 64):
  x = torch.randn(BATCH, FRAMES, K * depth, device=DEV)
  cot = torch.randn(BATCH, FRAMES, K, device=DEV)
  tables = core._critical_band_device_tables((K, depth, 10.0, 20.0, 8000.0, 'bark'), x.device)
  forward_bytes = (x.numel() + cot.numel()) * 4
  row = {'batch': BATCH, 'frames': FRAMES, 'sinusoids': K, 'depth': depth,
         'hbm_floor_us_forward': forward_bytes / HBM_BYTES_PER_US,
         'hbm_floor_us_forward_backward': (forward_bytes + (2 * x.numel() + cot.numel()) * 4) / HBM_BYTES_PER_US}
  measure(row, lambda v, d=depth: core.frequencies_critical_bands(v, depth=d),
          lambda v, d=depth, t=tables: chain_critical_bands(v, K, d, t), x, cot, 20 if depth == 64 else 50)
  result['shapes']['critical_bands_32x1000x100_depth%d' % depth] = row
  del x, cot
  torch.cuda.empty_cache()

for harmonics, points in ((100, 2048), (60, 512)):
  hd = torch.rand(BATCH, FRAMES, harmonics, device=DEV)
  hd = hd / hd.sum(-1, keepdim=True)
  cot = torch.randn(BATCH, FRAMES, points, device=DEV)
  forward_bytes = (hd.numel() + cot.numel()) * 4
  row = {'batch': BATCH, 'frames': FRAMES, 'harmonics': harmonics, 'n_wavetable': points,
         'hbm_floor_us_forward': forward_bytes / HBM_BYTES_PER_US,
         'hbm_floor_us_forward_backward': 2 * forward_bytes / HBM_BYTES_PER_US}
  measure(row, lambda v, n=points: core.harmonic_distribution_to_wavetable(v, n_wavetable=n),
          lambda v, n=points: chain_wavetable(v, n), hd, cot, 20)
  result['shapes']['harmonic_wavetable_32x1000x%d_to_%d' % (harmonics, points)] = row
  del hd, cot
  torch.cuda.empty_cache()

if len(sys.argv) > 1:
  with open(sys.argv[1], 'w') as fh:
    fh.write(json.dumps(result, indent=1) + '\n')
print(json.dumps(result))
