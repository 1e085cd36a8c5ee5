"""synths.Wavetable on its own: forward and forward + backward, against the input-once HBM floor and against the
materialised chain built from the project's existing ops (core.resample to [batch, n_samples, n_wavetable] + elementwise
torch, what the reference's graph amounts to), at batch 1 where that chain fits.

    python tools/bench_wavetable.py [batch] [n_frames] [n_wavetable] [n_samples]
"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import ddsp_amd as ddsp
from ddsp_amd import _lib, build
build.build()
B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
F = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
W = int(sys.argv[3]) if len(sys.argv) > 3 else 2048
N = int(sys.argv[4]) if len(sys.argv) > 4 else 64000
SR = 16000
HBM_PEAK = 8e12                                   # bench.py's roofline figure


def inputs(batch):
  rng = np.random.default_rng(0)
  amps = ddsp.core.tf_float32(rng.standard_normal((batch, F, 1)))
  tables = ddsp.core.tf_float32(rng.standard_normal((batch, F, W)))
  f0 = ddsp.core.tf_float32(np.exp(rng.uniform(np.log(60.0), np.log(2000.0), (batch, F, 1))))
  return amps, tables, f0


def timed(fn, steps):
  for _ in range(5): fn()
  t_settle = time.perf_counter()
  while time.perf_counter() - t_settle < 0.05:    # the GPU needs ~20 ms of load to reach its sustained clock
    for _ in range(5): fn()
    torch.cuda.synchronize()
  torch.cuda.synchronize(); t0 = time.perf_counter()
  for _ in range(steps): fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / steps


def chain(amps, tables, f0):
  """The materialised chain on existing ops, scale_fn included (batch 1: [1, N, W] is 0.5 GB at the defaults)."""
  a = ddsp.core.resample(ddsp.core.exp_sigmoid(amps), N, 'window')[:, :, 0]
  f = ddsp.core.resample(f0, N)[:, :, 0]
  w = ddsp.core.resample(ddsp.core.exp_sigmoid(tables), N)                     # [B, N, W]
  w = torch.cat([w, w[..., 0:1]], dim=-1)
  vel = f.double() / SR          # (in fp32 the division alone is a relative bias: 1e-4 cycles after 4 s at 2 kHz)
  phase = (torch.cumsum(vel, dim=1) - vel).remainder(1.0).float()
  grid = torch.linspace(0.0, 1.0, W + 1, device=w.device)
  weights = torch.relu(1.0 - (phase[:, :, None] - grid[None, None, :]).abs() * W)
  return (weights * w).sum(-1) * a


synth = ddsp.synths.Wavetable(n_samples=N, sample_rate=SR)
amps, tables, f0 = inputs(B)
with torch.no_grad():
  fwd = timed(lambda: synth(amps, tables, f0), 200)
  _lib.profile_begin(['wt_fused_kernel'], max_records=64)
  for _ in range(20): synth(amps, tables, f0)
  torch.cuda.synchronize()
  kernel = _lib.profile_end()
ga, gw, gf = (t.clone().requires_grad_(True) for t in (amps, tables, f0))
gout = torch.ones((B, N), device=amps.device)
def step():
  ga.grad = gw.grad = gf.grad = None
  synth(ga, gw, gf).backward(gout)
both = timed(step, 50)
a1, w1, f1 = inputs(1)
with torch.no_grad():
  one = timed(lambda: synth(a1, w1, f1), 200)
  ref = timed(lambda: chain(a1, w1, f1), 5)
  err = float((synth(a1, w1, f1) - chain(a1, w1, f1)).abs().max())
floor_bytes = 4.0 * B * (F * (W + 2) + N)
print(json.dumps({
    'workload': 'synths.Wavetable: batch=%d, %d frames, %d-point tables, %d samples' % (B, F, W, N),
    'us_per_call_forward': fwd * 1e6, 'us_per_call_forward_backward': both * 1e6,
    'kernel_us': {k: v[0] / v[1] * 1e3 for k, v in kernel.items()},
    'floor_bytes_inputs_once': floor_bytes, 'floor_us_at_8TBs': floor_bytes / HBM_PEAK * 1e6,
    'hbm_frac_forward': floor_bytes / fwd / HBM_PEAK,
    'batch1_us_fused': one * 1e6, 'batch1_us_materialised_chain': ref * 1e6, 'chain_over_fused_per_row': ref / one,
    'batch1_max_abs_diff_fused_vs_chain': err}))
