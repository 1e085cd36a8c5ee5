"""synths.Sinusoidal on its own at the shape of the reference's shipped self-supervised model (100 sinusoids, 1000 frames,
64 000 samples, 16 kHz): the fused forward, forward + backward, and the chain of materialised envelopes it replaces
(core.resample twice + core.oscillator_bank on [batch, n_samples, n_sinusoids]; at the largest batch that fits, per row).

    python tools/bench_sinusoidal.py [out.json]

One session, warm clocks, medians of repeated timed loops; the HBM floor of the chain is 5 envelopes at 8 TB/s."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import functools
import numpy as np, torch
import ddsp_amd as ddsp
from ddsp_amd import _lib, build
build.build()
F, K, N, SR = 1000, 100, 64000, 16000
HBM_PEAK = 8e12                                   # bench.py's roofline figure


def timed(fn, steps, repeats=5):
  for _ in range(3): fn()
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
  return statistics.median(out), min(out), max(out)


def controls(batch):
  rng = np.random.default_rng(0)
  a = ddsp.core.tf_float32(rng.uniform(0.0, 1.0, (batch, F, K)))
  f = ddsp.core.tf_float32(np.exp(rng.uniform(np.log(40.0), np.log(7900.0), (batch, F, K))))
  return a, f


def chain(a, f):
  return ddsp.core.oscillator_bank(ddsp.core.resample(f, N), ddsp.core.resample(a, N, 'window'), SR)


result = {'workload': 'synths.Sinusoidal: %d frames, %d sinusoids, %d samples at %d Hz' % (F, K, N, SR), 'batches': {}}
from_controls = ddsp.synths.Sinusoidal(n_samples=N, sample_rate=SR, amp_scale_fn=None, freq_scale_fn=None)
default = ddsp.synths.Sinusoidal(n_samples=N, sample_rate=SR)
shipped = ddsp.synths.Sinusoidal(n_samples=N, sample_rate=SR, freq_scale_fn=functools.partial(ddsp.core.frequencies_softmax, depth=64))
for B in (32, 128):
  a, f = controls(B)
  rng = np.random.default_rng(1)
  raw_a = ddsp.core.tf_float32(rng.standard_normal((B, F, K)))
  raw_f = ddsp.core.tf_float32(rng.standard_normal((B, F, K)))
  row = {}
  with torch.no_grad():
    row['us_forward_from_controls'] = [t * 1e6 for t in timed(lambda: from_controls.get_signal(a, f), 50)]
    row['us_forward_class_defaults'] = [t * 1e6 for t in timed(lambda: default(raw_a, raw_f), 50)]
    _lib.profile_begin(['sin_synth_kernel'], max_records=64)
    for _ in range(20): from_controls.get_signal(a, f)
    torch.cuda.synchronize()
    row['kernel_us'] = {k: v[0] / v[1] * 1e3 for k, v in _lib.profile_end().items()}
  ga, gf = raw_a.clone().requires_grad_(True), raw_f.clone().requires_grad_(True)
  gout = torch.ones((B, N), device=a.device)
  def step():
    ga.grad = gf.grad = None
    default(ga, gf).backward(gout)
  row['us_forward_backward_class_defaults'] = [t * 1e6 for t in timed(step, 20)]
  _lib.profile_begin(['sin_bwd_sums_kernel'], max_records=64)
  for _ in range(10): step()
  torch.cuda.synchronize()
  row['kernel_us'].update({k: v[0] / v[1] * 1e3 for k, v in _lib.profile_end().items()})
  row['backward_over_forward'] = (row['us_forward_backward_class_defaults'][0] - row['us_forward_class_defaults'][0]) / \
      row['us_forward_class_defaults'][0]
  row['chain_hbm_floor_us'] = 5.0 * B * N * K * 4 / HBM_PEAK * 1e6
  if B == 32:
    with torch.no_grad():
      raw_f64 = ddsp.core.tf_float32(rng.standard_normal((B, F, K * 64)))
      row['us_forward_shipped_softmax_depth64'] = [t * 1e6 for t in timed(lambda: shipped(raw_a, raw_f64), 20)]
      row['shipped_raw_input_bytes'] = 4 * B * F * K * 65
    del raw_f64
  result['batches'][str(B)] = row
  del a, f, raw_a, raw_f, ga, gf, gout
  torch.cuda.empty_cache()
# the chain: three [B, N, K] fp32 tensors live at once (two envelopes and the oscillator bank's scratch)
free = torch.cuda.mem_get_info()[0]
Bc = int(max(1, min(32, free // (6 * N * K * 4))))
a, f = controls(Bc)
with torch.no_grad():
  t = timed(lambda: chain(a, f), 5)
  err = float((from_controls.get_signal(a, f) - chain(a, f)).abs().max())
result['chain'] = {'batch': Bc, 'us': [x * 1e6 for x in t], 'us_per_row': t[0] * 1e6 / Bc, 'max_abs_diff_fused_vs_chain': err}
for B in (32, 128):
  row = result['batches'][str(B)]
  row['chain_us_at_this_batch_from_per_row'] = result['chain']['us_per_row'] * B
  row['chain_over_fused'] = row['chain_us_at_this_batch_from_per_row'] / row['us_forward_from_controls'][0]
  row['forward_below_chain_hbm_floor'] = row['us_forward_from_controls'][0] < row['chain_hbm_floor_us']
result['note'] = 'timings are [median, min, max] of 5 timed loops, host wall clock around synchronised loops'
text = json.dumps(result, indent=1)
print(text)
if len(sys.argv) > 1:
  with open(sys.argv[1], 'w') as fh:
    fh.write(text + '\n')
