"""The consistency losses on their own at the shape synths.Sinusoidal is benchmarked on (1000 frames, 100 sinusoids; 100
candidates, 30 harmonic Gaussians, 10 harmonic points, 100 harmonics): forward and forward + backward of TWMLoss (candidates =
the sinusoids, and one candidate), KDEConsistencyLoss and core.sinusoidal_to_harmonic at batch 32 and 128, and beside each the
materialised chain in torch elementwise ops (what the reference builds; the thing compared against, not product code) at the
largest batch that fits, per row.

    python tools/bench_consistency.py [out.json]

One session, warm clocks, medians of repeated timed loops (host wall clock around synchronised loops)."""
import json, math, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import ddsp_amd as ddsp
from ddsp_amd import build
build.build()
T, K, C, G, P, H = 1000, 100, 100, 30, 10, 100
CLOCK_HZ = 2.4e9                                  # the MI355X's peak engine clock


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


def inputs(batch, seed=0):
  rng = np.random.default_rng(seed)
  amps = ddsp.core.tf_float32(rng.uniform(0.01, 1.0, (batch, T, K)))
  freqs = ddsp.core.tf_float32(np.exp(rng.uniform(np.log(40.0), np.log(7600.0), (batch, T, K))))
  f0 = ddsp.core.tf_float32(np.exp(rng.uniform(np.log(60.0), np.log(1000.0), (batch, T, 1))))
  return amps, freqs, f0


def torch_twm_sinusoid_side(f0c, freqs, amps, scale=0.2):
  """The [B, T, C, K, G] chain of TWMLoss's first half in torch ops (the second half is a third of its size)."""
  ratios = freqs[:, :, None, :] / f0c[:, :, :, None]
  z = (ratios[..., None] - torch.arange(1, G + 1, device=freqs.device, dtype=torch.float32)) / scale
  nll = -(torch.logsumexp(-0.5 * z * z, -1) - math.log(G) - math.log(scale) - 0.5 * math.log(2 * math.pi))
  return (nll * amps[:, :, None, :]).sum(-1) / amps.sum(-1, keepdim=True)


def torch_kde_nll(amps, freqs, amps_t, freqs_t, scale=0.1):
  midi = lambda f: 12.0 * (torch.log2(f) - math.log2(440.0)) + 69.0
  z = (midi(freqs)[..., None] - midi(freqs_t)[:, :, None, :]) / scale
  lw = torch.log(amps_t / amps_t.sum(-1, keepdim=True))[:, :, None, :]
  nll = -(torch.logsumexp(-0.5 * z * z + lw, -1) - math.log(scale) - 0.5 * math.log(2 * math.pi))
  return (nll * amps / amps.sum(-1, keepdim=True)).mean(-1)


def torch_s2h(amps, freqs, f0, width=0.1):
  harm = f0 * torch.arange(1, H + 1, device=f0.device, dtype=torch.float32)
  ratio = (freqs[:, :, None, :] - harm[..., None]) / f0[..., None]
  ha = (torch.exp(-(ratio / width) ** 2) * amps[:, :, None, :]).sum(-1)
  ha = torch.where(harm >= 8000.0, torch.zeros_like(ha), ha)
  return ha.sum(-1, keepdim=True), ha


twm, kde = ddsp.losses.TWMLoss(), ddsp.losses.KDEConsistencyLoss()
result = {'workload': 'consistency losses: %d frames, %d sinusoids, %d candidates, %d gaussians, %d points, %d harmonics' % (T, K, C, G, P, H),
          'batches': {}}
for B in (32, 128):
  amps, freqs, f0 = inputs(B)
  amps_b, freqs_b, _ = inputs(B, 1)
  row = {}
  cases = {'twm_own_candidates': lambda a, f: twm(f, f, a), 'twm_c1': lambda a, f: twm(f0, f, a),
           'kde': lambda a, f: kde(a, f, amps_b, freqs_b),
           'sinusoidal_to_harmonic': lambda a, f: sum(o.sum() for o in ddsp.core.sinusoidal_to_harmonic(a, f, f0, n_harmonics=H))}
  for name, fn in cases.items():
    with torch.no_grad():
      row['us_forward_' + name] = timed(lambda: fn(amps, freqs), 5 if name == 'twm_own_candidates' else 20)
    ga, gf = amps.clone().requires_grad_(True), freqs.clone().requires_grad_(True)
    def step():
      ga.grad = gf.grad = None
      fn(ga, gf).backward()
    row['us_forward_backward_' + name] = timed(step, 3 if name == 'twm_own_candidates' else 10)
  # Gaussian terms per call, for the instruction floor (terms x issued instructions per term / (256 CUs x 4 SIMDs x 16 lanes x clock))
  row['gaussian_terms'] = {'twm_own_candidates': B * T * (C * K * G + C * P * K), 'twm_c1': B * T * (K * G + P * K),
                           'kde': 2 * B * T * K * K, 'sinusoidal_to_harmonic': B * T * H * K}
  # issued instructions per Gaussian term, counted in the inner loops of `hipcc -S --offload-arch=gfx950` (forward): 12 in
  # grid_eval's loop (one v_exp_f32), 18 + 20 in mix_eval's two passes (max, then one v_exp_f32 and two FMAs), 21 in
  # s2h_kernel's (unrolled by four, a division per term); one instruction per lane and clock on 256 CUs x 4 SIMDs x 16 lanes
  per_term = {'twm_own_candidates': (B * T * C * K * G * 12 + B * T * C * P * K * 38), 'twm_c1': B * T * (K * G * 12 + P * K * 38),
              'kde': 2 * B * T * K * K * 38, 'sinusoidal_to_harmonic': B * T * H * K * 21}
  row['instruction_floor_us_forward'] = {k: v / (256 * 4 * 16 * CLOCK_HZ) * 1e6 for k, v in per_term.items()}
  result['batches'][str(B)] = row
  del amps, freqs, f0, amps_b, freqs_b
  torch.cuda.empty_cache()
# the materialised chains, at the largest batch that fits (about eight tensors of the largest size live at once)
free = torch.cuda.mem_get_info()[0]
chains = {}
with torch.no_grad():
  Bc = int(max(1, min(8, free // (8 * T * C * K * G * 4))))
  amps, freqs, f0 = inputs(Bc)
  t = timed(lambda: torch_twm_sinusoid_side(freqs, freqs, amps), 2, repeats=3)
  chains['twm_sinusoid_side_own_candidates'] = {'batch': Bc, 'us': t, 'us_per_row': t[0] / Bc}
  Bc = int(max(1, min(32, free // (8 * T * K * K * 4))))
  amps, freqs, f0 = inputs(Bc)
  amps_b, freqs_b, _ = inputs(Bc, 1)
  t = timed(lambda: torch_kde_nll(amps, freqs, amps_b, freqs_b), 3, repeats=3)
  chains['kde_nll_one_direction'] = {'batch': Bc, 'us': t, 'us_per_row': t[0] / Bc}
  t = timed(lambda: torch_s2h(amps, freqs, f0), 3, repeats=3)
  chains['sinusoidal_to_harmonic'] = {'batch': Bc, 'us': t, 'us_per_row': t[0] / Bc}
result['torch_chains'] = chains
result['note'] = 'timings are [median, min, max] in microseconds, host wall clock around synchronised loops; the torch chains are per call at their own batch'
text = json.dumps(result, indent=1)
print(text)
if len(sys.argv) > 1:
  with open(sys.argv[1], 'w') as fh:
    fh.write(text + '\n')
