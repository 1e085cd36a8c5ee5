"""losses.SpectralLoss forward on its own: time per call and per-scale kernel time.

    python tools/bench_spectral_loss.py [batch] [n_samples] [--deterministic] [--sizes 6144,3072,...]

--deterministic adds a column: value + gradient with SpectralLoss(deterministic=True) (slabs + gather, no float atomics) beside
deterministic=False, the two taken in turn in this one session - host wall clock around synchronised loops of 50 calls, the
median of 7 such loops each - with the bytes of slab workspace the instance holds afterwards.  --sizes: other frame sizes than the default six.
"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import ddsp_amd as ddsp
from ddsp_amd import _lib, build
build.build()
WITH_DET = '--deterministic' in sys.argv
if WITH_DET: sys.argv.remove('--deterministic')
SIZES = (2048, 1024, 512, 256, 128, 64)
if '--sizes' in sys.argv:
  i = sys.argv.index('--sizes'); SIZES = tuple(int(v) for v in sys.argv[i + 1].split(',')); del sys.argv[i:i + 2]
B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
N = int(sys.argv[2]) if len(sys.argv) > 2 else 64000
rng = np.random.default_rng(0)
t = ddsp.core.tf_float32(0.3 * rng.standard_normal((B, N)))
a = ddsp.core.tf_float32(0.3 * rng.standard_normal((B, N)))
loss = ddsp.losses.SpectralLoss(fft_sizes=SIZES, mag_weight=1.0, logmag_weight=1.0)
for _ in range(5): loss(t, a)
t_settle = time.perf_counter()
while time.perf_counter() - t_settle < 0.05:      # the GPU needs ~20 ms of load to reach its sustained clock
  for _ in range(5): loss(t, a)
  torch.cuda.synchronize()
_lib.profile_begin(None, max_records=64)
for _ in range(10): loss(t, a)
torch.cuda.synchronize()
bd = _lib.profile_end()
steps = 100
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(steps): out = loss(t, a)
torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / steps
ag = a.clone().requires_grad_(True)
for _ in range(5):
  ag.grad = None; loss(t, ag).backward()
torch.cuda.synchronize(); t1 = time.perf_counter()
for _ in range(50):
  ag.grad = None; loss(t, ag).backward()
torch.cuda.synchronize(); dt_fb = (time.perf_counter() - t1) / 50
det = {}
if WITH_DET:
  variants = {flag: ddsp.losses.SpectralLoss(fft_sizes=SIZES, mag_weight=1.0, logmag_weight=1.0, deterministic=flag)
              for flag in (False, True)}
  def fwd_bwd(which, calls):
    for _ in range(calls):
      ag.grad = None; variants[which](t, ag).backward()
    torch.cuda.synchronize()
  for flag in variants: fwd_bwd(flag, 10)
  loops = {False: [], True: []}
  for _ in range(7):
    for flag in (False, True):                                  # in turn: both see the same clocks
      t2 = time.perf_counter(); fwd_bwd(flag, 50); loops[flag].append((time.perf_counter() - t2) / 50 * 1e3)
  slabs = sum(buf.numel() for buf in variants[True]._grad_ws._bufs.values())
  det = {'ms_per_fwd_bwd_atomics': statistics.median(loops[False]), 'ms_per_fwd_bwd_deterministic': statistics.median(loops[True]),
         'ms_per_fwd_bwd_atomics_loops': loops[False], 'ms_per_fwd_bwd_deterministic_loops': loops[True],
         'deterministic_over_atomics': statistics.median(loops[True]) / statistics.median(loops[False]),
         'slab_workspace_bytes': slabs}
alg = 4.0 * 2 * B * N                  # both signals read once (the 6 scales x 4 overlaps re-read from L2)
print(json.dumps(dict({'workload': 'SpectralLoss(mag+logmag, sizes %s) batch=%d, %d samples' % (','.join(map(str, SIZES)), B, N),
                       'ms_per_call': dt * 1e3, 'ms_per_fwd_bwd': dt_fb * 1e3, 'Msamples_per_s': B * N / dt / 1e6,
                       'kernel_us': {k: v[0] / v[1] * 1e3 for k, v in bd.items()},
                       'algorithmic_bytes': alg, 'hbm_frac': alg / dt / 8e12}, **det)))
