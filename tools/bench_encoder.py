"""training.nn.normalize_op and training.encoders.MfccTimeDistributedRnnEncoder on their own.

normalize_op (csrc/group_norm.hip) forward and forward + backward at [32, 250, 1, 30] instance (the encoder's own shape),
[32, 1000, 1, 256] layer and [32, 1000, 1, 256] group, beside three things on the same GPU in the same session: (a) the
reference's op chain restated in framework ops (reshape, moments, subtract, divide); (b) torch.nn.functional.group_norm on the
permuted tensor; (c) the HBM floor from the bytes (forward: read x, write y; backward: read x and dy, write dx).  Then the whole
encoder (MFCCs -> instance norm -> GRU -> Dense -> resample) at batch 32 x 64000 samples, z_time_steps 250 and 1000, rnn_channels
512, forward and forward + backward in every weight.

    python tools/bench_encoder.py [out.json]

Warm clocks, medians of five timed loops (host wall clock around synchronised loops); one JSON line at the end."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import ddsp_amd as ddsp
from ddsp_amd import build
from ddsp_amd.training import encoders, nn
build.build()

DEV = 'cuda'
HBM_BYTES_PER_US = 8e6             # the chip's peak: 8 TB/s
NORM_SHAPES = [((32, 250, 1, 30), 'instance'), ((32, 1000, 1, 256), 'layer'), ((32, 1000, 1, 256), 'group')]
GROUPS = {'instance': lambda ch: ch, 'layer': lambda ch: 1, 'group': lambda ch: 32}


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


def reference_chain(x, norm_type, eps=1e-5):
  """ddsp/training/nn.py:561-575 in framework ops."""
  shape = x.shape
  n_groups = GROUPS[norm_type](shape[-1])
  x = x.reshape(tuple(shape[:-1]) + (n_groups, shape[-1] // n_groups))
  var, mean = torch.var_mean(x, dim=(1, 2, 4), keepdim=True, unbiased=False)
  return ((x - mean) / torch.sqrt(var + eps)).reshape(shape)


def framework_group_norm(x, norm_type, eps=1e-5):
  return F.group_norm(x.permute(0, 3, 1, 2), GROUPS[norm_type](x.shape[-1]), eps=eps).permute(0, 2, 3, 1)


result = {'workload': 'normalize_op and MfccTimeDistributedRnnEncoder: fused kernels, the reference op chain in framework ops, F.group_norm',
          'note': 'timings are [median, min, max] in microseconds per call, host wall clock around synchronised loops; hbm_floor_us from '
                  'the bytes at 8 TB/s',
          'normalize_op': {}, 'encoder': {}}
torch.manual_seed(0)
for shape, norm_type in NORM_SHAPES:
  row = {'shape': list(shape), 'norm_type': norm_type}
  x = torch.randn(*shape, device=DEV, requires_grad=True)
  cot = torch.randn(*shape, device=DEV)
  ways = {'fused': lambda: nn.normalize_op(x, norm_type), 'reference_chain': lambda: reference_chain(x, norm_type),
          'framework_group_norm': lambda: framework_group_norm(x, norm_type)}
  with torch.no_grad():
    ours = ways['fused']()
    row['max_abs_difference_reference_chain'] = float((ours - ways['reference_chain']()).abs().max())
    row['max_abs_difference_framework_group_norm'] = float((ours - ways['framework_group_norm']()).abs().max())
  for key, fn in ways.items():
    def forward(fn=fn):
      with torch.no_grad(): fn()
    row['us_forward_' + key] = timed(forward, 50)
    row['us_forward_backward_' + key] = timed(lambda fn=fn: torch.autograd.grad(fn(), [x], cot), 20)
  row['hbm_floor_us_forward'] = 2 * x.numel() * 4 / HBM_BYTES_PER_US
  row['hbm_floor_us_forward_backward'] = 5 * x.numel() * 4 / HBM_BYTES_PER_US
  result['normalize_op']['%s_%s' % ('x'.join(map(str, shape)), norm_type)] = row
  print(json.dumps(row), flush=True)
  del x, cot

for z_time_steps in (250, 1000):
  row = {'batch': 32, 'n_samples': 64000, 'z_time_steps': z_time_steps, 'rnn_channels': 512, 'z_dims': 32}
  enc = encoders.MfccTimeDistributedRnnEncoder(rnn_channels=512, z_dims=32, z_time_steps=z_time_steps)
  audio = 0.3 * torch.randn(32, 64000, device=DEV)
  f0_scaled = torch.rand(32, 1000, 1, device=DEV)
  with torch.no_grad():
    z = enc(audio, f0_scaled)['z']                       # builds
  row['z_shape'] = list(z.shape)
  params = list(enc.parameters())
  cot = torch.randn_like(z)
  def forward():
    with torch.no_grad(): enc(audio, f0_scaled)
  def mfccs():
    with torch.no_grad(): enc.compute_mfccs(audio)
  row['us_mfccs'] = timed(mfccs, 5)
  row['us_forward'] = timed(forward, 3)
  row['us_forward_backward'] = timed(lambda: torch.autograd.grad(enc(audio, f0_scaled)['z'], params, cot), 2)
  result['encoder']['z_time_steps_%d' % z_time_steps] = row
  print(json.dumps(row), flush=True)
  del enc, audio, cot
  torch.cuda.empty_cache()

if len(sys.argv) > 1:
  with open(sys.argv[1], 'w') as fh:
    fh.write(json.dumps(result, indent=1) + '\n')
print(json.dumps(result))
