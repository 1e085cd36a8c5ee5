"""training.decoders.RnnFcDecoder on its own, at the decoder gin/models/solo_instrument.gin ships (rnn_channels = ch = 512, three
layers per stack, inputs ld_scaled and f0_scaled, outputs 1 + 60 + 65) over 1000 frames at batch 32 and 128: the GRU forward and
forward + backward, one bias + LayerNorm + activation layer, and the whole decoder - on the kernels of csrc/decoder.hip and,
beside each, the same thing built from framework ops (torch.nn.GRU, F.layer_norm, F.leaky_relu, torch.matmul; the thing compared
against, not product code) on the same GPU in the same session, eager and replayed from a captured graph.

    python tools/bench_decoder.py [out.json]

Warm clocks, medians of five timed loops (host wall clock around synchronised loops); one JSON line at the end.  Beside the GRU:
the floor its design implies - one dependent kernel boundary per step, 1.45 - 1.9 us each."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import ddsp_amd as ddsp
from ddsp_amd import build
from ddsp_amd.training import decoders, nn
build.build()

STEPS, HIDDEN, CH, LAYERS = 1000, 512, 512, 3
SPLITS = (('amps', 1), ('harmonic_distribution', 60), ('noise_magnitudes', 65))
KEYS = ('ld_scaled', 'f0_scaled')
BOUNDARY_US = (1.45, 1.9)          # a dependent kernel boundary on this chip
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


def graphed(fn):
  """fn captured once (after a warm-up on a side stream); -> the replay, or the error's text when the capture fails."""
  try:
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
      fn(); fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
      fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph.replay
  except Exception as e:      # the capture is the framework's; what it cannot capture is recorded, not hidden
    torch.cuda.synchronize()
    return '%s: %s' % (type(e).__name__, str(e).splitlines()[0][:200])


def both_ways(row, key, fn, steps):
  row['us_' + key] = timed(fn, steps)
  replay = graphed(fn)
  if callable(replay):
    row['us_' + key + '_graph'] = timed(replay, steps)
  else:
    row[key + '_graph_error'] = replay


# ---- the framework's decoder, holding the same weights ---------------------------------------------------------------------------
def torch_gru_from(layer):
  h = layer.units
  order = torch.cat([torch.arange(h, 2 * h), torch.arange(h), torch.arange(2 * h, 3 * h)]).to(DEV)     # (z, r, h) -> (r, z, n)
  gru = torch.nn.GRU(layer.kernel.shape[0], h, batch_first=True).to(DEV)
  with torch.no_grad():
    gru.weight_ih_l0.copy_(layer.kernel.t()[order]); gru.weight_hh_l0.copy_(layer.recurrent_kernel.t()[order])
    gru.bias_ih_l0.copy_(layer.bias[0][order]); gru.bias_hh_l0.copy_(layer.bias[1][order])
  return gru


def framework_fc(fc, x):
  v = torch.matmul(x, fc.dense.kernel) + fc.dense.bias
  return F.leaky_relu(F.layer_norm(v, (v.shape[-1],), fc.layer_norm.gamma, fc.layer_norm.beta, eps=1e-3), 0.2)


def framework_decoder(dec, gru):
  def run(ld, f0):
    stacks = []
    for stack, x in zip(dec.input_stacks, (ld, f0)):
      for fc in stack.layers: x = framework_fc(fc, x)
      stacks.append(x)
    y, _ = gru(torch.cat(stacks, -1))
    x = torch.cat(stacks + [y], -1)
    for fc in dec.out_stack.layers: x = framework_fc(fc, x)
    return torch.matmul(x, dec.dense_out.kernel) + dec.dense_out.bias
  return run


result = {'workload': 'RnnFcDecoder of solo_instrument.gin, 1000 frames: GRU, one norm layer, the whole decoder; fused kernels and framework ops',
          'note': 'timings are [median, min, max] in microseconds per call, host wall clock around synchronised loops; *_graph: replayed '
                  'from a captured graph; gru_floor_us: 1000 dependent kernel boundaries at 1.45 - 1.9 us',
          'gru_floor_us': [STEPS * b for b in BOUNDARY_US], 'shapes': {}}
torch.manual_seed(0)
for batch in (32, 128):
  row = {'batch': batch, 'steps': STEPS, 'hidden': HIDDEN, 'ch': CH}
  dec = decoders.RnnFcDecoder(rnn_channels=HIDDEN, ch=CH, layers_per_stack=LAYERS, input_keys=KEYS, output_splits=SPLITS)
  ld, f0 = torch.rand(batch, STEPS, 1, device=DEV), torch.rand(batch, STEPS, 1, device=DEV)
  with torch.no_grad():
    dec(ld, f0)                                        # builds
  layer = dec.rnn.rnn
  gru = torch_gru_from(layer)
  params = list(dec.parameters())

  # the GRU on its input: [batch, 1000, 1024] -> [batch, 1000, 512]
  x = torch.randn(batch, STEPS, 2 * CH, device=DEV, requires_grad=True)
  cot = torch.randn(batch, STEPS, HIDDEN, device=DEV)
  with torch.no_grad():
    row['gru_max_abs_difference'] = float((layer(x) - gru(x)[0]).abs().max())
  gru_leaves = [x, layer.kernel, layer.recurrent_kernel, layer.bias]
  torch_leaves = [x] + list(gru.parameters())
  def ours_fwd():
    with torch.no_grad(): layer(x)
  def theirs_fwd():
    with torch.no_grad(): gru(x)
  both_ways(row, 'gru_forward_fused', ours_fwd, 5)
  both_ways(row, 'gru_forward_framework', theirs_fwd, 5)
  both_ways(row, 'gru_forward_backward_fused', lambda: torch.autograd.grad(layer(x), gru_leaves, cot), 3)
  both_ways(row, 'gru_forward_backward_framework', lambda: torch.autograd.grad(gru(x)[0], torch_leaves, cot), 3)
  # the recurrence alone, on a given input projection (what csrc/decoder.hip runs: no matrix product of the framework's)
  with torch.no_grad():
    mx = torch.addmm(layer.bias[0], x.reshape(-1, 2 * CH), layer.kernel).reshape(batch, STEPS, 3 * HIDDEN)
  mx.requires_grad_(True)
  def scan_fwd():
    with torch.no_grad(): nn.gru_recurrence(mx, layer.recurrent_kernel, layer.bias[1])
  both_ways(row, 'gru_scan_forward_fused', scan_fwd, 5)
  both_ways(row, 'gru_scan_forward_backward_fused', lambda: torch.autograd.grad(nn.gru_recurrence(mx, layer.recurrent_kernel, layer.bias[1]), [mx], cot), 3)
  for key in ('gru_scan_forward_fused', 'gru_scan_forward_fused_graph'):
    if 'us_' + key in row:
      row[key + '_us_per_step'] = row['us_' + key][0] / STEPS
  del mx

  # one bias + LayerNorm + leaky_relu layer on [batch * 1000, 512]
  fc = dec.out_stack.layers[1]
  v = torch.randn(batch * STEPS, CH, device=DEV, requires_grad=True)
  vcot = torch.randn(batch * STEPS, CH, device=DEV)
  norm_leaves = [v, fc.dense.bias, fc.layer_norm.gamma, fc.layer_norm.beta]
  ours_norm = lambda: nn.bias_norm_act(v, fc.dense.bias, fc.layer_norm.gamma, fc.layer_norm.beta, 'leaky_relu')
  theirs_norm = lambda: F.leaky_relu(F.layer_norm(v + fc.dense.bias, (CH,), fc.layer_norm.gamma, fc.layer_norm.beta, eps=1e-3), 0.2)
  with torch.no_grad():
    row['norm_max_abs_difference'] = float((ours_norm() - theirs_norm()).abs().max())
    row['us_norm_forward_fused'] = timed(ours_norm, 20)
    row['us_norm_forward_framework'] = timed(theirs_norm, 20)
  row['us_norm_forward_backward_fused'] = timed(lambda: torch.autograd.grad(ours_norm(), norm_leaves, vcot), 10)
  row['us_norm_forward_backward_framework'] = timed(lambda: torch.autograd.grad(theirs_norm(), norm_leaves, vcot), 10)
  row['norm_hbm_floor_us_forward'] = 2 * v.numel() * 4 / 8e6
  del v, vcot

  # the whole decoder
  framework = framework_decoder(dec, gru)
  ocot = torch.randn(batch, STEPS, sum(n for _, n in SPLITS), device=DEV)
  ours_dec = lambda: torch.cat(list(dec(ld, f0).values()), -1)
  with torch.no_grad():
    row['decoder_max_abs_difference'] = float((ours_dec() - framework(ld, f0)).abs().max())
  def ours_dec_fwd():
    with torch.no_grad(): ours_dec()
  def theirs_dec_fwd():
    with torch.no_grad(): framework(ld, f0)
  both_ways(row, 'decoder_forward_fused', ours_dec_fwd, 3)
  both_ways(row, 'decoder_forward_framework', theirs_dec_fwd, 3)
  both_ways(row, 'decoder_forward_backward_fused', lambda: torch.autograd.grad(ours_dec(), params, ocot), 2)
  both_ways(row, 'decoder_forward_backward_framework', lambda: torch.autograd.grad(framework(ld, f0), params + list(gru.parameters()), ocot, allow_unused=True), 2)
  result['shapes']['batch_%d' % batch] = row
  del dec, gru, x, cot, ocot
  torch.cuda.empty_cache()
  print(json.dumps(row), flush=True)

if len(sys.argv) > 1:
  with open(sys.argv[1], 'w') as fh:
    fh.write(json.dumps(result, indent=1) + '\n')
print(json.dumps(result))
