"""losses.HmmTranscriber on its own: the likelihood (nll), nll + its backward pass, and the Viterbi decode (predict_midi) of the
fused path (csrc/hmm.hip) at batch 32 x 1000 steps x 128 states, and beside each the same thing as the dense recursion in
torch ops - a logsumexp, or a max, over a [batch, states, states] tensor per step, which is what
tfp.distributions.HiddenMarkovModel builds; the thing compared against, not product code - on the same GPU in the same
session.

    python tools/bench_hmm.py [out.json]

Warm clocks, medians of five timed loops (host wall clock around synchronised loops); one JSON line at the end."""
import json, math, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import ddsp_amd as ddsp
from ddsp_amd import build
build.build()

BATCH, STEPS, STATES = 32, 1000, 128


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


def inputs(seed):
  """Note-like sequences: notes of 3-40 steps at integer pitches with jitter, a quarter of the segments silent."""
  rng = np.random.default_rng(seed)
  pitch, amps = np.zeros((BATCH, STEPS)), np.zeros((BATCH, STEPS))
  for b in range(BATCH):
    t = 0
    while t < STEPS:
      n = min(int(rng.integers(3, 41)), STEPS - t)
      if rng.uniform() < 0.75:
        pitch[b, t:t + n], amps[b, t:t + n] = rng.integers(1, STATES) + rng.uniform(-0.3, 0.3, n), 1.5 + rng.uniform(-0.3, 0.3, n)
      else:
        pitch[b, t:t + n], amps[b, t:t + n] = rng.uniform(0.0, STATES, n), rng.normal(0.0, 0.03, n)
      t += n
  return ddsp.core.tf_float32(pitch[:, :, None]), ddsp.core.tf_float32(amps[:, :, None])


class TorchHmm:
  """ddsp/losses.py:246-345 as dense tensors and torch ops, fp32 on the GPU."""

  def __init__(self, device, avg_length=200, midi_std=0.5, on=(1.5, 0.5), off=(0.0, 0.1)):
    n = STATES
    hold = 1.0 - 1.0 / avg_length
    other = (1.0 - hold) / (n - 1)
    trans = (hold - other) * torch.eye(n, device=device) + other * torch.ones(n, n, device=device)
    self.log_trans = torch.log(trans / trans.sum(1, keepdim=True))
    one = torch.ones(1, device=device)
    self.p_loc = torch.cat([one * n / 2.0, torch.arange(1, n, device=device, dtype=torch.float32)])
    self.p_scale = torch.cat([one * n, torch.ones(n - 1, device=device) * midi_std])
    self.a_loc = torch.cat([one * off[0], torch.ones(n - 1, device=device) * on[0]])
    self.a_scale = torch.cat([one * off[1], torch.ones(n - 1, device=device) * on[1]])

  def log_obs(self, pitch, amps):
    zp, za = (pitch - self.p_loc) / self.p_scale, (amps - self.a_loc) / self.a_scale
    return -0.5 * (zp * zp + za * za) - torch.log(self.p_scale) - torch.log(self.a_scale) - math.log(2.0 * math.pi)

  def nll(self, pitch, amps):
    obs = self.log_obs(pitch, amps)
    alpha = obs[:, 0] - math.log(STATES)
    for t in range(1, STEPS):
      alpha = torch.logsumexp(alpha[:, :, None] + self.log_trans, dim=1) + obs[:, t]
    return (-torch.logsumexp(alpha, dim=-1) / STEPS).mean()

  def predict_midi(self, pitch, amps):
    obs = self.log_obs(pitch, amps)
    v = obs[:, 0] - math.log(STATES)
    back = []
    for t in range(1, STEPS):
      v, arg = torch.max(v[:, :, None] + self.log_trans, dim=1)
      v = v + obs[:, t]
      back.append(arg)
    state = torch.argmax(v, dim=-1)
    path = [state]
    for arg in reversed(back):
      state = torch.gather(arg, 1, state[:, None])[:, 0]
      path.append(state)
    return torch.stack(path[::-1], dim=1).to(torch.float32)[:, :, None]


pitch, amps = inputs(0)
fused, chain = ddsp.losses.HmmTranscriber(), TorchHmm(pitch.device)
row = {'batch': BATCH, 'steps': STEPS, 'states': STATES}
with torch.no_grad():
  row['fused_value'], row['torch_chain_value'] = float(fused.nll(pitch, amps)), float(chain.nll(pitch, amps))
  assert abs(row['fused_value'] - row['torch_chain_value']) <= 1e-4 * abs(row['torch_chain_value']), row
  row['viterbi_mismatches'] = int((fused.predict_midi(pitch, amps) != chain.predict_midi(pitch, amps)).sum())
for label, model, steps in (('fused', fused, 20), ('torch_chain', chain, 2)):
  with torch.no_grad():
    row['us_forward_' + label] = timed(lambda: model.nll(pitch, amps), steps)
    row['us_viterbi_' + label] = timed(lambda: model.predict_midi(pitch, amps), steps)
  leaves = [x.clone().requires_grad_(True) for x in (pitch, amps)]
  def step():
    for x in leaves: x.grad = None
    model.nll(*leaves).backward()
  row['us_forward_backward_' + label] = timed(step, steps)
for what in ('forward', 'forward_backward', 'viterbi'):
  row[what + '_speedup'] = row['us_%s_torch_chain' % what][0] / row['us_%s_fused' % what][0]
result = {'workload': 'HmmTranscriber: nll, nll + backward, predict_midi', 'shapes': {'32x1000x128': row},
          'note': 'timings are [median, min, max] in microseconds per call, host wall clock around synchronised loops'}
if len(sys.argv) > 1:
  with open(sys.argv[1], 'w') as fh:
    fh.write(json.dumps(result, indent=1) + '\n')
print(json.dumps(result))
