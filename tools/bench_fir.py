"""Time the differentiable FIR processors against the same functions composed from torch ops, in one session.

    python tools/bench_fir.py [--batch 32] [--n-samples 64000] [--frames 1000] [--loops 7] [--out profiles/fir_bench_mi355x.json]

Cases: effects.FIRFilter (65 bands, window 257) and core.sinc_filter (window 512), forward and forward + backward, at
B = 32, N = 64000, F = 1000 by default.  The torch side is the reference's chain as tests/fir_truth.py states it - framed
torch.fft.rfft, product, irfft, overlap-add by fold, crop - in fp32 on the device.  Each figure is the median of `loops`
synchronised loops of `inner` calls (after a warm-up), so launch gaps count as they would in training."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ddsp_amd import core, effects  # noqa: E402


def torch_fft_convolve(audio, ir, delay_compensation=-1):
  b, n = audio.shape
  f, l = ir.shape[1], ir.shape[2]
  frame = -(-n // f)
  fft_size = int(2 ** np.ceil(np.log2(frame + l - 1)))
  frames = torch.nn.functional.pad(audio, (0, f * frame - n)).reshape(b, f, frame)
  out_frames = torch.fft.irfft(torch.fft.rfft(frames, fft_size) * torch.fft.rfft(ir, fft_size), fft_size)
  total = (f - 1) * frame + fft_size
  out = torch.nn.functional.fold(out_frames.transpose(1, 2), (1, total), (1, fft_size), stride=(1, frame))[:, 0, 0]
  start = (l - 1) // 2 - 1 if delay_compensation < 0 else delay_compensation
  return out[:, start:start + n]


def torch_fir_filter(audio, mags, window_size=257):
  m = 2.0 * torch.sigmoid(mags) ** math.log(10.0) + 1e-7
  ir = torch.fft.irfft(torch.complex(m, torch.zeros_like(m)))
  size = ir.shape[-1]
  ws = size if window_size <= 0 or window_size > size else window_size
  assert ws == size, 'the bench uses the full window'
  window = torch.fft.fftshift(torch.hann_window(ws, periodic=True, device=audio.device))
  return torch_fft_convolve(audio, torch.fft.fftshift(window * ir, dim=-1))


def torch_sinc_filter(audio, cutoff, window_size=512):
  half = window_size // 2
  size = 2 * half + 1
  idx = torch.arange(-half, half + 1, dtype=torch.float32, device=audio.device)[None, None, :]
  x = cutoff * idx
  x = math.pi * torch.where(x.abs() < 1e-20, torch.full_like(x, 1e-20), x)
  window = 0.54 - 0.46 * torch.cos(2.0 * math.pi * torch.arange(size, dtype=torch.float32, device=audio.device) / (size - 1))
  ir = window * torch.sin(x) / x
  return torch_fft_convolve(audio, ir / ir.sum(-1, keepdim=True).abs())


def timed(fn, loops, inner):
  for _ in range(2):
    fn()
  torch.cuda.synchronize()
  samples = []
  for _ in range(loops):
    t0 = time.perf_counter()
    for _ in range(inner):
      fn()
    torch.cuda.synchronize()
    samples.append((time.perf_counter() - t0) / inner * 1e3)
  return {'median_ms': statistics.median(samples), 'min_ms': min(samples), 'max_ms': max(samples)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=32)
  ap.add_argument('--n-samples', type=int, default=64000)
  ap.add_argument('--frames', type=int, default=1000)
  ap.add_argument('--loops', type=int, default=7)
  ap.add_argument('--inner', type=int, default=5)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  b, n, f = args.batch, args.n_samples, args.frames
  dev = torch.device('cuda')
  gen = torch.Generator(device='cpu').manual_seed(0)
  audio = (torch.rand(b, n, generator=gen) * 2.0 - 1.0).to(dev)
  mags = torch.randn(b, f, 65, generator=gen).to(dev)
  cutoff = (torch.rand(b, f, 1, generator=gen) * 0.9 + 0.05).to(dev)
  cot = torch.randn(b, n, generator=gen).to(dev)
  fir = effects.FIRFilter(window_size=257)

  def fwd_bwd(fn, *inputs):
    xs = [x.detach().requires_grad_(True) for x in inputs]
    torch.autograd.grad(fn(*xs), xs, cot)

  cases = {
      'fir_filter': (lambda a, m: fir(a, m), torch_fir_filter, (audio, mags)),
      'sinc_filter': (lambda a, c: core.sinc_filter(a, c, window_size=512), torch_sinc_filter, (audio, cutoff)),
  }
  result = {'device': torch.cuda.get_device_name(0), 'batch': b, 'n_samples': n, 'frames': f, 'loops': args.loops,
            'inner_calls_per_loop': args.inner, 'cases': {}}
  for name, (ours, theirs, inputs) in cases.items():
    with torch.no_grad():
      diff = float((ours(*inputs) - theirs(*inputs)).abs().max())
    entry = {'max_abs_diff_forward': diff}
    for side, fn in (('hip', ours), ('torch', theirs)):
      with torch.no_grad():
        entry[side + '_forward'] = timed(lambda: fn(*inputs), args.loops, args.inner)
      entry[side + '_forward_backward'] = timed(lambda: fwd_bwd(fn, *inputs), args.loops, args.inner)
    for what in ('forward', 'forward_backward'):
      entry['torch_over_hip_' + what] = entry['torch_' + what]['median_ms'] / entry['hip_' + what]['median_ms']
    result['cases'][name] = entry
  line = json.dumps(result)
  print(line)
  if args.out:
    with open(args.out, 'w') as fh:
      fh.write(json.dumps(result, indent=1) + '\n')


if __name__ == '__main__':
  main()
