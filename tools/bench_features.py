"""spectral_ops.compute_mfcc / compute_logmel at the shapes the reference's encoders use them at (batch 32 and 128 x 64 000
samples at 16 kHz; the z encoder's four frame geometries with 128 mel bins and 30 MFCCs, and the 229-bin log-mel of
gin/papers/icml2020/pretrain_model.gin), three ways:

  (a) fused     the one-kernel path (ddsp_mel_features_f32);
  (b) composed  compute_mag, then the mel-matrix product, core.safe_log and the DCT product with torch;
  (c) mag       compute_mag alone - what (a) would cost if its epilogue were free and it stored nothing.

    python tools/bench_features.py [out.json]

One session, warm clocks, host wall clock around synchronised loops.  The three paths are timed INTERLEAVED, round after
round; a figure is the median of the rounds' medians (five timed loops each), and `spread_us` is the range of (c)'s round
medians: what this session cannot tell apart."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import ddsp_amd as ddsp
from ddsp_amd import build, spectral_ops as so
build.build()
N, SR, ROUNDS = 64000, 16000, 5
SHAPES = [('mfcc_fft1024_ov75', 'mfcc', 1024, 0.75), ('mfcc_fft512_ov75', 'mfcc', 512, 0.75), ('mfcc_fft256_ov75', 'mfcc', 256, 0.75),
          ('mfcc_fft1024_ov50', 'mfcc', 1024, 0.5), ('logmel229_fft2048', 'logmel', 2048, 0.75)]


def loop_median(fn, steps, repeats=5):
  out = []
  for _ in range(repeats):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(steps): fn()
    torch.cuda.synchronize()
    out.append((time.perf_counter() - t0) / steps)
  return statistics.median(out)


def settle(fn):
  for _ in range(3): fn()
  t0 = time.perf_counter()
  while time.perf_counter() - t0 < 0.05:          # the GPU needs ~20 ms of load to reach its sustained clock
    fn()
    torch.cuda.synchronize()


def paths(kind, audio, fft_size, overlap):
  if kind == 'mfcc':
    lo, hi, bins, coeffs = 20.0, 8000.0, 128, 30
    fused = lambda: so.compute_mfcc(audio, lo, hi, fft_size, bins, coeffs, overlap)
  else:
    lo, hi, bins, coeffs = 0.0, 8000.0, 229, None
    fused = lambda: so.compute_logmel(audio, lo, hi, bins, fft_size, overlap)
  matrix = torch.as_tensor(so.linear_to_mel_weight_matrix(bins, fft_size // 2 + 1, SR, lo, hi).copy(), device=audio.device)
  dct_t = torch.as_tensor(so.mfcc_dct_matrix(bins, coeffs).T.copy(), device=audio.device) if coeffs else None

  def composed():
    logmel = ddsp.core.safe_log(torch.matmul(so.compute_mag(audio, fft_size, overlap), matrix))
    return torch.matmul(logmel, dct_t) if dct_t is not None else logmel
  return fused, composed, lambda: so.compute_mag(audio, fft_size, overlap)


result = {'workload': 'compute_mfcc (128 mel bins, 30 coefficients) / compute_logmel (229 bins): %d samples at %d Hz' % (N, SR),
          'shapes': {}}
rng = np.random.default_rng(0)
with torch.no_grad():
  for B in (32, 128):
    audio = ddsp.core.tf_float32(0.3 * rng.standard_normal((B, N)) + 0.4 * np.sin(2.0 * np.pi * 440.0 * np.arange(N) / SR)[None, :])
    for name, kind, fft_size, overlap in SHAPES:
      fused, composed, mag = paths(kind, audio, fft_size, overlap)
      diff = float((fused() - composed()).abs().max())
      rounds = {'fused': [], 'composed': [], 'mag': []}
      for fn in (fused, composed, mag): settle(fn)
      for _ in range(ROUNDS):
        for key, fn in (('fused', fused), ('composed', composed), ('mag', mag)):
          rounds[key].append(loop_median(fn, 20) * 1e6)
      row = {'us_' + k: statistics.median(v) for k, v in rounds.items()}
      row['rounds_us'] = rounds
      row['spread_us'] = max(rounds['mag']) - min(rounds['mag'])
      row['fused_no_slower_than_composed'] = row['us_fused'] <= row['us_composed']
      row['fused_minus_mag_us'] = row['us_fused'] - row['us_mag']
      row['fused_within_spread_of_mag'] = row['fused_minus_mag_us'] <= row['spread_us']
      row['max_abs_diff_fused_vs_composed'] = diff
      result['shapes']['b%d_%s' % (B, name)] = row
    del audio
    torch.cuda.empty_cache()
result['note'] = 'us_* are medians over %d interleaved rounds of the median of 5 timed loops of 20 calls' % ROUNDS
text = json.dumps(result, indent=1)
print(text)
if len(sys.argv) > 1:
  with open(sys.argv[1], 'w') as fh:
    fh.write(text + '\n')
