"""The cases of tests/test_gpu_core_rest.py and their inputs, in one place: the GPU tests, their re-run under the CPU emulation,
the host tests and tests/golden/make_golden_core_rest.py all take them from here.  numpy only.  TEST INFRASTRUCTURE."""
import functools
import zlib

import numpy as np


def _rng(tag):
  return np.random.default_rng(zlib.crc32(('core_rest/' + tag).encode()))


# ---- frequencies_critical_bands: name -> (K, depth, scale, bandwidth_scale, (batch, time)) ---------------------------
CRITICAL_BAND_CASES = {
    'k100_d1_bark': (100, 1, 'bark', 1.0, (2, 9)),               # the base case
    'k100_d4_mel': (100, 4, 'mel', 1.0, (2, 9)),                 # the mel form with a depth sum
    'k7_d64_bark_bw3': (7, 64, 'bark', 3.0, (2, 9)),             # a row of 448 floats: the tile's tails
    'k7_d65_bark': (7, 65, 'bark', 1.0, (2, 9)),                 # beyond a wavefront per sinusoid
    'k1_d3_bark': (1, 3, 'bark', 1.0, (2, 9)),                   # K = 1: a linspace of one point
    'k65_d2_mel_bw20': (65, 2, 'mel', 20.0, (2, 9)),             # drives outputs onto both limits
    'k100_d4_bark_one_row': (100, 4, 'bark', 1.0, (1, 1)),       # rows = 1
    'k33_d3_bark_rows257': (33, 3, 'bark', 1.0, (1, 257)),       # rows = 257: more than one tile, a partial last one
    'k2_d2500_mel': (2, 2500, 'mel', 1.0, (1, 3)),               # a depth the tile takes in two chunks
}
CRITICAL_BAND_GOLDEN_CASES = ['k100_d1_bark', 'k100_d4_mel', 'k7_d64_bark_bw3', 'k7_d65_bark', 'k1_d3_bark', 'k65_d2_mel_bw20']
LIMITS_CASE = 'k65_d2_mel_bw20'


@functools.lru_cache(maxsize=None)
def _critical_band_arrays(name):
  k, depth, _, bandwidth_scale, (b, t) = CRITICAL_BAND_CASES[name]
  rng = _rng('critical_bands/' + name)
  spread = 3.0 if bandwidth_scale > 3.0 else 1.5
  x = (spread * rng.standard_normal((b, t, k * depth))).astype(np.float32)
  g = rng.standard_normal((b, t, k)).astype(np.float32)
  x.setflags(write=False)
  g.setflags(write=False)
  return x, g


def critical_band_input(name):
  return _critical_band_arrays(name)[0]


def critical_band_cotangent(name):
  return _critical_band_arrays(name)[1]


DEPTH_SCALES = {'k2_d2500_mel': 1.001}      # (the default of 10 leaves nothing of the second chunk: 10^-2048 is 0)


def critical_band_kwargs(name):
  _, depth, scale, bandwidth_scale, _ = CRITICAL_BAND_CASES[name]
  return dict(depth=depth, depth_scale=DEPTH_SCALES.get(name, 10.0), bandwidth_scale=bandwidth_scale, scale=scale)


# ---- harmonic_distribution_to_wavetable: name -> (K, n_wavetable, (batch, time)) ------------------------------------
WAVETABLE_CASES = {
    'k100_w2048': (100, 2048, (2, 5)),            # G = 4 rows per block: a partial last block
    'k32_w64_nyquist': (32, 64, (2, 65)),         # K == L / 2: the half-weighted last harmonic; 130 rows, G = 128
    'k60_w512': (60, 512, (2, 5)),                # a mid-size transform
    'k5_w64_one_row': (5, 64, (1, 1)),            # a single row
    'k3_w7_odd': (3, 7, (2, 5)),                  # odd: 6 points, the general path
    'k100_w1000': (100, 1000, (2, 5)),            # not a power of two: the general path
    'k100_w8192': (100, 8192, (1, 2)),            # the largest transform
}
WAVETABLE_GOLDEN_CASES = ['k100_w2048', 'k32_w64_nyquist', 'k60_w512', 'k5_w64_one_row', 'k3_w7_odd', 'k100_w1000']


def wavetable_length(k, n_wavetable):
  return 2 * (k + int(n_wavetable / 2 - k))


@functools.lru_cache(maxsize=None)
def _wavetable_arrays(name):
  k, n_wavetable, (b, t) = WAVETABLE_CASES[name]
  rng = _rng('wavetable/' + name)
  hd = rng.uniform(0.0, 1.0, (b, t, k))
  hd = (hd / hd.sum(axis=-1, keepdims=True)).astype(np.float32)
  g = rng.standard_normal((b, t, wavetable_length(k, n_wavetable))).astype(np.float32)
  hd.setflags(write=False)
  g.setflags(write=False)
  return hd, g


def wavetable_input(name):
  return _wavetable_arrays(name)[0]


def wavetable_cotangent(name):
  return _wavetable_arrays(name)[1]


# ---- elementwise: name -> (function, kwargs, grid) -------------------------------------------------------------------
def _hz_grid():
  return np.concatenate([[0.0], np.logspace(0.0, np.log10(20000.0), 47)])


ELEMENTWISE_CASES = {
    'hz_to_bark': ('hz_to_bark', {}, _hz_grid),                                                     # the pole at 0 Hz: -0.53
    'bark_to_hz': ('bark_to_hz', {}, lambda: np.concatenate([[-0.53], np.linspace(0.0, 24.0, 47)])),   # the pole at -0.53: 0
    'hz_to_mel': ('hz_to_mel', {}, lambda: np.concatenate([[-800.0, -700.0], _hz_grid()])),         # the safe log at and below -700
    'mel_to_hz': ('mel_to_hz', {}, lambda: np.linspace(0.0, 3000.0, 48)),
    'hz_to_erb': ('hz_to_erb', {}, _hz_grid),
    'soft_limit_hz': ('soft_limit', dict(x_min=20.0, x_max=8000.0), lambda: np.concatenate([[0.0], np.linspace(-30.0, 8030.0, 63)])),
    'soft_limit_unit': ('soft_limit', {}, lambda: np.linspace(-10.0, 10.0, 41)),
    'log_scale': ('log_scale', dict(min_x=20.0, max_x=8000.0), lambda: np.linspace(-1.0, 1.0, 41)),
    'sym_exp_sigmoid': ('sym_exp_sigmoid', dict(width=8.0), lambda: np.linspace(-6.0, 6.0, 49)),
    'sym_exp_sigmoid_w3': ('sym_exp_sigmoid', dict(width=3.0), lambda: np.linspace(-6.0, 6.0, 49)),
    'nan_to_num': ('nan_to_num', dict(value=3.5), lambda: np.array([np.nan, 0.0, -1.0, np.nan, 2.5, 1e30, -0.0, np.nan])),
}


def elementwise_input(name):
  x = ELEMENTWISE_CASES[name][2]().astype(np.float32)
  x.setflags(write=False)
  return x


def elementwise_cotangent(name):
  g = _rng('elementwise/' + name).standard_normal(elementwise_input(name).shape).astype(np.float32)
  g.setflags(write=False)
  return g
