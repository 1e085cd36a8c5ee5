"""synths.Wavetable, effects.ModDelay, core.linear_lookup / wavetable_synthesis / variable_length_delay on the MI355X,
forward and backward, against the fp64 truth of tests/wavetable_truth.py, the reference's fp32 chain (tests/golden/
wavetable_*.npz, written by tests/golden/make_golden_wavetable.py) and the reference's own unit tests, re-expressed
(ddsp/core_test.py:592-718, synths_test.py:53-70, effects_test.py:107-117).

Tolerances.  ULP = 2^-23.
  * lookups with a supplied phase, truth evaluated at the fp32 phase values: C_LOOKUP ULP max|table|.  The kernel's
    position split is exact up to one rounding of the fraction (<= 1 ULP of a table step, slope <= 2 max|table|) and the
    lerp rounds three times at the scale of max|table|: about 5 ULP max|table| in the worst case; the MI355X measures 1.1
    (profiles/wavetable_parity_errors.jsonl).
  * synthesis: a_max (C_SYNTH ULP max|w| + W max|dw| DPHI).  DPHI is the phase accuracy in cycles: the kernels carry the
    phase in fp64 up to the table position (up to 2^15 cycles in a 4 s clip at Nyquist: 2^-37 per rounding, a handful
    of roundings), so DPHI = 2^-35; the fraction's one fp32 rounding is inside C_SYNTH.  A phase in fp32 would need
    DPHI = 2^-23 and lose 2e-4 on white 1024-point tables.
  * gradients: relative to the largest reference gradient, C_GRAD = 2e-4 (the MI355X measures
    3.8e-5 at worst, ModDelay's gain), at any scale of the incoming gradient.
tests/test_wavetable_emulated.py runs the small cases of this file on the CPU emulation of the kernels."""
import numpy as np
import pytest
import torch

import wavetable_truth as T
from conftest import load_golden, parity_check

pytestmark = pytest.mark.gpu

DEV = 'cuda'
ULP = 2.0 ** -23
C_LOOKUP = 6.0          # measured 0.9 - 1.1 (linear_lookup, variable_length_delay)
C_SYNTH = 8.0           # measured 1.5: the frame blend and the envelope product round three times more
DPHI = 2.0 ** -35
C_GRAD = 2e-4


@pytest.fixture(scope='module')
def ddsp():
  if DEV == 'cuda':
    if not torch.cuda.is_available():
      pytest.skip('gpu tests need a GPU (run with -m gpu on an MI355X)')
    from ddsp_amd import build
    build.build()
  import ddsp_amd
  return ddsp_amd


def dev(x, grad=False):
  t = torch.as_tensor(np.asarray(x, np.float32), device=DEV)
  return t.requires_grad_(True) if grad else t


def npy(t):
  return t.detach().cpu().numpy()


def synth_tol(amps, tables, scale=False):
  a = T.exp_sigmoid(amps) if scale else np.asarray(amps, np.float64)
  w = T.exp_sigmoid(tables) if scale else np.asarray(tables, np.float64)
  W = w.shape[-1]
  dw = np.abs(np.diff(np.concatenate([w, w[..., :1]], -1), axis=-1)).max()
  return float(np.abs(a).max() * (C_SYNTH * ULP * np.abs(w).max() + W * dw * DPHI))


# ---- 1. lookups with a supplied phase ---------------------------------------------------------------------------------
def lookup_phases(rng, B, N):
  phase = rng.uniform(-0.01, 1.01, (B, N)).astype(np.float32)
  phase[:, :8] = np.array([0.0, 1.0, -1e-4, 1.0 + 1e-4, -0.5, 1.5, 0.5, np.float32(1.0) - np.float32(2.0 ** -24)], np.float32)
  return phase


@pytest.mark.parametrize('W', [64, 1000, 2048])
@pytest.mark.parametrize('audio_rate', [False, True])
def test_linear_lookup_vs_truth_at_fp32_phases(ddsp, W, audio_rate):
  rng = np.random.default_rng(W + audio_rate)
  B, N = 2, 3000
  phase = lookup_phases(rng, B, N)
  tables = rng.uniform(-1, 1, (B, N, W) if audio_rate else (B, W)).astype(np.float32)
  out = npy(ddsp.core.linear_lookup(dev(phase)[:, :, None], dev(tables)))
  truth = T.linear_lookup(phase, tables)
  assert out.shape == (B, N)
  assert np.all(out[:, 4:6] == 0.0)                                    # beyond one table step outside [0, 1]: exactly 0
  np.testing.assert_array_equal(out[:, 1], tables[:, 1, 0] if audio_rate else tables[:, 0])      # phase 1.0 reads w[0]
  parity_check(out, truth, C_LOOKUP * ULP * np.abs(tables).max(), 'linear_lookup W=%d' % W)


@pytest.mark.parametrize('L', [10, 400, 1000])
def test_variable_length_delay_vs_truth_at_fp32_phases(ddsp, L):
  rng = np.random.default_rng(L)
  B, N = 2, 4000
  phase = lookup_phases(rng, B, N)
  audio = rng.uniform(-1, 1, (B, N)).astype(np.float32)
  out = npy(ddsp.core.variable_length_delay(dev(phase)[:, :, None], dev(audio), L))
  truth = T.variable_length_delay(phase, audio, L)
  np.testing.assert_array_equal(out[:, 1], audio[:, 1])               # full phase reads the undelayed sample (the wrap point)
  parity_check(out, truth, C_LOOKUP * ULP * np.abs(audio).max(), 'variable_length_delay L=%d' % L)


# ---- 2. synthesis against fp64 truth -----------------------------------------------------------------------------------
SYNTH_CASES = {
    # name: (B, F, W, N, Fw, rough)
    'class_default_smooth': (3, 1000, 1024, 64000, None, False),
    'class_default_rough': (3, 1000, 1024, 64000, None, True),
    'w64_rough': (2, 250, 64, 16000, None, True),
    'w2048_smooth': (2, 250, 2048, 16000, None, False),
    'w2048_rough': (2, 250, 2048, 16000, None, True),
    'hop192_rough': (2, 125, 256, 24000, None, True),
    'hop192_smooth_w2048': (2, 125, 2048, 24000, None, False),
    'small_fused': (2, 25, 256, 1600, None, True),
    'small_w_not_multiple_of_4': (2, 25, 250, 1600, None, True),
    'table_frames_200_vs_100': (2, 100, 128, 1600, 200, True),
    'table_frames_not_dividing': (2, 25, 128, 1600, 7, True),
    'static_table': (2, 25, 512, 1600, 1, True),
    'audio_rate_tables': (1, 25, 64, 400, 400, True),
}


@pytest.mark.parametrize('case', sorted(SYNTH_CASES))
def test_wavetable_synthesis_vs_truth(ddsp, case):
  B, F, W, N, Fw, rough = SYNTH_CASES[case]
  amps, tables, f0 = T.synthesis_inputs(len(case) * 7 + W, B, F, W, Fw, rough)
  out = npy(ddsp.core.wavetable_synthesis(dev(f0), dev(amps), dev(tables[:, 0] if Fw == 1 else tables), N, 16000))
  truth = T.wavetable_synthesis(f0, amps, tables, N, 16000)
  assert out.shape == (B, N)
  parity_check(out, truth, synth_tol(amps, tables), 'wavetable_synthesis ' + case)


@pytest.mark.parametrize('case', ['class_default_rough', 'small_fused', 'hop192_rough'])
def test_wavetable_class_vs_truth_through_scale_fn(ddsp, case):
  B, F, W, N, _, _ = SYNTH_CASES[case]
  rng = np.random.default_rng(F + W)
  amps = rng.standard_normal((B, F, 1)).astype(np.float32)
  tables = rng.standard_normal((B, F, W)).astype(np.float32)
  f0 = T.synthesis_inputs(3, B, F, W)[2]
  synth = ddsp.synths.Wavetable(n_samples=N, sample_rate=16000)
  out = npy(synth(dev(amps), dev(tables), dev(f0)))
  truth = T.wavetable_synthesis(f0, amps, tables, N, 16000, scale=True)
  # exp_sigmoid on the hardware exp / log: relative error ~1e-6 of a value <= 2, on amplitudes and tables alike
  parity_check(out, truth, synth_tol(amps, tables, scale=True) + 2.0 * 2.0 * 4e-6, 'Wavetable() ' + case)
  two_steps = synth.get_signal(**synth.get_controls(dev(amps), dev(tables), dev(f0)))
  parity_check(npy(two_steps), truth, synth_tol(amps, tables, scale=True) + 2.0 * 2.0 * 4e-6, 'Wavetable get_signal ' + case)


def test_negative_frequency_and_phase_start(ddsp):
  B, F, W, N = 1, 10, 64, 640
  amps, tables, f0 = T.synthesis_inputs(5, B, F, W, rough=True)
  f0 = -f0
  out = npy(ddsp.core.wavetable_synthesis(dev(f0), dev(amps), dev(tables), N, 16000))
  parity_check(out, T.wavetable_synthesis(f0, amps, tables, N, 16000), synth_tol(amps, tables), 'negative f0')
  assert out[0, 0] == np.float32(amps[0, 0, 0]) * tables[0, 0, 0]       # exclusive cumsum: phase(0) = 0 reads w[0]


# ---- 3. the reference's fp32 chain (goldens; smooth tables, short clips) ----------------------------------------------
GOLDENS = ['wavetable_class_f25_w2048', 'wavetable_class_scaled_f25_w256', 'wavetable_synthesis_static_w1024',
           'wavetable_synthesis_frames50_vs_25']


@pytest.mark.parametrize('name', GOLDENS)
def test_wavetable_vs_reference_goldens(ddsp, name):
  g = load_golden(name)
  n, sr = int(g['n_samples']), int(g['sample_rate'])
  if 'class' in name:
    synth = ddsp.synths.Wavetable(n_samples=n, sample_rate=sr, scale_fn=ddsp.core.exp_sigmoid if int(g['scaled']) else None)
    out = synth(dev(g['amplitudes']), dev(g['wavetables']), dev(g['f0_hz']))
  else:
    out = ddsp.core.wavetable_synthesis(dev(g['f0_hz']), dev(g['amplitudes']), dev(g['wavetables']), n, sr)
  parity_check(npy(out), g['audio'], 2e-3, name)


@pytest.mark.parametrize('name', ['variable_length_delay_l400', 'mod_delay_default', 'mod_delay_no_dry_no_scale'])
def test_delay_vs_reference_goldens(ddsp, name):
  g = load_golden(name)
  if name.startswith('variable'):
    out = ddsp.core.variable_length_delay(dev(g['phase']), dev(g['audio']), int(g['max_length']))
  else:
    kw = {} if int(g['scaled']) else dict(gain_scale_fn=None, phase_scale_fn=None)
    fx = ddsp.effects.ModDelay(add_dry=bool(int(g['add_dry'])), **kw)
    out = fx(dev(g['audio']), dev(g['gain']), dev(g['phase']))
  # the reference's weights are 1 - |phase - i / L| L in fp32: |phase - i / L| carries half an ULP of the phase, times L
  tol = (int(g['max_length']) * ULP + C_LOOKUP * ULP) * 2.0 * np.abs(g['audio']).max() * max(1.0, np.abs(g['gain_max']))
  parity_check(npy(out), g['out'], tol + 2.0 * 4e-6 * np.abs(g['audio']).max() * int(g['scaled']), name)


# ---- 4. the reference's unit tests -------------------------------------------------------------------------------------
@pytest.mark.parametrize('batch_size,n_wavetable,n_frames,n_samples,n_cycles', [
    (1, 2048, 0, 10000, 1000), (2, 1024, 0, 20000, 10), (1, 2048, 1, 10000, 1000), (1, 2048, 10000, 10000, 1000)],
    ids=['high_frequency_wave', 'low_frequency_wave', 'one_frame', 'many_frames'])
def test_core_linear_lookup_is_accurate(ddsp, batch_size, n_wavetable, n_frames, n_samples, n_cycles):   # core_test.py:594-629
  two_pi = 2.0 * np.pi
  wavetable = np.sin(np.linspace(0, two_pi, n_wavetable).astype(np.float32))
  wavetable = np.tile(wavetable[np.newaxis, :], [batch_size, 1])
  if n_frames > 0:
    wavetable = np.tile(wavetable[:, np.newaxis, :], [1, n_frames, 1])
  phase = np.linspace(0, n_cycles, n_samples).astype(np.float32) % 1.0
  phase = np.tile(phase[np.newaxis, :, np.newaxis], [batch_size, 1, 1])
  wav_np = np.sin(two_pi * phase)[:, :, 0]
  wav = npy(ddsp.core.linear_lookup(dev(phase), dev(wavetable)))
  assert np.abs(wav_np - wav).mean() <= 2e-3


@pytest.mark.parametrize('batch_size,frequency,amplitude,n_wavetable,wavetable_frames', [
    (1, 440.0, 0.5, 2048, 0), (2, 1000.0, 0.1, 1024, 1), (2, 1000.0, 0.1, 1024, 200)],
    ids=['single_wavetable_no_frames', 'one_frame', 'many_frames'])
def test_core_wavetable_synth_is_accurate(ddsp, batch_size, frequency, amplitude, n_wavetable, wavetable_frames):
  sample_rate, seconds, n_frames = 16000, 0.1, 100                                               # core_test.py:631-674
  n_samples = int(sample_rate * seconds)
  n_cycles = seconds * frequency
  two_pi = 2.0 * np.pi
  wavetable = np.sin(np.linspace(0, two_pi, n_wavetable).astype(np.float32))
  wavetable = np.tile(wavetable[np.newaxis, :], [batch_size, 1])
  if wavetable_frames > 0:
    wavetable = np.tile(wavetable[:, np.newaxis, :], [1, wavetable_frames, 1])
  wav_np = amplitude * np.sin(two_pi * np.linspace(0, n_cycles, n_samples))
  wav_np = np.tile(wav_np[np.newaxis, :], [batch_size, 1]).astype(np.float32)
  amplitudes = np.ones([batch_size, n_frames, 1]) * amplitude
  frequencies = np.ones([batch_size, n_frames, 1]) * frequency
  wav = npy(ddsp.core.wavetable_synthesis(dev(frequencies), dev(amplitudes), dev(wavetable), n_samples, sample_rate))
  pad = n_samples // n_frames
  assert np.abs(wav_np[:, pad:-pad] - wav[:, pad:-pad]).mean() <= 3e-2


@pytest.mark.parametrize('batch_size,n_samples,max_length', [(1, 16000, 10), (2, 4000, 1000)], ids=['short_delay', 'long_delay'])
def test_core_variable_length_delay_is_accurate(ddsp, batch_size, n_samples, max_length):       # core_test.py:676-718
  n_cycles = float(n_samples) / max_length
  wav_np = np.sin(np.linspace(0, 2.0 * np.pi * n_cycles, n_samples))
  wav_np = np.tile(wav_np[np.newaxis, :], [batch_size, 1]).astype(np.float32)
  ones = np.ones_like(wav_np)[..., np.newaxis]
  for target, ph in [(wav_np, 0.0), (-wav_np, 0.5), (wav_np, 1.0)]:
    source = npy(ddsp.core.variable_length_delay(dev(ph * ones), dev(wav_np), max_length))
    assert np.abs(target[:, max_length:] - source[:, max_length:]).mean() <= 1e-2


def test_synths_wavetable_output_shape(ddsp):                                                    # synths_test.py:53-70
  synth = ddsp.synths.Wavetable(n_samples=64000, sample_rate=16000, scale_fn=None)
  amp = torch.zeros((3, 1000, 1), device=DEV) + 1.0
  wavetables = torch.zeros((3, 1000, 1024), device=DEV)
  f0_hz = torch.zeros((3, 1000, 1), device=DEV) + 440
  assert list(synth(amp, wavetables, f0_hz).shape) == [3, 64000]


def test_effects_mod_delay_output_shape(ddsp):                                                   # effects_test.py:107-117
  fx = ddsp.effects.ModDelay()
  out = fx(torch.zeros((3, 16000), device=DEV), torch.zeros((3, 16000, 1), device=DEV), torch.zeros((3, 16000, 1), device=DEV))
  assert list(out.shape) == [3, 16000]


# ---- 5. gradients ------------------------------------------------------------------------------------------------------
def grad_check(ours, ref, what):
  ref = np.asarray(ref, np.float64)
  parity_check(npy(ours).reshape(ref.shape), ref, C_GRAD * np.abs(ref).max(), what)


GRAD_CASES = {
    'fused_hop64': (2, 25, 256, 1600, None, False),
    'fused_scaled': (2, 25, 256, 1600, None, True),
    'fused_hop192_w2048': (1, 10, 2048, 1920, None, False),
    'table_frames_50_vs_25': (2, 25, 128, 1600, 50, False),
    'table_frames_not_dividing': (2, 25, 128, 1600, 7, False),
    'static_table': (2, 25, 128, 1600, 1, False),
    'audio_rate_tables': (1, 20, 32, 320, 320, False),
    'class_default': (3, 1000, 1024, 64000, None, True),
}


# every case at incoming-gradient scales 1e-6, 1 and 1e+6; the full-size one at 1
@pytest.mark.parametrize('case,gscale', [(c, g) for c in sorted(GRAD_CASES) for g in (1e-6, 1.0, 1e6)
                                         if c != 'class_default' or g == 1.0])
def test_wavetable_gradients_vs_truth(ddsp, case, gscale):
  B, F, W, N, Fw, scaled = GRAD_CASES[case]
  rng = np.random.default_rng(F + W + (Fw or 0))
  amps, tables, f0 = T.synthesis_inputs(11, B, F, W, Fw, rough=False, f_hi=2000.0)
  if scaled:
    amps = rng.standard_normal(amps.shape).astype(np.float32)
    tables = (4.0 * tables).astype(np.float32)
  gout = (gscale * rng.standard_normal((B, N))).astype(np.float32)
  ta, tw, tf = dev(amps, True), dev(tables[:, 0] if Fw == 1 else tables, True), dev(f0, True)
  if scaled:
    out = ddsp.synths.Wavetable(n_samples=N, sample_rate=16000)(ta, tw, tf)
  else:
    out = ddsp.core.wavetable_synthesis(tf, ta, tw, N, 16000)
  out.backward(dev(gout))
  _, g_amp, g_tab, g_f0 = T.wavetable_synthesis(f0, amps, tables, N, 16000, grad_out=gout, scale=scaled)
  grad_check(ta.grad, g_amp, 'd amplitudes %s x%g' % (case, gscale))
  grad_check(tw.grad, g_tab, 'd wavetables %s x%g' % (case, gscale))
  grad_check(tf.grad, g_f0, 'd f0_hz %s x%g' % (case, gscale))


@pytest.mark.parametrize('gscale', [1e-6, 1.0, 1e6])
@pytest.mark.parametrize('audio_rate', [False, True])
def test_linear_lookup_gradients_vs_truth(ddsp, audio_rate, gscale):
  rng = np.random.default_rng(17 + audio_rate)
  B, N, W = 2, 700, 100
  phase = lookup_phases(rng, B, N)
  tables = rng.uniform(-1, 1, (B, N, W) if audio_rate else (B, W)).astype(np.float32)
  gout = (gscale * rng.standard_normal((B, N))).astype(np.float32)
  tp, tw = dev(phase[:, :, None], True), dev(tables, True)
  ddsp.core.linear_lookup(tp, tw).backward(dev(gout))
  _, g_phase, g_tab = T.linear_lookup(phase, tables, gout)
  grad_check(tp.grad, g_phase, 'lookup d phase x%g' % gscale)
  grad_check(tw.grad, g_tab, 'lookup d wavetables x%g' % gscale)


@pytest.mark.parametrize('gscale', [1e-6, 1.0, 1e6])
@pytest.mark.parametrize('add_dry', [False, True])
@pytest.mark.parametrize('scaled', [False, True])
def test_mod_delay_gradients_vs_truth(ddsp, scaled, add_dry, gscale):
  rng = np.random.default_rng(23 + scaled + 2 * add_dry)
  B, N = 2, 2400
  audio = rng.uniform(-1, 1, (B, N)).astype(np.float32)
  gain = rng.standard_normal((B, N, 1)).astype(np.float32)
  phase = (rng.standard_normal((B, N, 1)) if scaled else rng.uniform(-1, 1, (B, N, 1))).astype(np.float32)
  gout = (gscale * rng.standard_normal((B, N))).astype(np.float32)
  kw = {} if scaled else dict(gain_scale_fn=None, phase_scale_fn=None)
  fx = ddsp.effects.ModDelay(add_dry=add_dry, **kw)
  tx, tg, tp = dev(audio, True), dev(gain, True), dev(phase, True)
  out = fx(tx, tg, tp)
  out.backward(dev(gout))
  ref, g_audio, g_gain, g_phase = T.mod_delay(audio, gain[..., 0], phase[..., 0], add_dry=add_dry, scale=scaled, grad_out=gout)
  # the mapped phase is rounded to fp32 before the lookup, as the reference rounds it: 1 ULP of phase is L ULP of a tap step
  parity_check(npy(out), ref, (400 + C_LOOKUP) * ULP * 2.0 * 2.0 + 2e-5, 'ModDelay forward scaled=%d' % scaled)
  grad_check(tx.grad, g_audio, 'ModDelay d audio x%g' % gscale)
  grad_check(tg.grad, g_gain, 'ModDelay d gain x%g' % gscale)
  grad_check(tp.grad, g_phase, 'ModDelay d phase x%g' % gscale)


def test_variable_length_delay_gradients_vs_truth(ddsp):
  rng = np.random.default_rng(29)
  B, N, L = 2, 1500, 1000
  phase, audio = lookup_phases(rng, B, N), rng.uniform(-1, 1, (B, N)).astype(np.float32)
  gout = rng.standard_normal((B, N)).astype(np.float32)
  tp, tx = dev(phase, True), dev(audio, True)
  ddsp.core.variable_length_delay(tp, tx, L).backward(dev(gout))
  _, g_phase, g_audio, _ = T.variable_length_delay(phase, audio, L, grad_out=gout)
  grad_check(tp.grad, g_phase, 'delay d phase')
  grad_check(tx.grad, g_audio, 'delay d audio')


# ---- 6. determinism ----------------------------------------------------------------------------------------------------
def _wavetable_all(ddsp, amps, tables, f0, gout, N, scaled):
  ta, tw, tf = dev(amps, True), dev(tables, True), dev(f0, True)
  synth = ddsp.synths.Wavetable(n_samples=N, sample_rate=16000, scale_fn=ddsp.core.exp_sigmoid if scaled else None)
  out = synth(ta, tw, tf)
  out.backward(dev(gout))
  return [npy(out), npy(ta.grad), npy(tw.grad), npy(tf.grad)]


def _mod_delay_all(ddsp, audio, gain, phase, gout):
  tx, tg, tp = dev(audio, True), dev(gain, True), dev(phase, True)
  out = ddsp.effects.ModDelay()(tx, tg, tp)
  out.backward(dev(gout))
  return [npy(out), npy(tx.grad), npy(tg.grad), npy(tp.grad)]


def _assert_rows_bit_identical(run, arrays, B):
  full, again = run(*arrays), run(*arrays)
  for a, b in zip(full, again):
    np.testing.assert_array_equal(a, b)
  for rows in (slice(B - 1, B), slice(1, 3)):
    part = run(*[x[rows] for x in arrays])
    for a, b in zip(full, part):
      np.testing.assert_array_equal(a[rows], b)


@pytest.mark.parametrize('shape', [(4, 50, 512, 3200, None), (4, 25, 128, 1600, 1), (4, 25, 128, 1600, 7)],
                         ids=['fused', 'static', 'table_frames_7'])
def test_wavetable_forward_and_backward_bit_identical(ddsp, shape):
  B, F, W, N, Fw = shape
  amps, tables, f0 = T.synthesis_inputs(31, B, F, W, Fw, rough=True)
  gout = np.random.default_rng(1).standard_normal((B, N)).astype(np.float32)
  _assert_rows_bit_identical(lambda a, w, f, g: _wavetable_all(ddsp, a, w, f, g, N, Fw is None), [amps, tables, f0, gout], B)


def test_mod_delay_forward_and_backward_bit_identical(ddsp):
  rng = np.random.default_rng(37)
  B, N = 4, 4000
  arrays = [rng.uniform(-1, 1, (B, N)).astype(np.float32), rng.standard_normal((B, N, 1)).astype(np.float32),
            rng.standard_normal((B, N, 1)).astype(np.float32), rng.standard_normal((B, N)).astype(np.float32)]
  _assert_rows_bit_identical(lambda *a: _mod_delay_all(ddsp, *a), arrays, B)


def test_linear_lookup_backward_bit_identical(ddsp):
  rng = np.random.default_rng(41)
  B, N, W = 4, 5000, 64
  phase, tables = lookup_phases(rng, B, N), rng.uniform(-1, 1, (B, W)).astype(np.float32)
  gout = rng.standard_normal((B, N)).astype(np.float32)

  def run(p, w, g):
    tp, tw = dev(p, True), dev(w, True)
    out = ddsp.core.linear_lookup(tp, tw)
    out.backward(dev(g))
    return [npy(out), npy(tp.grad), npy(tw.grad)]
  _assert_rows_bit_identical(run, [phase, tables, gout], B)


# ---- 7. no materialisation ---------------------------------------------------------------------------------------------
def test_wavetable_never_materialises_audio_rate_tables(ddsp):
  if DEV != 'cuda':
    pytest.skip('measures the caching allocator of the GPU')
  from ddsp_amd import _lib
  B, F, W, N = 8, 1000, 2048, 64000
  amps, tables, f0 = T.synthesis_inputs(43, B, F, W, rough=True)
  ta, tw, tf = dev(amps, True), dev(tables, True), dev(f0, True)
  gout = dev(np.ones((B, N), np.float32))
  synth = ddsp.synths.Wavetable(n_samples=N, sample_rate=16000)
  inputs = 4 * (B * F * (W + 2))
  ws = _lib.load().ddsp_wavetable_backward_workspace_bytes(B, F, F, W, N)
  torch.cuda.synchronize()
  base = torch.cuda.memory_allocated()
  torch.cuda.reset_peak_memory_stats()
  with torch.no_grad():
    out = synth(ta, tw, tf)
  torch.cuda.synchronize()
  fwd_peak = torch.cuda.max_memory_allocated() - base
  assert fwd_peak <= 4 * B * N + (1 << 20), fwd_peak                    # the output and nothing else
  del out
  torch.cuda.reset_peak_memory_stats()
  synth(ta, tw, tf).backward(gout)
  torch.cuda.synchronize()
  peak = torch.cuda.max_memory_allocated() - base
  # output + the three gradients + the backward workspace (its own query) + allocator rounding; [B, N, W] would be 4.2 GB
  assert peak <= 4 * B * N + inputs + ws + (8 << 20), (peak, inputs, ws)
