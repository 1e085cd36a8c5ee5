"""The backward passes of Harmonic, FilteredNoise, Wavetable / ModDelay, Reverb (and FIRFilter, SpectralLoss, ProcessorGroup
where named) as TRAINING uses them: several graphs alive on one Processor instance, gradients accumulating, rows re-batched, two
streams on one instance, inputs or attributes changed between forward and backward().  The host layer keeps state across calls -
core.Workspace (grow-only scratch per instance and stream), FilteredNoise's call counter packed into ctx.seed, what the autograd
nodes keep on ctx, the g_sched sets of csrc/harmonic.hip - and every other test runs one fresh instance, one forward, one
backward().  tests/test_backward_state_emulated.py runs this module through the SIMT emulation on the CPU (not the stream cases).

Oracles and tolerances are the existing tests', none is new:
  * Harmonic dL/d amplitudes, dL/d harmonic_distribution: oracle.harmonic_backward, grad_tol = 1e-6 + 2e-4 max|ref|
    (tests/test_gpu_parity.py:1258, imported).
  * dL/d f0_hz: oracle.harmonic_backward(with_f0=True); on the closed-form kernels all three gradients at 2e-4 max|ref|
    (tests/test_gpu_parity_general.py:280-282), through the chain of materialised envelopes dL/d f0_hz at 1e-6 + 5e-4 max|ref|
    (tests/test_gpu_parity_general.py:219).
  * FilteredNoise: oracle.filtered_noise_backward at 1e-6 + 2e-5 max|ref|, the audio against oracle.filtered_noise in fp64 at
    2e-6 + 1e-5 (tests/test_gpu_parity.py:1514-1516).  Generated noise is oracle.device_uniform_noise(b, n, seed | call << 32): the
    call counter is the high word of the 64-bit Philox key (synths.FilteredNoise._next_seed), the row is a word of the counter.
  * Reverb: oracle.reverb_backward, reverb_tol = 1e-6 + 1e-5 max|ref| (tests/test_gpu_parity.py:768, :1590-1592, imported).
  * Wavetable / ModDelay: tests/wavetable_truth.py, C_GRAD = 2e-4 of the largest reference gradient (tests/test_gpu_wavetable.py:32, :246).
  * SpectralLoss: oracle.spectral_loss_backward, 1e-9 + 2e-4 max|ref| for all but 0.1 % of the samples and ten times that for every
    sample (tests/test_gpu_parity.py:1734-1736).
Every comparison is appended to the file DDSP_PARITY_LOG names, when it is set.  Measured on the MI355X
(profiles/backward_state_parity.jsonl): no bit comparison differs in any element; the largest error against an oracle is 0.17 of
its tolerance (Reverb, dL/d ir of a row alone).

Bit equalities that are NOT demanded, each with its cause (DESIGN.md section 2 item 4 and section 8 list them):
  * Reverb rows across transform pairs: two batch rows share one complex transform (rows 2 p and 2 p + 1), so a row's last bits
    depend on its partner.  Demanded: the same bits twice and for the pair-preserving sub-batch [:2]; row 1 alone (then paired
    with nothing) is held to the analytic oracle.
  * The SpectralLoss gradient overlap-adds with fp32 atomics: last bits not reproducible run to run; held to its oracle.
  * Generated noise: the batch row is a word of the Philox counter, counted from 0 in every call, so a sub-batch that does not
    start at row 0 draws other noise.  Rows [0:1] and [0:2] are compared."""
import functools
import json
import os
import zlib

import numpy as np
import pytest
import torch

import wavetable_truth as WT
from oracle import ddsp_oracle as O
from test_gpu_parity import grad_tol, reverb_tol
from test_gpu_wavetable import C_GRAD

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SEED = 11


def _log(case, **figures):
  path = os.environ.get('DDSP_PARITY_LOG')
  if path:
    with open(path, 'a') as f:
      f.write(json.dumps(dict(case=case, **{k: float(v) for k, v in figures.items()})) + '\n')


def _t(x, grad=False):
  """A tensor of its own on DEV (a copy also on the CPU: the cases are shared and part 3 writes into its tensors in place)."""
  return torch.tensor(np.asarray(x, dtype=np.float32), device=DEV).requires_grad_(grad)


def _np(x):
  return x.detach().cpu().numpy().astype(np.float64)


def _close(case, got, ref, atol):
  """max |got - ref| <= atol, logged."""
  got, ref = _np(got).reshape(np.shape(ref)), np.asarray(ref, np.float64)
  err = float(np.abs(got - ref).max())
  _log(case, err=err, atol=atol, frac_of_tol=err / atol)
  assert np.isfinite(got).all() and err <= atol, (case, err, atol)


def _same_bits(case, got, ref):
  """torch.equal, with the number of differing elements logged."""
  assert got.shape == ref.shape, (case, tuple(got.shape), tuple(ref.shape))
  differing = int((got != ref).sum())
  _log(case, differing=differing, size=got.numel())
  assert torch.equal(got, ref), (case, differing, got.numel())


def _rows_twice_and_sub_batches(name, run, tols, refs, sub_batches):
  """`run(rows)` -> the gradients of the rows `rows` of the batch of 3.  The full batch against the oracle; then every
  sub-batch and the full batch again, bit for bit."""
  everything = slice(0, 3)
  full = run(everything)
  for i, (g, ref, tol) in enumerate(zip(full, refs, tols)):
    _close('%s/oracle/grad%d' % (name, i), g, ref, tol(ref))
  for rows in list(sub_batches) + [everything]:
    for i, (g, part) in enumerate(zip(full, run(rows))):
      _same_bits('%s/rows%d_%d/grad%d' % (name, rows.start, rows.stop, i), part, g[rows])
  return full


ROW_ALONE_AND_PAIR = (slice(1, 2), slice(1, 3))


# ---- the cases: inputs and oracle gradients, computed once and never changed ------------------------------------------------
# name: (n_frames, k, n_samples, sample_rate, amp_resample_method, f0 range)
HARMONIC = {
    'f25_k12_nyquist': (25, 12, 25 * 64, 16000, 'window', (300.0, 900.0)),     # frame groups of 8 straddle rows; harmonics cross Nyquist mid-frame
    'f20_k100': (20, 100, 20 * 64, 16000, 'window', (69.0, 71.0)),             # the shipped regime
    'f9_k200_linear': (9, 200, 9 * 100, 16000, 'linear', (30.0, 45.0)),        # 129 .. 200 harmonics, the plain sum inside the kernel
    'f12_k260': (12, 260, 12 * 64, 16000, 'window', (26.0, 34.0)),             # more than 256 harmonics: the chain's adjoint; 260 f0 crosses Nyquist at 30.8 Hz
    'f10_k8_cubic_ragged': (10, 8, 645, 16000, 'cubic', (100.0, 400.0)),       # _HarmonicMaterialisedFunction, n_samples no multiple of n_frames
}
HARMONIC_WITH_F0 = ('f25_k12_nyquist', 'f10_k8_cubic_ragged')
# (what parts 2 and 4 need beside them: the shipped regime on frames of 128 samples, and with harmonics crossing Nyquist)
HARMONIC_OTHER = {'f10_k100_hop128': (10, 100, 1280, 16000, 'window', (69.0, 71.0)),
                  'f20_k100_crossing': (20, 100, 20 * 64, 16000, 'window', (180.0, 420.0))}


def _rng(*what):
  return np.random.default_rng(zlib.crc32('/'.join(str(w) for w in what).encode()))


@functools.lru_cache(maxsize=None)
def _harmonic_case(name, batch=3):
  f, k, n, sr, method, (f_lo, f_hi) = HARMONIC[name] if name in HARMONIC else HARMONIC_OTHER[name]
  rng = _rng('harmonic', name, batch)
  c = dict(name='harmonic/' + name, n=n, sr=sr, method=method, closed_form=method != 'cubic' and k <= 256,
           amps=rng.standard_normal((batch, f, 1)).astype(np.float32), hd=rng.standard_normal((batch, f, k)).astype(np.float32),
           f0=rng.uniform(f_lo, f_hi, (batch, f, 1)).astype(np.float32), g=rng.standard_normal((batch, n)).astype(np.float32))
  c['grads'] = O.harmonic_backward(c['amps'], c['hd'], c['f0'], c['g'], n, sr, O.exp_sigmoid, True, method, with_f0=True)
  return c


def _harmonic_synth(ddsp, c):
  return ddsp.synths.Harmonic(n_samples=c['n'], sample_rate=c['sr'], amp_resample_method=c['method'])


def _harmonic_run(synth, c, rows=slice(None), with_f0=False, leaves=None):
  a, h, f = leaves or (_t(c['amps'][rows], True), _t(c['hd'][rows], True), _t(c['f0'][rows], with_f0))
  synth(a, h, f).backward(_t(c['g'][rows]))
  return [a.grad, h.grad] + ([f.grad] if with_f0 else [])


def _harmonic_tols(c, with_f0):
  if not with_f0:
    return [grad_tol, grad_tol]
  if c['closed_form']:
    return [lambda ref: 2e-4 * np.abs(ref).max()] * 3                        # tests/test_gpu_parity_general.py:280-282
  return [grad_tol, grad_tol, lambda ref: 1e-6 + 5e-4 * np.abs(ref).max()]    # tests/test_gpu_parity_general.py:214-219


# name: (n_frames, n_bands, n_samples, window_size)
NOISE = {'mfma_f10_m65': (10, 65, 640, 0),         # the matrix-core kernel of the canonical filter
         'general_f7_m33_w17': (7, 33, 448, 17)}   # any band count and window: the general path


def _noise_seed(call):
  return SEED | (call << 32)


def _noise_tol(ref):
  return 1e-6 + 2e-5 * np.abs(ref).max()          # tests/test_gpu_parity.py:1514


AUDIO_ATOL = 2e-6 + 1e-5                          # tests/test_gpu_parity.py:1516


@functools.lru_cache(maxsize=None)
def _noise_case(name, batch=3, calls=1, variant=0):
  """`calls` sets of magnitudes; gradients and audio for supplied noise and for the generated noise of call 0 .. calls - 1."""
  f, m, n, ws = NOISE[name]
  rng = _rng('noise', name, batch, calls, variant)
  c = dict(name='noise/' + name, n=n, ws=ws, mags=[(rng.standard_normal((batch, f, m)) + 4.0).astype(np.float32) for _ in range(calls)],
           g=rng.standard_normal((batch, n)).astype(np.float32), noise=rng.uniform(-1, 1, (batch, n)).astype(np.float32),
           generated=[O.device_uniform_noise(batch, n, seed=_noise_seed(call)) for call in range(calls)])
  c['grad_supplied'] = O.filtered_noise_backward(c['mags'][0], c['noise'], c['g'], ws, O.exp_sigmoid)
  c['grad_generated'] = [O.filtered_noise_backward(mags, x, c['g'], ws, O.exp_sigmoid) for mags, x in zip(c['mags'], c['generated'])]
  c['audio_generated'] = [O.filtered_noise(mags, x, ws, O.exp_sigmoid, dtype=np.float64) for mags, x in zip(c['mags'], c['generated'])]
  return c


def _noise_synth(ddsp, c):
  return ddsp.synths.FilteredNoise(n_samples=c['n'], window_size=c['ws'], seed=SEED)


# Wavetable: 'audio_rate_tables' (tests/test_gpu_wavetable.py:258), the smallest of GRAD_CASES, at batch 3
WT_F, WT_W, WT_N, WT_FW = 20, 32, 320, 320


@functools.lru_cache(maxsize=None)
def _wavetable_case(n_frames=WT_F, n=WT_N, table_frames=WT_FW, batch=3):
  amps, tables, f0 = WT.synthesis_inputs(11 + n, batch, n_frames, WT_W, table_frames, rough=False, f_hi=2000.0)
  g = np.random.default_rng(n_frames + WT_W + table_frames).standard_normal((batch, n)).astype(np.float32)
  c = dict(name='wavetable/f%d_w%d_n%d' % (n_frames, WT_W, n), n=n, amps=amps, tables=tables, f0=f0, g=g)
  c['grads'] = WT.wavetable_synthesis(f0, amps, tables, n, 16000, grad_out=g, scale=False)[1:]
  return c


def _wavetable_run(ddsp, c, rows=slice(None), leaves=None):
  a, w, f = leaves or (_t(c['amps'][rows], True), _t(c['tables'][rows], True), _t(c['f0'][rows], True))
  ddsp.synths.Wavetable(n_samples=c['n'], sample_rate=16000, scale_fn=None)(a, w, f).backward(_t(c['g'][rows]))
  return [a.grad, w.grad, f.grad]


def _c_grad(ref):
  return C_GRAD * np.abs(ref).max()


@functools.lru_cache(maxsize=None)
def _mod_delay_case():
  """The shape of test_mod_delay_gradients_vs_truth (tests/test_gpu_wavetable.py:306), default scale functions, at batch 3."""
  rng = np.random.default_rng(23)
  b, n = 3, 2400
  c = dict(name='mod_delay/n2400', audio=rng.uniform(-1, 1, (b, n)).astype(np.float32), gain=rng.standard_normal((b, n, 1)).astype(np.float32),
           phase=rng.standard_normal((b, n, 1)).astype(np.float32), g=rng.standard_normal((b, n)).astype(np.float32))
  c['grads'] = WT.mod_delay(c['audio'], c['gain'][..., 0], c['phase'][..., 0], add_dry=True, scale=True, grad_out=c['g'])[1:]
  return c


def _mod_delay_run(ddsp, c, rows=slice(None), leaves=None):
  x, gain, phase = leaves or (_t(c['audio'][rows], True), _t(c['gain'][rows], True), _t(c['phase'][rows], True))
  ddsp.effects.ModDelay()(x, gain, phase).backward(_t(c['g'][rows]))
  return [x.grad, gain.grad, phase.grad]


@functools.lru_cache(maxsize=None)
def _reverb_case(batch=3, n=700, l=90):
  rng = _rng('reverb', batch, n, l)
  c = dict(name='reverb/b%d_n%d_l%d' % (batch, n, l), x=rng.standard_normal((batch, n)).astype(np.float32),
           h=(rng.standard_normal((batch, l)) * np.exp(-np.arange(l) / (0.3 * l))).astype(np.float32),
           g=rng.standard_normal((batch, n)).astype(np.float32))
  c['grads_per_row'] = O.reverb_backward(c['x'], c['h'], c['g'], True)
  c['grads_shared'] = O.reverb_backward(c['x'], c['h'][:1], c['g'], True)
  return c


def _reverb_run(rev, c, rows=slice(None), shared=False, leaves=None):
  x, h = leaves or (_t(c['x'][rows], True), _t(c['h'][0] if shared else c['h'][rows], True))
  rev(x, h).backward(_t(c['g'][rows]))
  return [x.grad, h.grad]


# ---- 1. a row alone, a sub-batch, twice: gradients bit for bit ---------------------------------------------------------------
@pytest.mark.parametrize('name,with_f0', [(name, False) for name in HARMONIC] + [(name, True) for name in HARMONIC_WITH_F0])
def test_harmonic_gradients_row_alone_sub_batch_and_twice(ddsp, name, with_f0):
  """One instance, batch 3, then row 1, rows [1:3] and batch 3 again (its workspaces sized by the largest call): the same bits.
  With 25, 20, 9, 12 or 10 frames a group of 8 frames of the flattened [B F] rows spans two batch rows."""
  c = _harmonic_case(name)
  synth = _harmonic_synth(ddsp, c)
  _rows_twice_and_sub_batches(c['name'] + ('/f0' if with_f0 else ''), lambda rows: _harmonic_run(synth, c, rows, with_f0),
                              _harmonic_tols(c, with_f0), c['grads'][:3 if with_f0 else 2], ROW_ALONE_AND_PAIR)


@pytest.mark.parametrize('name', list(NOISE))
def test_filtered_noise_gradients_row_alone_sub_batch_and_twice_supplied_noise(ddsp, name):
  c = _noise_case(name)
  synth = _noise_synth(ddsp, c)

  def run(rows):
    mags = _t(c['mags'][0][rows], True)
    synth(mags, noise=_t(c['noise'][rows])).backward(_t(c['g'][rows]))
    return [mags.grad]
  _rows_twice_and_sub_batches(c['name'] + '/supplied', run, [_noise_tol], [c['grad_supplied']], ROW_ALONE_AND_PAIR)


@pytest.mark.parametrize('name', list(NOISE))
def test_filtered_noise_gradients_row_alone_sub_batch_and_twice_generated_noise(ddsp, name):
  """Generated noise is Philox4x32-10 with key (seed, call counter) and counter (sample octet, ROW OF THIS CALL, half, 0): row r
  of a call draws the same samples whatever the batch size, but rows [1:3] of the batch are rows 0 and 1 of their own call and
  draw other noise.  So row 0 alone and rows [0:2], each on a fresh instance (call counter 0), are what can be compared."""
  c = _noise_case(name)

  def run(rows):
    mags = _t(c['mags'][0][rows], True)
    _noise_synth(ddsp, c)(mags).backward(_t(c['g'][rows]))
    return [mags.grad]
  _rows_twice_and_sub_batches(c['name'] + '/generated', run, [_noise_tol], [c['grad_generated'][0]], (slice(0, 1), slice(0, 2)))


def test_wavetable_gradients_row_alone_sub_batch_and_twice(ddsp):
  c = _wavetable_case()
  _rows_twice_and_sub_batches(c['name'], lambda rows: _wavetable_run(ddsp, c, rows), [_c_grad] * 3, c['grads'], ROW_ALONE_AND_PAIR)


def test_mod_delay_gradients_row_alone_sub_batch_and_twice(ddsp):
  c = _mod_delay_case()
  _rows_twice_and_sub_batches(c['name'], lambda rows: _mod_delay_run(ddsp, c, rows), [_c_grad] * 3, c['grads'], ROW_ALONE_AND_PAIR)


@pytest.mark.parametrize('shared', [True, False], ids=['shared_ir', 'per_row_ir'])
def test_reverb_gradients_twice_pair_preserving_sub_batch_and_row_alone(ddsp, shared):
  """The transform pairs batch rows (2 p, 2 p + 1 share one complex FFT; csrc/reverb.hip), so the last bits of a row depend on
  its partner: bits are demanded for the same call twice and for the sub-batch [:2], which keeps the pair; row 1 alone - paired
  with nothing - is held to the analytic oracle at reverb_tol.  One shared impulse response collects the gradient of the rows it
  served, so its gradient is compared with the oracle's for those rows."""
  c = _reverb_case()
  rev = ddsp.effects.Reverb()
  name = c['name'] + ('/shared' if shared else '/per_row')
  dx, dh = c['grads_shared'] if shared else c['grads_per_row']
  full = _reverb_run(rev, c, slice(0, 3), shared)
  _close(name + '/oracle/d_audio', full[0], dx, reverb_tol(dx))
  _close(name + '/oracle/d_ir', full[1], dh, reverb_tol(dh))
  for i, g in enumerate(_reverb_run(rev, c, slice(0, 3), shared)):
    _same_bits('%s/twice/grad%d' % (name, i), g, full[i])
  pair = _reverb_run(rev, c, slice(0, 2), shared)
  _same_bits(name + '/rows0_2/d_audio', pair[0], full[0][:2])
  if shared:
    ref = O.reverb_backward(c['x'][:2], c['h'][:1], c['g'][:2], True)[1]
    _close(name + '/rows0_2/d_ir', pair[1], ref, reverb_tol(ref))
  else:
    _same_bits(name + '/rows0_2/d_ir', pair[1], full[1][:2])
  alone = _reverb_run(rev, c, slice(1, 2), shared)
  _close(name + '/row1_alone/d_audio', alone[0], dx[1:2], reverb_tol(dx[1:2]))
  ref = O.reverb_backward(c['x'][1:2], c['h'][:1] if shared else c['h'][1:2], c['g'][1:2], True)[1]
  _close(name + '/row1_alone/d_ir', alone[1], ref, reverb_tol(ref))


# ---- 2. several live graphs on one instance ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(NOISE))
def test_filtered_noise_three_live_graphs_each_on_its_own_calls_noise(ddsp, name):
  """Three forwards on three sets of magnitudes (call counters 0, 1, 2), all three graphs kept, backward() in the order 2, 0, 1:
  every audio and every gradient belongs to the noise of its own call.  A gradient formed on another call's noise cannot pass:
  the oracle's gradients of call 1's magnitudes on the noise of calls 0 and 1 differ by far more than the tolerance."""
  c = _noise_case(name, batch=2, calls=3)
  wrong = O.filtered_noise_backward(c['mags'][1], c['generated'][0], c['g'], c['ws'], O.exp_sigmoid)
  assert np.abs(wrong - c['grad_generated'][1]).max() > 1000 * _noise_tol(c['grad_generated'][1])
  synth = _noise_synth(ddsp, c)
  mags = [_t(m, True) for m in c['mags']]
  audio = [synth(m) for m in mags]
  for call in (2, 0, 1):
    audio[call].backward(_t(c['g']))
  for call in range(3):
    _close('%s/live/call%d/audio' % (c['name'], call), audio[call], c['audio_generated'][call], AUDIO_ATOL)
    _close('%s/live/call%d/grad' % (c['name'], call), mags[call].grad, c['grad_generated'][call], _noise_tol(c['grad_generated'][call]))


def _two_live_graphs(name, first, second):
  """first / second: (run, fresh) - `run(leaves)` records a forward on the shared instance and returns (leaves, output, cotangent),
  `fresh()` the gradients of the same call on a fresh instance, one graph at a time.  Both forwards, then both backwards."""
  graphs = [run() for run, _ in (first, second)]
  for leaves, out, cot in graphs:
    out.backward(cot)
  for which, ((leaves, _, _), (_, fresh)) in enumerate(zip(graphs, (first, second))):
    for i, (leaf, ref) in enumerate(zip(leaves, fresh())):
      _same_bits('%s/graph%d/grad%d' % (name, which, i), leaf.grad, ref)


def test_harmonic_two_live_graphs_of_different_shapes(ddsp):
  """One instance (n_samples 1280): batch 1 x 10 frames of 128 samples, then batch 3 x 20 frames of 64 - both workspaces grow
  between the first forward and the first backward."""
  small, large = _harmonic_case('f10_k100_hop128', 1), _harmonic_case('f20_k100')
  synth = _harmonic_synth(ddsp, large)

  def recorded(c):
    def run():
      leaves = (_t(c['amps'], True), _t(c['hd'], True), _t(c['f0'], True))
      return leaves, synth(*leaves), _t(c['g'])
    return run, lambda: _harmonic_run(_harmonic_synth(ddsp, c), c, with_f0=True)
  _two_live_graphs('harmonic/two_graphs', recorded(small), recorded(large))



def test_wavetable_two_live_graphs_of_different_shapes(ddsp):
  """synths.Wavetable holds n_samples and its backward scratch is the module's one Workspace: two instances, 10 frames -> 160
  samples first, then 20 frames -> 320 samples at batch 3."""
  small, large = _wavetable_case(10, 160, 160, 1), _wavetable_case()

  def recorded(c):
    def run():
      leaves = (_t(c['amps'], True), _t(c['tables'], True), _t(c['f0'], True))
      return leaves, ddsp.synths.Wavetable(n_samples=c['n'], sample_rate=16000, scale_fn=None)(*leaves), _t(c['g'])
    return run, lambda: _wavetable_run(ddsp, c)
  _two_live_graphs('wavetable/two_graphs', recorded(small), recorded(large))


def test_reverb_two_live_graphs_of_different_shapes(ddsp):
  """One instance: batch 1, 300 samples, 40 taps, then batch 3, 700 samples, 90 taps."""
  small, large = _reverb_case(1, 300, 40), _reverb_case()
  rev = ddsp.effects.Reverb()

  def recorded(c):
    def run():
      leaves = (_t(c['x'], True), _t(c['h'], True))
      return leaves, rev(*leaves), _t(c['g'])
    return run, lambda: _reverb_run(ddsp.effects.Reverb(), c)
  _two_live_graphs('reverb/two_graphs', recorded(small), recorded(large))


def _twice_into_the_same_leaves(name, leaves, out, cot):
  """backward(retain_graph=True), then backward() again: the leaves hold exactly twice the single gradient."""
  out.backward(cot, retain_graph=True)
  single = [leaf.grad.clone() for leaf in leaves]
  out.backward(cot)
  for i, (leaf, g) in enumerate(zip(leaves, single)):
    assert float(g.abs().max()) > 0.0
    _same_bits('%s/retain_graph/grad%d' % (name, i), leaf.grad, 2 * g)


@pytest.mark.parametrize('op', ['harmonic', 'harmonic_chain', 'noise_supplied', 'noise_generated', 'wavetable', 'reverb'])
def test_backward_twice_with_retain_graph_doubles_the_gradient(ddsp, op):
  if op.startswith('harmonic'):
    c = _harmonic_case('f20_k100' if op == 'harmonic' else 'f10_k8_cubic_ragged')
    leaves = (_t(c['amps'], True), _t(c['hd'], True), _t(c['f0'], True))
    out = _harmonic_synth(ddsp, c)(*leaves)
  elif op.startswith('noise'):
    c = _noise_case('mfma_f10_m65')
    leaves = (_t(c['mags'][0], True),)
    out = _noise_synth(ddsp, c)(leaves[0], noise=_t(c['noise']) if op == 'noise_supplied' else None)
  elif op == 'wavetable':
    c = _wavetable_case()
    leaves = (_t(c['amps'], True), _t(c['tables'], True), _t(c['f0'], True))
    out = ddsp.synths.Wavetable(n_samples=c['n'], sample_rate=16000, scale_fn=None)(*leaves)
  else:
    c = _reverb_case()
    leaves = (_t(c['x'], True), _t(c['h'], True))
    out = ddsp.effects.Reverb()(*leaves)
  _twice_into_the_same_leaves(op, leaves, out, _t(c['g']))


def test_spectral_loss_backward_twice_with_retain_graph(ddsp):
  """The gradient kernel of the loss overlap-adds its frames with fp32 atomics ("last bits not reproducible
  run to run"), so twice the gradient is held to the analytic oracle at the tolerance of
  test_spectral_loss_backward_vs_analytic_oracle, not to the bits of the first."""
  rng = np.random.default_rng(1024)
  sizes = (256, 128)
  t = (0.3 * rng.standard_normal((2, 1024))).astype(np.float32)
  a = (0.8 * t + 0.05 * rng.standard_normal((2, 1024))).astype(np.float32)
  ta = _t(a, True)
  val = ddsp.losses.SpectralLoss(fft_sizes=sizes, mag_weight=1.0, logmag_weight=0.5)(_t(t), ta)
  ref = O.spectral_loss_backward(t, a, sizes, 1.0, 0.5)
  for times in (1, 2):
    val.backward(retain_graph=times == 1)
    atol = 1e-9 + 2e-4 * np.abs(times * ref).max()
    err = np.abs(_np(ta.grad) - times * ref)
    _log('spectral_loss/retain_graph/x%d' % times, err=err.max(), atol=atol, frac_of_tol=err.max() / atol, above=(err > atol).mean())
    assert (err > atol).mean() <= 1e-3 and err.max() <= 10 * atol, (times, float((err > atol).mean()), float(err.max()), atol)


def test_processor_group_called_twice_into_one_backward(ddsp):
  """Harmonic + FilteredNoise + Add (the DAG of ae.gin) called on two feature dicts that share the amplitude and
  harmonic-distribution leaves (as two batches share a decoder's weights); the two losses summed into ONE backward().  Against a
  second group run one graph at a time - same call counters of its FilteredNoise - the shared leaves hold the sum of the two
  gradients (one fp32 addition, the same in either order), the others their own, bit for bit."""
  c, n = _harmonic_case('f20_k100'), 1280
  rng = _rng('group')
  f0 = [c['f0'], rng.uniform(180.0, 420.0, c['f0'].shape).astype(np.float32)]
  mags = [(rng.standard_normal((3, 20, 65)) + 4.0).astype(np.float32) for _ in range(2)]
  cots = [_t(c['g']), _t(rng.standard_normal((3, n)))]

  def build():
    dag = [(ddsp.synths.Harmonic(n_samples=n), ['amps', 'harmonic_distribution', 'f0_hz']),
           (ddsp.synths.FilteredNoise(n_samples=n, window_size=0, seed=SEED), ['magnitudes']),
           (ddsp.processors.Add(), ['filtered_noise/signal', 'harmonic/signal'])]
    return ddsp.processors.ProcessorGroup(dag=dag)

  def leaves():
    return _t(c['amps'], True), _t(c['hd'], True), [_t(m, True) for m in mags]

  def features(amps, hd, m, i):
    return {'amps': amps, 'harmonic_distribution': hd, 'f0_hz': _t(f0[i]), 'magnitudes': m[i]}
  amps, hd, m = leaves()
  group = build()
  losses = [(group(features(amps, hd, m, i)) * cots[i]).sum() for i in range(2)]
  (losses[0] + losses[1]).backward()
  amps1, hd1, m1 = leaves()
  group = build()
  separate = []
  for i in range(2):
    (group(features(amps1, hd1, m1, i)) * cots[i]).sum().backward()
    separate.append((amps1.grad.clone(), hd1.grad.clone()))
    amps1.grad = hd1.grad = None
  _same_bits('group/amps', amps.grad, separate[0][0] + separate[1][0])
  _same_bits('group/harmonic_distribution', hd.grad, separate[0][1] + separate[1][1])
  for i in range(2):
    assert float(m[i].grad.abs().max()) > 0.0
    _same_bits('group/magnitudes%d' % i, m[i].grad, m1[i].grad)


# ---- 3. inputs overwritten, attributes changed between forward and backward ----------------------------------------------------
def _overwritten(name, record, victim):
  """`record()` -> (leaves, output, cotangent, tensors by name).  The gradients of the untouched call; then the same call with
  `victim` halved in place before backward(): torch's in-place RuntimeError, or the untouched gradients - never other values."""
  leaves, out, cot, _ = record()
  out.backward(cot)
  wanted = [leaf.grad.clone() for leaf in leaves]
  leaves, out, cot, tensors = record()
  with torch.no_grad():
    tensors[victim].mul_(0.5)
  try:
    out.backward(cot)
  except RuntimeError as e:
    assert 'inplace operation' in str(e), e
    _log('%s/overwritten/%s' % (name, victim), raised=1)
    return
  _log('%s/overwritten/%s' % (name, victim), raised=0)
  for i, (leaf, g) in enumerate(zip(leaves, wanted)):
    _same_bits('%s/overwritten/%s/grad%d' % (name, victim, i), leaf.grad, g)


OVERWRITTEN = [('harmonic', 'f0'), ('harmonic', 'hd'), ('noise', 'noise'), ('noise', 'mags'), ('wavetable', 'tables'),
               ('mod_delay', 'audio'), ('reverb', 'ir'), ('reverb', 'audio'), ('fir_filter', 'audio'), ('fir_filter', 'mags')]


@pytest.mark.parametrize('op,victim', OVERWRITTEN, ids=['%s-%s' % case for case in OVERWRITTEN])
def test_input_overwritten_between_forward_and_backward(ddsp, op, victim):
  """FilteredNoise kept supplied noise as a plain attribute of ctx - the caller's own tensor when it was a contiguous fp32 device
  tensor already - and an in-place write to it before backward() gave another gradient in silence (the 'noise-noise' case)."""
  if op == 'harmonic':
    c = _harmonic_case('f20_k100')

    def record():
      t = dict(amps=_t(c['amps'], True), hd=_t(c['hd'], True), f0=_t(c['f0']))
      return (t['amps'], t['hd']), _harmonic_synth(ddsp, c)(t['amps'], t['hd'], t['f0']), _t(c['g']), t
  elif op == 'noise':
    c = _noise_case('mfma_f10_m65')

    def record():
      t = dict(mags=_t(c['mags'][0], True), noise=_t(c['noise']))
      return (t['mags'],), _noise_synth(ddsp, c)(t['mags'], noise=t['noise']), _t(c['g']), t
  elif op == 'wavetable':
    c = _wavetable_case()

    def record():
      t = dict(amps=_t(c['amps'], True), tables=_t(c['tables']), f0=_t(c['f0'], True))
      out = ddsp.synths.Wavetable(n_samples=c['n'], sample_rate=16000, scale_fn=None)(t['amps'], t['tables'], t['f0'])
      return (t['amps'], t['f0']), out, _t(c['g']), t
  elif op == 'mod_delay':
    c = _mod_delay_case()

    def record():
      t = dict(audio=_t(c['audio']), gain=_t(c['gain'], True), phase=_t(c['phase'], True))
      return (t['gain'], t['phase']), ddsp.effects.ModDelay()(t['audio'], t['gain'], t['phase']), _t(c['g']), t
  elif op == 'reverb':
    c = _reverb_case()

    def record():
      t = dict(audio=_t(c['x'], True), ir=_t(c['h'], True))
      return (t['audio'], t['ir']), ddsp.effects.Reverb()(t['audio'], t['ir']), _t(c['g']), t
  else:
    c = _noise_case('general_f7_m33_w17')

    def record():
      t = dict(audio=_t(c['noise'], True), mags=_t(c['mags'][0], True))
      return (t['audio'], t['mags']), ddsp.effects.FIRFilter(window_size=c['ws'])(t['audio'], t['mags']), _t(c['g']), t
  _overwritten(op, record, victim)


@pytest.mark.parametrize('op', ['harmonic', 'harmonic_chain', 'noise', 'reverb'])
def test_attribute_changed_between_forward_and_backward(ddsp, op):
  """The autograd nodes take the scalars their backward needs (n_samples, sample_rate, the method and flag words, window_size,
  initial_bias, noise_bits, add_dry) in forward: a graph gives the gradient of the call it recorded although the instance's
  attribute has changed since - here n_samples halved (Reverb: add_dry switched off)."""
  if op.startswith('harmonic'):
    c = _harmonic_case('f20_k100' if op == 'harmonic' else 'f10_k8_cubic_ragged')
    wanted = _harmonic_run(_harmonic_synth(ddsp, c), c, with_f0=True)
    leaves = (_t(c['amps'], True), _t(c['hd'], True), _t(c['f0'], True))
    synth = _harmonic_synth(ddsp, c)
    out = synth(*leaves)
    synth.n_samples, synth.sample_rate, synth.amp_resample_method = c['n'] // 2, 8000, 'linear'
  elif op == 'noise':
    c = _noise_case('general_f7_m33_w17')
    leaves = (_t(c['mags'][0], True),)
    _noise_synth(ddsp, c)(leaves[0]).backward(_t(c['g']))
    wanted, leaves = [leaves[0].grad], (_t(c['mags'][0], True),)
    synth = _noise_synth(ddsp, c)
    out = synth(*leaves)
    synth.n_samples, synth.window_size, synth.initial_bias = c['n'] // 2, 0, 0.0
  else:
    c = _reverb_case()
    wanted = _reverb_run(ddsp.effects.Reverb(), c)
    leaves = (_t(c['x'], True), _t(c['h'], True))
    rev = ddsp.effects.Reverb()
    out = rev(*leaves)
    rev._add_dry = False
  out.backward(_t(c['g']))
  for i, (leaf, g) in enumerate(zip(leaves, wanted)):
    _same_bits('%s/attribute_changed/grad%d' % (op, i), leaf.grad, g)


# ---- 4. two streams, one instance ------------------------------------------------------------------------------------------
def test_two_streams_share_one_harmonic_and_one_filtered_noise_instance(ddsp):
  """Forward + backward of batch A on one side stream and of batch B on another, three rounds, one Harmonic and one
  FilteredNoise instance (scratch per stream in core.Workspace, a g_sched set per launch): audio and gradients bit-equal to the
  same work run serially on the default stream."""
  if DEV != 'cuda' or not torch.cuda.is_available():
    pytest.skip('needs real streams: left to the GPU run')
  hc = [_harmonic_case('f20_k100', 2), _harmonic_case('f20_k100_crossing', 2)]
  zc = [_noise_case('mfma_f10_m65', 2), _noise_case('mfma_f10_m65', 2, variant=1)]

  def work(harm, fnoise, which):
    h, z = hc[which], zc[which]
    leaves = (_t(h['amps'], True), _t(h['hd'], True), _t(z['mags'][0], True))
    audio = harm(leaves[0], leaves[1], _t(h['f0'])), fnoise(leaves[2], noise=_t(z['noise']))
    audio[0].backward(_t(h['g']))
    audio[1].backward(_t(z['g']))
    return [a.detach() for a in audio] + [leaf.grad for leaf in leaves]
  harm, fnoise = _harmonic_synth(ddsp, hc[0]), _noise_synth(ddsp, zc[0])
  serial = [work(harm, fnoise, 0), work(harm, fnoise, 1)]
  torch.cuda.synchronize()
  harm, fnoise = _harmonic_synth(ddsp, hc[0]), _noise_synth(ddsp, zc[0])
  streams = [torch.cuda.Stream(), torch.cuda.Stream()]
  results = []
  for side in streams:
    side.wait_stream(torch.cuda.current_stream())
  for _ in range(3):
    round_results = []
    for which, side in enumerate(streams):
      with torch.cuda.stream(side):
        round_results.append(work(harm, fnoise, which))
    results.append(round_results)
  for side in streams:
    torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  for r, round_results in enumerate(results):
    for which in range(2):
      for i, (got, ref) in enumerate(zip(round_results[which], serial[which])):
        _same_bits('streams/round%d/batch%s/tensor%d' % (r, 'AB'[which], i), got, ref)



@pytest.fixture(scope='module')
def ddsp():
  import ddsp_amd
  return ddsp_amd
