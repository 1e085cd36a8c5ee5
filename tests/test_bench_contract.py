"""CPU checks of bench.py's JSON line (the driver's contract): build_result() is pure, so the fields, the
roofline arithmetic and the optional blocks are exercised here on the numbers of profiles/r01_bench_*.json;
parse_args() defaults must describe the shape BASELINE.json's target is quoted on (configs[1]'s clips at batch 128)."""
import importlib.util
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def bench():
  spec = importlib.util.spec_from_file_location('bench_module', os.path.join(ROOT, 'bench.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def _args(bench, *argv):
  old = sys.argv
  sys.argv = ['bench.py'] + list(argv)
  try:
    return bench.parse_args()
  finally:
    sys.argv = old


def test_defaults_are_the_north_star_shape(bench):
  a = _args(bench)
  assert (a.gpus, a.batch, a.n_frames, a.n_harmonics, a.n_bands, a.n_samples, a.sample_rate) == (
      1, 128, 1000, 100, 65, 64000, 16000)
  assert a.second_batch == 32                      # configs[1] rides along as `configs_1`
  assert a.f0 == 70.0 and a.steps > 0 and a.warmup > 0
  # 664 000 + 516 000 bytes per clip
  assert bench.algorithmic_bytes(a, 1) == (664000, 516000)
  assert bench.algorithmic_bytes(a, 128)[0] + bench.algorithmic_bytes(a, 128)[1] == 151040000
  harm_flops, noise_flops = bench.algorithmic_flops(a, 1)
  assert harm_flops == 64000 * 3 * 100 * 2 and noise_flops == 64000 * 2 * 128


@pytest.mark.parametrize('world,batch,dominant', [(1, 32, 'noise_fused65_kernel'), (8, 128, 'harm_table_kernel')])
def test_json_line_fields_and_roofline_arithmetic(bench, world, batch, dominant):
  a = _args(bench, '--gpus', str(world), '--batch', str(batch), '--steps', '1000', '--warmup', '500', '--full')
  elapsed = 0.0368 if batch == 32 else 0.1172                       # seconds for 1000 steps (profiles/r01_bench_*)
  launch_us = 31.0 if batch == 32 else 59.96
  prof = {dominant: (launch_us * 125 * 1e-3, 125)}
  breakdown = {'noise_fused65_kernel': (0.0247 * 3, 3), 'harm_table_kernel': (0.0204 * 3, 3)}
  aux = {'measured_copy_GBs': 4000.0,
         'f0_regimes': {'200+-1 Hz': {'ms_per_step': elapsed * 1.5, 'steps': 200, 'value': 1.0},
                        '333+-1 Hz': {'ms_per_step': elapsed * 1.2, 'steps': 200, 'value': 1.0}}}
  r = bench.build_result(a, world, batch, elapsed, prof, breakdown, dominant, overlap=batch < 64, aux=aux,
                         alt_elapsed=0.05, gather_ms=0.4 if world > 1 else None,
                         cpu_baseline_fn=lambda args: {'value': 0.77, 'unit': 'Msamples/s', 'cores': 1,
                                                       'kind': 'port', 'sample': 'stub'})
  line = json.loads(json.dumps(r))                                   # serialisable, one line
  for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better',
              'scaling', 'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
    assert key in line, key
  assert line['unit'] == 'Msamples/s' and line['higher_is_better'] is True and line['scaling'] == 'weak'
  assert line['vs_baseline'] is None and line['dtype'].startswith('f32') and 'MFMA' in line['dtype']
  assert line['data'] == 'synthetic' and line['per_gpu_value'] == pytest.approx(line['value'] / world)
  assert line['n_gpus'] == world and line['steps'] == 1000 and line['warmup'] == 500
  assert 'model' not in line['config'] and 'workload' in line['config']
  assert line['config']['global_batch'] == world * batch
  # whole-job aggregate: every rank's samples over the max-over-ranks time
  assert line['value'] == pytest.approx(world * batch * 64000 * 1000 / elapsed / 1e6)
  assert line['ms_per_step'] == pytest.approx(elapsed)
  roof = line['roofline']
  per_clip = 664000 if dominant.startswith('harm') else 516000
  assert roof['bound'] == 'hbm' and roof['unit'] == 'GB/s' and roof['peak'] == 8000.0
  assert roof['achieved'] == pytest.approx(per_clip * batch / (launch_us * 1e-6) / 1e9)
  assert roof['frac'] == pytest.approx(roof['achieved'] / 8000.0)
  assert roof['frac_of_measured_copy'] == pytest.approx(roof['achieved'] / 4000.0)
  # the ALU note says what its flop count is (the reference formulation's, which the wavetable kernel does not execute:
  # VERDICT r3, weak #6b) and carries what the kernel executes when an SQ counter pass of the shape is committed
  note = roof['alu_note']
  assert 'achieved_TFLOPs' not in note and 'frac' not in note
  assert 0 < note['reference_formulation_equivalent_frac'] < 1 and 0 < note['whole_step_reference_formulation_equivalent_frac'] < 1
  assert note['reference_formulation_equivalent_TFLOPs'] == pytest.approx(
      note['reference_formulation_flop_per_launch'] / (launch_us * 1e-6) / 1e12)
  assert 'executed' in note and (note['executed'] is None or note['executed']['wave_instructions_per_launch'] > 0)
  assert roof['traffic'] is None or roof['traffic'] > 0
  assert line['other_issue_mode']['value'] > 0
  # every f0 regime with its whole-step roofline fraction, the worst at the top level
  step_bytes = 1180000 * batch
  regimes = line['f0_regimes']
  assert set(regimes) == {'200+-1 Hz', '333+-1 Hz', '70+-1 Hz (headline)'}
  for r_ in regimes.values():
    assert r_['frac'] == pytest.approx(step_bytes / (r_['ms_per_step'] * 1e-3) / 1e9 / 8000.0)
  assert line['f0_200_regime'] == regimes['200+-1 Hz'] and line['f0_200_regime']['steps'] == 200
  assert line['worst_regime']['regime'] == '200+-1 Hz' and line['min_regime_frac'] == pytest.approx(regimes['200+-1 Hz']['frac'])
  assert line['min_regime_frac'] == pytest.approx(roof['whole_step']['frac'] / 1.5)
  assert line['regime_worst_over_best_time'] == pytest.approx(1.5)
  if world == 1:
    assert line['cpu_baseline']['kind'] == 'port' and 'allgather_ms' not in line
  else:
    assert line['cpu_baseline'] is None and line['allgather_ms'] == 0.4       # rank 0 at N=1 only


def test_minimal_call_without_optional_blocks(bench):
  a = _args(bench, '--no-cpu-baseline')
  r = bench.build_result(a, 1, 32, 0.04, {'harm_table_kernel': (2.0, 100)}, {'harm_table_kernel': (0.06, 3)},
                         'harm_table_kernel', overlap=True)
  assert 'cpu_baseline' not in r and 'other_issue_mode' not in r and 'f0_200_regime' not in r and 'min_regime_frac' not in r
  assert 'measured_copy_GBs' not in r['roofline']
  json.dumps(r)


def test_main_control_flow_with_the_gpu_mocked_out(bench, monkeypatch, capsys):
  """bench.main() end to end with every device call replaced by a stand-in: guards the control flow of the
  timed region, the auxiliary yardsticks and the JSON print against NameErrors / TypeErrors that would only
  show at round end on the GPU box.  No kernel runs and no number printed here means anything."""
  import numpy as np
  import torch
  import ddsp_amd
  from ddsp_amd import _lib, build

  class _Stream:
    def wait_event(self, event):
      pass

  class _Event:
    def __init__(self, enable_timing=False):
      pass

    def record(self, stream=None):
      pass

    def elapsed_time(self, other):
      return 1.0

  calls = {'harm': 0, 'noise': 0, 'begin': 0}
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
  monkeypatch.setattr(torch.cuda, 'set_device', lambda d: None)
  monkeypatch.setattr(torch.cuda, 'Stream', _Stream)
  monkeypatch.setattr(torch.cuda, 'Event', _Event)
  monkeypatch.setattr(torch.cuda, 'current_stream', lambda: _Stream())
  monkeypatch.setattr(torch.cuda, 'set_stream', lambda s: None)
  monkeypatch.setattr(torch.cuda, 'synchronize', lambda: None)
  real_empty = torch.empty
  monkeypatch.setattr(torch, 'empty', lambda *a, device=None, **k: real_empty(*a, **k))
  monkeypatch.setattr(build, 'build', lambda *a, **k: None)
  monkeypatch.setattr(_lib, 'load', lambda: None)

  def fake_begin(names, max_records=0, stride=1):
    calls['begin'] += 1
    calls['names'] = names

  def fake_end():
    if calls['names'] is None:       # the diagnostic pass: every kernel
      return {'harm_table_kernel': (0.06, 3), 'noise_fused65_kernel': (0.075, 3)}
    return {calls['names'][0]: (3.1, 100)}
  monkeypatch.setattr(_lib, 'profile_begin', fake_begin)
  monkeypatch.setattr(_lib, 'profile_end', fake_end)
  monkeypatch.setattr(ddsp_amd.core, 'tf_float32', lambda x: torch.as_tensor(np.asarray(x, np.float32)))

  class _Harmonic:
    def __init__(self, n_samples, sample_rate):
      self.n = n_samples

    def __call__(self, amplitudes, harmonic_distribution, f0_hz):
      calls['harm'] += 1
      calls['last_f0'] = float(f0_hz.mean())
      calls.setdefault('f0s', []).append(calls['last_f0'])
      calls.setdefault('batches', set()).add(int(amplitudes.shape[0]))
      return torch.zeros(amplitudes.shape[0], self.n)

    def call_add(self, amplitudes, harmonic_distribution, f0_hz, add_signal):
      calls['harm'] += 1
      calls['fused'] = calls.get('fused', 0) + 1
      return add_signal

  class _Noise:
    def __init__(self, n_samples, window_size, seed, noise_bits=23):
      self.n = n_samples
      calls.setdefault('noise_bits', set()).add(noise_bits)

    def __call__(self, magnitudes):
      calls['noise'] += 1
      return torch.zeros(magnitudes.shape[0], self.n)
  monkeypatch.setattr(ddsp_amd.synths, 'Harmonic', _Harmonic)
  monkeypatch.setattr(ddsp_amd.synths, 'FilteredNoise', _Noise)
  monkeypatch.setattr(bench, 'cpu_baseline', lambda a: {'value': 1.0, 'unit': 'Msamples/s', 'cores': 1,
                                                        'kind': 'port', 'sample': 'stub'})
  monkeypatch.setenv('WORLD_SIZE', '1')
  monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '7', '--warmup', '2', '--batch', '2', '--n-frames', '10',
                                    '--n-samples', '640', '--also-other-mode', '--full'])
  bench.main()
  out = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')]
  assert len(out) == 1                                               # ONE JSON line
  line = json.loads(out[0])
  assert line['steps'] == 7 and line['warmup'] == 2 and line['n_gpus'] == 1
  assert line['roofline']['kernel'] == 'noise_fused65_kernel'         # the larger isolated time above
  assert 'aux_error' not in line, line.get('aux_error')
  assert line['roofline']['measured_copy_GBs'] > 0 and line['f0_200_regime']['steps'] == 7
  assert len(line['f0_regimes']) == 5 and all(r_['frac'] > 0 for r_ in line['f0_regimes'].values())
  assert 0 < line['min_regime_frac'] <= line['roofline']['whole_step']['frac'] and line['regime_worst_over_best_time'] >= 1.0
  for centre in (220.0, 333.0, 500.0):
    assert any(abs(f - centre) < 7.0 for f in calls['f0s']), centre
  assert line['cpu_baseline']['kind'] == 'port' and 'other_issue_mode' in line
  assert calls['harm'] == calls['noise'] and calls['harm'] >= 2 + 3 + 7 + 7 + 20 + 10
  assert calls['fused'] >= 7 and line['fused_add']['bytes_per_sample'] < 18.44 and line['fused_add']['value'] > 0
  assert any(abs(f - 200.0) < 2.0 for f in calls['f0s'])              # the f0 = 200 regime ran...
  assert abs(calls['last_f0'] - 70.0) < 2.0                            # ...and the second shape after it, on its own inputs
  assert calls['batches'] == {2, 32}
  ns = line['configs_1']
  assert ns['batch_per_gpu'] == 32 and ns['value'] > 0 and 0 < ns['whole_step']['frac'] and 'dominant_kernel' in ns
  assert line['ms_per_step_host_clock'] > 0
  assert line['timing']['repeats'] >= 10 and line['timing']['region_ms_median'] > 0
  # ...and the headline inputs were put back afterwards (nothing after the regime reads them, but a later edit might)


def _mock_device(monkeypatch, bench, calls):
  """Everything bench.main() touches on the device, replaced by stand-ins (shared by the two main() tests)."""
  import numpy as np
  import torch
  import ddsp_amd
  from ddsp_amd import _lib, build

  class _Stream:
    def wait_event(self, event):
      pass

  class _Event:
    def __init__(self, enable_timing=False):
      pass

    def record(self, stream=None):
      pass

    def elapsed_time(self, other):
      return 1.0
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
  monkeypatch.setattr(torch.cuda, 'set_device', lambda d: None)
  monkeypatch.setattr(torch.cuda, 'Stream', _Stream)
  monkeypatch.setattr(torch.cuda, 'Event', _Event)
  monkeypatch.setattr(torch.cuda, 'current_stream', lambda: _Stream())
  monkeypatch.setattr(torch.cuda, 'set_stream', lambda s: None)
  monkeypatch.setattr(torch.cuda, 'synchronize', lambda: None)
  real_empty, real_tensor = torch.empty, torch.tensor
  monkeypatch.setattr(torch, 'empty', lambda *a, device=None, **k: real_empty(*a, **k))
  monkeypatch.setattr(torch, 'tensor', lambda *a, device=None, **k: real_tensor(*a, **k))
  monkeypatch.setattr(build, 'build', lambda *a, **k: None)
  monkeypatch.setattr(_lib, 'load', lambda: None)

  def fake_begin(names, max_records=0, stride=1):
    calls['names'] = names

  def fake_end():
    if calls['names'] is None:
      return {'harm_table_kernel': (0.06, 3), 'noise_fused65_kernel': (0.075, 3)}
    return {calls['names'][0]: (3.1, 100)}
  monkeypatch.setattr(_lib, 'profile_begin', fake_begin)
  monkeypatch.setattr(_lib, 'profile_end', fake_end)
  monkeypatch.setattr(ddsp_amd.core, 'tf_float32', lambda x: torch.as_tensor(np.asarray(x, np.float32)))

  class _Harmonic:
    def __init__(self, n_samples, sample_rate):
      self.n = n_samples

    def __call__(self, amplitudes, harmonic_distribution, f0_hz):
      calls['harm'] = calls.get('harm', 0) + 1
      return torch.zeros(amplitudes.shape[0], self.n)

    def call_add(self, amplitudes, harmonic_distribution, f0_hz, add_signal):
      calls['fused'] = calls.get('fused', 0) + 1
      return add_signal.clone()

  class _Loss:
    def __init__(self, **kwargs):
      calls['loss_kwargs'] = kwargs

    def __call__(self, target, audio):
      calls['loss'] = calls.get('loss', 0) + 1
      return (audio * 0.0).sum()

  class _Reverb:
    def __init__(self, trainable=False, reverb_length=48000, add_dry=True):
      self.trainable, self._ir = trainable, None

    def build(self, device=None):
      pass

    def __call__(self, audio, ir=None):
      assert (ir is None) == self.trainable
      calls['reverb'] = calls.get('reverb', 0) + 1
      return audio
  monkeypatch.setattr(ddsp_amd.losses, 'SpectralLoss', _Loss)
  monkeypatch.setattr(ddsp_amd.effects, 'Reverb', _Reverb)

  class _Noise:
    def __init__(self, n_samples, window_size, seed, noise_bits=23):
      self.n = n_samples
      calls.setdefault('noise_bits', set()).add(noise_bits)

    def __call__(self, magnitudes):
      calls['noise'] = calls.get('noise', 0) + 1
      return torch.zeros(magnitudes.shape[0], self.n)
  monkeypatch.setattr(ddsp_amd.synths, 'Harmonic', _Harmonic)
  monkeypatch.setattr(ddsp_amd.synths, 'FilteredNoise', _Noise)
  monkeypatch.setattr(bench, 'cpu_baseline', lambda a: {'value': 1.0, 'unit': 'Msamples/s', 'cores': 1,
                                                        'kind': 'port', 'sample': 'stub'})


def test_main_multi_rank_branches_with_device_and_collectives_mocked_out(bench, monkeypatch, capsys):
  """The N > 1 branches of bench.main() as rank 0 of a world of 2 (process group, barriers, the max-over-ranks
  reduction, --allgather, no CPU leg): collectives are no-ops here, only the control flow is exercised."""
  import torch.distributed as dist
  calls = {}
  _mock_device(monkeypatch, bench, calls)
  log = []
  monkeypatch.setattr(dist, 'init_process_group', lambda *a, **k: log.append(('init', a, sorted(k))))
  monkeypatch.setattr(dist, 'barrier', lambda *a, **k: log.append('barrier'))
  monkeypatch.setattr(dist, 'all_reduce', lambda t, op=None: log.append('all_reduce'))
  monkeypatch.setattr(dist, 'all_gather_into_tensor', lambda out, x: log.append('all_gather'))
  monkeypatch.setattr(dist, 'destroy_process_group', lambda: log.append('destroy'))
  for key, value in (('WORLD_SIZE', '2'), ('RANK', '0'), ('LOCAL_RANK', '0')):
    monkeypatch.setenv(key, value)
  monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '2', '--steps', '5', '--warmup', '2', '--batch', '2',
                                    '--n-frames', '10', '--n-samples', '640', '--allgather', '--full'])
  bench.main()
  out = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')]
  assert len(out) == 1
  line = json.loads(out[0])
  assert line['n_gpus'] == 2 and line['config']['global_batch'] == 4 and line['scaling'] == 'weak'
  assert line['cpu_baseline'] is None and 'allgather_ms' in line and 'aux_error' not in line
  assert line['value'] > 0 and line['config']['parallelism'].startswith('batch-sharded x2')
  assert log[0][0] == 'init' and log[0][1][0] == 'nccl' and log[-1] == 'destroy'
  assert log.count('all_reduce') >= 2 and log.count('all_gather') == 13 and log.count('barrier') >= 6
  with pytest.raises(SystemExit, match='WORLD_SIZE'):
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '4'])
    bench.main()


def test_main_other_configs_blocks_with_the_device_mocked_out(bench, monkeypatch, capsys):
  """The default-shape run's extra blocks - configs_2 (SpectralLoss), configs_3 (Reverb, one trainable impulse response and one per
  clip), fnoise_11_bit_levels (noise_bits=11 beside the 23-bit headline) - end to end with every device call replaced by a stand-in (these
  blocks must be in the driver's line; a NameError here would only show on the GPU box at round end)."""
  calls = {}
  _mock_device(monkeypatch, bench, calls)
  monkeypatch.setenv('WORLD_SIZE', '1')
  monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '3', '--warmup', '1', '--settle', '0', '--full'])
  bench.main()
  out = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')]
  assert len(out) == 1
  line = json.loads(out[0])
  assert 'aux_error' not in line, line.get('aux_error')
  for key in ('configs_1', 'configs_4', 'configs_2', 'configs_3', 'fnoise_11_bit_levels'):
    assert key in line and 'error' not in line[key], (key, line.get(key))
    blk = line[key]
    assert blk['ms_per_step'] > 0 and blk['value'] > 0 and 0 < blk['whole_step']['frac'] and blk['whole_step']['algorithmic_bytes'] > 0
  c2, c3, fr = line['configs_2'], line['configs_3'], line['fnoise_11_bit_levels']
  assert c2['batch_per_gpu'] == 128 and c3['batch_per_gpu'] == 128 and fr['batch_per_gpu'] == 128
  # algorithmic bytes: the DAG's controls in and one audio stream out (14.44 B / sample at this shape), + what the caller reads / writes
  synth = 4 * 128 * (1000 * 102 + 1000 * 65 + 64000)
  assert c2['whole_step']['algorithmic_bytes'] == synth + 8 * 128 * 64000
  assert c3['whole_step']['algorithmic_bytes'] == synth + 8 * 128 * 64000 + 4 * 48000
  assert c3['per_clip_ir']['whole_step']['algorithmic_bytes'] == synth + 8 * 128 * 64000 + 4 * 48000 * 128
  assert fr['whole_step']['algorithmic_bytes'] == line['roofline']['whole_step']['algorithmic_bytes']
  assert 'kernel_breakdown_us' in c2 and 'kernel_breakdown_us' in c3 and c2['with_gradient_wrt_audio']['ms_per_step'] > 0
  assert 'cost_of_the_twelve_bits_us' in fr and fr['headline_ms_per_step'] == line['ms_per_step']
  assert calls['noise_bits'] == {11, 23} and calls['loss'] > 10 and calls['reverb'] > 20 and calls['fused'] > 30
  assert calls['loss_kwargs'] == {'logmag_weight': 1.0}
  assert '2^23 levels' in line['config']['workload'] and 'noise_bits=23' in line['config']['workload']


def test_plain_run_times_exactly_k_steps_and_only_the_headline(bench, monkeypatch, capsys):
  """Without --full the run sets up, warms up, times exactly --steps steps in one region and prints the headline: no
  diagnostic pass, no side blocks, no CPU leg (with the clock settle off every step called is a warm-up or a timed one)."""
  calls = {}
  _mock_device(monkeypatch, bench, calls)
  monkeypatch.setattr(bench, 'cpu_baseline', lambda a: pytest.fail('the CPU leg is a --full block'))
  monkeypatch.setenv('WORLD_SIZE', '1')
  monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '7', '--warmup', '3', '--settle', '0'])
  bench.main()
  out = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')]
  assert len(out) == 1
  line = json.loads(out[0])
  assert calls['harm'] == calls['noise'] == 3 + 7 and 'names' not in calls and 'fused' not in calls
  for key in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'steps', 'warmup', 'n_gpus'):
    assert key in line, key
  assert line['steps'] == 7 and line['warmup'] == 3 and line['timing']['repeats'] == 1
  assert line['ms_per_step'] == pytest.approx(1.0 / 7)                 # the one region's event time (1 ms here) over K
  assert line['value'] == pytest.approx(128 * 64000 * 7 / 1e-3 / 1e6) and line['unit'] == 'Msamples/s'
  assert line['roofline']['whole_step']['frac'] > 0 and 'kernel' not in line['roofline']
  for key in ('cpu_baseline', 'kernel_breakdown_us_isolated', 'configs_1', 'configs_2', 'configs_3', 'configs_4',
              'fnoise_11_bit_levels', 'f0_regimes', 'fused_add', 'one_stream', 'shards', 'dumped_outputs'):
    assert key not in line, key


def test_dump_outputs_are_the_last_timed_step_and_the_same_from_run_to_run(bench, monkeypatch, capsys, tmp_path):
  """--dump-outputs DIR: the two arrays the timed path returned from its last step, float32; the noise is keyed by a call
  counter and the clock settle runs for a time, so the counter is rewound before the timed steps - two runs write the same."""
  import numpy as np
  import torch
  import ddsp_amd
  calls = {}
  _mock_device(monkeypatch, bench, calls)

  class _Harmonic:
    def __init__(self, n_samples, sample_rate):
      self.n = n_samples

    def __call__(self, amplitudes, harmonic_distribution, f0_hz):
      return amplitudes.mean(dim=(1, 2))[:, None] * torch.arange(self.n, dtype=torch.float32)

  class _Noise:
    def __init__(self, n_samples, window_size, seed, noise_bits=23):
      self.n, self._calls = n_samples, 0

    def __call__(self, magnitudes):
      self._calls += 1
      return magnitudes.mean(dim=(1, 2))[:, None] + torch.full((magnitudes.shape[0], self.n), float(self._calls))
  monkeypatch.setattr(ddsp_amd.synths, 'Harmonic', _Harmonic)
  monkeypatch.setattr(ddsp_amd.synths, 'FilteredNoise', _Noise)
  monkeypatch.setenv('WORLD_SIZE', '1')
  got = []
  for run in ('a', 'b'):
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '5', '--warmup', '2', '--settle', '0.02', '--batch', '3',
                                      '--n-frames', '10', '--n-samples', '640', '--dump-outputs', str(tmp_path / run)])
    bench.main()
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')][0])
    assert line['dumped_outputs']['harmonic'] == {'file': 'harmonic.npy', 'shape': [3, 640], 'rows': 'all'}
    got.append({name: np.load(str(tmp_path / run / (name + '.npy'))) for name in ('harmonic', 'filtered_noise')})
  x = bench.make_inputs(3, bench.parse_args(['--n-frames', '10']), seed=1000)
  for name, arr in got[0].items():
    assert arr.dtype == np.float32 and arr.shape == (3, 640)
    np.testing.assert_array_equal(arr, got[1][name])
  np.testing.assert_allclose(got[0]['harmonic'][:, 1], x['amplitudes'].mean(axis=(1, 2)), rtol=1e-6)
  np.testing.assert_allclose(got[0]['filtered_noise'][:, 0] - x['magnitudes'].mean(axis=(1, 2)), 5.0, rtol=1e-6)   # call 5 of 5


def test_dump_outputs_keeps_a_seeded_sample_of_rows_within_the_budget(bench, tmp_path):
  import numpy as np
  rng = np.random.default_rng(3)
  arrays = {'harmonic': rng.standard_normal((10, 100)).astype(np.float32), 'filtered_noise': rng.standard_normal((10, 100))}
  info = bench.dump_outputs(str(tmp_path / 'a'), arrays, budget=3000)
  again = bench.dump_outputs(str(tmp_path / 'b'), arrays, budget=3000)
  rows = info['harmonic']['rows']
  assert info == again and rows == info['filtered_noise']['rows'] and rows == sorted(rows) and len(rows) == 3
  total = 0
  for name, x in arrays.items():
    got = np.load(str(tmp_path / 'a' / (name + '.npy')))
    assert got.dtype == np.float32 and info[name]['shape'] == [10, 100]
    np.testing.assert_array_equal(got, x[rows].astype(np.float32))
    total += got.nbytes
  assert total <= 3000
  assert bench.dump_outputs(str(tmp_path / 'c'), arrays)['harmonic']['rows'] == 'all'


def test_plain_dry_run_line_and_dump():
  """The plain command line end to end (dry: no device): one JSON line, exactly K timed steps in one region, outputs written."""
  import tempfile
  import numpy as np
  with tempfile.TemporaryDirectory() as d:
    r = _run_bench('--dry-run', '--steps', '5', '--warmup', '2', '--batch', '2', '--n-frames', '10', '--n-samples', '640',
                   '--dump-outputs', d)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(out) == 1
    line = json.loads(out[0])
    assert line['steps'] == 5 and line['timing']['repeats'] == 1 and line['ms_per_step'] > 0 and 'cpu_baseline' not in line
    assert sorted(os.listdir(d)) == ['filtered_noise.npy', 'harmonic.npy']
    assert np.load(os.path.join(d, 'harmonic.npy')).dtype == np.float32


def test_cpu_baseline_leg_runs_concurrent_workers_and_falls_back(monkeypatch):
  from oracle import cpu_baseline as leg
  r = leg.measure(2, 2, 10, 8, 9, 640, 16000, 200.0, timeout_s=60.0)
  assert r['kind'] == 'port' and r['unit'] == 'Msamples/s' and r['cores'] == 2
  assert r['value'] > 0 and r['single_process_value'] > 0 and '2 concurrent worker' in r['sample']
  assert leg.measure(1, 1, 10, 8, 9, 640, 16000, 200.0)['cores'] == 1
  monkeypatch.setattr(leg.sys, 'executable', '/nonexistent/python')            # workers cannot start
  r = leg.measure(1, 2, 10, 8, 9, 640, 16000, 200.0, timeout_s=10.0)
  assert r['cores'] == 1 and r['value'] == r['single_process_value'] and 'workers failed' in r['sample']
  assert 1 <= leg.default_procs() <= 256


def _run_bench(*argv, timeout=300):
  import subprocess
  env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
  return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(argv), cwd=ROOT, env=env,
                        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)


def test_gpus_2_without_a_launcher_starts_its_own_ranks():
  """`python bench.py --gpus 2` with no torchrun around it becomes the launcher: two ranks through
  torch.distributed.run on 127.0.0.1, rank 0's single JSON line passed through.  --dry-run (gloo, no device, the
  step is a sleep) is the plumbing-test mode: what is checked is the launch, the rank logic, the barriers, the
  max-over-ranks reduction, the all-gather and the shape of the line - no number in it is a measurement."""
  r = _run_bench('--gpus', '2', '--dry-run', '--steps', '5', '--warmup', '2', '--batch', '2', '--n-frames', '10',
                 '--n-samples', '640', '--allgather', '--no-cpu-baseline', '--north-star-batch', '4', '--full')
  assert r.returncode == 0, r.stderr[-2000:]
  out = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
  assert len(out) == 1
  line = json.loads(out[0])
  assert line['n_gpus'] == 2 and line['dry_run'] is True and line['config']['global_batch'] == 4
  assert line['scaling'] == 'weak' and line['per_gpu_value'] == pytest.approx(line['value'] / 2)
  assert 'allgather_ms' in line and line['second_shape']['batch_per_gpu'] == 4
  assert 'cpu_baseline' not in line and line['steps'] == 5 and line['timing']['repeats'] >= 10


def test_default_shape_carries_configs_1_and_configs_4_two_ranks():
  """The default (north-star) shape on two ranks, dry: the line carries `configs_1` (BASELINE configs[1], batch 32) and
  `configs_4` (configs[4] per GPU: 48 kHz, 200 harmonics, 10 s clips, batch 32 - the 129 .. 200-harmonic instances of the
  Harmonic kernel) with the headline's definitions; every rank walks the same collectives through both blocks."""
  r = _run_bench('--gpus', '2', '--dry-run', '--steps', '4', '--warmup', '1', '--no-cpu-baseline', '--full')
  assert r.returncode == 0, r.stderr[-2000:]
  line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][0])
  assert line['config']['batch_per_gpu'] == 128 and line['configs_1']['batch_per_gpu'] == 32
  c4 = line['configs_4']
  assert c4['batch_per_gpu'] == 32 and '200 harmonics' in c4['workload'] and c4['steps'] == 50
  assert c4['whole_step']['algorithmic_bytes'] == 4 * 32 * (2500 * 202 + 480000 + 2500 * 65 + 480000)
  assert c4['value'] == pytest.approx(2 * 32 * 480000 / (c4['ms_per_step'] * 1e-3) / 1e6) and 'one_stream' in c4


def test_eight_ranks_dry_run_shards_of_the_sharded_configs_and_a_separate_gather_time():
  """the 8-GPU launch as the driver makes it, dry (gloo, no device): `n_gpus` = 8, every rank's rows of
  BASELINE's sharded configurations as ddsp_amd.distributed.shard_bounds hands them out - configs[3] 1024 -> 128 per GPU,
  configs[4] 256 -> 32, the headline 1024 -> 128: contiguous, disjoint, covering -, weak scaling, and --allgather reporting the
  gather's time in a field of its own, outside `ms_per_step`."""
  r = _run_bench('--gpus', '8', '--dry-run', '--steps', '3', '--warmup', '1', '--no-cpu-baseline', '--allgather', '--repeats', '3',
                 '--full', timeout=600)
  assert r.returncode == 0, r.stderr[-2000:]
  out = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
  assert len(out) == 1
  line = json.loads(out[0])
  assert line['n_gpus'] == 8 and line['dry_run'] is True and line['scaling'] == 'weak'
  assert line['config']['batch_per_gpu'] == 128 and line['config']['global_batch'] == 1024
  assert line['per_gpu_value'] == pytest.approx(line['value'] / 8)
  for name, gb, per in (('configs_3', 1024, 128), ('configs_4', 256, 32), ('headline', 1024, 128)):
    sh = line['shards'][name]
    assert sh['global_batch'] == gb
    assert sh['rows_of_rank'] == [[per * r_, per * (r_ + 1)] for r_ in range(8)], (name, sh)
  assert line['allgather_ms'] > 0 and 'allgather' not in line['timing']['method']
  assert line['configs_1']['batch_per_gpu'] == 32 and line['configs_4']['batch_per_gpu'] == 32
  assert line['configs_4']['value'] == pytest.approx(8 * 32 * 480000 / (line['configs_4']['ms_per_step'] * 1e-3) / 1e6)


def test_gpus_2_on_a_box_without_two_gpus_refuses_instead_of_reporting_one():
  r = _run_bench('--gpus', '2', '--steps', '5', '--warmup', '2')
  assert r.returncode != 0 and 'refusing' in r.stderr and not [ln for ln in r.stdout.splitlines() if ln.startswith('{')]


def test_pmc_records_are_matched_on_kernel_batch_and_shape(bench, tmp_path, monkeypatch):
  """VERDICT r3, weak #6a: `traffic` of configs[4]'s 126 MB launch was the 16 kHz batch-32 figure - the lookup was keyed on the
  batch alone.  A PMC record is used for a launch of the same kernel at the same batch AND shape."""
  prof = tmp_path / 'profiles'
  prof.mkdir()
  (prof / 'pmc_traffic.json').write_text(json.dumps({'batch': 32, 'kernels': {'harm_table_kernel': 23.5e6}}))
  (prof / 'pmc_traffic_config5.json').write_text(json.dumps({
      'batch': 32, 'shape': {'n_frames': 2500, 'n_harmonics': 200, 'n_samples': 480000, 'sample_rate': 48000},
      'kernels': {'harm_table_kernel': 130e6}}))
  (prof / 'pmc_sq_b128.json').write_text(json.dumps({
      'batch': 128, 'source': 'stub', 'sq': {'harm_table_kernel': {'SQ_INSTS_VALU': 12e6, 'SQ_INSTS_SALU': 4e6, 'SQ_INSTS_LDS': 2e6,
                                                                  'SQ_WAVE_CYCLES': 100e6, 'SQ_WAIT_INST_ANY': 30e6}}}))
  monkeypatch.setattr(bench, 'ROOT', str(tmp_path))
  a = _args(bench)
  assert bench.load_traffic(a, 'harm_table_kernel', 32) == 23.5e6
  assert bench.load_traffic(a, 'harm_table_kernel', 128) is None
  a5 = _args(bench, '--n-frames', '2500', '--n-harmonics', '200', '--n-samples', '480000', '--sample-rate', '48000')
  assert bench.load_traffic(a5, 'harm_table_kernel', 32) == 130e6
  assert bench.load_traffic(a5, 'noise_mfma65_kernel', 32) is None
  ex = bench.load_issue_counters(a, 'harm_table_kernel', 128, 38e-6)
  assert ex['wave_instructions_per_launch'] == 18e6 and ex['per_simd_clock'] == pytest.approx(18e6 / (1024 * 38e-6 * 2.4e9))
  assert ex['wave_cycles_waiting_for_an_instruction'] == pytest.approx(0.3)
  assert bench.load_issue_counters(a5, 'harm_table_kernel', 32, 80e-6) is None
