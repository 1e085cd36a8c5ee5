"""core.Workspace's lifetime rule, on the host: a buffer handed out while the current stream is capturing is never freed by
growth or by the eviction of the least recently used stream, for as long as the Workspace lives; a buffer handed out only
outside a capture is replaced and evicted as it always was.  A captured graph holds the scratch pointer as a kernel argument,
and with the usual pattern (warm up on the capture stream, then capture on it) that pointer is of a buffer from the ordinary
pool: were it freed by a later, larger eager call on that stream, every replay would write its scratch into whatever was
allocated there next.  tests/test_gpu_graph_replay.py holds the same rule on real streams and graphs.

Three stand-ins make the CUDA path of Workspace.get run without a GPU: core._capturing (the one predicate that asks the
runtime whether the current stream is capturing), core._stream_of (the raw handle of the current stream) and torch.empty for a
CUDA device (host memory instead).  Lifetimes are observed through weak references to the returned tensors.

The one-shot `core.Workspace().get(...)` temporaries of effects.py and core.fft_convolve need no such rule and have no test
here: the Workspace, and with it the buffer, is made and dropped inside the call, so under a capture the allocation and the
free both lie inside the capture, in the graph's own memory pool, which the graph keeps for its replays."""
import gc
import sys
import weakref

import pytest
import torch

from ddsp_amd import core

CUDA = torch.device('cuda', 0)
CPU = torch.device('cpu')


class _Runtime:
  """What the stand-ins answer: the current stream's handle, whether it is capturing, and how often that was asked."""

  def __init__(self):
    self.stream, self.capturing, self.asked = 1, False, 0

  def is_capturing(self):
    self.asked += 1
    return self.capturing


@pytest.fixture
def runtime(monkeypatch):
  rt = _Runtime()
  empty = torch.empty

  def empty_on_host(*size, device=None, **kwargs):
    if device is not None and torch.device(device).type == 'cuda':
      device = CPU
    return empty(*size, device=device, **kwargs)
  monkeypatch.setattr(core, '_capturing', rt.is_capturing)
  monkeypatch.setattr(core, '_stream_of', lambda device: rt.stream)
  monkeypatch.setattr(torch, 'empty', empty_on_host)
  return rt


def _alive(ref):
  gc.collect()
  return ref() is not None


def _get_ref(ws, nbytes, device=CUDA):
  """A weak reference to what ws.get hands out (and its size and address): the caller keeps no strong one."""
  buf = ws.get(nbytes, device)
  return weakref.ref(buf), buf.numel(), buf.data_ptr()


def test_a_captured_buffer_outlives_a_larger_request_on_its_key(runtime):
  ws = core.Workspace()
  runtime.capturing = True
  ref, _, _ = _get_ref(ws, 1024)
  runtime.capturing = False
  ws.get(4096, CUDA)                                   # the evaluation batch on the capture stream
  assert _alive(ref), 'the scratch a captured graph points to was freed when its slot grew'


def test_a_captured_buffer_outlives_its_eviction_by_eight_other_streams(runtime):
  ws = core.Workspace()
  runtime.capturing = True
  ref, _, _ = _get_ref(ws, 1024)
  runtime.capturing = False
  for stream in range(2, 2 + core.Workspace.kMaxStreams):
    runtime.stream = stream
    ws.get(1024, CUDA)
  assert (CUDA, 1) not in ws._bufs and len(ws._bufs) == core.Workspace.kMaxStreams      # evicted from the slots, as before
  assert _alive(ref), 'the scratch a captured graph points to was freed when its stream was evicted'


def test_a_captured_buffer_lives_exactly_as_long_as_the_workspace(runtime):
  ws = core.Workspace()
  runtime.capturing = True
  ref, _, _ = _get_ref(ws, 1024)
  runtime.capturing = False
  ws.get(1 << 16, CUDA)
  runtime.stream = 2
  ws.get(1 << 16, CUDA)
  assert _alive(ref)
  del ws
  assert not _alive(ref), 'a captured buffer must die with its Workspace'


def test_eager_buffers_are_released_on_growth_and_never_pile_up(runtime):
  ws = core.Workspace()
  refs = []
  for step in range(64):                               # a loop of growing requests, none under a capture
    refs.append(_get_ref(ws, 1024 * (step + 1))[0])
    gc.collect()
    assert [r() is not None for r in refs] == [False] * step + [True], 'eager use accumulates scratch (step %d)' % step


def test_eager_buffers_are_released_on_eviction(runtime):
  ws = core.Workspace()
  refs = []
  for stream in range(1, 4 * core.Workspace.kMaxStreams + 1):
    runtime.stream = stream
    refs.append(_get_ref(ws, 1024)[0])
    gc.collect()
    alive = [r() is not None for r in refs]
    keep = min(stream, core.Workspace.kMaxStreams)
    assert alive == [False] * (stream - keep) + [True] * keep, 'stream %d: %s' % (stream, alive)


def test_a_buffer_handed_out_a_hundred_times_under_capture_is_retained_once(runtime):
  ws = core.Workspace()
  runtime.capturing = True
  buf = ws.get(1024, CUDA)
  once = sys.getrefcount(buf)
  for _ in range(100):
    assert ws.get(1024, CUDA) is buf and ws.get(512, CUDA) is buf
  assert sys.getrefcount(buf) == once and len(ws._captured) == 1


def test_the_request_after_an_outgrown_captured_buffer_gets_a_new_one_and_keeps_it(runtime):
  ws = core.Workspace()
  runtime.capturing = True
  ref, size, ptr = _get_ref(ws, 1024)
  runtime.capturing = False
  big = ws.get(4096, CUDA)
  assert big.numel() >= 4096 and big.data_ptr() != ptr and _alive(ref)
  for nbytes in (4096, 4096, 1024, 16):
    assert ws.get(nbytes, CUDA) is big                 # equal and smaller requests keep returning that one
  runtime.capturing = True                             # a second capture, on the grown slot: both are kept from now on
  assert ws.get(4096, CUDA) is big
  runtime.capturing = False
  ref_big = weakref.ref(big)
  del big
  ws.get(8192, CUDA)
  assert _alive(ref) and _alive(ref_big)


def test_a_buffer_made_under_capture_is_kept_too(runtime):
  """Growth inside the capture: the new buffer comes from the graph's pool, and the slot must not free it either."""
  ws = core.Workspace()
  ws.get(1024, CUDA)
  runtime.capturing = True
  ref, size, _ = _get_ref(ws, 4096)
  runtime.capturing = False
  assert size >= 4096
  ws.get(1 << 16, CUDA)
  assert _alive(ref)


def test_the_cpu_key_never_asks_whether_a_stream_is_capturing(runtime, monkeypatch):
  def refuse():
    raise AssertionError('the capture predicate was consulted for a CPU tensor')
  monkeypatch.setattr(core, '_capturing', refuse)
  ws = core.Workspace()
  ref, size, _ = _get_ref(ws, 1024, CPU)
  assert size == 1024 and list(ws._bufs) == [(CPU, None)]
  ws.get(4096, CPU)
  assert not _alive(ref)                               # released on growth, as ever


def test_the_null_stream_never_asks_either(runtime):
  """Handle 0 is the null stream, which the runtime refuses to capture (and asking about it while another stream captures in
  the global mode is itself an error that invalidates that capture): the eager default path pays no query."""
  runtime.stream, runtime.capturing = 0, True
  ws = core.Workspace()
  ref, _, _ = _get_ref(ws, 1024)
  ws.get(4096, CUDA)
  assert runtime.asked == 0 and not _alive(ref)
  runtime.stream = 1
  ws.get(1024, CUDA)
  assert runtime.asked == 1


def test_the_predicate_itself_is_not_called_without_a_gpu():
  """Unpatched: the predicate asks the GPU runtime, which a machine without a GPU does not have; the CPU path never reaches it."""
  ws = core.Workspace()
  assert ws.get(100, CPU).numel() == 100 and ws.get(50, CPU).numel() == 100
