"""tests/test_gpu_backward_state.py on the CPU, through the SIMT emulation of tests/hip_emu (TEST INFRASTRUCTURE, see
tests/test_simt_emulated.py): the host layer's state across calls - workspaces that grow between a forward and its backward, the
noise call counter in ctx.seed, what the autograd nodes save - and the row independence of the backward kernels, checked without
GPU time.  The two-stream case needs real streams and skips itself here.  It does not replace the `-m gpu` run."""
import test_gpu_backward_state as G
from tests.hip_emu import emu_simt

ddsp = emu_simt.ddsp_fixture(G)
emu_simt.reexport(globals(), G)
