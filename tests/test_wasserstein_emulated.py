"""tests/test_gpu_wasserstein.py on the CPU, through the SIMT emulation of tests/hip_emu (TEST INFRASTRUCTURE, see
tests/test_simt_emulated.py): kernel logic - staging, the counting ranks, the scatter, the block scans in both directions and
the gradients written through the ranks - checked without GPU time.  It does not replace the `-m gpu` run.

The kernels come from the one emulated library of tests/hip_emu/emu_simt.py, which is built from the product's own list of
sources; the `ddsp` fixture is emu_simt's harness with this module's GPU tests pointed at host memory."""
import test_gpu_wasserstein as G
from tests.hip_emu import emu_simt

ddsp = emu_simt.ddsp_fixture(G)
emu_simt.reexport(globals(), G)

# left to the GPU run: the allocator statistic of the device
SLOW_UNDER_EMULATION = ('test_peak_memory',)
