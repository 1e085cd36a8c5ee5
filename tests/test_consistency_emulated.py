"""The small cases of tests/test_gpu_consistency.py on the CPU, through the SIMT emulation of tests/hip_emu (TEST
INFRASTRUCTURE, see tests/test_simt_emulated.py): kernel logic - LDS staging, tiles, barriers, the per-candidate wavefront sums
and the per-sinusoid sums of the backward passes - checked without GPU time.  It does not replace the `-m gpu` run.

The kernels come from the one emulated library of tests/hip_emu/emu_simt.py, which is built from the product's own list of
sources; the `ddsp` fixture is emu_simt's harness with this module's GPU tests pointed at host memory."""
import test_gpu_consistency as G
from tests.hip_emu import emu_simt

ddsp = emu_simt.ddsp_fixture(G)
emu_simt.reexport(globals(), G)

# left to the GPU run: the 1000-frame and the wide cases (a thread is a fiber here) and the allocator statistic of the device
SLOW_UNDER_EMULATION = ('shipped_k100_c100', 'k1024', 'k257', 'test_peak_memory', 'test_shipped_1000_frames')
