"""The small cases of tests/test_gpu_sinusoidal.py on the CPU, through the SIMT emulation of tests/hip_emu (TEST
INFRASTRUCTURE, see tests/test_simt_emulated.py): kernel logic - indexing, LDS staging, barriers, the frame-rate scans and
the per-frame sums of the backward pass - checked without GPU time.  It does not replace the `-m gpu` run.

The kernels come from the one emulated library of tests/hip_emu/emu_simt.py, which is built from the product's own list of
sources; the `ddsp` fixture is emu_simt's harness with this module's GPU tests pointed at host memory."""
import test_gpu_sinusoidal as G
from tests.hip_emu import emu_simt

ddsp = emu_simt.ddsp_fixture(G)
emu_simt.reexport(globals(), G)

# left to the GPU run: the 64 000-sample clips (a thread is a fiber here), the peak-memory figure (an allocator statistic of
# the device) and the cross-check against Harmonic, whose direct-sum kernel the emulation takes minutes over
SLOW_UNDER_EMULATION = (
    'shipped_f1000_k100', 'test_synths_sinusoidal_output_shape_is_correct', 'test_peak_memory', 'hop2048',
    'test_sinusoidal_of_harmonic_controls_equals_harmonic', 'test_processor_group_with_sinusoidal',
)
