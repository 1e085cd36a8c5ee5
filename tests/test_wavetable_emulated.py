"""The small cases of tests/test_gpu_wavetable.py on the CPU, through the SIMT emulation of tests/hip_emu (TEST
INFRASTRUCTURE, see tests/test_simt_emulated.py): kernel logic - indexing, LDS staging, barriers, the ordered
accumulations of the backward pass - checked without GPU time.  It does not replace the `-m gpu` run.

The kernels come from the one emulated library of tests/hip_emu/emu_simt.py, which is built from the product's own list of
sources; the `ddsp` fixture is emu_simt's harness with this module's GPU tests pointed at host memory."""
import test_gpu_wavetable as G
from tests.hip_emu import emu_simt

ddsp = emu_simt.ddsp_fixture(G)
emu_simt.reexport(globals(), G)

# left to the GPU run: the 64 000-sample clips (a thread is a fiber here) and the lookups of the reference's own sizes
SLOW_UNDER_EMULATION = (
    'class_default', 'test_synths_wavetable_output_shape', 'test_effects_mod_delay_output_shape',
    'test_core_linear_lookup_is_accurate', 'w2048_smooth', 'w2048_rough', 'w64_rough', 'hop192_rough', 'hop192_smooth_w2048',
    'test_core_variable_length_delay_is_accurate',
)
