"""tests/test_gpu_dilated_conv.py on the CPU, through the SIMT emulation of tests/hip_emu (TEST INFRASTRUCTURE, see
tests/test_simt_emulated.py): kernel logic - the fragment layouts of csrc/dilated_conv.hip, the taps' row offsets and the padding
at both ends, the skipped steps, K and column tails, the staged weight fragments, the per-row scales, the adjoint's reversed and
transposed taps, the plain kernel, the autograd node and the stack's wiring - checked without GPU time.  The graph-capture case
needs a real stream and skips itself here.  It does not replace the `-m gpu` run.

The kernels come from the one emulated library of tests/hip_emu/emu_simt.py, which is built from the product's own list of
sources; the `ddsp` fixture is emu_simt's harness with this module's GPU tests pointed at host memory."""
import test_gpu_dilated_conv as G
from tests.hip_emu import emu_simt

ddsp = emu_simt.ddsp_fixture(G)
emu_simt.reexport(globals(), G)
