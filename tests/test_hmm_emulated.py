"""tests/test_gpu_hmm.py on the CPU, through the SIMT emulation of tests/hip_emu (TEST INFRASTRUCTURE, see
tests/test_simt_emulated.py): kernel logic - the closed-form maximum of a step's observations, the rescaled forward and
backward recursions on DPP reductions, the 256-thread variant's LDS exchange, the transposed back-trace bits and the back
trace itself - checked without GPU time.  It does not replace the `-m gpu` run.

The kernels come from the one emulated library of tests/hip_emu/emu_simt.py, which is built from the product's own list of
sources; the `ddsp` fixture is emu_simt's harness with this module's GPU tests pointed at host memory."""
import test_gpu_hmm as G
from tests.hip_emu import emu_simt

ddsp = emu_simt.ddsp_fixture(G)
emu_simt.reexport(globals(), G)
