"""tests/test_gpu_vq.py on the CPU, through the SIMT emulation of tests/hip_emu (TEST INFRASTRUCTURE, see
tests/test_simt_emulated.py): kernel logic - the MFMA fragment layout of the packed codebook, the D tails, the per-vector scales,
the running argmin over column tiles and chunks and across lanes, the lowest-index rule, the plain kernel, the ballot walk and the
fixed-order sums of the statistics - checked without GPU time.  The graph-capture case needs a real stream and skips itself here.
It does not replace the `-m gpu` run.

The kernels come from the one emulated library of tests/hip_emu/emu_simt.py, which is built from the product's own list of
sources; the `ddsp` fixture is emu_simt's harness with this module's GPU tests pointed at host memory."""
import test_gpu_vq as G
from tests.hip_emu import emu_simt

ddsp = emu_simt.ddsp_fixture(G)
emu_simt.reexport(globals(), G)
