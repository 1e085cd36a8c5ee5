"""tests/test_gpu_layouts.py on the CPU, through the SIMT emulation of tests/hip_emu (TEST INFRASTRUCTURE, see
tests/test_simt_emulated.py): the Python layer's handling of offset, strided, expanded and non-fp32 tensors, and both sides of
every address-dependent dispatch of csrc/, checked without GPU time.  Host memory stands in for HBM here, so the 'cpu' variant
is the plain call.  It does not replace the `-m gpu` run.

The kernels come from the one emulated library of tests/hip_emu/emu_simt.py, which is built from the product's own list of
sources; the `ddsp` fixture is emu_simt's harness with this module's GPU tests pointed at host memory."""
import test_gpu_layouts as G
from tests.hip_emu import emu_simt

ddsp = emu_simt.ddsp_fixture(G)
emu_simt.reexport(globals(), G)
