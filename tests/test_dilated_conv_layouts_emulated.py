"""tests/test_gpu_dilated_conv_layouts.py on the CPU, through the SIMT emulation of tests/hip_emu (TEST INFRASTRUCTURE, see
tests/test_simt_emulated.py).  Host memory stands in for HBM here, so the 'cpu' variant is the plain call.  It does not replace
the `-m gpu` run.  The helpers that module borrows from tests/test_gpu_layouts.py are pointed at host memory with it."""
import test_gpu_dilated_conv_layouts as G
import test_gpu_layouts as GL
from tests.hip_emu import emu_simt

ddsp = emu_simt.ddsp_fixture(G, GL)
emu_simt.reexport(globals(), G)
