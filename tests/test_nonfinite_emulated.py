"""tests/test_gpu_nonfinite.py on the CPU, through the SIMT emulation of tests/hip_emu (TEST INFRASTRUCTURE, see
tests/test_simt_emulated.py).  The emulation follows gfx950 where a float becomes an integer (csrc/common.h, cvt_i32_saturating), so
a non-finite value takes the same path through an index here as on the device.  It does not replace the `-m gpu` run.  The helpers
that module borrows from tests/test_gpu_layouts.py are pointed at host memory with it."""
import test_gpu_layouts as GL
import test_gpu_nonfinite as G
from tests.hip_emu import emu_simt

ddsp = emu_simt.ddsp_fixture(G, GL)
emu_simt.reexport(globals(), G)
