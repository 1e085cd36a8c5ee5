"""tests/test_gpu_encoder.py on the CPU, through the SIMT emulation of tests/hip_emu (TEST INFRASTRUCTURE, see
tests/test_simt_emulated.py): kernel logic - the lane-to-channel maps of csrc/group_norm.hip for narrow and tiled channel counts,
the chunk-channel moments and their fixed-order merge, the one-block and the split path, the partial rows of the parameter
gradients, the autograd node of core.resample, the encoders' wiring - checked without GPU time.  The graph-capture case needs a
real stream and skips itself here.  It does not replace the `-m gpu` run.

The kernels come from the one emulated library of tests/hip_emu/emu_simt.py, which is built from the product's own list of
sources; the `ddsp` fixture is emu_simt's harness with this module's GPU tests pointed at host memory."""
import test_gpu_encoder as G
from tests.hip_emu import emu_simt

ddsp = emu_simt.ddsp_fixture(G)
emu_simt.reexport(globals(), G)
