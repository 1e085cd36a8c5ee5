"""tests/test_gpu_resnet.py on the CPU, through the SIMT emulation of tests/hip_emu (TEST INFRASTRUCTURE, see
tests/test_simt_emulated.py): kernel logic - the fragment layouts of csrc/conv2d.hip, the flattened K axis and its tail, the
per-lane position map of the convolution and of its adjoint (padding on all four sides, strides, the divisibility test), runs that
cross image rows, the staged weight fragments, the per-row scales, the plain kernel, the autograd node and the wiring of the
ResNet layers and the two encoders - checked without GPU time.  The graph-capture case needs a real stream and skips itself here.
It does not replace the `-m gpu` run."""
import test_gpu_resnet as G
from tests.hip_emu import emu_simt

ddsp = emu_simt.ddsp_fixture(G)
emu_simt.reexport(globals(), G)
