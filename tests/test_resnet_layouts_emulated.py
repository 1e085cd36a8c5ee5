"""tests/test_gpu_resnet_layouts.py on the CPU, through the SIMT emulation of tests/hip_emu (TEST INFRASTRUCTURE, see
tests/test_simt_emulated.py).  Host memory stands in for HBM here, so the 'cpu' variant is the plain call; the graphed training
step needs a real stream and skips itself.  It does not replace the `-m gpu` run.  The ResNet and encoder rows are the 41
convolutions of ResNet('small'), up to 1024 channels wide, at every variant: 50 s each here, 14 minutes on one core for the module.  The helpers that module borrows from
tests/test_gpu_layouts.py, test_gpu_nonfinite.py, test_gpu_graph_replay.py and test_gpu_resnet.py are pointed at host memory with it."""
import test_gpu_graph_replay as GR
import test_gpu_layouts as GL
import test_gpu_nonfinite as NFT
import test_gpu_resnet as RG
import test_gpu_resnet_layouts as G
from tests.hip_emu import emu_simt

ddsp = emu_simt.ddsp_fixture(G, GL, NFT, GR, RG)
emu_simt.reexport(globals(), G)
