"""tests/test_gpu_spectral_loss_deterministic.py on the CPU, through the SIMT emulation of tests/hip_emu (TEST INFRASTRUCTURE, see
tests/test_simt_emulated.py).  Fibers run in one order, so the bitwise checks pass trivially here; what this run checks is the
slab indexing of every gradient instance and the gather's covering-block arithmetic - against the analytic oracle and against the
atomic kernels - without GPU time.  The second stream of the first test needs real streams and is left out there.  It does not
replace the `-m gpu` run."""
import test_gpu_spectral_loss_deterministic as G
from tests.hip_emu import emu_simt

ddsp = emu_simt.ddsp_fixture(G)
emu_simt.reexport(globals(), G)

# left to the GPU run: the case with every term AND the loudness term (half a minute a test here; 'loudness_only' runs the same
# loudness geometry - pad_left > 0, nine covering blocks - and the other cases the same term kernels), but for its gradient check
SLOW_UNDER_EMULATION = tuple('%s[loudness_and_all_terms]' % test for test in (
    'test_twice_on_a_fresh_instance_and_beside_another_stream_same_bits', 'test_rows_do_not_see_each_other',
    'test_value_is_the_default_paths_to_the_bits', 'test_backward_twice_with_retain_graph_doubles_the_gradient_exactly',
    'test_torch_deterministic_algorithms_switch_selects_the_slab_path'))
