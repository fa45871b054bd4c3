"""GPU: every pair of a call against its reference at the batch sizes above the position sweep, up to the largest max_batch
se3tn_create accepts (257 .. SE3TN_MAX_BATCH_LIMIT = 1982 pairs).

Above 256 pairs no tile map changes any more; what grows is the size of whole tensors, and with it every index a kernel forms from
the base of one: `stem` passes 2^31 bytes at 542 pairs and 2^32 at 1084, the F(4x4) V / M planes 2^31 at 1619, the 46 x 46 x 128 trunk
maps end just below 2^31 at the limit.  tests/test_largest_batch_plan.py derives the sizes from the table of tensor sizes and audits
every 32-bit expression of the kernels in Python integers (no GPU); this file runs them.

The checks are those of tests/test_gpu_batch_positions.py, (a) .. (f) of its docstring, through its own helper -- same pool of 12
pairs with float64 logits and stage maps, same seeded slot assignment, every slot its own poseA (1982 distinct poses), the call before
the checked one holding other pairs and other poses in every slot -- on one live context per configuration with max_batch = 1982
(about 17 MB of workspace per pair, 33 GB, one alive at a time).  (d) is the sharp one here: an offset that wraps sends a slot's rows
into another slot or reads them from there, and the seeded draw makes that other data; every word of every stage map of every slot
is compared with the first slot of its pool pair, 128 slots at a time (`stem` alone is 7.9 GB at the limit)."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_batch_positions as BP
import test_largest_batch_plan as LPLAN
import test_gpu_routes as RT

N_MAX = LPLAN.LIMIT
ORDER = ("default", "direct", "f16x3", "F4", "F6", "keep")     # ascending n within a configuration: the first failing size ends a -x run
CASES = [(cfg, n) for cfg in ORDER for n in LPLAN.LARGE_SIZES[cfg]]
WORST = {}      # class -> worst |d logit| against float64 over the sweep
SECONDS = {}    # (cfg, n) -> wall time of the case
PEAK = [0]      # bytes in use on the device (contexts and the test's own tensors), the most seen after a case
T0 = [None]


@pytest.fixture(scope="module")
def se3():
    import se3tracknet_amd
    assert se3tracknet_amd._lib.MAX_BATCH_LIMIT == N_MAX and sorted(ORDER) == sorted(LPLAN.CONFIGS)
    return se3tracknet_amd


@pytest.fixture(scope="module")
def ref():
    """the 12 pool pairs of tests/test_gpu_batch_positions.py and 1982 distinct poses"""
    T0[0] = time.time()
    r = BP.make_ref(N_MAX)
    assert len({p.tobytes() for p in r["poses"]}) == N_MAX
    return r


@pytest.fixture(scope="module")
def live(se3, ref):
    yield from BP.live_contexts(se3, ref, N_MAX)


@pytest.mark.parametrize("cfg,n", CASES, ids=["%s-%d" % c for c in CASES])
def test_every_slot_of_a_call(se3, ref, live, cfg, n):
    assert [lo for lo, _ in LPLAN.chunks(n)] == list(range(0, n, LPLAN.CHUNK))
    BP.check_every_slot_of_a_call(se3, ref, live, cfg, n, WORST, SECONDS, chunk=LPLAN.CHUNK)
    free, total = torch.cuda.mem_get_info()
    PEAK[0] = max(PEAK[0], total - free)


def test_zz_report_worst_logit_error_per_class_over_the_largest_batches():
    """(runs last) the worst |d logit| against float64 per tolerance class over the sweep, beside its bound; the slowest case; the most
    device memory in use after a case"""
    for cls, bound in RT.CLASS_TOL.items():
        print("%-14s worst |d logit| vs float64 %s (bound %.0e)" % (cls, "%.2e" % WORST[cls] if cls in WORST else "not run", bound))
        assert WORST.get(cls, 0.0) <= bound
    if SECONDS:
        slow = max(SECONDS, key=SECONDS.get)
        print("%d cases, slowest %s-%d %.2f s, sum %.1f s, module %.1f s since the reference was started, peak device memory %.1f GB" % (
            len(SECONDS), slow[0], slow[1], SECONDS[slow], sum(SECONDS.values()), time.time() - T0[0], PEAK[0] / 1e9))
