"""`jtp_joint` survives the failure of each of its allocations (the pattern of `tests/test_gpu_alloc_failures.py`): for N = 1, 2, ...
the N-th allocation of the call reports out of memory (`jtp_debug_set "fail_alloc"`), the call raises `MemoryError` (`JTP_ENOMEM`),
the bytes the library holds are what they were before, and the call that finally goes through returns what a plan that never saw a
failure returns."""
import ctypes as C
import gc

import numpy as np
import pytest

from junctiontree_amd import _capi, engine, synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_cached_plans():
    engine.clear_plan_cache()
    gc.collect()
    yield
    engine.clear_plan_cache()


def live_bytes():
    dev, pin = C.c_int64(-1), C.c_int64(-1)
    _capi.check(_capi.lib().jtp_debug_live_bytes(C.byref(dev), C.byref(pin)))
    return dev.value, pin.value


def loaded(spec):
    plan = engine.Plan(spec["tree"], spec["node_vars"], spec["sizes"], dtype="f64")
    plan.fill_synthetic(3)
    plan.propagate()
    return plan


def test_the_call_survives_the_failure_of_each_of_its_allocations():
    spec = synthetic.wide_binary_tree(n_cliques=7, width=12, sep=6, card=2, seed=1)
    fresh_vars = [[v for v in spec["node_vars"][c] if c == 0 or v not in spec["node_vars"][(c - 1) // 2]] for c in range(7)]
    small, large = [fresh_vars[3][0], fresh_vars[4][1]], [fresh_vars[3][0], fresh_vars[6][1], fresh_vars[5][2], fresh_vars[0][0], fresh_vars[3][3]]
    fresh = loaded(spec)
    want_small, want_large = fresh.joint(small)[0], fresh.joint(large)[0]
    fresh.close()
    plan = loaded(spec)
    failed = 0
    for n in range(1, 16):
        before = live_bytes()
        plan.debug_set("fail_alloc", n)
        try:
            got = plan.joint(small)[0]
        except MemoryError:
            failed += 1
            assert live_bytes() == before, "allocation %d of the call failed and something stayed behind" % n
            continue
        break
    assert failed == n - 1 and failed >= 2, (failed, n)          # the records, the work area
    plan.debug_set("fail_alloc", 0)
    np.testing.assert_array_equal(got, want_small)
    # a larger query grows both buffers: either allocation failing leaves the smaller ones in place, and they still serve
    for n in (1, 2):
        before = live_bytes()
        plan.debug_set("fail_alloc", n)
        with pytest.raises(MemoryError):
            plan.joint(large)
        assert live_bytes() == before
        plan.debug_set("fail_alloc", 0)
        np.testing.assert_array_equal(plan.joint(small)[0], want_small)
    np.testing.assert_array_equal(plan.joint(large)[0], want_large)
    np.testing.assert_array_equal(plan.joint(small)[0], want_small)
    before = live_bytes()
    plan.close()
    assert live_bytes()[0] < before[0]
