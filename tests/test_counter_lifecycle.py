"""CPU tier of the counter lifecycle (tests/counter_lifecycle.py): the scripted scenario on the host
emulation, so that the GPU tier's run of the same script cannot pass vacuously. What holds without a
device: the slot map shows every release and reuse, the slot counts cross every array size of the
script, counts are non-zero ahead of each growth and for each victim, the emulation's per-batch
metrics equal the oracle's, and the layout hook's error returns."""
import ctypes as C

import pytest

from antrea_amd import gpc, workload
from tests import counter_lifecycle as cl


@pytest.fixture(scope="module", autouse=True)
def _built():
    from antrea_amd.build import build
    build()


def test_layout_hook_without_device_and_errors():
    """gpc_debug_counter_layout: a bad slot or no context is GPC_EINVAL; 0 / 0 before the first commit
    (and on a host without a device, where no array is ever allocated); null outputs are accepted."""
    c = gpc.Classifier()
    cap, copies = C.c_size_t(7), C.c_uint32(7)
    assert c.lib.gpc_debug_counter_layout(c.h, 1, C.byref(cap), C.byref(copies)) == -gpc.GPC_EINVAL
    assert c.lib.gpc_debug_counter_layout(None, 0, C.byref(cap), C.byref(copies)) == -gpc.GPC_EINVAL
    assert (cap.value, copies.value) == (7, 7)
    assert c.lib.gpc_debug_counter_layout(c.h, 0, None, None) == 0
    assert c.debug_counter_layout() == (0, 0)
    c.initialize()
    assert c.debug_counter_layout() == (0, 0)


def test_fixture_first_batch_matches_live_oracle():
    """The recorded oracle results are the live oracle's: batch A (C1 alone, under a second) is
    recomputed; the later batches are tied to their inputs by the digests the replay checks."""
    pool = cl.Pool(n_policies_per_dir=1)
    cols = cl.make_batch([(pool.c1, cl.N)], 110)
    want_v, want_m = cl.live_oracle(pool.c1.rules, cols)
    got_v, got_m = cl.Oracle()("A", pool.c1.rules, cols)
    assert (got_v == want_v).all() and got_m == want_m and want_m


def test_scripted_scenario_on_host(monkeypatch):
    s = cl.Scenario(cl.HostSide(), cl.Oracle(), monkeypatch.setenv, monkeypatch.delenv).run()
    # the slot counts cross 30, 60, 120, 240, 2048, 2 * 2100 in this order, then slots are only reused
    counts = [n for _, n, _ in s.log]
    assert counts[:7] == [30, 55, 95, 155, 2100, 2110, 4215] and set(counts[7:]) == {4215}
    for lo, hi, bound in ((30, 55, 30), (55, 95, 60), (95, 155, 120), (2100, 2110, 2100), (2110, 4215, 4200)):
        assert lo <= bound < hi


def test_pool_is_disjoint_from_c1_and_large_enough():
    pool = cl.Pool()
    ids = [r["flow_id"] for r in pool.free]
    assert min(ids) > 30 and len(set(ids)) == len(ids)
    assert sum(cl.is_counted(r) for r in pool.free) > 4215 - 30 + 2
    assert isinstance(pool.c1, workload.Workload) and [r["flow_id"] for r in pool.c1.rules] == list(range(1, 31))
