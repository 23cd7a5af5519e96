"""GPU tier: a gpc_commit / gpc_compact / gpc_replay that fails at any one of its device allocations,
copies or synchronizes (gpc_debug_fail_upload_at: the error is returned before the device call, nothing
on the device is made to fail) leaves every slot serving the epoch it had, and the next call catches
up. The context, the scenarios, the recovery ways and every check are tests/commit_failure_cases.py;
here its batches run on the two device slots (gpc_classify*_pin_on: verdicts, LB results and the
packet-in queue of both families in one call per family).

Per (scenario, way): one unarmed reference run (device == emulation == oracle; it yields the number of
points the call passes), then for EVERY k below that number a fresh context that fails at point k.
The sweep stops at the first assertion failure; nothing is retried."""
import numpy as np
import pytest

from antrea_amd import gpc
from tests import commit_failure_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    from antrea_amd.build import build
    build()
    import torch
    assert torch.cuda.is_available(), "GPU tier needs a HIP device"


class DeviceSide:
    device = True

    def __init__(self):
        self.cols = {}

    def _columns(self, key, cols):
        """The batch's columns in device memory (the same bits in torch dtypes), copied once."""
        import torch
        if key not in self.cols:
            signed = {4: np.int32, 2: np.int16, 1: np.uint8}
            dev = torch.device("cuda", 0)
            d = {}
            for k, a in cols.items():
                a = np.ascontiguousarray(a, dtype=gpc.PKT_COLUMNS[k])
                d[k] = torch.as_tensor(a.view(signed[a.dtype.itemsize])).to(dev)
            self.cols[key] = d
        return self.cols[key]

    def commit(self, ctx, how):
        ctx.c.compact() if how == "compact" else ctx.c.commit()

    def _family(self, ctx, slot, count, v6):
        import torch
        cols = ctx.w.cols6 if v6 else ctx.w.cols
        n = len(cols["sport"])
        d = self._columns(6 if v6 else 4, cols)
        dev = torch.device("cuda", 0)
        lbsz, cap = (32 if v6 else 16), 2 * n
        buf = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        out, lbo, recs, cnt = buf(16 * n), buf(lbsz * n), buf(16 * cap), buf(8)
        sb = ctx.c.pin_scratch_bytes(n)
        scratch = buf(sb)
        q = gpc.gpc_pin_queue(records=recs.data_ptr(), cap=cap, count=cnt.data_ptr(), scratch=scratch.data_ptr(),
                              scratch_bytes=sb)
        call = ctx.c.classify6_pin_device if v6 else ctx.c.classify_pin_device
        call(gpc.pkt_soa_device(d), n, out.data_ptr(), q, count=count, lb_ptr=lbo.data_ptr(), slot=slot)
        torch.cuda.synchronize()
        total = int(cnt.cpu().numpy().view(np.uint64)[0])
        assert total <= cap
        return (out.cpu().numpy().view(gpc.VERDICT_DTYPE).reshape(n, 2),
                lbo.cpu().numpy().view(gpc.LB6_DTYPE if v6 else gpc.LB_DTYPE),
                recs.cpu().numpy()[:16 * total].view(gpc.PACKET_IN_DTYPE))

    def batch(self, ctx, slot, count):
        v4, lb4, rec4 = self._family(ctx, slot, count, False)
        v6, lb6, rec6 = self._family(ctx, slot, count, True)
        return {"v4": v4, "lb4": lb4, "rec4": rec4, "v6": v6, "lb6": lb6, "rec6": rec6}


SIDE = DeviceSide()
CASES = [(s, w) for s in cases.SCENARIOS for w in cases.WAYS[s]]


@pytest.mark.parametrize("scn,way", CASES, ids=["%s-%s" % c for c in CASES])
def test_failure_at_every_point_then_recovery(scn, way, monkeypatch):
    points, ref = cases.run_case(scn, way, SIDE, monkeypatch)
    assert points >= cases.MIN_POINTS[scn], (points, cases.MIN_POINTS[scn])
    swept = []
    for k in range(points):
        try:
            cases.run_case(scn, way, SIDE, monkeypatch, k=k, ref=ref)
        except AssertionError as e:
            raise AssertionError("%s, way %s, point %d of %d: %s" % (scn, way, k, points, e)) from e
        swept.append(k)
    assert swept == list(range(points))
    print("%s-%s: %d points swept" % (scn, way, points))


def test_point_past_the_last_disarms_and_fail_uploads_keeps_its_meaning(monkeypatch):
    """A skip count the call never reaches does not carry over to the next call; the older hook
    (gpc_debug_fail_uploads: the next n base image uploads) still fails a compaction at its first base
    upload, which is point 0 of that call."""
    ctx = cases.Ctx(SIDE)
    try:
        ctx.call("commit")
        n = ctx.c.debug_upload_points()
        assert n >= cases.MIN_POINTS["first"]
        ctx.c.debug_fail_upload_at(n + 5)
        ctx.call("commit")   # passes fewer points: succeeds, and the hook is spent
        cases.small_change(ctx)
        ctx.call("commit")
        ctx.c.debug_fail_uploads(1)
        with pytest.raises(gpc.GpcError):
            ctx.call("compact")
        assert ctx.c.debug_upload_points() == 1
        ctx.c.debug_fail_uploads(0)
        ctx.call("compact")
        cases.check_resident(ctx)
        r = [ctx.batch(slot) for slot in (0, 1)]
        cases.same(r[0], r[1], "slot 0 against slot 1")
    finally:
        ctx.close()


def test_successful_replay_with_services_packet_in_and_two_slots(monkeypatch):
    """The sibling of test_gpu_boundary.py::test_gpu_replay_rebuilds_device_state for the full context: a
    successful gpc_replay of a delta epoch with Services of both families, learned affinity entries, a
    packet-in image and counts, on two slots -- device == emulation == oracle afterwards, the tables
    learn again, the counters restart, and a delta commit continues on the replayed journals."""
    points, ref = cases.run_case("replay", "c", SIDE, monkeypatch)
    assert points >= cases.MIN_POINTS["replay"]
    ctx = cases.Ctx(SIDE)
    try:
        cases.pre_state("replay", ctx, monkeypatch.setenv)
        epoch = ctx.c.image_stats()["epoch"]
        ctx.call("replay")
        assert ctx.c.image_stats()["epoch"] == epoch + 1
        cases.check_resident(ctx)
        assert ctx.metrics() == {}
        r = [ctx.batch(slot, count=True) for slot in (0, 1)]
        cases.same(r[0], ref["final"], "after the replay against the reference run (itself against the oracle)")
        cases.same(r[0], r[1], "slot 0 against slot 1")
        assert ctx.metrics() == ctx.model_metrics() != {}
        cases.small_change(ctx)
        ctx.call("commit")   # a delta on the replayed journals
        assert ctx.c.image_stats()["n_overlay_rules"] > 0
        r = [ctx.batch(slot) for slot in (0, 1)]
        cases.same(r[0], r[1], "slot 0 against slot 1 after the delta")
        oracle = cases.Oracle()
        oracle.refresh(ctx.w, ctx.c)
        oracle.run(ctx.w)
        cases.same(r[0], oracle.run(ctx.w), "the delta after the replay against the oracle")
    finally:
        ctx.close()
