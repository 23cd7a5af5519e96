"""The scenarios of tests/commit_failure_cases.py on a host without a device: the pre-state and the
final state of every pending change, as the host images hold them (emulation), equal the independent
oracle of the rule and Service set, and the batch exercises what each scenario is about. The device
tier (tests/test_gpu_commit_failure.py) then compares the slots with these same two references."""
import pytest

from tests import commit_failure_cases as cases


@pytest.mark.parametrize("scn", [s for s in cases.SCENARIOS if s != "replay"])  # (gpc_replay needs the device)
def test_scenario_states_against_the_oracle(scn, monkeypatch):
    points, out = cases.run_case(scn, "b" if scn in ("delta", "svc_only") else "a", cases.HostSide(), monkeypatch)
    assert points == 0 and len(out["final"]["v4"]) == len(out["final"]["v6"]) == cases.N


def test_hook_calls_without_a_context_or_a_call():
    import ctypes as C
    from antrea_amd import gpc
    c = gpc.Classifier()
    n = C.c_uint32(7)
    assert c.lib.gpc_debug_fail_upload_at(None, 0) == -gpc.GPC_EINVAL
    assert c.lib.gpc_debug_upload_points(None, C.byref(n)) == -gpc.GPC_EINVAL
    assert c.lib.gpc_debug_upload_points(c.h, None) == -gpc.GPC_EINVAL
    assert c.debug_upload_points() == 0
    c.debug_fail_upload_at(3)
    c.debug_fail_upload_at(-5)  # disarmed again
    c.close()
