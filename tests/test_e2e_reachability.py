"""Classifier parity pinned by the reference's own verdict tables: the e2e reachability matrices
and NetworkPolicyEvaluation answers of test/e2e/antreapolicy_test.go / networkpolicy_test.go
(fixture: tests/golden/e2e_reachability.json, extracted and checked against the reference by
tests/golden/make_e2e_reachability.py).

CPU tier: for every step of every case, the oracle (Python OVS classifier over the oracle
compiler's flows) and the product image under the host emulation of the kernel body both give
the reference's expected mark for every probed Pod pair and port, the product's verdicts equal
the oracle's bit for bit, the product flow dump equals the oracle's, and each NPEvaluation
assertion names the policy of the deciding conjunction. The same cases run on the device in
tests/test_gpu_e2e.py.
"""
import pytest

from tests import e2e_run
from tests.util import load_golden

FIX = load_golden("e2e_reachability.json")
CASES = FIX["cases"]


def _check(steps, product_phases=("delta", "compacted")):
    n = 0
    for st in steps:
        assert st["flows_equal"], st["name"]
        for pr in st["pairs"]:
            assert st["oracle"][pr] == st["expected"][pr], (st["name"], pr, "oracle", st["oracle"][pr])
            n += 1
        for ph, (marks, verdicts) in st["product"].items():
            if ph not in product_phases:
                continue
            assert verdicts == st["oracle_verdicts"], (st["name"], ph)
            for pr in st["pairs"]:
                assert marks[pr] == st["expected"][pr], (st["name"], ph, pr)
        for e in st["eval"]:
            assert e2e_run.check_eval(e), (st["name"], e)
    return n


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_e2e_case_oracle_and_emulation(case):
    steps = e2e_run.run_case(case, backend="emu")
    assert _check(steps) > 0


def test_fixture_covers_reference_cases():
    """The fixture was checked against the reference's text (expectations parsed from the cited
    line ranges) and covers the cases the verdict review named (antreapolicy_test.go :412, :688,
    :1719, :1800, :1883, :2125, :2155, :3244) plus the K8s NetworkPolicy suite."""
    assert FIX["steps_checked"] == sum(len(c["steps"]) for c in CASES)
    funcs = {c["go_func"] for c in CASES}
    for f in ("testACNPAllowXBtoA", "testACNPDropIPBlockWithExcept", "testBaselineNamespaceIsolation",
              "testACNPPriorityOverride", "testACNPTierOverride", "testACNPPortRange", "testACNPRejectEgress",
              "testACNPStrictNamespacesIsolation", "testEgressToServerInCIDRBlockWithException"):
        assert f in funcs
    n_eval = sum(len(s["eval"]) for c in CASES for s in c["steps"])
    n_pairs = sum(len(s["expected"]) for c in CASES for s in c["steps"])
    assert n_eval >= 30 and n_pairs >= 5000
    # every antreapolicy_test.go test function that builds a Reachability (48; the fixture records the
    # reference's SHA-256, so this list is the one of that snapshot)
    assert len({c["go_func"] for c in CASES if c["go_file"].endswith("antreapolicy_test.go")}) >= 48
    assert {"testANNPGroupServiceRefPodAdd", "testANNPGroupServiceRefDelete"} <= funcs


def test_fixture_covers_every_reachability_function():
    """Each test function of antreapolicy_test.go that calls NewReachability (helpers excepted) has
    a case in the fixture. The function names were scanned from the reference text when the
    fixture was made (`reachability_functions`, make_e2e_reachability.py)."""
    helpers = {"applyDefaultDenyToAllNamespaces", "cleanupDefaultDenyNPs"}
    has = set(FIX["reachability_functions"])
    assert helpers <= has
    funcs = {c["go_func"] for c in CASES}
    assert has - helpers <= funcs, sorted(has - helpers - funcs)
    assert len(has - helpers) == 48


def test_churn_steps_use_incremental_calls():
    """Group-membership steps reach the product through Add/DeletePolicyRuleAddress (delta
    epochs) and spec changes through Uninstall + Install -- the reference's churn entry points
    (ReassignFlowPriorities is exercised by the fuzz churn of tests/test_fuzz.py)."""
    seen = set()
    for c in CASES:
        if len(c["steps"]) < 2 and c["go_func"] not in ("testACNPPriorityOverride",):
            continue
        for st in e2e_run.run_case(c, backend="emu", compact_last=False):
            seen |= {call[0] for call in st["calls"]}
    assert {"AddPolicyRuleAddress", "DeletePolicyRuleAddress", "UninstallPolicyRuleFlows",
            "InstallPolicyRuleFlows"} <= seen, seen


def test_fixture_matches_transcription():
    """The stored fixture is what the generator writes from the transcription in e2e_cases.py (the
    generator itself refuses to write unless every step equals the reference text it cites; the
    fixture records that text's digests and the number of steps checked)."""
    import json

    from tests.golden import make_e2e_reachability as mk
    out = mk.fixture(FIX["steps_checked"], FIX["reference_files"], FIX["reachability_functions"])
    assert json.loads(json.dumps(out)) == FIX
    assert FIX["steps_checked"] == sum(len(c["steps"]) for c in mk.CASES)
    assert all(len(d) == 64 for d in FIX["reference_files"].values()) and len(FIX["reference_files"]) >= 2
