"""Records tests/golden/counter_lifecycle.npz: the Python oracle's verdicts and per-rule metrics of
every batch of the counter-lifecycle scenario (tests/counter_lifecycle.py), each with a digest of the
rules and packets it was computed for. The scenario runs on the host emulation with the live oracle
as its reference, so a recording only succeeds if every assertion of the CPU tier holds against it.
Takes several minutes (the pure-Python oracle over up to 4700 rules, 600 packets per batch).

    python -m tests.golden.make_counter_lifecycle
"""
import os

from tests import counter_lifecycle as cl


def main():
    oracle = cl.Oracle(record=True)
    cl.Scenario(cl.HostSide(), oracle, os.environ.__setitem__, lambda k: os.environ.pop(k, None)).run()
    oracle.save()
    print("%s: %d batches, %d bytes" % (cl.FIXTURE, len(oracle.out) // 3, os.path.getsize(cl.FIXTURE)))


if __name__ == "__main__":
    main()
