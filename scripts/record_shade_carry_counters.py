"""Record tests/golden/shade_carry_counters.json (needs a GPU).

    MCPT_LIB_PATH=<library of the commit before the carry> python scripts/record_shade_carry_counters.py [out.json]

Runs the GPU cases of tests/test_shade_carry.py against the library MCPT_LIB_PATH
names and writes the counters each case's lean render reported (the test module
collects them in SEEN before it compares them).  The comparisons against the
fixture fail or error in this run when the fixture is missing or stale; the
image and ray-count assertions before them must still hold.
"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


class Recorder:
    def __init__(self, out):
        self.out = out

    def pytest_sessionfinish(self, session):
        import test_shade_carry
        with open(self.out, "w") as f:
            json.dump(dict(sorted(test_shade_carry.SEEN.items())), f, indent=1)
            f.write("\n")
        print("\nrecorded %d cases -> %s" % (len(test_shade_carry.SEEN), self.out))


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "shade_carry_counters.json")
    pytest.main([os.path.join(ROOT, "tests", "test_shade_carry.py"), "-m", "gpu", "-q", "-p", "no:cacheprovider"],
                plugins=[Recorder(out)])
