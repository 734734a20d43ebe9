#!/usr/bin/env python
"""(Re)write tests/golden/api_errors.json: what every case of tests/api_error_cases.py answers -- return code and lp_last_error() --
from the library this runs against (lightplane_amd/liblightplane_hip.so, or the one LIGHTPLANE_AMD_LIB names).

    python scripts/record_api_errors.py            # rewrite the fixture
    python scripts/record_api_errors.py --diff     # print what differs from the committed fixture, write nothing

No case reaches a kernel (see the module's docstring), so this runs on a machine without a GPU; tests/test_api_errors_host.py holds the
library to the fixture.  A change of lp_api.hip that is meant to leave the ABI's answers alone leaves the fixture alone; one that
rewords a message shows up as that entry's diff."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
FIXTURE = os.path.join(REPO, "tests", "golden", "api_errors.json")


def main():
    from tests import api_error_cases as A

    got = {cid: A.run(cid) for cid in A.CASES}
    if "--diff" in sys.argv:
        with open(FIXTURE) as f:
            old = json.load(f)
        for cid in sorted(set(old) | set(got)):
            if old.get(cid) != got.get(cid):
                print(f"{cid}\n  - {old.get(cid)}\n  + {got.get(cid)}")
        return
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(cid)}: {json.dumps(got[cid])}" for cid in sorted(got)) + "\n}\n")  # one line per case
    print(f"{len(got)} cases -> {FIXTURE}")


if __name__ == "__main__":
    main()
