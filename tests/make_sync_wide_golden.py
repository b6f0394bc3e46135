#!/usr/bin/env python3
"""Makes tests/golden/sync_wide_ref.json: what tests/sync_oracle.js (oracle/harness.js's getMissingChanges + applyChanges) answers for the pair of
test_emu_sync.wide_case_docs() — logs of more than 65 535 changes, which take the oracle half a minute to rebuild three times.  The logs are built in
Python and not stored: the fixture keeps a hash of them, and the tests refuse it when they differ.  Needs node; the tests only read the fixture."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import helpers as H  # noqa: E402
import sync_cases as SC  # noqa: E402

if __name__ == "__main__":
    case = SC.with_oracle(SC.wide_case_docs())
    out = {"inputs_sha16": H.inputs_sha16(case["docs"]), "oracle": case["oracle"]}
    with open(os.path.join(H.GOLDEN, "sync_wide_ref.json"), "w") as f:
        json.dump(out, f, sort_keys=True, separators=(",", ":"))
    print("wrote sync_wide_ref.json:", len(case["oracle"][0]["applied"]), "changes applied in", case["oracle"][0]["attempts"], "attempts")
