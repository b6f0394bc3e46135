#!/usr/bin/env python3
"""Makes tests/golden/wide_envelope_ref.json.gz: what the REFERENCE itself (type-erased build oracle/_ref, `--impl ref`) answers for the logs of more
than 65 535 changes that test_emu_biglog.wide_envelope_docs() builds (spans and text of every replica, or the error it throws) and the Changes its
change() makes on test_emu_change.past_65535_replica().  The logs are built in Python and not stored: the fixture keeps a hash of them, and the
tests refuse it when they differ.  Needs node and the reference (oracle/build_ref.js); the tests only read the committed fixture."""
import gzip
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import helpers as H  # noqa: E402
from test_emu_biglog import wide_envelope_docs  # noqa: E402
from test_emu_change import past_65535_replica  # noqa: E402

if __name__ == "__main__":
    docs = wide_envelope_docs()
    exp = H.oracle_apply([docs[k] for k in docs], impl="ref", no_patches=True, timeout=900)
    log, calls = past_65535_replica()
    made = H.oracle_change([[log]], calls, ["a"], impl="ref")
    out = {"impl": "ref", "apply_sha16": H.inputs_sha16(docs), "apply": dict(zip(docs, exp)),
           "change_sha16": H.inputs_sha16({"log": log, "calls": calls}), "change": made}
    with open(os.path.join(H.GOLDEN, "wide_envelope_ref.json.gz"), "wb") as f:  # (gzip: 681 KB of JSON, most of it two long typed texts)
        f.write(gzip.compress(json.dumps(out, sort_keys=True, separators=(",", ":")).encode("utf-8"), 9, mtime=0))
    print("wrote wide_envelope_ref.json.gz:", len(exp), "documents,", len(made), "Changes made")
