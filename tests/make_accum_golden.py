#!/usr/bin/env python3
"""Fixture maker (test infrastructure): what the reference itself (oracle/_ref, types erased by oracle/build_ref.js) answers for the documents of
tests/accum_cases.py that no committed fixture covers yet — the chunk-edge document (its logs are committed with the answer), and spans + text of the 46
KATs and the 9 traces (their logs are committed already; the KAT literals carry no text) — so that tests/test_gpu_accum.py needs neither node nor the
reference on the GPU box.

    python tests/make_accum_golden.py          # writes tests/golden/accum_edges.json
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import accum_cases as AC  # noqa: E402
import helpers as H  # noqa: E402


def main():
    keep = lambda e: {"spans": e["spans"], "text": e["text"]}  # noqa: E731
    log = AC.edges_log()
    kat = AC.kat_and_trace_docs()
    out = {
        "impl": "ref",
        "edges": {"logs": [log], "expected": keep(H.oracle_apply([[log]], impl="ref")[0][0])},
        "kat_inputs": H.inputs_sha16(kat),
        "kat": [[keep(e) for e in d] for d in H.oracle_apply(kat, impl="ref")],
    }
    path = os.path.join(H.GOLDEN, "accum_edges.json")
    with open(path, "w") as f:
        json.dump(out, f)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
