#!/usr/bin/env python3
"""Writes tests/golden/bases_sample_v1.json: G_0 .. G_3 of every curve over the domain b"amsm-test", from the big-integer sampler of
tests/sample_ref.py (hashlib's BLAKE2s, pow, the oracle's square root and scalar multiplication) -- no library code.  The file pins
the derivation "amsm-sample-v1" (include/amsm.h: amsm_bases_sample) against silent change; tests/test_bases_sample_cpu.py reads it.

    python tools/gen_bases_sample_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import sample_ref as sr  # noqa: E402

DOMAIN = b"amsm-test"


def main():
    out = {"derivation": "amsm-sample-v1", "domain_hex": DOMAIN.hex(), "curves": {}}
    for name, c in sr.CURVES.items():
        out["curves"][name] = [{"index": i, "attempt": sr.sample_one(c, DOMAIN, i)[1], "x": "%x" % P[0], "y": "%x" % P[1]}
                               for i, P in enumerate(sr.sample(c, DOMAIN, 0, 4))]
    path = os.path.join(ROOT, "tests", "golden", "bases_sample_v1.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path)


if __name__ == "__main__":
    main()
