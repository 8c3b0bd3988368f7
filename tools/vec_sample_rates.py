#!/usr/bin/env python3
"""amsm_vec_sample times in ONE process: the kernel forms of k_vec_sample (AMSM_VEC_SAMPLE_FORM at context creation: tiles of
1024 scalars, the default, or of 4096; profiles/vec_sample_rates.jsonl also holds the lane-per-scalar loop, measured before it was
deleted) beside amsm_vec_random, at 2^18 and 2^20
scalars on Pallas, BLS12-381 and BLS12-377.  Each figure is the minimum of R timed blocking repetitions (a host clock around the call
and the synchronisation that follows) after one untimed call; the forms alternate inside every repetition.  Montgomery output, as the
drivers ask for it.  One JSON line per (curve, size).

    python tools/vec_sample_rates.py [--reps R] [--out profiles/vec_sample_rates.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CURVES = {"pallas": 0, "bls12_381": 1, "bls12_377": 8}
FORMS = {"tile_1024": "1", "tile_4096": "2"}
KEY = bytes(range(32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from accumulation_amd import Context
    lines = []
    for name, cid in CURVES.items():
        ctxs = {}
        for form, env in FORMS.items():
            os.environ["AMSM_VEC_SAMPLE_FORM"] = env
            ctxs[form] = Context(cid)
        os.environ.pop("AMSM_VEC_SAMPLE_FORM", None)
        for log2n in (18, 20):
            n = 1 << log2n
            out = {form: c.vector(n) for form, c in ctxs.items()}
            lib = ctxs["tile_1024"]._lib

            def timed(form, call):
                c = ctxs[form if form in ctxs else "tile_1024"]
                c.synchronize()
                t0 = time.perf_counter()
                call(c)
                c.synchronize()
                return time.perf_counter() - t0

            calls = {form: (lambda c, f=form: lib.amsm_vec_sample(c._h, KEY, 0, 0, n, 1, out[f].ptr)) for form in FORMS}
            calls["vec_random"] = lambda c: lib.amsm_vec_random(c._h, 1, n, 1, out["tile_1024"].ptr)
            for k, f in calls.items():
                timed(k, f)
            best = {k: float("inf") for k in calls}
            for _ in range(args.reps):
                for k, f in calls.items():
                    best[k] = min(best[k], timed(k, f))
            rec = {"kind": "vec_sample_rates", "curve": name, "log2_n": log2n, "reps": args.reps,
                   "min_us": {k: round(v * 1e6, 1) for k, v in best.items()},
                   "ns_per_scalar": {k: round(v * 1e9 / n, 3) for k, v in best.items()}}
            print("JSON " + json.dumps(rec), flush=True)
            lines.append(rec)
            for v in out.values():
                v.free()
        for c in ctxs.values():
            c.close()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
