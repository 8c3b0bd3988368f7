#!/usr/bin/env python3
"""MSM rates of Pallas and Vesta in ONE process, timed the way bench.py times its headline: a generated key (bench.py's point
seed), four resident scalar vectors (its scalar seed) cycled over the steps, PREHEAT untimed MSMs, W warm-up steps, then K steps
issued as one batch call between two device synchronisations.  Sizes 2^16, 2^18, 2^20, each with a precomputed and a plain key;
the two curves alternate per configuration so that clock drift hits both alike.

    python tools/curve_rates.py [--steps K] [--warmup W] [--sizes 16,18,20] [--out FILE]

One JSON line per (curve, size, key) and a summary line with Vesta / Pallas per configuration and the source hash of the tree."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import PREHEAT_MSMS, SEED_POINTS, SEED_SCALARS  # noqa: E402


def source_hash() -> str:
    """sha256 over the library's sources (accumulation_amd/csrc, include, the package's Python files): names the tree measured
    whether or not it is a git checkout"""
    import hashlib
    hs = hashlib.sha256()
    for d in ("accumulation_amd/csrc", "include", "accumulation_amd"):
        for f in sorted(os.listdir(os.path.join(ROOT, d))):
            p = os.path.join(ROOT, d, f)
            if os.path.isfile(p) and (d != "accumulation_amd" or f.endswith(".py")):
                hs.update(f"{d}/{f}\n".encode())
                hs.update(open(p, "rb").read())
    return hs.hexdigest()[:16]


def rate(curve: int, log2n: int, precomp: bool, steps: int, warmup: int) -> dict:
    from accumulation_amd import CommitterKey, Context, VariableBaseMSM, ffi
    ctx = Context(curve)
    try:
        n = 1 << log2n
        ck = CommitterKey.generate(ctx, SEED_POINTS, n, ffi.AMSM_BASES_PRECOMPUTE if precomp else ffi.AMSM_BASES_NO_PRECOMPUTE)
        vecs = [ctx.random_vector(SEED_SCALARS + 1000 * j, n, mont=False) for j in range(4)]
        ctx.synchronize()

        def run_steps(k):
            VariableBaseMSM.multi_scalar_mul_batch(ck, [vecs[i % 4] for i in range(k)], mont=False)

        run_steps(PREHEAT_MSMS)
        run_steps(warmup)
        ctx.synchronize()
        t0 = time.perf_counter()
        run_steps(steps)
        ctx.synchronize()
        elapsed = time.perf_counter() - t0
        for v in vecs:
            v.free()
        ck.free()
        return {"curve": {ffi.AMSM_PALLAS: "pallas", ffi.AMSM_VESTA: "vesta"}[curve], "log2n": log2n,
                "key": "precomputed" if precomp else "plain", "pairs_per_s": n * steps / elapsed, "ms_per_msm": elapsed / steps * 1e3,
                "steps": steps, "warmup": warmup}
    finally:
        ctx.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="16,18,20")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    from accumulation_amd import ffi
    lines, ratio = [], {}
    for log2n in (int(s) for s in args.sizes.split(",")):
        for precomp in (True, False):
            r = {}
            for curve in (ffi.AMSM_PALLAS, ffi.AMSM_VESTA):
                line = rate(curve, log2n, precomp, args.steps, args.warmup)
                r[line["curve"]] = line["pairs_per_s"]
                lines.append(line)
                print(json.dumps(line), flush=True)
            ratio[f"2^{log2n} {'precomputed' if precomp else 'plain'}"] = round(r["vesta"] / r["pallas"], 4)
    summary = {"summary": "vesta / pallas pairs per second", "ratio": ratio, "source": source_hash()}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines + [summary]:
                f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
