#!/usr/bin/env python3
"""MSM rates of Pallas and the other 9 x 29-bit curves (Vesta, BN254 G1, Grumpkin), or of the two 14 x 28-bit ones (BLS12-381 G1, BLS12-377 G1), in ONE process, timed the way bench.py times its headline: a generated key (bench.py's point
seed), four resident scalar vectors (its scalar seed) cycled over the steps, PREHEAT untimed MSMs, W warm-up steps, then K steps
issued as one batch call between two device synchronisations.  Sizes 2^16, 2^18, 2^20, each with a precomputed and a plain key;
the curves alternate per configuration so that clock drift hits all alike.

    python tools/curve_rates.py [--curves pallas,vesta] [--steps K] [--warmup W] [--sizes 16,18,20] [--keys precomputed,plain]
                                [--only 20:plain,...] [--out FILE]

One JSON line per (curve, size, key) and a summary line with <curve> / Pallas per configuration and the source hash of the tree.
Pallas is always measured: it is the reference point of every ratio."""
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


def curve_ids() -> dict:
    from accumulation_amd import ffi
    return {"pallas": ffi.AMSM_PALLAS, "vesta": ffi.AMSM_VESTA, "bn254_g1": ffi.AMSM_BN254_G1,
            "grumpkin": ffi.AMSM_GRUMPKIN, "bls12_381_g1": ffi.AMSM_BLS12_381_G1, "bls12_377_g1": ffi.AMSM_BLS12_377_G1}


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
        before = ctx.pipeline_stats()
        t0 = time.perf_counter()
        run_steps(steps)
        ctx.synchronize()
        elapsed = time.perf_counter() - t0
        moved = {k: x - before[k] for k, x in ctx.pipeline_stats().items() if x != before[k]}  # which pipeline the timed steps took
        for v in vecs:
            v.free()
        ck.free()
        return {"curve": {v: k for k, v in curve_ids().items()}[curve], "log2n": log2n,
                "key": "precomputed" if precomp else "plain", "pairs_per_s": n * steps / elapsed, "ms_per_msm": elapsed / steps * 1e3,
                "steps": steps, "warmup": warmup, "pipeline_stats": moved}
    finally:
        ctx.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="16,18,20")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--curves", default="pallas,vesta", help="comma-separated: pallas, vesta, bn254_g1, grumpkin, bls12_381_g1, bls12_377_g1")
    ap.add_argument("--base", default="pallas", help="the curve the ratios are taken against (it runs first at every configuration)")
    ap.add_argument("--keys", default="precomputed,plain")
    ap.add_argument("--only", default=None, help="comma-separated size:key pairs to keep of sizes x keys, e.g. 16:precomputed,20:plain")
    args = ap.parse_args()
    ids = curve_ids()
    names = [args.base] + [c for c in args.curves.split(",") if c != args.base]
    only = None if args.only is None else {tuple(x.split(":")) for x in args.only.split(",")}
    lines, ratio = [], {c: {} for c in names[1:]}
    for log2n in (int(s) for s in args.sizes.split(",")):
        for key in args.keys.split(","):
            if only is not None and (str(log2n), key) not in only:
                continue
            r = {}
            for name in names:
                line = rate(ids[name], log2n, key == "precomputed", args.steps, args.warmup)
                r[name] = line["pairs_per_s"]
                lines.append(line)
                print(json.dumps(line), flush=True)
            for name in names[1:]:
                ratio[name][f"2^{log2n} {key}"] = round(r[name] / r[args.base], 4)
    summary = {"summary": f"pairs per second relative to {args.base} in the same run", "ratio": ratio, "source": source_hash()}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines + [summary]:
                f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
