#!/usr/bin/env python3
"""Key set-up times in ONE process: the transparent key of amsm_bases_sample (BLAKE2s try-and-increment on the device) against the
seeded synthetic key of amsm_bases_generate (a 254-step ladder per generator), both with AMSM_BASES_NO_PRECOMPUTE so that only the
generation is compared.  Per curve and size the two calls alternate (clock drift hits both alike): one untimed call of each, then
R timed calls of each, every one a host clock around a call that returns after its device synchronisation; the medians are
reported.  Sizes 2^16, 2^20, 2^22 on the GPU and 2^16 on the host backend.

    python tools/key_setup_rates.py [--reps R] [--sizes 16,20,22] [--host-sizes 16] [--out FILE]

One JSON line per (backend, curve, size) and the source hash of the tree."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def source_hash() -> str:
    """sha256 over the library's sources (as tools/curve_rates.py names the tree it measured)"""
    import hashlib
    hs = hashlib.sha256()
    for d in ("accumulation_amd/csrc", "include", "accumulation_amd"):
        for f in sorted(os.listdir(os.path.join(ROOT, d))):
            p = os.path.join(ROOT, d, f)
            if os.path.isfile(p) and (d != "accumulation_amd" or f.endswith(".py")):
                hs.update(f"{d}/{f}\n".encode())
                hs.update(open(p, "rb").read())
    return hs.hexdigest()[:16]

DOMAIN = b"PC-DL-2020"
SEED = 0x5EED1001


def measure(curve: int, name: str, log2n: int, reps: int, device: int) -> dict:
    from accumulation_amd import CommitterKey, Context, ffi
    ctx = Context(curve, device=device)
    try:
        n, flags = 1 << log2n, ffi.AMSM_BASES_NO_PRECOMPUTE

        def once(what):
            ctx.synchronize()
            t0 = time.perf_counter()
            ck = CommitterKey.sample(ctx, DOMAIN, n, flags) if what == "sample" else CommitterKey.generate(ctx, SEED, n, flags)
            ctx.synchronize()
            dt = time.perf_counter() - t0
            ck.free()
            return dt

        times = {"sample": [], "generate": []}
        for what in times:
            once(what)  # untimed: code objects, first allocations
        for _ in range(reps):
            for what in times:
                times[what].append(once(what))
        med = {k: statistics.median(v) for k, v in times.items()}
        return {"backend": "host" if device < 0 else "gpu", "curve": name, "log2n": log2n, "reps": reps,
                "sample_ms": round(med["sample"] * 1e3, 3), "generate_ms": round(med["generate"] * 1e3, 3),
                "sample_ms_min_max": [round(min(times["sample"]) * 1e3, 3), round(max(times["sample"]) * 1e3, 3)],
                "generate_ms_min_max": [round(min(times["generate"]) * 1e3, 3), round(max(times["generate"]) * 1e3, 3)],
                "sample_over_generate": round(med["sample"] / med["generate"], 3),
                "sample_generators_per_s": round(n / med["sample"])}
    finally:
        ctx.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="16,20,22")
    ap.add_argument("--host-sizes", default="16")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    from accumulation_amd import ffi
    if ffi.load().amsm_device_count() < 1:
        raise SystemExit("key_setup_rates.py needs a GPU: it times the device sampler (the host backend is measured beside it, not instead)")
    curves = ((ffi.AMSM_PALLAS, "pallas"), (ffi.AMSM_VESTA, "vesta"), (ffi.AMSM_BLS12_381_G1, "bls12_381"))
    lines = []
    for device, sizes in ((0, args.sizes), (ffi.AMSM_DEVICE_HOST, args.host_sizes)):
        for log2n in (int(s) for s in sizes.split(",") if s):
            for curve, name in curves:
                line = measure(curve, name, log2n, args.reps, device)
                lines.append(line)
                print(json.dumps(line), flush=True)
    lines.append({"source": source_hash()})
    print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
