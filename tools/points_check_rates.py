#!/usr/bin/env python3
"""Point validation times in ONE process (the protocol of tools/key_setup_rates.py: the variants alternate, one untimed call of each
shape, then R timed calls of each, every one a host clock around a call that ends in a device synchronisation; medians reported):
  (a) amsm_bases_load against amsm_bases_load | AMSM_BASES_CHECK, both AMSM_BASES_NO_PRECOMPUTE
      (Pallas 2^16, 2^20, 2^22; BLS12-381 2^16, 2^20)
  (b) amsm_points_check_device alone on resident points, per curve and size (BLS12-381: the two ladder shapes of
      points_check_kernels.h, each in a context of its own, alternating)
  (c) the host backend's amsm_points_check at 2^16
The kernels' own times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/points_check_rates.py --only b` run.

    python tools/points_check_rates.py [--reps R] [--only a,b,c] [--out profiles/points_check_rates.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.key_setup_rates import source_hash  # noqa: E402

SIZES = {"pallas": (16, 20, 22), "bls12_381": (16, 20)}


def ms(v):
    return round(v * 1e3, 3)


def stats(ts):
    return {"ms": ms(statistics.median(ts)), "ms_min_max": [ms(min(ts)), ms(max(ts))]}


def alternate(variants: dict, reps: int) -> dict:
    times = {k: [] for k in variants}
    for k, f in variants.items():
        f()  # untimed: code objects, first allocations
    for _ in range(reps):
        for k, f in variants.items():
            times[k].append(f())
    return {k: stats(v) for k, v in times.items()}


def measure(curve, name, log2n, reps, only):
    from accumulation_amd import ffi
    from accumulation_amd.engine import CommitterKey, Context, PointVector
    n, NP = 1 << log2n, ffi.AMSM_BASES_NO_PRECOMPUTE
    ctx = Context(curve)
    out = []
    try:
        ck = CommitterKey.generate(ctx, 0x5EED1001, n, NP)
        xy, _ = ck.read()

        def load(flags):
            ctx.synchronize()
            t0 = time.perf_counter()
            k = CommitterKey.load(ctx, xy, flags=flags)
            ctx.synchronize()
            dt = time.perf_counter() - t0
            k.free()
            return dt

        if "a" in only:
            r = alternate({"load": lambda: load(NP), "load_checked": lambda: load(NP | ffi.AMSM_BASES_CHECK)}, reps)
            out.append({"what": "a_load", "curve": name, "log2n": log2n, "reps": reps, **{k + "_" + kk: vv for k, v in r.items() for kk, vv in v.items()},
                        "checked_minus_plain_ms": round(r["load_checked"]["ms"] - r["load"]["ms"], 3)})
        if "b" in only:
            ctxs = {"ladder1": ctx}
            if name == "bls12_381":
                os.environ["AMSM_SUBGROUP_LADDER"] = "2"
                ctxs["ladder2"] = Context(curve)
                del os.environ["AMSM_SUBGROUP_LADDER"]
            vecs = {}
            for k, c in ctxs.items():
                key = ck if c is ctx else CommitterKey.load(c, xy, flags=NP)
                vecs[k] = (PointVector.of_key(key, n), key)

            def dev_check(k):
                c, v = ctxs[k], vecs[k][0]
                c.synchronize()
                t0 = time.perf_counter()
                rep = v.check()
                dt = time.perf_counter() - t0
                assert rep["first_bad"] == n, rep
                return dt

            r = alternate({k: (lambda k=k: dev_check(k)) for k in ctxs}, reps)
            out.append({"what": "b_check_device", "curve": name, "log2n": log2n, "reps": reps,
                        **{k + "_" + kk: vv for k, v in r.items() for kk, vv in v.items()}})
            for k, c in ctxs.items():
                if c is not ctx:
                    vecs[k][1].free()
                    c.close()
        if "c" in only and log2n == 16:
            host = Context(curve, device=ffi.AMSM_DEVICE_HOST)

            def host_check():
                t0 = time.perf_counter()
                rep = host.check_points(xy)
                dt = time.perf_counter() - t0
                assert rep["first_bad"] == n
                return dt

            r = alternate({"host_backend": host_check}, reps)
            out.append({"what": "c_check_host_backend", "curve": name, "log2n": log2n, "reps": reps, "threads": host._lib.amsm_host_threads(),
                        **r["host_backend"]})
            host.close()
        ck.free()
    finally:
        ctx.close()
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="a,b,c")
    ap.add_argument("--max-log", type=int, default=22)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    from accumulation_amd import ffi
    if ffi.load().amsm_device_count() < 1:
        raise SystemExit("points_check_rates.py needs a GPU: it times the device check (the host backend is measured beside it, not instead)")
    ids = {"pallas": ffi.AMSM_PALLAS, "bls12_381": ffi.AMSM_BLS12_381_G1}
    lines = []
    for name, sizes in SIZES.items():
        for log2n in sizes:
            if log2n > args.max_log:
                continue
            for line in measure(ids[name], name, log2n, args.reps, set(args.only.split(","))):
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
