"""Batches the size a prover issues (2, 3, 6 MSMs per call) next to the 40-MSM batches of tools/mid_sizes.py: ms per CALL.
`AMSM_LIB_PATH` selects another build for an A/B.  Not a test.

    python tools/short_batches.py [--curve pallas|bls12_381|vesta|bn254|grumpkin|bls12_377] [--k 1,2,3,6,40] [--jsonl FILE --label NAME] [--scale S] [LOG2 ...]

--jsonl appends one record per (size, k) to FILE, tagged with --label (which build ran): what profiles/bps_batch_ab.jsonl holds."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402

from accumulation_amd import CommitterKey, Context, VariableBaseMSM, ffi  # noqa: E402

CURVES = {"pallas": ffi.AMSM_PALLAS, "bls12_381": ffi.AMSM_BLS12_381_G1, "vesta": ffi.AMSM_VESTA, "bn254": ffi.AMSM_BN254_G1,
          "grumpkin": ffi.AMSM_GRUMPKIN, "bls12_377": ffi.AMSM_BLS12_377_G1}

ap = argparse.ArgumentParser()
ap.add_argument("--curve", default="pallas", choices=sorted(CURVES))
ap.add_argument("--k", default="", help="MSMs per call, comma separated (default 1,2,3,6 and 40, or 12 above 2^20)")
ap.add_argument("--jsonl", default="")
ap.add_argument("--label", default="")
ap.add_argument("--scale", type=int, default=1, help="multiply the timed repetitions (60 // k calls) by this")
ap.add_argument("log2", nargs="*", type=int)
args = ap.parse_args()

for lg in (args.log2 or [16, 18, 20, 22]):
    ctx = Context(CURVES[args.curve])
    n = 1 << lg
    ck = CommitterKey.generate(ctx, 1, n, ffi.AMSM_BASES_PRECOMPUTE)
    vecs = [ctx.random_vector(10 + j, n, mont=True) for j in range(4)]
    out = []
    ks = [int(k) for k in args.k.split(",")] if args.k else [1, 2, 3, 6, 40 if lg <= 20 else 12]
    for k in ks:
        reps = max(3, 60 * args.scale // k)
        for _ in range(3):
            VariableBaseMSM.multi_scalar_mul_batch(ck, [vecs[i % 4] for i in range(k)], mont=True)
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            VariableBaseMSM.multi_scalar_mul_batch(ck, [vecs[i % 4] for i in range(k)], mont=True)
        ms = (time.perf_counter() - t0) / reps * 1e3
        out.append(f"{k} MSMs {ms:.3f} ms")
        if args.jsonl:
            with open(args.jsonl, "a") as f:
                f.write(json.dumps({"tool": "short_batches", "build": args.label, "curve": args.curve, "log2_pairs": lg, "k": k, "reps": reps,
                                    "ms_per_call": round(ms, 4), "M_pairs_per_s": round(k * n / ms / 1e3, 1)}) + "\n")
    print(f"{args.curve} 2^{lg}: " + ", ".join(out), flush=True)
    ck.free()
    ctx.close()
