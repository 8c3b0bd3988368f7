"""Child process of tests/test_tail_forms_gpu.py (run with AMSM_DEBUG=1, which the library reads once per process): the MSMs of
that test, one marker line on stderr before each so that the parent can tell whose stage lines follow.

    python tests/tail_forms_child.py <inputs.npz> <results.npz>
    python tests/tail_forms_child.py <inputs.npz> <results.npz> <curve id>     the batches of tests/test_skew_gpu.py on that curve"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(inputs, results):
    from accumulation_amd import CommitterKey, Context, VariableBaseMSM, ffi
    d = np.load(inputs)
    out = {}

    def mark(name):
        sys.stderr.write("== %s\n" % name)
        sys.stderr.flush()

    def keep(name, pts, infs):
        out[name + "_xy"] = np.atleast_2d(np.asarray(pts, dtype=np.uint64))
        out[name + "_inf"] = np.atleast_1d(np.asarray(infs, dtype=np.uint8))

    for curve, tag in ((ffi.AMSM_PALLAS, "pallas"), (ffi.AMSM_BLS12_381_G1, "bls12_381")):
        ctx = Context(curve)
        try:
            xy, frs = d[tag + "_xy"], d[tag + "_frs"]
            if tag == "pallas":
                # (a) a plain key, 2^10 pairs, a blocking call
                ck = CommitterKey.load(ctx, xy[:1 << 10], None, ffi.AMSM_BASES_NO_PRECOMPUTE)
                v = ctx.upload(frs[0, :1 << 10])
                mark("a")
                keep("a", *VariableBaseMSM.multi_scalar_mul(ck, v, mont=False))
                ck.free()
            # (b) a precomputed key of 2^15 generators without the direct-sum table, 2^12 pairs, a blocking call
            ck = CommitterKey.load(ctx, xy[:1 << 15], None, ffi.AMSM_BASES_PRECOMPUTE | ffi.AMSM_BASES_NO_DIRECT_TABLE)
            v = ctx.upload(frs[0, :1 << 12])
            mark("b_" + tag)
            keep("b_" + tag, *VariableBaseMSM.multi_scalar_mul(ck, v, mont=False))
            ck.free()
            if tag == "pallas":
                # (c) a device batch of two MSMs of 2^17 + 64 pairs over a plain key of as many generators
                n = (1 << 17) + 64
                ck = CommitterKey.load(ctx, xy[:n], None, ffi.AMSM_BASES_NO_PRECOMPUTE)
                vs = [ctx.upload(frs[j, :n]) for j in range(2)]
                mark("c")
                keep("c", *VariableBaseMSM.multi_scalar_mul_batch(ck, vs, mont=False))
                ck.free()
            mark("end")
        finally:
            ctx.close()
    np.savez(results, **out)


def hidden_tails(inputs, results, curve):
    """two batches of two uniform vectors of 2^18 + 1 pairs each, over generated keys (seed: inputs): "plain", a plain key of as many
    generators, and "table20", the 20-bit key of 2^20 -- the first MSM of a batch has a hidden tail.  The results, and the scalars the
    device drew, go to `results`; table20_skipped is set where the long key finds no memory"""
    from accumulation_amd import CommitterKey, Context, VariableBaseMSM, ffi
    seed = int(np.load(inputs)["seed"])
    n = (1 << 18) + 1
    out = {}
    ctx = Context(curve)
    try:
        for tag, gens, flags in (("plain", n, ffi.AMSM_BASES_NO_PRECOMPUTE), ("table20", 1 << 20, ffi.AMSM_BASES_PRECOMPUTE)):
            try:
                ck = CommitterKey.generate(ctx, seed, gens, flags)
            except ffi.AmsmError as e:
                if tag != "table20" or e.status != ffi.AMSM_E_OOM:
                    raise
                out[tag + "_skipped"] = np.uint8(1)
                continue
            assert tag == "plain" or ck.window_bits == 20
            vs = [ctx.random_vector(seed + 2 + j, n, False) for j in range(2)]
            sys.stderr.write("== %s\n" % tag)
            sys.stderr.flush()
            pts, infs = VariableBaseMSM.multi_scalar_mul_batch(ck, vs, mont=False)
            sys.stderr.write("== end\n")
            sys.stderr.flush()
            out[tag + "_xy"], out[tag + "_inf"] = np.asarray(pts, dtype=np.uint64), np.asarray(infs, dtype=np.uint8)
            out[tag + "_scalars"] = np.stack([v.download() for v in vs])
            for v in vs:
                v.free()
            ck.free()
    finally:
        ctx.close()
    np.savez(results, **out)


if __name__ == "__main__":
    if len(sys.argv) > 3:
        hidden_tails(sys.argv[1], sys.argv[2], int(sys.argv[3]))
    else:
        main(sys.argv[1], sys.argv[2])
