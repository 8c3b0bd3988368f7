"""Child process of tests/test_tail_forms_gpu.py (run with AMSM_DEBUG=1, which the library reads once per process): the MSMs of
that test, one marker line on stderr before each so that the parent can tell whose stage lines follow.

    python tests/tail_forms_child.py <inputs.npz> <results.npz>"""
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


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
