#!/usr/bin/env python3
"""Generate tests/golden/bn254_adversarial_points.json (or, with --curve grumpkin, tests/golden/grumpkin_adversarial_points.json for
the other curve of the cycle, whose base field is BN254's r): points whose coordinates sit at the edges the lazy arithmetic of
csrc/ec.h cares about, by the construction of tests/golden/make_adversarial_points.py (pick the coordinate, solve the curve equation
by a cube or square root; the cofactor is 1, so every solution is in the group) for p = BN254's base field.

The device holds a coordinate v as v * 2^261 mod p on 9 limbs of 29 bits (csrc/fpu.h: Bn254FqU, GrumpkinFqU), so "the coordinate" is picked
twice: as the INTERNAL value (what the limbs hold) and as the plain integer (what the wire format and the C ABI's words hold).
Kinds, per coordinate (x or y) and radix -- the nearest value at or beyond the target that gives a point, walking away from the edge:
  at_0, at_1, at_p_minus_1, at_half_minus ((p - 1) / 2), at_half_plus ((p + 1) / 2)
and, for the internal y only, the limb patterns that drive the `K p - y` forms (u_kp_minus_lazy, u_neg_lazy, u_sub_k: formed limb
by limb from a constant whose limbs 0..7 are >= 2^29 - 1, no carry pass; needs y < K p - 2^232) to their bounds:
  low_limbs_all_ones   limbs 0..7 = 2^29 - 1 and top limb 0: the largest value below 2^232 (every limb difference at its minimum)
  top_limb_only        limbs 0..7 = 0, top limb = that of p: the largest multiple of 2^232 below p (every limb difference at its maximum)
  just_above_2p232     the smallest values whose top limb is 1
The fixture also holds one pair (l, r) in the shape of tests/golden/bls12_381_negated_doubling.json: r's internal y is below 2^232,
so that l + (r_order - 2) r ends its ladder by doubling the NEGATED r.

Data only; run from the repository root:  python tools/gen_bn254_adversarial_points.py [--curve bn254_g1|grumpkin]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pyref as o  # noqa: E402
from oracle.pyref_ser import _sqrt  # noqa: E402
from tests.golden.make_adversarial_points import cube_root  # noqa: E402

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BN254 = o.Curve("bn254_g1", 4, P, R, b=3, gx=1, gy=2, limbs=4)
# Grumpkin: y^2 = x^3 - 17 over BN254's scalar field, of order BN254's base-field modulus; generator (1, sqrt(-16))
GRUMPKIN = o.Curve("grumpkin", 6, R, P, b=R - 17, gx=1, gy=0x2CF135E7506A45D632D270D45F1181294833FC48D823F272C, limbs=4)
# curve -> (the oracle's curve, its name in the comment, the fixture's file)
CURVES = {"bn254_g1": (BN254, "BN254 G1", "bn254_adversarial_points.json"),
          "grumpkin": (GRUMPKIN, "Grumpkin", "grumpkin_adversarial_points.json")}
INTERNAL_BITS, LIMB_BITS, LIMBS = 261, 29, 9
PER_KIND = 2


def point_with(c, coord, v):
    """the point whose `coord` is the integer v, or None"""
    p = c.p
    if coord == "y":
        x = cube_root((v * v - c.b) % p, p)
        pt = None if x is None else (x, v)
    else:
        y = _sqrt((v * v * v + c.b) % p, p)
        pt = None if y is None or y == 0 else (v, y)
    return pt if pt is not None and o.is_on_curve(c, pt) else None


def walk(c, coord, radix_bits, start, step):
    """PER_KIND points whose coordinate, times 2^radix_bits mod p, is start, start + step, ... (the first ones that exist)"""
    rinv = pow(1 << radix_bits, -1, c.p)
    out, t = [], start
    while len(out) < PER_KIND:
        assert 0 <= t < c.p
        pt = point_with(c, coord, t * rinv % c.p)
        if pt is not None:
            out.append(pt)
        t += step
    return out


def build(c):
    p = c.p
    kinds = {}
    for radix, bits in (("internal", INTERNAL_BITS), ("plain", 0)):
        for coord in ("x", "y"):
            for name, start, step in (("at_0", 0, 1), ("at_1", 1, 1), ("at_p_minus_1", p - 1, -1), ("at_half_minus", (p - 1) // 2, -1),
                                      ("at_half_plus", (p + 1) // 2, 1)):
                kinds[f"{radix}_{coord}_{name}"] = walk(c, coord, bits, start, step)
    top = LIMB_BITS * (LIMBS - 1)  # 232
    assert (p >> top) << top < p
    kinds["internal_y_low_limbs_all_ones"] = walk(c, "y", INTERNAL_BITS, (1 << top) - 1, -1)
    kinds["internal_y_top_limb_only"] = walk(c, "y", INTERNAL_BITS, (p >> top) << top, 1)
    kinds["internal_y_just_above_2p232"] = walk(c, "y", INTERNAL_BITS, 1 << top, 1)
    return kinds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curve", default="bn254_g1", choices=sorted(CURVES))
    c, title, fname = CURVES[ap.parse_args().curve]
    kinds = build(c)
    r_pt = kinds["internal_y_low_limbs_all_ones"][0]
    assert r_pt[1] * (1 << INTERNAL_BITS) % c.p < 1 << (LIMB_BITS * (LIMBS - 1))
    l_pt = o.mul(c, 0xABCDEF, o.generator(c))
    doc = {"comment": f"{title} affine points (canonical integers, hex) with coordinates at 0, 1, p - 1, (p +- 1) / 2 -- as plain integers "
                      "and in the device's internal Montgomery radix -- and at the limb patterns that bound the K p - y forms of csrc/ec.h; "
                      "negated_doubling_pair: l + (r_order - 2) r doubles the negated r, whose internal y is below 2^232; "
                      "made by tools/gen_bn254_adversarial_points.py",
           "internal_radix_bits": {c.name: INTERNAL_BITS},
           "curves": {c.name: {k: [[hex(pt[0]), hex(pt[1])] for pt in v] for k, v in kinds.items()}},
           "negated_doubling_pair": {"l": [hex(l_pt[0]), hex(l_pt[1])], "r": [hex(r_pt[0]), hex(r_pt[1])]}}
    path = os.path.join(ROOT, "tests", "golden", fname)
    json.dump(doc, open(path, "w"), indent=1)
    print("written", path, sum(len(v) for v in kinds.values()), "points")


if __name__ == "__main__":
    main()
