#!/usr/bin/env python3
"""Generate tests/golden/bls12_377_adversarial_points.json: BLS12-377 G1 points whose coordinates sit at the edges the lazy arithmetic
of csrc/ec.h cares about.  The cofactor is not 1 and the key folds use GLV, so the points must lie in the prime-order subgroup: a pool
of 2^16 consecutive multiples of the generator ([1]G .. [2^16]G, one affine addition each with the big-integer oracle) is SEARCHED for
the most extreme coordinates, as tests/golden/make_adversarial_points.py does for BLS12-381.

The device holds a coordinate v as v * 2^392 mod p on 14 limbs of 28 bits (csrc/fpu.h: Bls12377FqU), so every kind is taken twice: on
the INTERNAL value (what the limbs hold) and on the plain integer (what the wire format and the C ABI's words hold).
Kinds, per radix and coordinate (x or y), the PER_KIND nearest points of the pool:
  tiny (towards 0 and 1), near_p (towards p - 1), below_half (towards (p - 1) / 2 from below), above_half ((p + 1) / 2 from above)
and for the internal y, around 2^364 = 2^(B (L - 1)), the bound of the K p - y forms (fpu.h: u_kp_minus_lazy -- K p - y limb by limb
with no carry pass; an internal y below 2^364 occurs once in about 6883 points):
  below_2p364          top limb zero: the smallest and the largest such y of the pool
  just_above_2p364     top limb one, the smallest such y
  top_limb_of_p        top limb equal to p's (0x1ae3): the values nearest p's top limb alone from above
The fixture also holds one pair (l, r) in the shape of tests/golden/bls12_381_negated_doubling.json: r's internal y is below 2^364,
so that l + (r_order - 2) r ends its ladder by doubling the NEGATED r.

Data only; run from the repository root:  python tools/gen_bls12_377_adversarial_points.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pyref as o  # noqa: E402

Z = 0x8508C00000000001
R = Z**4 - Z**2 + 1
P = (Z - 1) ** 2 * R // 3 + Z
GX = 81937999373150964239938255573465948239988671502647976594219695644855304257327692006745978603320413799295628339695
GY = 241266749859715473739788878240585681733927191168601896383759122102112907357779751001206799952863815012735208165030
BLS12_377 = o.Curve("bls12_377_g1", 8, P, R, b=1, gx=GX, gy=GY, limbs=6)
INTERNAL_BITS, LIMB_BITS, LIMBS = 392, 28, 14
TOP = LIMB_BITS * (LIMBS - 1)  # 364
POOL = 1 << 16
PER_KIND = 2


def pool(c, n):
    """[1]G .. [n]G"""
    g = o.generator(c)
    out, acc = [], None
    for _ in range(n):
        acc = o.add(c, acc, g)
        out.append(acc)
    return out


def nearest(pts, key, count=PER_KIND):
    """the `count` points with the smallest non-negative key"""
    return [pt for _, pt in sorted((key(pt), pt) for pt in pts if key(pt) >= 0)[:count]]


def build(c, n_pool=POOL):
    p, half = c.p, (c.p - 1) // 2
    pts = pool(c, n_pool)
    kinds = {}
    for radix, bits in (("internal", INTERNAL_BITS), ("plain", 0)):
        for ci, coord in enumerate(("x", "y")):
            val = lambda pt, ci=ci, bits=bits: (pt[ci] << bits) % p  # noqa: E731
            kinds[f"{radix}_{coord}_tiny"] = nearest(pts, val)
            kinds[f"{radix}_{coord}_near_p"] = nearest(pts, lambda pt: p - 1 - val(pt))
            kinds[f"{radix}_{coord}_below_half"] = nearest(pts, lambda pt: half - val(pt))
            kinds[f"{radix}_{coord}_above_half"] = nearest(pts, lambda pt: val(pt) - (half + 1))
    yi = lambda pt: (pt[1] << INTERNAL_BITS) % p  # noqa: E731
    below = sorted((pt for pt in pts if yi(pt) < 1 << TOP), key=yi)
    assert len(below) >= 4, "the pool holds no internal y below 2^364"
    kinds["internal_y_below_2p364"] = below[:PER_KIND] + below[-PER_KIND:]
    kinds["internal_y_just_above_2p364"] = nearest(pts, lambda pt: yi(pt) - (1 << TOP))
    kinds["internal_y_top_limb_of_p"] = nearest(pts, lambda pt: yi(pt) - ((p >> TOP) << TOP))
    return kinds


def main():
    c = BLS12_377
    kinds = build(c)
    r_pt = kinds["internal_y_below_2p364"][0]
    assert (r_pt[1] << INTERNAL_BITS) % c.p < 1 << TOP
    l_pt = o.mul(c, 0xABCDEF, o.generator(c))
    doc = {"comment": "BLS12-377 G1 affine points of the prime-order subgroup (canonical integers, hex), searched among [1]G .. [2^16]G for "
                      "coordinates nearest 0, p - 1 and (p +- 1) / 2 -- as plain integers and in the device's internal Montgomery radix -- and "
                      "for internal y around 2^364, the bound of the K p - y forms of csrc/ec.h; negated_doubling_pair: l + (r_order - 2) r "
                      "doubles the negated r, whose internal y is below 2^364; made by tools/gen_bls12_377_adversarial_points.py",
           "internal_radix_bits": {c.name: INTERNAL_BITS},
           "curves": {c.name: {k: [[hex(pt[0]), hex(pt[1])] for pt in v] for k, v in kinds.items()}},
           "negated_doubling_pair": {"l": [hex(l_pt[0]), hex(l_pt[1])], "r": [hex(r_pt[0]), hex(r_pt[1])]}}
    path = os.path.join(ROOT, "tests", "golden", "bls12_377_adversarial_points.json")
    # one kind per line: a coordinate has 95 hex digits, and a line per coordinate is no easier to read
    kinds_txt = ",\n".join(f'   {json.dumps(k)}: {json.dumps(v)}' for k, v in doc["curves"][c.name].items())
    head = {k: doc[k] for k in ("comment", "internal_radix_bits")}
    with open(path, "w") as f:
        f.write(json.dumps(head, indent=1)[:-2] + ',\n "curves": {\n  ' + json.dumps(c.name) + ": {\n" + kinds_txt + "\n  }\n },\n"
                ' "negated_doubling_pair": ' + json.dumps(doc["negated_doubling_pair"]) + "\n}\n")
    assert json.load(open(path)) == doc
    print("written", path, sum(len(v) for v in kinds.values()), "points")


if __name__ == "__main__":
    main()
