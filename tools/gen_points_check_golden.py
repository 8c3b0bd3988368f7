#!/usr/bin/env python3
"""Writes tests/golden/points_check_v1.json: per curve, points with the status amsm_points_check (include/amsm.h) must give them,
from the big-integer oracle alone (oracle/pyref.py, the sampler of tests/sample_ref.py, hashlib) -- no library code.

Every entry holds the integers in the limbs of x and of y AS THE C ABI TAKES THEM (Montgomery form, or deliberately not a field
element at all), the infinity byte, the class the point was built as, and the expected status:
    0 valid, 1 non-canonical (x or y >= p), 2 not on the curve, 3 outside the prime-order subgroup (BLS12-381 G1 only).
The statuses written here follow from how each point was CONSTRUCTED; tests/test_points_check_cpu.py derives them a second time from
the definition (integer compare, is_on_curve, mul by r) so that the file cannot go stale silently.

    python tools/gen_points_check_golden.py
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import pyref as o  # noqa: E402
from oracle.pyref_ser import _sqrt  # noqa: E402
from tests import sample_ref as sr  # noqa: E402

DOMAIN = b"amsm-test"
BLS_SMALL_PRIMES = (3, 11, 10177)  # prime factors of the cofactor h = 3 * 11^2 * 10177^2 * 859267^2 * 52437899^2


def raw_curve_point(c, tag: bytes, i: int, b=None):
    """a point of y^2 = x^3 + b (default: the curve's b) from a hashed x, before any cofactor clearing"""
    b = c.b if b is None else b
    j = 0
    while True:
        x = int.from_bytes(hashlib.sha512(tag + b"/%d/%d/%d" % (c.curve_id, i, j)).digest(), "little") % c.p
        y = _sqrt((x * x * x + b) % c.p, c.p)
        if y:
            return (x, y)
        j += 1


def build(name, c):
    R, p = c.R, c.p
    out = []

    def mont(v):
        return v * R % p

    def put(cls, status, x_raw, y_raw, inf=0):
        out.append({"class": cls, "status": status, "inf": inf, "x": "%x" % x_raw, "y": "%x" % y_raw})

    def put_point(cls, status, P):
        put(cls, status, mont(P[0]), mont(P[1]))

    G = o.generator(c)
    # ---- valid ----
    put_point("generator", 0, G)
    put_point("generator_neg", 0, o.neg(c, G))
    for k in range(2, 10 if name != "vesta" else 18):
        put_point("generator_multiple", 0, o.mul(c, o.rng_scalar(0xC4EC, k) % c.r, G))
    for P in sr.sample(c, DOMAIN, 0, 8 if name != "bls12_381" else 4):
        put_point("sampled", 0, P)
    adv_name = {"pallas": "pallas", "bls12_381": "bls12_381_g1"}.get(name)
    if adv_name:  # coordinates at the edges of the device's lazy arithmetic (every K p - y bound): must be accepted
        adv = json.load(open(os.path.join(ROOT, "tests", "golden", "adversarial_points.json")))["curves"][adv_name]
        for kind in sorted(adv):
            for x, y in adv[kind][:2]:
                put_point("adversarial_" + kind, 0, (int(x, 16), int(y, 16)))
    # ---- identity and infinity flag ----
    ones = (1 << (64 * c.limbs)) - 1
    put("identity", 0, 0, 0)
    put("identity_flagged", 0, 0, 0, inf=1)
    put("flagged_garbage", 0, ones, p + 5, inf=1)          # non-canonical words under the flag: ignored
    put("flagged_garbage", 0, mont(G[0]), mont(G[1] + 1), inf=1)  # an off-curve point under the flag: ignored
    # ---- non-canonical ----
    gx, gy = mont(G[0]), mont(G[1])
    for v in (p, p + 1, ones):
        put("non_canonical_x", 1, v, gy)
        put("non_canonical_y", 1, gx, v)
    put("non_canonical_both", 1, p, p)
    put("non_canonical_x_zero_y", 1, p, 0)  # not (0, 0): the words of x are not zero
    # ---- not on the curve ----
    bases = [G, o.mul(c, 7, G), sr.sample(c, DOMAIN, 8, 1)[0]]
    for P in bases:
        put_point("off_curve_y_plus_1", 2, (P[0], (P[1] + 1) % p))
        if P[0] != P[1]:
            put_point("off_curve_swapped", 2, (P[1], P[0]))
    for i in range(3):
        put_point("off_curve_b_plus_1", 2, raw_curve_point(c, b"points-check-b1", i, c.b + 1))
    put_point("off_curve_x_zero", 2, (0, 1))
    put_point("off_curve_y_zero", 2, (1, 0))
    # ---- BLS12-381 G1: on the curve, outside the subgroup ----
    if name == "bls12_381":
        N = sr.BLS_COFACTOR * c.r
        put_point("order_3", 3, (0, 2))
        put_point("order_3", 3, (0, p - 2))
        small = {}
        for ell in BLS_SMALL_PRIMES[1:]:
            pts = []
            for i in range(16):  # ell^2 divides N: [N / ell^2] of a raw curve point has order ell^2, ell or 1
                Q = o.mul(c, N // (ell * ell), raw_curve_point(c, b"points-check-small", 16 * ell + i))
                if o.mul(c, ell, Q) is not None:
                    Q = o.mul(c, ell, Q)
                if Q is not None and Q not in pts and o.neg(c, Q) not in pts:
                    assert o.mul(c, ell, Q) is None
                    pts.append(Q)
                if len(pts) == 3:
                    break
            assert len(pts) >= 2
            small[ell] = pts
            for Q in pts:
                put_point("order_%d" % ell, 3, Q)
                put_point("order_%d" % ell, 3, o.neg(c, Q))
        raws = [raw_curve_point(c, b"points-check-raw", i) for i in range(4)]
        for Rp in raws:
            put_point("raw_hash_to_curve", 3, Rp)
        for Rp in raws[:2]:
            put_point("pure_cofactor", 3, o.mul(c, c.r, Rp))  # [r] of a raw point: in the cofactor's torsion, not in G1
        g1 = [o.mul(c, sr.BLS_COFACTOR, Rp) for Rp in raws[:3]] + [G]
        for P, Q in zip(g1, [(0, 2), small[11][0], small[10177][0], small[11][1]]):
            put_point("g1_plus_small_order", 3, o.add(c, P, Q))
        for P in g1[:3]:  # and the cleared points themselves are in G1
            put_point("cofactor_cleared", 0, P)
    return out


def main():
    doc = {"format": "points_check_v1",
           "comment": "x, y: the integers held in the limbs (hex), Montgomery form unless the class says otherwise; inf: the infinity byte",
           "curves": {name: build(name, c) for name, c in sr.CURVES.items()}}
    path = os.path.join(ROOT, "tests", "golden", "points_check_v1.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(path, {k: len(v) for k, v in doc["curves"].items()})


if __name__ == "__main__":
    main()
