"""Shared helpers for the parity tests (numpy <-> oracle conversions)."""
import json
import os

import numpy as np

from oracle import pyref as o

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msm_golden.json")

# The curves beyond the oracle's own table (pyref.CURVES knows 0 and 1 and is curve-generic).  These four objects are built HERE and nowhere
# else under tests/: tests/curve_rows.py holds the per-curve record the shared suites need beside them.
# Pallas's partner in the Pasta cycle (AMSM_VESTA = 2): the two fields swapped.
VESTA = o.Curve("vesta", 2, p=o.PALLAS.r, r=o.PALLAS.p, b=5, gx=o.PALLAS.r - 1, gy=2, limbs=4)

# The BN254 / Grumpkin cycle (AMSM_BN254_G1 = 4, AMSM_GRUMPKIN = 6): each curve's base field is the other's scalar field.
_BN_P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
_BN_R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BN254 = o.Curve("bn254_g1", 4, p=_BN_P, r=_BN_R, b=3, gx=1, gy=2, limbs=4)
GRUMPKIN = o.Curve("grumpkin", 6, p=_BN_R, r=_BN_P, b=_BN_R - 17, gx=1, gy=17631683881184975370165255887551781615748388533673675138860, limbs=4)

# BLS12-377 G1 (AMSM_BLS12_377_G1 = 8): y^2 = x^3 + 1 over a 377-bit field, the one curve here of EVEN order (#E = h r, 2^92 | h).
# tests/test_bls12_377_cpu.py::test_curve_facts re-derives p, r and h from the curve's parameter z and checks this object against them.
BLS12_377_P = 0x1AE3A4617C510EAC63B05C06CA1493B1A22D9F300F5138F1EF3622FBA094800170B5D44300000008508C00000000001
BLS12_377_R = 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001
BLS12_377_H = 0x170B5D44300000000000000000000000  # the cofactor
BLS12_377 = o.Curve("bls12_377_g1", 8, BLS12_377_P, BLS12_377_R, b=1,
                    gx=81937999373150964239938255573465948239988671502647976594219695644855304257327692006745978603320413799295628339695,
                    gy=241266749859715473739788878240585681733927191168601896383759122102112907357779751001206799952863815012735208165030, limbs=6)


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def pt_from_hex(h):
    return None if h is None else (int(h[0], 16), int(h[1], 16))


def points_to_np(c, pts):
    """list of affine points (None = infinity) -> ((n, 2L) uint64 Montgomery, (n,) uint8)."""
    n = len(pts)
    xy = np.zeros((n, 2 * c.limbs), dtype=np.uint64)
    inf = np.zeros((n,), dtype=np.uint8)
    for i, P in enumerate(pts):
        w, f = o.point_to_mont_limbs(c, P)
        xy[i] = np.array(w, dtype=np.uint64)
        inf[i] = f
    return xy, inf


def np_to_point(c, xy, is_inf):
    return o.point_from_mont_limbs(c, [int(v) for v in np.asarray(xy).reshape(-1)], int(bool(is_inf)))


def scalars_to_np(scalars):
    return np.array([o.int_to_limbs(int(s), 4) for s in scalars], dtype=np.uint64).reshape(-1, 4)


def np_to_ints(a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
    return [o.limbs_to_int([int(x) for x in row]) for row in a]


def fr_mont_np(c, vals):
    """canonical ints -> (n,4) uint64 Montgomery (raw Vec<Fr> memory)."""
    return scalars_to_np([o.fr_to_mont(c, int(v) % c.r) for v in vals])


def fr_from_mont_np(c, a):
    return [o.fr_from_mont(c, v) for v in np_to_ints(a)]
