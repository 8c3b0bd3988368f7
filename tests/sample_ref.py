"""Reference for the transparent key derivation "amsm-sample-v1" (include/amsm.h: amsm_bases_sample), in big integers:
hashlib's BLAKE2s, pow(), the oracle's Tonelli-Shanks and scalar multiplication.  Shared by the tests of amsm_bases_sample and by
tools/gen_bases_sample_golden.py (which writes tests/golden/bases_sample_v1.json)."""
import hashlib
import struct

from oracle import pyref as o
from oracle import pyref_ser as ser
from tests.helpers import VESTA

PALLAS = o.PALLAS
BLS = o.BLS12_381_G1
CURVES = {"pallas": PALLAS, "bls12_381": BLS, "vesta": VESTA}
BLS_COFACTOR = 0x396C8C005555E1568C00AAAB0000AAAB
MAX_ATTEMPTS = 256


def cofactor(c):
    return BLS_COFACTOR if c.curve_id == BLS.curve_id else 1


def sample_one(c, domain: bytes, i: int):
    """(G_i, the attempt j that gave it)"""
    assert len(domain) <= 32
    bits = c.p.bit_length()
    head = b"amsm-sample-v1" + bytes([c.curve_id, len(domain)]) + domain + struct.pack("<Q", i)
    for j in range(MAX_ATTEMPTS):
        d = b"".join(hashlib.blake2s(head + struct.pack("<IB", j, k)).digest() for k in (0, 1))
        v = int.from_bytes(d, "little")
        x, sign = v & ((1 << bits) - 1), v >> 511
        if x >= c.p:
            continue
        rhs = (x * x * x + c.b) % c.p
        y = ser._sqrt(rhs, c.p)
        if y is None or y == 0:
            continue
        if (y > c.p - y) != bool(sign):
            y = c.p - y
        P = (x, y)
        if cofactor(c) != 1:
            P = o.mul(c, cofactor(c), P)
            if P is None:
                continue
        return P, j
    raise RuntimeError("256 attempts exhausted")


def sample(c, domain: bytes, first: int, n: int):
    return [sample_one(c, domain, first + t)[0] for t in range(n)]


def to_words(c, pts):
    """points -> the C ABI's array (n, 2 * limbs) of Montgomery-form u64 words"""
    import numpy as np
    out = np.zeros((len(pts), 2 * c.limbs), dtype=np.uint64)
    for t, P in enumerate(pts):
        w, inf = o.point_to_mont_limbs(c, P)
        assert not inf
        out[t] = np.array(w, dtype=np.uint64)
    return out
