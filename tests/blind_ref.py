"""The derivation "amsm-blind-v1" of amsm_vec_sample (include/amsm.h, accumulation_amd/csrc/blind.h) in plain Python: hashlib's
BLAKE2s and integers.  Scalar i of stream `stream` under `key` on curve `curve_id` is the first candidate t = 0, 1, .. below r of
BLAKE2s-256(key || "amsm-blind-v1" || u8 curve_id || u16_le t || u32_le stream || u64_le i), little-endian, masked to bitlen(r)
bits; after 128 rejections candidate 127 minus r."""
import hashlib
import struct

from accumulation_amd.scalar_field import MODULI

TAG = b"amsm-blind-v1"
MAX_ATTEMPTS = 128


def scalar_attempts(curve_id: int, key: bytes, stream: int, i: int):
    """(the scalar, the number of candidates hashed for it)"""
    assert len(key) == 32
    r = MODULI[curve_id]
    mask = (1 << r.bit_length()) - 1
    for t in range(MAX_ATTEMPTS):
        m = key + TAG + struct.pack("<BHIQ", curve_id, t, stream, i)
        cand = int.from_bytes(hashlib.blake2s(m, digest_size=32).digest(), "little") & mask
        if cand < r:
            return cand, t + 1
    return cand - r, MAX_ATTEMPTS


def scalar(curve_id: int, key: bytes, stream: int, i: int) -> int:
    return scalar_attempts(curve_id, key, stream, i)[0]


def scalars(curve_id: int, key: bytes, stream: int, n: int, first: int = 0):
    return [scalar(curve_id, key, stream, first + j) for j in range(n)]


_K = bytes(range(32))
assert scalar_attempts(0, _K, 0, 0) == (0x34A660FCB1EFB8FB03B22B6E33B1004575500D797C1F476BE61D7C01979B4474, 2)
assert scalar(0, _K, 1, 0) == 0x3853777D453AA15FB27D799C208D0FE14383F7BA3FB5A874C658DE84CC6D2FF0
assert scalar(0, _K, 0, 1 << 32) == 0x26F14FCBBA59A349502F28653BD40CE9ABF7F0263F6B5428AEFE1F3F3EE6BF17
