"""BLS12-377 G1 (AMSM_BLS12_377_G1 = 8) without a GPU: the facts the port rests on, re-derived; the field tables compiled into the HIP
code; the host scalar-field helpers, the GLV set-up, the 48 / 96 / 32-byte wire format (with a point of the curve outside the
subgroup among the rejections), the Poseidon sponge, host MSMs over the adversarial-point fixture, the key stream, the scalar stream
with its reduced fallback (r has 253 bits), transparent keys (Tonelli-Shanks with 2-adicity 46 on a 12-word field, and an EVEN
cofactor), point validation over the curve's small-order points ((p - 1, 0) of order 2, (0, 1) of order 3, (2, 3) of order 6), the four
schemes on the library's host backend and the C++ drivers' dumps -- each against the big-int oracle with the BLS12-377 `Curve` of
tests/helpers.py (oracle/ knows curves 0 and 1 only and is curve-generic), checked here against the re-derived p, r and h."""
import functools
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyref as o
from oracle import pyref_poseidon as pp
from oracle import pyref_ser as ser
from oracle import pyref_transcript as ot  # noqa: F401  (the transcript tests below run against it)
from tests import helpers as h

Z = 0x8508C00000000001
R = Z**4 - Z**2 + 1
P = (Z - 1) ** 2 * R // 3 + Z
H = (Z - 1) ** 2 // 3  # the cofactor
GX = 81937999373150964239938255573465948239988671502647976594219695644855304257327692006745978603320413799295628339695
GY = 241266749859715473739788878240585681733927191168601896383759122102112907357779751001206799952863815012735208165030
BETA = 0x1AE3A4617C510EABC8756BA8F8C524EB8882A75CC9BC8E359064EE822FB5BFFD1E945779FFFFFFFFFFFFFFFFFFFFFFF
BLS12_377 = h.BLS12_377  # the one definition (tests/helpers.py; tests/field_model.py takes it from there too)
C = BLS12_377
assert (C.name, C.curve_id, C.p, C.r, C.b, C.gx, C.gy, C.limbs) == ("bls12_377_g1", 8, P, R, 1, GX, GY, 6) and h.BLS12_377_H == H
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "accumulation_amd", "csrc")
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "bls12_377_adversarial_points.json")))
P_LIMBS_28 = [1, 0x8C0000, 0x85, 0x5D44300, 0x800170B, 0x2FBA094, 0xF1EF362, 0xF5138, 0xA22D9F3, 0xA1493B1, 0xB05C06C, 0x10EAC63,
              0xA4617C5, 0x1AE3]
FALLBACK_INDICES = (2008, 14921, 38735, 45849, 61982)  # seed 1, below 2^16: the scalars whose 64 candidates are all >= r


@pytest.fixture
def by_name(monkeypatch):
    """the curve-parametrised modules look curves up by name in the oracle's table: add BLS12-377 for the duration of one test"""
    monkeypatch.setitem(o.CURVES, C.name, C)
    monkeypatch.setitem(o.CURVES_BY_ID, C.curve_id, C)


@pytest.fixture
def host_ctx(built_lib):
    from accumulation_amd import Context, ffi
    ctx = Context(ffi.AMSM_BLS12_377_G1, device=ffi.AMSM_DEVICE_HOST)
    yield ctx
    ctx.close()


def two_adicity(m):
    return ((m - 1) & -(m - 1)).bit_length() - 1


# ---- the facts (the issue's list, re-derived) -------------------------------------------------------------------------------------------
def test_curve_facts():
    g = o.generator(C)
    assert Z.bit_length() == 64 and bin(Z).count("1") == 7 and Z > 0
    assert R == 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001 and R.bit_length() == 253 and two_adicity(R) == 47
    assert P == 0x1AE3A4617C510EAC63B05C06CA1493B1A22D9F300F5138F1EF3622FBA094800170B5D44300000008508C00000000001
    assert P.bit_length() == 377 and P % 4 == 1 and two_adicity(P) == 46 and P % 3 == 1 and R % 3 == 1
    assert (Z - 1) ** 2 % 3 == 0 and (Z - 1) ** 2 * R % 3 == 0  # the divisions above are exact
    assert H == 0x170B5D44300000000000000000000000 and H.bit_length() == 125 and H % (1 << 92) == 0 and (H >> 92) % 2 == 1
    # #E = h r is the curve's order: by Hasse's bound it is the only multiple of r near p + 1, and it kills a point outside G1
    assert abs(H * R - (P + 1)) <= 2 * math.isqrt(P) + 1
    assert o.is_on_curve(C, g) and o.mul(C, R, g) is None
    assert pow(2, R - 1, R) == 1 and pow(3, R - 1, R) == 1 and pow(2, P - 1, P) == 1 and pow(3, P - 1, P) == 1  # Fermat witnesses
    # the endomorphism: beta is a primitive cube root of unity and [z^2] G = (beta Gx, -Gy), i.e. phi = -[z^2] on G1
    z2 = Z * Z
    assert z2 == 0x452217CC900000010A11800000000001 and z2.bit_length() == 127 and bin(z2).count("1") == 22
    assert 1 < BETA < P and pow(BETA, 3, P) == 1
    assert o.mul(C, z2, g) == (BETA * GX % P, P - GY)
    # head-room of a tight value and the exact condition of u_kp_minus_lazy
    assert (1 << 392) // P == 38996 and P > 6883 * (1 << 364) and P >> 364 == 6883
    for K in (2, 4, 10, 16):  # y < (K - 1) p  =>  y < K p - 2^364
        assert (K - 1) * P <= K * P - (1 << 364)
    assert math.gcd(17, P - 1) == 1  # the sponge's alpha = 17 permutes Fq
    assert ser.point_size(C, True) == 48 and ser.point_size(C, False) == 96 and ser.fp_size(R) == 32  # 377 + 2 bits; 253 bits
    # small-order points of E
    for pt, order in (((P - 1, 0), 2), ((0, 1), 3), ((2, 3), 6)):
        assert o.is_on_curve(C, pt) and o.mul(C, order, pt) is None
        assert all(o.mul(C, d, pt) is not None for d in range(1, order))
        assert o.mul(C, R, pt) is not None  # outside the prime-order subgroup
    assert o.mul(C, 3, (2, 3)) == (P - 1, 0)
    # the scalar stream: acceptance per 255-bit candidate, the fallback's probability, and how far its value can exceed r
    assert abs(R / (1 << 255) - 0.146) < 0.001 and abs((1 - R / (1 << 255)) ** 64 - 4.1e-5) < 1e-6
    assert 3 * R < (1 << 254) < 4 * R  # at most three subtractions reduce a 254-bit value
    assert R >> 240 == 0x12AB  # the narrowest top 16-bit window so far (BN254: 0x3064)


def test_modulus_shape_in_radix_2p28():
    """limb 0 is 1 (NINV = 2^28 - 1: the p_0 = 1 branch of csrc/fpu.h at B = 28, L = 14), no limb is zero, none above limb 0 is a power
    of two, and the column sums of the 14-limb shape fit 64 bits"""
    limbs = [(P >> (28 * i)) & ((1 << 28) - 1) for i in range(14)]
    assert limbs == P_LIMBS_28 and limbs[0] == 1
    assert all(v != 0 for v in limbs) and all(v & (v - 1) != 0 for v in limbs[1:])
    assert (-pow(P, -1, 1 << 28)) % (1 << 28) == (1 << 28) - 1
    lazy, tight = (1 << 29) - 1, (1 << 28) - 1
    carry = 1 << 36
    assert 14 * lazy * tight + 13 * tight * tight + carry < 1 << 62  # one product, one lazy operand, 13 reduction products
    assert 28 * lazy * tight + 13 * tight * tight + carry + (1 << 32) < 1 << 63  # u_mul_add_mul, an addend riding along


def _tables(src, name, limbs, bits):
    blk = src[src.index("struct " + name + " {"):]
    blk = blk[:blk.index("};")]

    def tab(t):
        mm = re.search(r"AMSM_TABLE\(" + t + r", \d+, ([^)]*)\)", blk, re.S)
        vals = [int(x.strip().rstrip("u"), 16) for x in mm.group(1).replace("\n", " ").split(",")]
        assert len(vals) == limbs and all(v < (1 << bits) for v in vals)
        return sum(v << (bits * i) for i, v in enumerate(vals))
    return blk, tab


@pytest.mark.parametrize("name,m,words", [("Bls12377Fq", P, 12), ("Bls12377Fr", R, 8)])
def test_saturated_tables(name, m, words):
    src = open(os.path.join(CSRC, "fp.h")).read()
    blk, tab = _tables(src, name, words, 32)
    Rm = 1 << (32 * words)
    assert tab("mod") == m and tab("one") == Rm % m and tab("r2") == Rm * Rm % m
    assert int(re.search(r"INV = (0x[0-9a-f]+)u", blk).group(1), 16) == (-pow(m, -1, 1 << 32)) % (1 << 32) == 0xFFFFFFFF
    assert [int(x) for x in re.findall(r"int (?:L|W) = (\d+);", blk)] == [words, words]
    assert "struct DevField<Bls12377Fq>" in src


def test_unsaturated_table():
    blk, tab = _tables(open(os.path.join(CSRC, "fpu.h")).read(), "Bls12377FqU", 14, 28)
    R_abi, R_dev = 1 << 384, 1 << 392
    assert [int(x) for x in re.findall(r"int (?:L|W|B) = (\d+);", blk)] == [14, 12, 28]
    assert tab("mod") == P and tab("one") == R_dev % P
    assert tab("k_import") == R_dev * R_dev * pow(R_abi, -1, P) % P and tab("k_export") == R_abi % P
    ninv = int(re.search(r"NINV = (0x[0-9a-f]+)u", blk).group(1), 16)
    assert ninv == (-pow(P, -1, 1 << 28)) % (1 << 28) == 0x0FFFFFFF == (1 << 28) - 1  # the p_0 = 1 reduction step
    assert "using Sat = Bls12377Fq;" in blk


def test_curve_table():
    """csrc/curves.h: b, the generator, the cofactor and the subgroup ladder's constants, against big integers"""
    src = open(os.path.join(CSRC, "curves.h")).read()
    blk = src[src.index("struct Bls12377Curve {"):]
    blk = blk[:blk.index("\n};")]

    def words(name, bits):
        mm = re.search(name + r"(?:\[\d+\] = \{|, \d+, )([^;)}]*)", blk)
        vals = [int(x.strip().rstrip("ul"), 16) for x in mm.group(1).replace("\n", " ").split(",")]
        return sum(v << (bits * i) for i, v in enumerate(vals))
    assert "int b = 1;" in blk and "subgroup_check = true" in blk and "id = AMSM_BLS12_377_G1" in blk
    assert words("gx", 64) == GX and words("gy", 64) == GY and words("cofactor", 64) == H and words("beta", 64) == BETA
    assert words("z_word", 32) == Z and words("z2_word", 32) == Z * Z
    assert re.search(r"z_bits = (\d+), z2_bits = (\d+)", blk).groups() == ("64", "127")
    # BLS12-381's constants moved into its entry unchanged
    b381 = src[src.index("struct Bls12381Curve {"):src.index("struct VestaCurve")]
    assert "0x00010000u, 0xd2010000u" in b381 and "0x00000000u, 0x00000001u, 0x0001a402u, 0xac45a401u" in b381
    assert "z_bits = 64, z2_bits = 128" in b381 and "0x2e01fffffffefffeull" in b381


def test_pack_names_stay_in_the_field_headers():
    """everything else follows through SatOf, DevField, CurveOf and the templates; the new unit names no pack of another curve, and
    the subgroup test's constants are no longer BLS12-381's alone"""
    for f in sorted(os.listdir(CSRC)):
        if f in ("fp.h", "fpu.h", "fp_mul_gfx950.h"):
            continue
        src = open(os.path.join(CSRC, f)).read()
        assert "Bls12377FqU" not in src, f
        if f not in ("curves.h", "kern_bls12_377.hip", "kern_fr.hip", "api_types.h"):  # the table, the two units, the sponge's state tuple
            assert "Bls12377F" not in src, f
    unit = open(os.path.join(CSRC, "kern_bls12_377.hip")).read()
    assert "Bls12381" not in unit and "AMSM_FQ Bls12377Fq" in unit and "AMSM_FR Bls12377Fr" in unit and "AMSM_CURVE_ID 8" in unit
    assert "AMSM_FR_LAUNCHERS(Bls12377Fr)" in open(os.path.join(CSRC, "kern_fr.hip")).read()
    for f in ("points_check_kernels.h", "host_points_check.h"):
        src = open(os.path.join(CSRC, f)).read()
        assert "bls_z" not in src and "BLS12_381_BETA" not in src and "0xd2010000u" not in src, f
    from accumulation_amd import build
    assert "kern_bls12_377.hip" in build.UNITS


def test_generated_multiplication_header_is_current():
    out = subprocess.run(["python3", os.path.join(ROOT, "tools", "gen_fp_asm.py")], capture_output=True, text=True, check=True).stdout
    assert out == open(os.path.join(CSRC, "fp_mul_gfx950.h")).read()
    for fn in ("fe_mul<Bls12377Fq>", "fe_mul<Bls12377Fr>", "fe_dot2<Bls12377Fr>", "fe_dot3<Bls12377Fr>"):
        assert fn in out, fn
    assert "fe_dot2<Bls12377Fq>" not in out and "fe_dot3<Bls12377Fq>" not in out  # no curve's scalar field
    for name, m, words in (("fe_mul<Bls12377Fq>", P, 12), ("fe_dot3<Bls12377Fr>", R, 8)):
        body = out[out.index("> " + name):]
        body = body[:body.index("return r;")]
        assert all(f"0x{(m >> (32 * j)) & 0xFFFFFFFF:08x}u" in body for j in range(1, words))  # every limb above p_0 = 1 in its reduction


# ---- the curve id ----------------------------------------------------------------------------------------------------------------------
def test_id_8_is_accepted_where_3_5_and_7_are_refused(built_lib):
    from accumulation_amd import ffi
    from accumulation_amd.engine import Context
    assert ffi.AMSM_BLS12_377_G1 == 8
    a = np.ones(4, dtype=np.uint64)
    for bad in (3, 5, 7, 9):
        with pytest.raises(Exception):
            Context(bad, device=ffi.AMSM_DEVICE_HOST)
        assert built_lib.amsm_fr_to_mont(bad, a.ctypes.data, 1, a.ctypes.data) == ffi.AMSM_E_INVALID_ARG
        assert built_lib.amsm_point_serialized_size(bad, 1) == 0 and built_lib.amsm_fr_serialized_size(bad) == 0
    ctx = Context(8, device=ffi.AMSM_DEVICE_HOST)
    assert ctx.curve == 8 and ctx.fq_limbs == 6
    ctx.close()
    assert built_lib.amsm_fr_to_mont(8, a.ctypes.data, 1, a.ctypes.data) == ffi.AMSM_OK
    assert o.limbs_to_int([int(v) for v in a]) == o.fr_to_mont(C, 1 + (1 << 64) + (1 << 128) + (1 << 192))
    assert built_lib.amsm_fr_serialized_size(8) == 32
    assert built_lib.amsm_point_serialized_size(8, 1) == 48 and built_lib.amsm_point_serialized_size(8, 0) == 96


def test_python_tables():
    from accumulation_amd import AMSM_BLS12_377_G1, ipa_pc
    from accumulation_amd.scalar_field import MODULI, Fr
    assert AMSM_BLS12_377_G1 == 8 and MODULI[AMSM_BLS12_377_G1] == R
    assert ipa_pc.IPA_FOLD[AMSM_BLS12_377_G1] == ipa_pc.IPA_FOLD[1] == (16, 15)  # BLS12-381's, unmeasured
    hpp = open(os.path.join(ROOT, "include", "amsm.hpp")).read()
    assert re.search(r"case AMSM_BLS12_377_G1: return \{6, 16, 15\};", hpp)
    assert re.search(r"AMSM_BLS12_377_G1 = 8,", open(os.path.join(ROOT, "include", "amsm.h")).read())
    fr = Fr(AMSM_BLS12_377_G1)
    assert fr.from_limbs(fr.to_limbs(R - 1)) == R - 1


# ---- host helpers ----------------------------------------------------------------------------------------------------------------------
def test_fr_helpers(built_lib):
    from tests import test_host_fr_cpu as t
    t.test_host_fr_helpers(built_lib, C)
    t.test_host_fr_inverse_many(built_lib, C)


def test_host_lincomb(built_lib):
    from tests import test_host_fr_cpu as t
    t.test_host_lincomb_vs_oracle(built_lib, C)
    t.test_host_lincomb_batch_equals_single_calls_and_oracle(built_lib, C)


def test_glv_pairing_and_split():
    """host_glv.h on BLS12-377: lambda and beta pair up, [lambda] G = (beta Gx, Gy), and edge scalars split into short halves that
    give the same point (tests/cpp_host/bls12_377_glv_check.cpp)"""
    out = os.path.join(ROOT, "build", "bls12_377_glv_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["hipcc", "-std=c++17", "-O2", "--offload-host-only", "--offload-arch=gfx950", "-x", "hip", "-w",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp_host", "bls12_377_glv_check.cpp"), "-o", out])
    res = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lam, beta = (int(x, 16) for x in re.search(r"lambda (\w+) beta (\w+)", res.stdout).groups())
    g = o.generator(C)
    assert 1 < lam < R and 1 < beta < P and pow(lam, 3, R) == 1 and pow(beta, 3, P) == 1
    assert o.mul(C, lam, g) == (beta * g[0] % P, g[1])
    assert "OK" in res.stdout


# ---- wire format -----------------------------------------------------------------------------------------------------------------------
def outside_subgroup_point():
    """the first x = 1, 2, ... with a point on the curve that [r] does not kill"""
    x = 1
    while True:
        y = ser._sqrt((x * x * x + C.b) % P, P)
        if y is not None and y != 0 and o.mul(C, R, (x, y)) is not None:
            return x, y
        x += 1


def test_wire_format(built_lib, by_name):
    from tests import test_wire_format_cpu as t
    t.test_scalars(built_lib, C.name)
    for compressed in (True, False):
        t.test_points(built_lib, C.name, compressed)
    t.test_rejections(built_lib, C.name)
    assert built_lib.amsm_fr_serialized_size(8) == ser.fp_size(R) == 32
    assert built_lib.amsm_point_serialized_size(8, 1) == ser.point_size(C, True) == 48
    assert built_lib.amsm_point_serialized_size(8, 0) == ser.point_size(C, False) == 96


def test_flag_bits_and_rejections(built_lib):
    from tests.test_wire_format_cpu import lib_points_deserialize, lib_points_serialize
    g, ng = o.generator(C), o.neg(C, o.generator(C))
    (blob,), sz = lib_points_serialize(built_lib, C, [g], True)
    assert sz == 48 and blob == ser.point_serialize(C, g) and lib_points_deserialize(built_lib, C, [blob], True) == (0, [g])
    (nblob,), _ = lib_points_serialize(built_lib, C, [ng], True)
    # x is 377 bits: it ends in bit 0 of the last byte, the flags sit in bits 7 and 6 of that byte
    assert blob[:47] == nblob[:47] and blob[47] ^ nblob[47] == 0x80 and (blob[47] & 0x3F) == GX >> 376
    assert (GY > P - GY) == bool(blob[47] & 0x80)
    assert lib_points_deserialize(built_lib, C, [nblob], True) == (0, [ng])
    (iblob,), _ = lib_points_serialize(built_lib, C, [None], True)
    assert iblob == bytes(47) + b"\x40" and lib_points_deserialize(built_lib, C, [iblob], True) == (0, [None])
    assert lib_points_deserialize(built_lib, C, [bytes(47) + b"\xc0"], True)[0] != 0  # both flags
    (ublob,), usz = lib_points_serialize(built_lib, C, [ng], False)
    assert usz == 96 and ublob == GX.to_bytes(48, "little") + (P - GY).to_bytes(48, "little") == ser.point_serialize(C, ng, False)
    assert lib_points_deserialize(built_lib, C, [ublob], False) == (0, [ng])
    assert lib_points_deserialize(built_lib, C, [GX.to_bytes(48, "little") + (GY + 1).to_bytes(48, "little")], False)[0] != 0  # off the curve
    for x in (P, (1 << 377) - 1):  # x >= p
        assert lib_points_deserialize(built_lib, C, [x.to_bytes(48, "little")], True)[0] != 0
        assert lib_points_deserialize(built_lib, C, [x.to_bytes(48, "little") + GY.to_bytes(48, "little")], False)[0] != 0
    x = 1
    while ser._sqrt((x * x * x + C.b) % P, P) is not None:  # an x with no point on the curve
        x += 1
    assert lib_points_deserialize(built_lib, C, [x.to_bytes(48, "little")], True)[0] != 0
    # on the curve, outside the subgroup: a compressed x, the uncompressed pair, and the three small-order points
    bad = outside_subgroup_point()
    assert o.is_on_curve(C, bad)
    for pt in (bad, (P - 1, 0), (0, 1), (2, 3)):
        assert lib_points_deserialize(built_lib, C, [pt[0].to_bytes(48, "little") + pt[1].to_bytes(48, "little")], False)[0] != 0
    xb = bytearray(bad[0].to_bytes(48, "little"))
    for flag in (0, 0x80):
        xb[47] = (xb[47] & 0x3F) | flag
        assert lib_points_deserialize(built_lib, C, [bytes(xb)], True)[0] != 0


# ---- Poseidon --------------------------------------------------------------------------------------------------------------------------
def test_poseidon(built_lib, by_name):
    from tests import test_poseidon_cpu as t
    t.test_round_constants_and_permutation(built_lib, C.name)
    t.test_duplex_sequences(built_lib, C.name)
    t.test_encodings_fork_and_challenges(built_lib, C.name)
    assert pp.PoseidonSponge(P).ark != pp.PoseidonSponge(o.BLS12_381_G1.p).ark  # the sponge is its own


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------
def _fixture_points(kind=None):
    out = []
    for k, pts in FIX["curves"][C.name].items():
        if kind is None or k == kind:
            out += [(int(x, 16), int(y, 16)) for x, y in pts]
    return out


def test_adversarial_fixture_is_what_it_claims():
    assert FIX["internal_radix_bits"] == {C.name: 392}
    Rd, half = 1 << 392, (P - 1) // 2
    kinds = FIX["curves"][C.name]
    assert 36 <= sum(len(v) for v in kinds.values()) <= 60
    internal_y = lambda pt: pt[1] * Rd % P  # noqa: E731
    for kind, pts in kinds.items():
        for x, y in pts:
            pt = (int(x, 16), int(y, 16))
            assert o.is_on_curve(C, pt) and o.mul(C, R, pt) is None, kind  # in the prime-order subgroup
        radix, coord, name = kind.split("_", 2)
        if name in ("tiny", "near_p", "below_half", "above_half"):
            for x, y in pts:
                v = (int(y, 16) if coord == "y" else int(x, 16)) * (Rd if radix == "internal" else 1) % P
                d = {"tiny": v, "near_p": P - 1 - v, "below_half": half - v, "above_half": v - (half + 1)}[name]
                assert 0 <= d < P >> 13, kind  # the nearest two of 2^16: within p / 2^13 of the edge
    below = [internal_y((int(x, 16), int(y, 16))) for x, y in kinds["internal_y_below_2p364"]]
    assert len(below) == 4 and all(v < 1 << 364 for v in below)  # top limb zero
    assert all((1 << 364) <= internal_y((int(x, 16), int(y, 16))) < 2 << 364 for x, y in kinds["internal_y_just_above_2p364"])
    assert all(internal_y((int(x, 16), int(y, 16))) >> 364 == P >> 364 == 0x1AE3 for x, y in kinds["internal_y_top_limb_of_p"])
    pair = FIX["negated_doubling_pair"]
    l, r = ((int(pair[k][0], 16), int(pair[k][1], 16)) for k in ("l", "r"))
    assert o.mul(C, R, l) is None and o.mul(C, R, r) is None and l != r and internal_y(r) < 1 << 364


def test_fixture_generator_reproduces_the_fixture():
    """tools/gen_bls12_377_adversarial_points.py run again: the committed fixture, point for point (the search of [1]G .. [2^16]G)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_adv_377", os.path.join(ROOT, "tools", "gen_bls12_377_adversarial_points.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert (gen.BLS12_377.p, gen.BLS12_377.r, gen.BLS12_377.b, gen.POOL) == (P, R, 1, 1 << 16)
    kinds = gen.build(gen.BLS12_377)
    assert FIX["curves"][C.name] == {k: [[hex(pt[0]), hex(pt[1])] for pt in v] for k, v in kinds.items()}


def adversarial(seed, n):
    """n points: the fixture's, each also doubled up, negated and in the negated-doubling shape (P, P, -P, P), then stream points with
    identities, duplicates and P / -P pairs; scalars with 0, 1, r - 1 and equal digits on the duplicates among them"""
    fix = _fixture_points()
    pts = []
    for pt in fix:
        pts += [pt, pt, o.neg(C, pt), pt]
    pair = FIX["negated_doubling_pair"]
    pts += [(int(pair[k][0], 16), int(pair[k][1], 16)) for k in ("l", "r", "r")]
    head = len(pts)
    assert head < n
    pts += o.rng_points(C, seed, n - head)
    for i in range(head, n, 97):
        pts[i] = None
    for i in range(head + 5, n, 61):
        pts[i] = pts[i - 3]
    for i in range(head + 11, n, 53):
        pts[i] = o.neg(C, pts[i - 1])
    sc = [o.rng_fr(C, seed + 1, i) % R for i in range(n)]
    for k in range(len(fix)):  # one scalar per fixture point's four entries: same bucket in every window, doubled, negated, cancelled
        s = [R - 1, R - 2, (1 << 17) - 1, 15, (1 << 200) - 1, sc[4 * k]][k % 6]
        sc[4 * k: 4 * k + 4] = [s, s, s, s]
    sc[head - 2], sc[head - 1] = R - 2, R - 2
    sc[head + 1], sc[head + 2], sc[head + 3] = 0, 1, R - 1
    return pts, sc


@pytest.mark.parametrize("flags", [1, 2], ids=["precomp", "plain"])
def test_host_msm_adversarial(host_ctx, flags):
    from tests.test_msm_gpu import run_msm
    pts, sc = adversarial(21, 1 << 9)
    xy, inf = run_msm(host_ctx, C, pts, sc, flags)
    assert h.np_to_point(C, xy, inf) == o.msm_pippenger(C, pts, sc)
    xy, inf = run_msm(host_ctx, C, [pts[0], pts[2]], [5, 5], flags)  # P + (-P)
    assert h.np_to_point(C, xy, inf) is None and pts[2] == o.neg(C, pts[0])


def test_host_bases_generate_matches_the_oracle_stream(host_ctx):
    """G_i = k_i G with the 254-bit multiplier stream taken over the integers: most k_i exceed r here (r < 2^253)"""
    from accumulation_amd import CommitterKey, ffi
    assert sum(o.rng_scalar(99, i) >= R for i in range(64)) > 32
    ck = CommitterKey.generate(host_ctx, 99, 64, ffi.AMSM_BASES_NO_PRECOMPUTE)
    xy, inf = ck.read()
    assert [h.np_to_point(C, xy[i], inf[i]) for i in range(64)] == o.rng_points(C, 99, 64)
    ck.free()


# ---- the scalar stream -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scalar_stream(seed, n):
    """the rule of csrc/rng.h restated for a modulus of 253 bits or fewer: pyref.rng_fr's value -- the first of 64 candidates below r,
    else candidate 63 with bit 254 cleared -- reduced mod r; -> (the canonical values, the indices where the literal rule gives >= r)"""
    lit = [o.rng_fr(C, seed, i) for i in range(n)]
    return tuple(v % R for v in lit), tuple(i for i, v in enumerate(lit) if v >= R)


def test_host_vec_random_is_canonical(host_ctx):
    """amsm_vec_random, seed 1, 2^16 scalars: every value below r and equal to rng_fr(..) % r; the literal rule gives >= r at index
    2008 (and four more indices), so the reduction is not vacuous"""
    n = 1 << 16
    want, over = scalar_stream(1, n)
    assert o.rng_fr(C, 1, 2008) >= R and over == FALLBACK_INDICES
    assert all(R <= o.rng_fr(C, 1, i) < 1 << 254 and o.rng_fr(C, 1, i) // R <= 3 for i in over)
    v = host_ctx.random_vector(1, n, False)
    got = h.np_to_ints(v.download())
    v.free()
    assert all(x < R for x in got) and tuple(got) == want
    assert [got[i] for i in over] == [o.rng_fr(C, 1, i) % R for i in over]
    assert any(x >> 252 for x in got)  # (the top bit of the field is reached)


def test_wider_fields_keep_the_literal_rule(built_lib):
    """the 254- and 255-bit fields are untouched: rng_fr as it stands (BN254's r < 2^254 keeps the unreduced fallback by compile-time
    branch; its fallback is out of any test's reach, so the stream's head is what can be compared)"""
    from accumulation_amd import Context, ffi
    for cid, c in ((0, o.PALLAS), (1, o.BLS12_381_G1)):
        ctx = Context(cid, device=ffi.AMSM_DEVICE_HOST)
        v = ctx.random_vector(1, 2100, False)
        assert h.np_to_ints(v.download()) == [o.rng_fr(c, 1, i) for i in range(2100)]
        v.free()
        ctx.close()
    src = open(os.path.join(CSRC, "rng.h")).read()
    assert "if constexpr (rng_fr_reduces_fallback<Fr>())" in src and "Fr::mod(7) < (1u << 29)" in src


# ---- transparent keys ------------------------------------------------------------------------------------------------------------------
def test_host_bases_sample_against_the_python_sampler(host_ctx, monkeypatch):
    """amsm_bases_sample: two digest words cut to 377 bits, Tonelli-Shanks with 2-adicity 46 on a 12-word field (h_sqrt; BLS12-381
    takes the direct root) and the multiplication by the even cofactor, against tests/sample_ref.py with this curve's cofactor"""
    from accumulation_amd.engine import CommitterKey
    from accumulation_amd import ffi
    from tests import sample_ref as sr
    monkeypatch.setattr(sr, "cofactor", lambda c: H if c.curve_id == 8 else 1)
    assert two_adicity(P) == 46
    for first, n in ((0, 24), ((1 << 32) + 5, 8)):
        ck = CommitterKey.sample(host_ctx, b"PC-DL-2020", n, ffi.AMSM_BASES_NO_PRECOMPUTE, first=first)
        xy, inf = ck.read()
        ck.free()
        want = sr.sample(C, b"PC-DL-2020", first, n)
        assert not inf.any() and np.array_equal(xy, sr.to_words(C, want))
        assert all(o.is_on_curve(C, pt) and o.mul(C, R, pt) is None for pt in want) and len(set(want)) == n


# ---- point validation ------------------------------------------------------------------------------------------------------------------
def raw_points(pts):
    """(x, y) integers -> the ABI's Montgomery words, whether or not the point is on the curve"""
    return np.array([o.int_to_limbs(x * C.R % P, 6) + o.int_to_limbs(y * C.R % P, 6) for x, y in pts], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def cofactor_group_points():
    """[r]Q for the first curve points Q with x = 1, 2, ... outside the subgroup: points of the cofactor's torsion"""
    out, x = [], 1
    while len(out) < 3:
        y = ser._sqrt((x * x * x + C.b) % P, P)
        if y is not None and y != 0:
            q = o.mul(C, R, (x, y))
            if q is not None:
                assert o.is_on_curve(C, q) and o.mul(C, H, q) is None
                out.append(q)
        x += 1
    return tuple(out)


def points_check_case(n=None):
    """(xy, infinity bytes, expected statuses, index of the first bad point): the fixture's points (0), (p - 1, 0), (0, 1), (2, 3) and
    three [r]Q (3 each: on the curve, outside the subgroup), a non-canonical coordinate (1), an off-curve point (2), the identity's
    forms, then the generator up to n points, the last one with y = p (1)"""
    fix = _fixture_points()
    bad = [(P - 1, 0), (0, 1), (2, 3)] + list(cofactor_group_points()) + [outside_subgroup_point()]
    k = len(fix)
    total = n if n is not None else k + len(bad) + 10
    pts = fix + bad + [o.generator(C)] * (total - k - len(bad))
    xy = raw_points(pts)
    want = np.zeros(total, dtype=np.uint8)
    want[k:k + len(bad)] = 3
    raw = lambda v: np.array(o.int_to_limbs(v, 6), dtype=np.uint64)  # noqa: E731
    j = k + len(bad)
    xy[j, :6], want[j] = raw(P), 1                        # x = p
    xy[j + 1, 6:], want[j + 1] = raw((1 << 384) - 1), 1   # every bit of y set
    xy[j + 2, 6:], want[j + 2] = raw(P - 1), 2            # canonical words, off the curve
    xy[j + 3, :6], want[j + 3] = xy[j + 3, 6:], 2         # (y, y)
    xy[j + 4] = 0                                         # (0, 0): the identity
    inf = np.zeros(total, dtype=np.uint8)
    xy[j + 5, :6], inf[j + 5] = raw(P), 1                 # flagged infinite: the words are ignored
    xy[total - 1, 6:], want[total - 1] = raw(P), 1        # the last point: y = p
    return xy, inf, want, k


def test_host_points_check(host_ctx):
    """amsm_points_check on the host backend: statuses 0 / 3 / 3 / 3 / 3 / 1 / 2 for the fixture, (p - 1, 0), (0, 1), (2, 3), [r]Q, a
    non-canonical coordinate and an off-curve point"""
    from accumulation_amd import CommitterKey, ffi
    from tests.test_points_check_cpu import report_of
    xy, inf, want, k = points_check_case()
    assert list(want[k:k + 9]) == [3, 3, 3, 3, 3, 3, 3, 1, 1] and not want[:k].any() and (want == 2).sum() == 2
    rep, st = host_ctx.check_points(xy, inf, want_status=True)
    assert np.array_equal(st, want) and rep == report_of(want) and rep["off_subgroup"] == 7 and rep["first_bad"] == k
    with pytest.raises(ffi.AmsmError) as e:
        CommitterKey.load(host_ctx, xy, inf, flags=ffi.AMSM_BASES_CHECK | ffi.AMSM_BASES_NO_PRECOMPUTE)
    assert e.value.status == ffi.AMSM_E_INVALID_POINT
    ok = want == 0
    ck = CommitterKey.load(host_ctx, np.ascontiguousarray(xy[ok]), np.ascontiguousarray(inf[ok]), flags=ffi.AMSM_BASES_CHECK | ffi.AMSM_BASES_NO_PRECOMPUTE)
    assert len(ck) == int(ok.sum())
    ck.free()


@pytest.mark.parametrize("flags", [1, 2], ids=["precomp", "plain"])
def test_host_group_law_on_the_small_order_points(host_ctx, flags):
    """doubling the point of order 2 gives the identity and the identity plus P gives P: MSMs over a plain and over a precomputed key
    of small-order points on the host backend -- 2 (p - 1, 0) = O, 3 (2, 3) = (p - 1, 0), 6 (2, 3) = O, 3 (0, 1) = O, and O + G = G behind them"""
    from tests.test_msm_gpu import run_msm
    g = o.generator(C)
    for pts, sc in (([(P - 1, 0)], [2]), ([(2, 3)], [3]), ([(2, 3)], [6]), ([(0, 1)], [3]), ([(P - 1, 0), g], [2, 1]),
                    ([(2, 3), (P - 1, 0), g], [3, 1, 5]), ([(P - 1, 0), (P - 1, 0)], [1, 1])):
        want = None
        for pt, s in zip(pts, sc):
            want = o.add(C, want, o.mul(C, s, pt))
        xy, inf = run_msm(host_ctx, C, pts, sc, flags)
        assert h.np_to_point(C, xy, inf) == want, (pts, sc)


# ---- the schemes ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def env(host_ctx):
    return C, host_ctx


def test_scheme_transcripts(env):
    """the four schemes on the host backend: every challenge the product squeezes equals the one the oracle derives from the
    public data alone (oracle/pyref_transcript.py over the BLS12-377 Fq sponge)"""
    from tests import test_transcripts_vs_oracle as t
    t.test_hp_as_transcript(env, 2, 1, True)
    t.test_trivial_pc_as_transcript(env, 2, 0)
    t.test_r1cs_nark_as_transcript(env, 2, 1, True)
    t.test_ipa_pc_as_transcript(env, 1, 1, True)


@pytest.mark.parametrize("scheme,lg", [("hp_as", 6), ("r1cs_nark_as", 5), ("ipa_pc_as", 4), ("trivial_pc_as", 5)])
def test_profile_as_dump_equals_the_mirror(built_lib, tmp_path, scheme, lg):
    """`profile_as --curve 8 --dump` on the host backend, byte for byte against the Python mirror (tests/harness_mirror.py); the
    harness stream's 254-bit integers take up to three subtractions of r here"""
    from tests.test_profile_as_dump import compare
    compare(tmp_path, scheme, lg, "harness", "poseidon", -1, seed=6, curve=8)
