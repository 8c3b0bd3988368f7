"""BLS12-377 G1 (AMSM_BLS12_377_G1 = 8: y^2 = x^3 + 1 over a 377-bit field, a 253-bit r, the one curve here of EVEN order --
(p - 1, 0) has order 2, (0, 1) order 3, (2, 3) order 6; p, r and h re-derived from the curve's parameter z) without a GPU: the cases its row of tests/curve_rows.py lists (Row.cpu_cases), whose bodies
tests/curve_cases_cpu.py holds once for all four curves, and behind them the curve's own."""
import importlib.util
import math
import os
import re

import pytest

pytest.register_assert_rewrite("tests.curve_cases_cpu")
from oracle import pyref as o  # noqa: E402
from oracle import pyref_ser as ser  # noqa: E402
from tests import curve_cases_cpu as cases  # noqa: E402
from tests import curve_rows as cr  # noqa: E402
from tests import helpers as h  # noqa: E402
from tests.curve_rows import CSRC, ROOT  # noqa: E402

BLS12_377 = h.BLS12_377
ROW = cr.BLS12_377
globals().update(cr.take(cases, ROW.cpu_cases, ROW.aliases))


def two_adicity(m):
    return ((m - 1) & -(m - 1)).bit_length() - 1


Z = 0x8508C00000000001
R377 = Z**4 - Z**2 + 1
P377 = (Z - 1) ** 2 * R377 // 3 + Z
H377 = (Z - 1) ** 2 // 3  # the cofactor
GX = 81937999373150964239938255573465948239988671502647976594219695644855304257327692006745978603320413799295628339695
GY = 241266749859715473739788878240585681733927191168601896383759122102112907357779751001206799952863815012735208165030
BETA = 0x1AE3A4617C510EABC8756BA8F8C524EB8882A75CC9BC8E359064EE822FB5BFFD1E945779FFFFFFFFFFFFFFFFFFFFFFF
P_LIMBS_28 = [1, 0x8C0000, 0x85, 0x5D44300, 0x800170B, 0x2FBA094, 0xF1EF362, 0xF5138, 0xA22D9F3, 0xA1493B1, 0xB05C06C, 0x10EAC63,
              0xA4617C5, 0x1AE3]


def test_curve_facts():
    C, P, R, H = BLS12_377, P377, R377, H377
    assert (C.name, C.curve_id, C.p, C.r, C.b, C.gx, C.gy, C.limbs) == ("bls12_377_g1", 8, P, R, 1, GX, GY, 6) and h.BLS12_377_H == H
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
    assert (-pow(P, -1, 1 << 32)) % (1 << 32) == (-pow(R, -1, 1 << 32)) % (1 << 32) == 0xFFFFFFFF  # INV of both saturated packs


def test_modulus_shape_in_radix_2p28():
    """limb 0 is 1 (NINV = 2^28 - 1: the p_0 = 1 branch of csrc/fpu.h at B = 28, L = 14), no limb is zero, none above limb 0 is a power
    of two, and the column sums of the 14-limb shape fit 64 bits"""
    P = P377
    limbs = [(P >> (28 * i)) & ((1 << 28) - 1) for i in range(14)]
    assert limbs == P_LIMBS_28 and limbs[0] == 1
    assert all(v != 0 for v in limbs) and all(v & (v - 1) != 0 for v in limbs[1:])
    assert (-pow(P, -1, 1 << 28)) % (1 << 28) == (1 << 28) - 1 == 0x0FFFFFFF
    lazy, tight = (1 << 29) - 1, (1 << 28) - 1
    carry = 1 << 36
    assert 14 * lazy * tight + 13 * tight * tight + carry < 1 << 62  # one product, one lazy operand, 13 reduction products
    assert 28 * lazy * tight + 13 * tight * tight + carry + (1 << 32) < 1 << 63  # u_mul_add_mul, an addend riding along


def test_curve_table():
    """csrc/curves.h: b, the generator, the cofactor and the subgroup ladder's constants, against big integers; the subgroup test's
    constants are no longer BLS12-381's alone"""
    src = open(os.path.join(CSRC, "curves.h")).read()
    blk = src[src.index("struct Bls12377Curve {"):]
    blk = blk[:blk.index("\n};")]

    def words(name, bits):
        mm = re.search(name + r"(?:\[\d+\] = \{|, \d+, )([^;)}]*)", blk)
        vals = [int(x.strip().rstrip("ul"), 16) for x in mm.group(1).replace("\n", " ").split(",")]
        return sum(v << (bits * i) for i, v in enumerate(vals))
    assert "int b = 1;" in blk and "subgroup_check = true" in blk and "id = AMSM_BLS12_377_G1" in blk
    assert words("gx", 64) == GX and words("gy", 64) == GY and words("cofactor", 64) == H377 and words("beta", 64) == BETA
    assert words("z_word", 32) == Z and words("z2_word", 32) == Z * Z
    assert re.search(r"z_bits = (\d+), z2_bits = (\d+)", blk).groups() == ("64", "127")
    # BLS12-381's constants moved into its entry unchanged
    b381 = src[src.index("struct Bls12381Curve {"):src.index("struct VestaCurve")]
    assert "0x00010000u, 0xd2010000u" in b381 and "0x00000000u, 0x00000001u, 0x0001a402u, 0xac45a401u" in b381
    assert "z_bits = 64, z2_bits = 128" in b381 and "0x2e01fffffffefffeull" in b381
    for f in ("points_check_kernels.h", "host_points_check.h"):
        src = open(os.path.join(CSRC, f)).read()
        assert "bls_z" not in src and "BLS12_381_BETA" not in src and "0xd2010000u" not in src, f


def test_flag_bits_and_rejections(built_lib):
    from tests.test_wire_format_cpu import lib_points_deserialize, lib_points_serialize
    C, P, R = BLS12_377, P377, R377
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
    bad = cr.outside_subgroup_point()
    assert o.is_on_curve(C, bad)
    for pt in (bad, (P - 1, 0), (0, 1), (2, 3)):
        assert lib_points_deserialize(built_lib, C, [pt[0].to_bytes(48, "little") + pt[1].to_bytes(48, "little")], False)[0] != 0
    xb = bytearray(bad[0].to_bytes(48, "little"))
    for flag in (0, 0x80):
        xb[47] = (xb[47] & 0x3F) | flag
        assert lib_points_deserialize(built_lib, C, [bytes(xb)], True)[0] != 0


def test_adversarial_fixture_is_what_it_claims():
    C, P, R = BLS12_377, P377, R377
    FIX = cr.fixture(cr.BLS12_377)
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
    l, r = cr.negated_doubling_pair(cr.BLS12_377)
    assert o.mul(C, R, l) is None and o.mul(C, R, r) is None and l != r and internal_y(r) < 1 << 364


def test_fixture_generator_reproduces_the_fixture():
    """tools/gen_bls12_377_adversarial_points.py run again: the committed fixture, point for point (the search of [1]G .. [2^16]G)"""
    spec = importlib.util.spec_from_file_location("gen_adv_377", os.path.join(ROOT, "tools", "gen_bls12_377_adversarial_points.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert (gen.BLS12_377.p, gen.BLS12_377.r, gen.BLS12_377.b, gen.POOL) == (P377, R377, 1, 1 << 16)
    kinds = gen.build(gen.BLS12_377)
    assert cr.fixture(cr.BLS12_377)["curves"][BLS12_377.name] == {k: [[hex(pt[0]), hex(pt[1])] for pt in v] for k, v in kinds.items()}


def test_host_vec_random_is_canonical(host_ctx, row):
    """amsm_vec_random, seed 1, 2^16 scalars: every value below r and equal to rng_fr(..) % r; the literal rule gives >= r at index
    2008 (and four more indices), so the reduction is not vacuous"""
    C, R = BLS12_377, R377
    n = 1 << 16
    want, over = cr.scalar_stream(1, n)
    assert o.rng_fr(C, 1, 2008) >= R and over == cr.FALLBACK_INDICES
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


@pytest.mark.parametrize("flags", [1, 2], ids=["precomp", "plain"])
def test_host_group_law_on_the_small_order_points(host_ctx, row, flags):
    """doubling the point of order 2 gives the identity and the identity plus P gives P: MSMs over a plain and over a precomputed key
    of small-order points on the host backend -- 2 (p - 1, 0) = O, 3 (2, 3) = (p - 1, 0), 6 (2, 3) = O, 3 (0, 1) = O, and O + G = G behind them"""
    from tests.test_msm_gpu import run_msm
    C, P = BLS12_377, P377
    g = o.generator(C)
    for pts, sc in (([(P - 1, 0)], [2]), ([(2, 3)], [3]), ([(2, 3)], [6]), ([(0, 1)], [3]), ([(P - 1, 0), g], [2, 1]),
                    ([(2, 3), (P - 1, 0), g], [3, 1, 5]), ([(P - 1, 0), (P - 1, 0)], [1, 1])):
        want = None
        for pt, s in zip(pts, sc):
            want = o.add(C, want, o.mul(C, s, pt))
        xy, inf = run_msm(host_ctx, C, pts, sc, flags)
        assert h.np_to_point(C, xy, inf) == want, (pts, sc)
