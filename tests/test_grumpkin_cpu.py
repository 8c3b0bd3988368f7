"""Grumpkin (AMSM_GRUMPKIN = 6) without a GPU: the facts the port rests on, the field tables compiled into the HIP code, the signed
`b` of the curve table (y^2 = x^3 - 17), the host scalar-field helpers, the GLV set-up, the 32 / 64-byte wire format, the Poseidon
sponge, host linear combinations, MSMs over the adversarial-point fixture, the key streams, transparent keys (Tonelli-Shanks with
2-adicity 28), point validation and the four schemes on the library's host backend, the C++ drivers' dumps, and the cycle itself:
BN254 coordinates as Grumpkin scalars and back -- each against the big-int oracle with a Grumpkin `Curve` built here (base field
BN254's r, order BN254's p, generator (1, sqrt(-16)), cofactor 1; oracle/ knows curves 0 and 1 only and is curve-generic)."""
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

P_BN = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
R_BN = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
P, R = R_BN, P_BN  # Grumpkin's base field (coordinates) and scalar field (group order): BN254's, swapped
GY = 17631683881184975370165255887551781615748388533673675138860
GRUMPKIN = o.Curve("grumpkin", 6, p=R_BN, r=P_BN, b=R_BN - 17, gx=1, gy=GY, limbs=4)
BN254 = o.Curve("bn254_g1", 4, P_BN, R_BN, b=3, gx=1, gy=2, limbs=4)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "accumulation_amd", "csrc")
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "grumpkin_adversarial_points.json")))
Q_LIMBS_29 = [0x10000001, 0x1F0FAC9F, 0x0E5C2450, 0x07D090F3, 0x1585D283, 0x02DB40C0, 0x00A6E141, 0x0E5C2634, 0x0030644E]


@pytest.fixture
def grumpkin_by_name(monkeypatch):
    """the curve-parametrised modules look curves up by name in the oracle's table: add Grumpkin for the duration of one test"""
    monkeypatch.setitem(o.CURVES, GRUMPKIN.name, GRUMPKIN)
    monkeypatch.setitem(o.CURVES_BY_ID, GRUMPKIN.curve_id, GRUMPKIN)


@pytest.fixture
def host_ctx(built_lib):
    from accumulation_amd import Context, ffi
    ctx = Context(ffi.AMSM_GRUMPKIN, device=ffi.AMSM_DEVICE_HOST)
    yield ctx
    ctx.close()


# ---- the facts (the issue's list, re-derived) -------------------------------------------------------------------------------------------
def test_curve_facts():
    g = o.generator(GRUMPKIN)
    assert GY == 0x2CF135E7506A45D632D270D45F1181294833FC48D823F272C and GY * GY % P == P - 16
    assert g == (1, GY) and o.is_on_curve(GRUMPKIN, g) and o.mul(GRUMPKIN, R, g) is None  # order p_BN, prime: cofactor 1
    assert GRUMPKIN.b == P - 17 and P.bit_length() == R.bit_length() == 254
    assert P % 4 == 1 and (P - 1) % (1 << 28) == 0 and ((P - 1) >> 28) % 2 == 1  # Tonelli-Shanks, 2-adicity 28
    assert P % 3 == 1 and R % 3 == 1  # cube roots of unity in both fields: GLV (j = 0)
    assert math.gcd(17, P - 1) == 1  # the sponge's alpha = 17 permutes Fq
    assert (1 << 261) // P == 169 and abs((1 << 261) / P - 169.28) < 0.01  # head-room of a tight value: BN254's
    assert R < (1 << 254) and abs(R / (1 << 255) - 0.378) < 0.001  # the scalar stream's acceptance rate per candidate
    assert R >> 240 == 0x3064  # the top 16-bit window of a scalar: BN254's, so a plain 2^20 MSM takes BN254's pipeline
    assert ser.point_size(GRUMPKIN, True) == 32 and ser.point_size(GRUMPKIN, False) == 64  # 254 + 2 flag bits


def test_modulus_shape_in_radix_2p29():
    """no zero limb, no power-of-two limb above limb 0, q_0 = 2^28 + 1 and NINV = 2^28 - 1: the general reduction branch of
    csrc/fpu.h, and the column sums of the nine-limb general shape still fit"""
    limbs = [(P >> (29 * i)) & ((1 << 29) - 1) for i in range(9)]
    assert limbs == Q_LIMBS_29 and limbs[0] == (1 << 28) + 1
    assert all(v != 0 for v in limbs) and all(v & (v - 1) != 0 for v in limbs[1:])
    ninv = (-pow(P, -1, 1 << 29)) % (1 << 29)
    assert ninv == 0x0FFFFFFF and ninv != (1 << 29) - 1
    lazy, tight = (1 << 30) - 1, (1 << 29) - 1
    carry = 1 << 35
    assert 9 * lazy * tight + 9 * tight * tight + carry < 1 << 63  # one product, one lazy operand
    assert 18 * lazy * tight + 9 * tight * tight + carry + (1 << 32) < 1 << 64  # u_mul_add_mul, an addend riding along
    assert (4 * 9 + 9) * tight * tight + carry < 1 << 64  # four tight products under one reduction (the removed u_dot<4>)


def _tables(src, name, limbs, bits):
    blk = src[src.index("struct " + name + " {"):]
    blk = blk[:blk.index("};")]

    def tab(t):
        mm = re.search(r"AMSM_TABLE\(" + t + r", \d+, ([^)]*)\)", blk, re.S)
        vals = [int(x.strip().rstrip("u"), 16) for x in mm.group(1).replace("\n", " ").split(",")]
        assert len(vals) == limbs and all(v < (1 << bits) for v in vals)
        return sum(v << (bits * i) for i, v in enumerate(vals))
    return blk, tab


@pytest.mark.parametrize("name,m,twin", [("GrumpkinFq", P, "Bn254Fr"), ("GrumpkinFr", R, "Bn254Fq")])
def test_saturated_tables(name, m, twin):
    src = open(os.path.join(CSRC, "fp.h")).read()
    blk, tab = _tables(src, name, 8, 32)
    Rm = 1 << 256
    assert tab("mod") == m and tab("one") == Rm % m and tab("r2") == Rm * Rm % m
    assert int(re.search(r"INV = (0x[0-9a-f]+)u", blk).group(1), 16) == (-pow(m, -1, 1 << 32)) % (1 << 32)
    _, ttab = _tables(src, twin, 8, 32)  # the tables of the other curve's other field
    assert all(tab(t) == ttab(t) for t in ("mod", "one", "r2"))
    assert "struct DevField<GrumpkinFq>" in src


def test_unsaturated_table():
    blk, tab = _tables(open(os.path.join(CSRC, "fpu.h")).read(), "GrumpkinFqU", 9, 29)
    m, R_abi, R_dev = P, 1 << 256, 1 << 261
    assert [int(x) for x in re.findall(r"int (?:L|W|B) = (\d+);", blk)] == [9, 8, 29]
    assert tab("mod") == m and tab("one") == R_dev % m
    assert tab("k_import") == R_dev * R_dev * pow(R_abi, -1, m) % m and tab("k_export") == R_abi % m
    ninv = int(re.search(r"NINV = (0x[0-9a-f]+)u", blk).group(1), 16)
    assert ninv == (-pow(m, -1, 1 << 29)) % (1 << 29) == 0x0FFFFFFF and ninv != (1 << 29) - 1  # the general reduction step
    assert "using Sat = GrumpkinFq;" in blk


def test_pack_names_stay_in_the_field_headers():
    """everything else follows through SatOf, DevField, CurveOf and the templates; the new unit names no pack of the other curve"""
    for f in sorted(os.listdir(CSRC)):
        if f in ("fp.h", "fpu.h", "fp_mul_gfx950.h"):
            continue
        src = open(os.path.join(CSRC, f)).read()
        assert "GrumpkinFqU" not in src, f
        if f not in ("curves.h", "kern_grumpkin.hip", "kern_fr.hip", "api_types.h"):  # the table, the two units, the sponge's state tuple
            assert "GrumpkinF" not in src, f
    unit = open(os.path.join(CSRC, "kern_grumpkin.hip")).read()
    assert "Bn254" not in unit and "AMSM_FQ GrumpkinFq" in unit and "AMSM_FR GrumpkinFr" in unit and "AMSM_CURVE_ID 6" in unit
    assert "AMSM_FR_LAUNCHERS(GrumpkinFr)" in open(os.path.join(CSRC, "kern_fr.hip")).read()


def test_generated_multiplication_header_is_current():
    out = subprocess.run(["python3", os.path.join(ROOT, "tools", "gen_fp_asm.py")], capture_output=True, text=True, check=True).stdout
    assert out == open(os.path.join(CSRC, "fp_mul_gfx950.h")).read()
    for fn in ("fe_mul<GrumpkinFq>", "fe_mul<GrumpkinFr>", "fe_dot2<GrumpkinFr>", "fe_dot3<GrumpkinFr>"):
        assert fn in out, fn
    # the products forward to the schedules of the same moduli; the sums of products are generated for p_BN under the new name,
    # and nothing is added for the field that is no curve's scalar field
    assert "return fe_cast<GrumpkinFq>(fe_mul<Bn254Fr>(" in out and "return fe_cast<GrumpkinFr>(fe_mul<Bn254Fq>(" in out
    assert "fe_dot2<Bn254Fq>" not in out and "fe_dot3<Bn254Fq>" not in out and "fe_dot2<GrumpkinFq>" not in out
    dot = out[out.index("fe_dot3<GrumpkinFr>"):]
    dot = dot[:dot.index("return r;")]
    assert all(f"0x{(R >> (32 * j)) & 0xFFFFFFFF:08x}u" in dot for j in range(8))  # every limb of p_BN in its reduction


# ---- the curve id ----------------------------------------------------------------------------------------------------------------------
def test_id_6_is_accepted_where_3_5_and_7_are_refused(built_lib):
    from accumulation_amd import ffi
    from accumulation_amd.engine import Context
    assert ffi.AMSM_GRUMPKIN == 6
    a = np.ones(4, dtype=np.uint64)
    for bad in (3, 5, 7):
        with pytest.raises(Exception):
            Context(bad, device=ffi.AMSM_DEVICE_HOST)
        assert built_lib.amsm_fr_to_mont(bad, a.ctypes.data, 1, a.ctypes.data) == ffi.AMSM_E_INVALID_ARG
        assert built_lib.amsm_point_serialized_size(bad, 1) == 0 and built_lib.amsm_fr_serialized_size(bad) == 0
    ctx = Context(6, device=ffi.AMSM_DEVICE_HOST)
    assert ctx.curve == 6 and ctx.fq_limbs == 4
    ctx.close()
    assert built_lib.amsm_fr_to_mont(6, a.ctypes.data, 1, a.ctypes.data) == ffi.AMSM_OK
    assert o.limbs_to_int([int(v) for v in a]) == o.fr_to_mont(GRUMPKIN, 1 + (1 << 64) + (1 << 128) + (1 << 192))
    assert built_lib.amsm_fr_serialized_size(6) == 32
    assert built_lib.amsm_point_serialized_size(6, 1) == 32 and built_lib.amsm_point_serialized_size(6, 0) == 64


def test_python_tables():
    from accumulation_amd import AMSM_GRUMPKIN, ipa_pc
    from accumulation_amd.scalar_field import MODULI, Fr
    assert AMSM_GRUMPKIN == 6 and MODULI[AMSM_GRUMPKIN] == R == P_BN and MODULI[4] == P
    assert ipa_pc.IPA_FOLD[AMSM_GRUMPKIN] == ipa_pc.IPA_FOLD[0]
    fr = Fr(AMSM_GRUMPKIN)
    assert fr.from_limbs(fr.to_limbs(R - 1)) == R - 1


# ---- the signed b of the curve table ---------------------------------------------------------------------------------------------------
def old_cast_point():
    """a point of y^2 = x^3 + (2^64 - 17) over q: what `(u64)(-17)` made of b before curve_b_mont took a signed value"""
    x = 1
    while True:
        y = ser._sqrt((x * x * x + (1 << 64) - 17) % P, P)
        if y:
            return x, y
        x += 1


def b_cases():
    """(points as (x, y) integers, expected statuses): G, -G, (1, y + 1), a point of the curve the old cast of b described"""
    g = o.generator(GRUMPKIN)
    wrong = old_cast_point()
    assert not o.is_on_curve(GRUMPKIN, wrong) and (wrong[1] ** 2 - wrong[0] ** 3 - ((1 << 64) - 17)) % P == 0
    return [g, o.neg(GRUMPKIN, g), (1, GY + 1), wrong], [0, 0, 2, 2]


def raw_points(pts):
    """(x, y) integers -> the ABI's Montgomery words, whether or not the point is on the curve"""
    return np.array([o.int_to_limbs(x * GRUMPKIN.R % P, 4) + o.int_to_limbs(y * GRUMPKIN.R % P, 4) for x, y in pts], dtype=np.uint64)


def test_curve_b_is_q_minus_17(host_ctx):
    """curve_b_mont through amsm_points_check on the host backend"""
    from tests.test_points_check_cpu import report_of
    pts, want = b_cases()
    rep, st = host_ctx.check_points(raw_points(pts), np.zeros(len(pts), dtype=np.uint8), want_status=True)
    assert list(st) == want and rep == report_of(np.array(want, dtype=np.uint8)) and rep["first_bad"] == 2


# ---- host helpers ----------------------------------------------------------------------------------------------------------------------
def test_fr_helpers(built_lib):
    from tests import test_host_fr_cpu as t
    t.test_host_fr_helpers(built_lib, GRUMPKIN)
    t.test_host_fr_inverse_many(built_lib, GRUMPKIN)


def test_host_lincomb(built_lib):
    from tests import test_host_fr_cpu as t
    t.test_host_lincomb_vs_oracle(built_lib, GRUMPKIN)
    t.test_host_lincomb_batch_equals_single_calls_and_oracle(built_lib, GRUMPKIN)


def test_glv_pairing_and_split():
    """host_glv.h on Grumpkin: lambda and beta pair up, [lambda] G = (beta Gx, Gy), and edge scalars split into short halves that
    give the same point (tests/cpp_host/grumpkin_glv_check.cpp)"""
    out = os.path.join(ROOT, "build", "grumpkin_glv_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["hipcc", "-std=c++17", "-O2", "--offload-host-only", "--offload-arch=gfx950", "-x", "hip", "-w",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp_host", "grumpkin_glv_check.cpp"), "-o", out])
    res = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lam, beta = (int(x, 16) for x in re.search(r"lambda (\w+) beta (\w+)", res.stdout).groups())
    g = o.generator(GRUMPKIN)
    assert 1 < lam < R and 1 < beta < P and pow(lam, 3, R) == 1 and pow(beta, 3, P) == 1
    assert o.mul(GRUMPKIN, lam, g) == (beta * g[0] % P, g[1])
    assert "OK" in res.stdout


# ---- wire format -----------------------------------------------------------------------------------------------------------------------
def test_wire_format(built_lib, grumpkin_by_name):
    from tests import test_wire_format_cpu as t
    t.test_scalars(built_lib, GRUMPKIN.name)
    for compressed in (True, False):
        t.test_points(built_lib, GRUMPKIN.name, compressed)
    t.test_rejections(built_lib, GRUMPKIN.name)
    # 254 bits + 2 flag bits fill 32 bytes exactly: no 33rd byte as on the 255-bit curves
    assert built_lib.amsm_fr_serialized_size(6) == 32
    assert built_lib.amsm_point_serialized_size(6, 1) == ser.point_size(GRUMPKIN, True) == 32
    assert built_lib.amsm_point_serialized_size(6, 0) == ser.point_size(GRUMPKIN, False) == 64


def test_generator_encoding_flag_bits_and_rejections(built_lib):
    from tests.test_wire_format_cpu import lib_points_deserialize, lib_points_serialize
    g = o.generator(GRUMPKIN)
    (blob,), sz = lib_points_serialize(built_lib, GRUMPKIN, [g], True)
    # x = 1 little-endian; y (195 bits) is the smaller root: no flag bit
    assert GY < P - GY
    assert sz == 32 and blob == (1).to_bytes(32, "little") == ser.point_serialize(GRUMPKIN, g)
    rc, (back,) = lib_points_deserialize(built_lib, GRUMPKIN, [blob], True)
    assert rc == 0 and back == g
    # -G: the larger root, bit 7 of the last byte -- beside the top bits of a 254-bit x in the same byte
    ng = o.neg(GRUMPKIN, g)
    (nblob,), _ = lib_points_serialize(built_lib, GRUMPKIN, [ng], True)
    assert nblob == b"\x01" + bytes(30) + b"\x80" == ser.point_serialize(GRUMPKIN, ng)
    assert lib_points_deserialize(built_lib, GRUMPKIN, [nblob], True) == (0, [ng])
    # a point whose x has bit 253 set keeps it under both flags' bits
    big = next(pt for kind in ("plain_x_at_p_minus_1",) for pt in _fixture_points(kind))
    for pt in (big, o.neg(GRUMPKIN, big)):
        (b,), _ = lib_points_serialize(built_lib, GRUMPKIN, [pt], True)
        assert b == ser.point_serialize(GRUMPKIN, pt) and (b[31] & 0x3F) == (pt[0] >> 248) and lib_points_deserialize(built_lib, GRUMPKIN, [b], True) == (0, [pt])
    # the identity: bit 6, x = 0; both flag bits: invalid
    (iblob,), _ = lib_points_serialize(built_lib, GRUMPKIN, [None], True)
    assert iblob == bytes(31) + b"\x40" and lib_points_deserialize(built_lib, GRUMPKIN, [iblob], True) == (0, [None])
    assert lib_points_deserialize(built_lib, GRUMPKIN, [bytes(31) + b"\xc0"], True)[0] != 0
    # uncompressed: x without flags, y with the infinity bit only
    (ublob,), usz = lib_points_serialize(built_lib, GRUMPKIN, [ng], False)
    assert usz == 64 and ublob == (1).to_bytes(32, "little") + (P - GY).to_bytes(32, "little") == ser.point_serialize(GRUMPKIN, ng, False)
    assert lib_points_deserialize(built_lib, GRUMPKIN, [ublob], False) == (0, [ng])
    assert lib_points_deserialize(built_lib, GRUMPKIN, [(1).to_bytes(32, "little") + (GY + 1).to_bytes(32, "little")], False)[0] != 0  # off the curve
    wx, wy = old_cast_point()  # on the curve the old cast of b described, not on this one
    assert lib_points_deserialize(built_lib, GRUMPKIN, [wx.to_bytes(32, "little") + wy.to_bytes(32, "little")], False)[0] != 0
    # x >= q: q itself and the largest 254-bit integer (q < 2^254, so both fit beside the flags), compressed and uncompressed
    for x in (P, (1 << 254) - 1):
        assert lib_points_deserialize(built_lib, GRUMPKIN, [x.to_bytes(32, "little")], True)[0] != 0
        assert lib_points_deserialize(built_lib, GRUMPKIN, [x.to_bytes(32, "little") + GY.to_bytes(32, "little")], False)[0] != 0
    x = 1
    while ser._sqrt(x * x * x + GRUMPKIN.b, P) is not None:  # an x with no point on the curve
        x += 1
    assert lib_points_deserialize(built_lib, GRUMPKIN, [x.to_bytes(32, "little")], True)[0] != 0


# ---- Poseidon --------------------------------------------------------------------------------------------------------------------------
def test_poseidon(built_lib, grumpkin_by_name):
    from tests import test_poseidon_cpu as t
    t.test_round_constants_and_permutation(built_lib, GRUMPKIN.name)
    t.test_duplex_sequences(built_lib, GRUMPKIN.name)
    t.test_encodings_fork_and_challenges(built_lib, GRUMPKIN.name)
    # the sponge is its own: the other 4-limb fields' round constants are over other moduli
    assert pp.PoseidonSponge(P).ark != pp.PoseidonSponge(P_BN).ark != pp.PoseidonSponge(o.PALLAS.p).ark


# ---- host backend: MSMs over the adversarial points ---------------------------------------------------------------------------------------
def _fixture_points(kind=None):
    out = []
    for k, pts in FIX["curves"][GRUMPKIN.name].items():
        if kind is None or k == kind:
            out += [(int(x, 16), int(y, 16)) for x, y in pts]
    return out


def test_adversarial_fixture_is_what_it_claims():
    assert FIX["internal_radix_bits"] == {GRUMPKIN.name: 261}
    Rd, half = 1 << 261, (P - 1) // 2
    kinds = FIX["curves"][GRUMPKIN.name]
    assert 40 <= sum(len(v) for v in kinds.values()) <= 60
    for kind, pts in kinds.items():
        radix, coord, name = kind.split("_", 2)
        for x, y in pts:
            pt = (int(x, 16), int(y, 16))
            assert o.is_on_curve(GRUMPKIN, pt) and o.mul(GRUMPKIN, R, pt) is None
            v = (pt[1] if coord == "y" else pt[0]) * (Rd if radix == "internal" else 1) % P
            target = {"at_0": 0, "at_1": 1, "at_p_minus_1": P - 1, "at_half_minus": half, "at_half_plus": half + 1,
                      "low_limbs_all_ones": (1 << 232) - 1, "top_limb_only": (P >> 232) << 232, "just_above_2p232": 1 << 232}[name]
            assert abs(v - target) < 64, kind  # (a coordinate gives a point with probability about 1 / 2 (x) or 1 / 3 (y))
    limbs = lambda v: [(v >> (29 * i)) & ((1 << 29) - 1) for i in range(9)]  # noqa: E731
    lo = limbs(int(kinds["internal_y_low_limbs_all_ones"][0][1], 16) * Rd % P)
    assert lo[8] == 0 and lo[1:8] == [(1 << 29) - 1] * 7
    hi = limbs(int(kinds["internal_y_top_limb_only"][0][1], 16) * Rd % P)
    assert hi[8] == Q_LIMBS_29[8] and hi[1:8] == [0] * 7
    pair = FIX["negated_doubling_pair"]
    l, r = ((int(pair[k][0], 16), int(pair[k][1], 16)) for k in ("l", "r"))
    assert o.is_on_curve(GRUMPKIN, l) and o.is_on_curve(GRUMPKIN, r) and r[1] * Rd % P < 1 << 232


def test_fixture_generator_reproduces_both_fixtures(tmp_path):
    """tools/gen_bn254_adversarial_points.py --curve: the committed Grumpkin fixture, and BN254's byte for byte as before"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_adv", os.path.join(ROOT, "tools", "gen_bn254_adversarial_points.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for name, fname in (("grumpkin", "grumpkin_adversarial_points.json"), ("bn254_g1", "bn254_adversarial_points.json")):
        c, _, f = gen.CURVES[name]
        assert f == fname and (c.p, c.r, c.b) == ((P, R, P - 17) if name == "grumpkin" else (P_BN, R_BN, 3))
        committed = json.load(open(os.path.join(ROOT, "tests", "golden", fname)))
        kinds = gen.build(c)
        assert committed["curves"][c.name] == {k: [[hex(pt[0]), hex(pt[1])] for pt in v] for k, v in kinds.items()}


def adversarial(seed, n):
    """n points: the fixture's, each also doubled up, negated and in the negated-doubling shape (P, P, -P, P), then stream points with
    identities, duplicates and P / -P pairs; scalars with 0, 1, r - 1 and equal digits on the duplicates among them"""
    fix = _fixture_points()
    pts = []
    for pt in fix:
        pts += [pt, pt, o.neg(GRUMPKIN, pt), pt]
    pair = FIX["negated_doubling_pair"]
    pts += [(int(pair[k][0], 16), int(pair[k][1], 16)) for k in ("l", "r", "r")]
    head = len(pts)
    assert head < n
    pts += o.rng_points(GRUMPKIN, seed, n - head)
    for i in range(head, n, 97):
        pts[i] = None
    for i in range(head + 5, n, 61):
        pts[i] = pts[i - 3]
    for i in range(head + 11, n, 53):
        pts[i] = o.neg(GRUMPKIN, pts[i - 1])
    sc = [o.rng_fr(GRUMPKIN, seed + 1, i) for i in range(n)]
    for k in range(len(fix)):  # one scalar per fixture point's four entries: same bucket in every window, doubled, negated, cancelled
        s = [R - 1, R - 2, (1 << 17) - 1, 15, (1 << 200) - 1, sc[4 * k]][k % 6]
        sc[4 * k: 4 * k + 4] = [s, s, s, s]
    sc[head - 2], sc[head - 1] = R - 2, R - 2
    sc[head + 1], sc[head + 2], sc[head + 3] = 0, 1, R - 1
    return pts, sc


@pytest.mark.parametrize("flags", [1, 2], ids=["precomp", "plain"])
def test_host_msm_adversarial(host_ctx, flags):
    from tests.test_msm_gpu import run_msm
    pts, sc = adversarial(21, 1 << 10)
    xy, inf = run_msm(host_ctx, GRUMPKIN, pts, sc, flags)
    assert h.np_to_point(GRUMPKIN, xy, inf) == o.msm_pippenger(GRUMPKIN, pts, sc)
    # P + (-P) and an identity alone
    xy, inf = run_msm(host_ctx, GRUMPKIN, [pts[0], pts[2]], [5, 5], flags)
    assert h.np_to_point(GRUMPKIN, xy, inf) is None and pts[2] == o.neg(GRUMPKIN, pts[0])


def test_host_bases_generate_matches_the_oracle_stream(host_ctx):
    """G_i = k_i G with the 254-bit multiplier stream taken over the integers: some k_i exceed r here (r < 2^254)"""
    from accumulation_amd import CommitterKey, ffi
    assert any(o.rng_scalar(99, i) >= R for i in range(64))
    ck = CommitterKey.generate(host_ctx, 99, 64, ffi.AMSM_BASES_NO_PRECOMPUTE)
    xy, inf = ck.read()
    assert [h.np_to_point(GRUMPKIN, xy[i], inf[i]) for i in range(64)] == o.rng_points(GRUMPKIN, 99, 64)
    ck.free()


def test_host_vec_random_is_uniform_below_r(host_ctx):
    """amsm_vec_random over r = p_BN: the rejection rule of pyref.rng_fr restated with this r, whose candidates fail 62 % of the time"""
    v = host_ctx.random_vector(7, 300, False)
    got = h.np_to_ints(v.download())
    assert got == [o.rng_fr(GRUMPKIN, 7, i) for i in range(300)] and all(x < R for x in got)
    assert any(x >> 253 for x in got)  # (the top bit of the field is reached)


def test_host_bases_sample_against_the_python_sampler(host_ctx):
    """amsm_bases_sample: one 254-bit digest word and Tonelli-Shanks with 2-adicity 28 (h_sqrt) together, against
    tests/sample_ref.py; b = q - 17 reaches the sampler through curve_b_mont"""
    from accumulation_amd.engine import CommitterKey
    from accumulation_amd import ffi
    from tests import sample_ref as sr
    for first, n in ((0, 48), ((1 << 32) + 5, 16)):  # 64 indices
        ck = CommitterKey.sample(host_ctx, b"PC-DL-2020", n, ffi.AMSM_BASES_NO_PRECOMPUTE, first=first)
        xy, inf = ck.read()
        ck.free()
        want = sr.sample(GRUMPKIN, b"PC-DL-2020", first, n)
        assert not inf.any() and np.array_equal(xy, sr.to_words(GRUMPKIN, want))
        assert all(o.is_on_curve(GRUMPKIN, pt) for pt in want) and len(set(want)) == n


def points_check_case(extra=0):
    """(xy, infinity bytes, expected statuses, index of the first bad point): the fixture's points and `extra + 14` copies of the
    generator, eight of them overwritten with non-canonical words, points off the curve and the identity's forms, four with the
    b-cases (G, -G, (1, y + 1), a point of the curve the old cast of b described)"""
    pts = _fixture_points()
    xy, _ = h.points_to_np(GRUMPKIN, pts + [o.generator(GRUMPKIN)] * (14 + extra))
    n = xy.shape[0]
    want = np.zeros(n, dtype=np.uint8)
    raw = lambda v: np.array(o.int_to_limbs(v, 4), dtype=np.uint64)  # noqa: E731
    k = len(pts)
    xy[k, :4], want[k] = raw(P), 1                          # x = q
    xy[k + 1, 4:], want[k + 1] = raw(P + 1), 1              # y = q + 1
    xy[k + 2, :4], want[k + 2] = raw((1 << 256) - 1), 1     # every bit set
    xy[k + 3, 4:], want[k + 3] = raw(P - 1), 2              # canonical words, off the curve
    xy[k + 4, :4], want[k + 4] = xy[k + 4, 4:], 2           # (y, y)
    xy[k + 5] = 0                                           # (0, 0): the identity
    xy[k + 6, 4:], want[k + 6] = 0, 2                       # (x, 0)
    inf = np.zeros(n, dtype=np.uint8)
    xy[k + 7, :4], inf[k + 7] = raw(P), 1                   # flagged infinite: the words are ignored
    bp, bw = b_cases()
    xy[k + 8:k + 12], want[k + 8:k + 12] = raw_points(bp), bw
    xy[n - 1, 4:], want[n - 1] = raw(P), 1                  # the last point: y = q
    return xy, inf, want, k


def test_host_points_check(host_ctx):
    """amsm_points_check: non-canonical words, points off the curve, the identity forms; status 3 is never reported (cofactor 1)"""
    from accumulation_amd import CommitterKey, ffi
    from tests.test_points_check_cpu import report_of
    xy, inf, want, k = points_check_case()
    rep, st = host_ctx.check_points(xy, inf, want_status=True)
    assert np.array_equal(st, want) and rep == report_of(want) and rep["off_subgroup"] == 0 and rep["first_bad"] == k
    with pytest.raises(ffi.AmsmError) as e:
        CommitterKey.load(host_ctx, xy, inf, flags=ffi.AMSM_BASES_CHECK | ffi.AMSM_BASES_NO_PRECOMPUTE)
    assert e.value.status == ffi.AMSM_E_INVALID_POINT
    ok = want == 0
    ck = CommitterKey.load(host_ctx, np.ascontiguousarray(xy[ok]), np.ascontiguousarray(inf[ok]), flags=ffi.AMSM_BASES_CHECK | ffi.AMSM_BASES_NO_PRECOMPUTE)
    assert len(ck) == int(ok.sum())
    ck.free()


# ---- the schemes ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def env(host_ctx):
    return GRUMPKIN, host_ctx


def test_scheme_transcripts(env):
    """the four schemes on the host backend: every challenge the product squeezes equals the one the oracle derives from the
    public data alone (oracle/pyref_transcript.py over the Grumpkin Fq sponge)"""
    from tests import test_transcripts_vs_oracle as t
    t.test_hp_as_transcript(env, 2, 1, True)
    t.test_trivial_pc_as_transcript(env, 2, 0)
    t.test_r1cs_nark_as_transcript(env, 2, 1, True)
    t.test_ipa_pc_as_transcript(env, 1, 1, True)


@pytest.mark.parametrize("scheme,lg", [("hp_as", 6), ("r1cs_nark_as", 5), ("ipa_pc_as", 4), ("trivial_pc_as", 5)])
def test_profile_as_dump_equals_the_mirror(built_lib, tmp_path, scheme, lg):
    """`profile_as --curve 6 --dump` on the host backend, byte for byte against the Python mirror (tests/harness_mirror.py)"""
    from tests.test_profile_as_dump import compare
    compare(tmp_path, scheme, lg, "harness", "poseidon", -1, seed=6, curve=6)


# ---- the cycle -------------------------------------------------------------------------------------------------------------------------
def cycle_closes(ctx_a, A, ctx_b, B, seed):
    """Commit on curve A: four MSMs of 2^6 pairs.  The result points' x | y words -- ABI Montgomery form over A's base field, as
    the library returns them -- go UNCHANGED as `mont=True` scalars into one MSM on curve B, whose scalar field is that field;
    the oracle sums over the canonical integers."""
    from accumulation_amd import CommitterKey, VariableBaseMSM, ffi
    assert A.p == B.r and A.limbs == 4
    n, m = 1 << 6, 4
    ck_a = CommitterKey.generate(ctx_a, seed, n, ffi.AMSM_BASES_NO_PRECOMPUTE)
    pts_a = o.rng_points(A, seed, n)
    words, coords = [], []
    for t in range(m):
        sc = [o.rng_fr(A, seed + 1 + t, i) for i in range(n)]
        xy, inf = VariableBaseMSM.multi_scalar_mul(ck_a, h.scalars_to_np(sc))
        pt = h.np_to_point(A, xy, inf)
        assert pt is not None and pt == o.msm_pippenger(A, pts_a, sc)
        words.append(np.asarray(xy, dtype=np.uint64).reshape(2, 4))
        coords += [pt[0], pt[1]]
    ck_a.free()
    scalars = np.ascontiguousarray(np.concatenate(words))  # (2 m, 4): x_0, y_0, x_1, y_1, ...
    assert h.fr_from_mont_np(B, scalars) == coords
    ck_b = CommitterKey.generate(ctx_b, seed + 100, 2 * m, ffi.AMSM_BASES_NO_PRECOMPUTE)
    out, oinf = VariableBaseMSM.multi_scalar_mul(ck_b, scalars, mont=True)
    ck_b.free()
    want = None
    for c, g in zip(coords, o.rng_points(B, seed + 100, 2 * m)):
        want = o.add(B, want, o.mul(B, c, g))
    assert want is not None and h.np_to_point(B, out, oinf) == want


def test_the_cycle_closes(built_lib, host_ctx):
    from accumulation_amd import Context, ffi
    bn = Context(ffi.AMSM_BN254_G1, device=ffi.AMSM_DEVICE_HOST)
    try:
        cycle_closes(bn, BN254, host_ctx, GRUMPKIN, 41)  # BN254 commitments' coordinates, committed to on Grumpkin
        cycle_closes(host_ctx, GRUMPKIN, bn, BN254, 43)  # and the other way round
    finally:
        bn.close()
