"""BN254 G1 (AMSM_BN254_G1 = 4) without a GPU: the facts the port rests on, the field tables compiled into the HIP code, the host
scalar-field helpers, the GLV set-up, the 32 / 64-byte wire format, the Poseidon sponge, host linear combinations, MSMs over the
adversarial-point fixture, the key streams, transparent keys, point validation and the four schemes on the library's host backend,
and the C++ drivers' dumps -- each against the big-int oracle with a BN254 `Curve` built here (y^2 = x^3 + 3, generator (1, 2),
cofactor 1; oracle/ knows curves 0 and 1 only and is curve-generic)."""
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

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BN254 = o.Curve("bn254_g1", 4, P, R, b=3, gx=1, gy=2, limbs=4)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "accumulation_amd", "csrc")
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "bn254_adversarial_points.json")))
P_LIMBS_29 = [0x187CFD47, 0x010460B6, 0x1C72A34F, 0x02D522D0, 0x1585D978, 0x02DB40C0, 0x00A6E141, 0x0E5C2634, 0x0030644E]


@pytest.fixture
def bn254_by_name(monkeypatch):
    """the curve-parametrised modules look curves up by name in the oracle's table: add BN254 for the duration of one test"""
    monkeypatch.setitem(o.CURVES, BN254.name, BN254)
    monkeypatch.setitem(o.CURVES_BY_ID, BN254.curve_id, BN254)


@pytest.fixture
def host_ctx(built_lib):
    from accumulation_amd import Context, ffi
    ctx = Context(ffi.AMSM_BN254_G1, device=ffi.AMSM_DEVICE_HOST)
    yield ctx
    ctx.close()


# ---- the facts (the issue's list, re-derived) -------------------------------------------------------------------------------------------
def test_curve_facts():
    g = o.generator(BN254)
    assert g == (1, 2) and o.is_on_curve(BN254, g) and o.mul(BN254, R, g) is None  # prime order r (cofactor 1)
    assert P.bit_length() == R.bit_length() == 254
    assert P % 4 == 3  # the direct square root
    assert P % 3 == 1 and R % 3 == 1  # cube roots of unity in both fields: GLV (j = 0)
    assert (R - 1) % (1 << 28) == 0 and ((R - 1) >> 28) % 2 == 1  # 2-adicity 28
    assert math.gcd(17, P - 1) == 1 and math.gcd(17, R - 1) == 1  # the sponge's alpha = 17 permutes
    assert (1 << 261) // P == 169 and (1 << 261) // o.PALLAS.p == 127  # head-room of a tight value
    assert R < (1 << 254) and abs(R / (1 << 255) - 0.378) < 0.001  # the scalar stream's acceptance rate per candidate
    assert 0.622 ** 64 < 1e-13  # its fallback


def test_modulus_shape_in_radix_2p29():
    """no zero limb, p_0 != 1, no power-of-two limb: none of the Pallas shortcuts of csrc/fpu.h applies, and the column sums still fit"""
    limbs = [(P >> (29 * i)) & ((1 << 29) - 1) for i in range(9)]
    assert limbs == P_LIMBS_29
    assert all(v != 0 and v & (v - 1) != 0 for v in limbs) and limbs[0] != 1
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


@pytest.mark.parametrize("name,m", [("Bn254Fq", P), ("Bn254Fr", R)])
def test_saturated_tables(name, m):
    blk, tab = _tables(open(os.path.join(CSRC, "fp.h")).read(), name, 8, 32)
    Rm = 1 << 256
    assert tab("mod") == m and tab("one") == Rm % m and tab("r2") == Rm * Rm % m
    assert int(re.search(r"INV = (0x[0-9a-f]+)u", blk).group(1), 16) == (-pow(m, -1, 1 << 32)) % (1 << 32)


def test_unsaturated_table():
    blk, tab = _tables(open(os.path.join(CSRC, "fpu.h")).read(), "Bn254FqU", 9, 29)
    m, R_abi, R_dev = P, 1 << 256, 1 << 261
    assert [int(x) for x in re.findall(r"int (?:L|W|B) = (\d+);", blk)] == [9, 8, 29]
    assert tab("mod") == m and tab("one") == R_dev % m
    assert tab("k_import") == R_dev * R_dev * pow(R_abi, -1, m) % m and tab("k_export") == R_abi % m
    ninv = int(re.search(r"NINV = (0x[0-9a-f]+)u", blk).group(1), 16)
    assert ninv == (-pow(m, -1, 1 << 29)) % (1 << 29) and ninv != (1 << 29) - 1  # the general reduction step


def test_pack_names_stay_in_the_field_headers():
    """everything else follows through SatOf, DevField, CurveOf and the templates"""
    for f in sorted(os.listdir(CSRC)):
        if f in ("fp.h", "fpu.h", "fp_mul_gfx950.h"):
            continue
        src = open(os.path.join(CSRC, f)).read()
        assert "Bn254FqU" not in src, f
        if f not in ("curves.h", "kern_bn254.hip", "kern_fr.hip", "api_types.h"):  # the table, the two units, the sponge's state tuple
            assert "Bn254F" not in src, f


def test_generated_multiplication_header_is_current():
    out = subprocess.run(["python3", os.path.join(ROOT, "tools", "gen_fp_asm.py")], capture_output=True, text=True, check=True).stdout
    assert out == open(os.path.join(CSRC, "fp_mul_gfx950.h")).read()
    for fn in ("fe_mul<Bn254Fq>", "fe_mul<Bn254Fr>", "fe_dot2<Bn254Fr>", "fe_dot3<Bn254Fr>"):
        assert fn in out, fn


# ---- the curve id ----------------------------------------------------------------------------------------------------------------------
def test_id_4_is_accepted_where_3_and_5_are_refused(built_lib):
    from accumulation_amd import ffi
    from accumulation_amd.engine import Context
    assert ffi.AMSM_BN254_G1 == 4
    a = np.ones(4, dtype=np.uint64)
    for bad in (3, 5):
        with pytest.raises(Exception):
            Context(bad, device=ffi.AMSM_DEVICE_HOST)
        assert built_lib.amsm_fr_to_mont(bad, a.ctypes.data, 1, a.ctypes.data) == ffi.AMSM_E_INVALID_ARG
        assert built_lib.amsm_point_serialized_size(bad, 1) == 0 and built_lib.amsm_fr_serialized_size(bad) == 0
    ctx = Context(4, device=ffi.AMSM_DEVICE_HOST)
    assert ctx.curve == 4 and ctx.fq_limbs == 4
    ctx.close()
    assert built_lib.amsm_fr_to_mont(4, a.ctypes.data, 1, a.ctypes.data) == ffi.AMSM_OK
    assert o.limbs_to_int([int(v) for v in a]) == o.fr_to_mont(BN254, 1 + (1 << 64) + (1 << 128) + (1 << 192))


def test_python_tables():
    from accumulation_amd import AMSM_BN254_G1, ipa_pc
    from accumulation_amd.scalar_field import MODULI, Fr
    assert AMSM_BN254_G1 == 4 and MODULI[AMSM_BN254_G1] == R
    assert ipa_pc.IPA_FOLD[AMSM_BN254_G1] == ipa_pc.IPA_FOLD[0]
    fr = Fr(AMSM_BN254_G1)
    assert fr.from_limbs(fr.to_limbs(R - 1)) == R - 1


# ---- host helpers ----------------------------------------------------------------------------------------------------------------------
def test_fr_helpers(built_lib):
    from tests import test_host_fr_cpu as t
    t.test_host_fr_helpers(built_lib, BN254)
    t.test_host_fr_inverse_many(built_lib, BN254)


def test_host_lincomb(built_lib):
    from tests import test_host_fr_cpu as t
    t.test_host_lincomb_vs_oracle(built_lib, BN254)
    t.test_host_lincomb_batch_equals_single_calls_and_oracle(built_lib, BN254)


def test_glv_pairing_and_split():
    """host_glv.h on BN254: lambda and beta pair up, [lambda] G = (beta Gx, Gy), and edge scalars split into short halves that give
    the same point (tests/cpp_host/bn254_glv_check.cpp)"""
    out = os.path.join(ROOT, "build", "bn254_glv_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["hipcc", "-std=c++17", "-O2", "--offload-host-only", "--offload-arch=gfx950", "-x", "hip", "-w",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp_host", "bn254_glv_check.cpp"), "-o", out])
    res = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lam, beta = (int(x, 16) for x in re.search(r"lambda (\w+) beta (\w+)", res.stdout).groups())
    g = o.generator(BN254)
    assert 1 < lam < R and 1 < beta < P and pow(lam, 3, R) == 1 and pow(beta, 3, P) == 1
    assert o.mul(BN254, lam, g) == (beta * g[0] % P, g[1])
    assert "OK" in res.stdout


# ---- wire format -----------------------------------------------------------------------------------------------------------------------
def test_wire_format(built_lib, bn254_by_name):
    from tests import test_wire_format_cpu as t
    t.test_scalars(built_lib, BN254.name)
    for compressed in (True, False):
        t.test_points(built_lib, BN254.name, compressed)
    t.test_rejections(built_lib, BN254.name)
    # 254 bits + 2 flag bits fill 32 bytes exactly: no 33rd byte as on the 255-bit curves
    assert built_lib.amsm_fr_serialized_size(4) == 32
    assert built_lib.amsm_point_serialized_size(4, 1) == ser.point_size(BN254, True) == 32
    assert built_lib.amsm_point_serialized_size(4, 0) == ser.point_size(BN254, False) == 64


def test_generator_encoding_flag_bits_and_rejections(built_lib):
    from tests.test_wire_format_cpu import lib_points_deserialize, lib_points_serialize
    g = o.generator(BN254)
    (blob,), sz = lib_points_serialize(built_lib, BN254, [g], True)
    # x = 1 little-endian; y = 2 is the smaller root: no flag bit
    assert sz == 32 and blob == (1).to_bytes(32, "little") == ser.point_serialize(BN254, g)
    rc, (back,) = lib_points_deserialize(built_lib, BN254, [blob], True)
    assert rc == 0 and back == g
    # -G: the larger root, bit 7 of the last byte -- beside the top bits of a 254-bit x in the same byte
    ng = o.neg(BN254, g)
    (nblob,), _ = lib_points_serialize(built_lib, BN254, [ng], True)
    assert nblob == b"\x01" + bytes(30) + b"\x80" == ser.point_serialize(BN254, ng)
    assert lib_points_deserialize(built_lib, BN254, [nblob], True) == (0, [ng])
    # a point whose x has bit 253 set keeps it under both flags' bits
    big = next(pt for kind in ("plain_x_at_p_minus_1",) for pt in _fixture_points(kind))
    for pt in (big, o.neg(BN254, big)):
        (b,), _ = lib_points_serialize(built_lib, BN254, [pt], True)
        assert b == ser.point_serialize(BN254, pt) and (b[31] & 0x3F) == (pt[0] >> 248) and lib_points_deserialize(built_lib, BN254, [b], True) == (0, [pt])
    # the identity: bit 6, x = 0; both flag bits: invalid
    (iblob,), _ = lib_points_serialize(built_lib, BN254, [None], True)
    assert iblob == bytes(31) + b"\x40" and lib_points_deserialize(built_lib, BN254, [iblob], True) == (0, [None])
    assert lib_points_deserialize(built_lib, BN254, [bytes(31) + b"\xc0"], True)[0] != 0
    # uncompressed: x without flags, y with the infinity bit only
    (ublob,), usz = lib_points_serialize(built_lib, BN254, [ng], False)
    assert usz == 64 and ublob == (1).to_bytes(32, "little") + (P - 2).to_bytes(32, "little") == ser.point_serialize(BN254, ng, False)
    assert lib_points_deserialize(built_lib, BN254, [ublob], False) == (0, [ng])
    assert lib_points_deserialize(built_lib, BN254, [(1).to_bytes(32, "little") + (3).to_bytes(32, "little")], False)[0] != 0  # off the curve
    # x >= p: p itself and the largest 254-bit integer (p < 2^254, so both fit beside the flags), compressed and uncompressed
    for x in (P, (1 << 254) - 1):
        assert lib_points_deserialize(built_lib, BN254, [x.to_bytes(32, "little")], True)[0] != 0
        assert lib_points_deserialize(built_lib, BN254, [x.to_bytes(32, "little") + (2).to_bytes(32, "little")], False)[0] != 0
    x = 1
    while ser._sqrt(x * x * x + BN254.b, P) is not None:  # an x with no point on the curve
        x += 1
    assert lib_points_deserialize(built_lib, BN254, [x.to_bytes(32, "little")], True)[0] != 0


# ---- Poseidon --------------------------------------------------------------------------------------------------------------------------
def test_poseidon(built_lib, bn254_by_name):
    from tests import test_poseidon_cpu as t
    t.test_round_constants_and_permutation(built_lib, BN254.name)
    t.test_duplex_sequences(built_lib, BN254.name)
    t.test_encodings_fork_and_challenges(built_lib, BN254.name)
    # the sponge is its own: the other 4-limb fields' round constants are over other moduli
    assert pp.PoseidonSponge(P).ark != pp.PoseidonSponge(o.PALLAS.p).ark


# ---- host backend: MSMs over the adversarial points ---------------------------------------------------------------------------------------
def _fixture_points(kind=None):
    out = []
    for k, pts in FIX["curves"][BN254.name].items():
        if kind is None or k == kind:
            out += [(int(x, 16), int(y, 16)) for x, y in pts]
    return out


def test_adversarial_fixture_is_what_it_claims():
    assert FIX["internal_radix_bits"] == {BN254.name: 261}
    Rd, half = 1 << 261, (P - 1) // 2
    kinds = FIX["curves"][BN254.name]
    assert 40 <= sum(len(v) for v in kinds.values()) <= 60
    for kind, pts in kinds.items():
        radix, coord, name = kind.split("_", 2)
        for x, y in pts:
            pt = (int(x, 16), int(y, 16))
            assert o.is_on_curve(BN254, pt) and o.mul(BN254, R, pt) is None
            v = (pt[1] if coord == "y" else pt[0]) * (Rd if radix == "internal" else 1) % P
            target = {"at_0": 0, "at_1": 1, "at_p_minus_1": P - 1, "at_half_minus": half, "at_half_plus": half + 1,
                      "low_limbs_all_ones": (1 << 232) - 1, "top_limb_only": (P >> 232) << 232, "just_above_2p232": 1 << 232}[name]
            assert abs(v - target) < 64, kind  # (a coordinate gives a point with probability about 1 / 2 (x) or 1 / 3 (y))
    limbs = lambda v: [(v >> (29 * i)) & ((1 << 29) - 1) for i in range(9)]  # noqa: E731
    lo = limbs(int(kinds["internal_y_low_limbs_all_ones"][0][1], 16) * Rd % P)
    assert lo[8] == 0 and lo[1:8] == [(1 << 29) - 1] * 7
    hi = limbs(int(kinds["internal_y_top_limb_only"][0][1], 16) * Rd % P)
    assert hi[8] == P_LIMBS_29[8] and hi[1:8] == [0] * 7
    pair = FIX["negated_doubling_pair"]
    l, r = ((int(pair[k][0], 16), int(pair[k][1], 16)) for k in ("l", "r"))
    assert o.is_on_curve(BN254, l) and o.is_on_curve(BN254, r) and r[1] * Rd % P < 1 << 232


def adversarial(seed, n):
    """n points: the fixture's, each also doubled up, negated and in the negated-doubling shape (P, P, -P, P), then stream points with
    identities, duplicates and P / -P pairs; scalars with 0, 1, r - 1 and equal digits on the duplicates among them"""
    fix = _fixture_points()
    pts = []
    for pt in fix:
        pts += [pt, pt, o.neg(BN254, pt), pt]
    pair = FIX["negated_doubling_pair"]
    pts += [(int(pair[k][0], 16), int(pair[k][1], 16)) for k in ("l", "r", "r")]
    head = len(pts)
    assert head < n
    pts += o.rng_points(BN254, seed, n - head)
    for i in range(head, n, 97):
        pts[i] = None
    for i in range(head + 5, n, 61):
        pts[i] = pts[i - 3]
    for i in range(head + 11, n, 53):
        pts[i] = o.neg(BN254, pts[i - 1])
    sc = [o.rng_fr(BN254, seed + 1, i) for i in range(n)]
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
    xy, inf = run_msm(host_ctx, BN254, pts, sc, flags)
    assert h.np_to_point(BN254, xy, inf) == o.msm_pippenger(BN254, pts, sc)
    # P + (-P) and an identity alone
    xy, inf = run_msm(host_ctx, BN254, [pts[0], pts[2]], [5, 5], flags)
    assert h.np_to_point(BN254, xy, inf) is None and pts[2] == o.neg(BN254, pts[0])


def test_host_bases_generate_matches_the_oracle_stream(host_ctx):
    """G_i = k_i G with the 254-bit multiplier stream taken over the integers: some k_i exceed r here (r < 2^254)"""
    from accumulation_amd import CommitterKey, ffi
    assert any(o.rng_scalar(99, i) >= R for i in range(64))
    ck = CommitterKey.generate(host_ctx, 99, 64, ffi.AMSM_BASES_NO_PRECOMPUTE)
    xy, inf = ck.read()
    assert [h.np_to_point(BN254, xy[i], inf[i]) for i in range(64)] == o.rng_points(BN254, 99, 64)
    ck.free()


def test_host_vec_random_is_uniform_below_r(host_ctx):
    """amsm_vec_random over r: the rejection rule of pyref.rng_fr restated with BN254's r, whose candidates fail 62 % of the time"""
    v = host_ctx.random_vector(7, 300, False)
    got = h.np_to_ints(v.download())
    assert got == [o.rng_fr(BN254, 7, i) for i in range(300)] and all(x < R for x in got)
    assert any(x >> 253 for x in got)  # (the top bit of the field is reached)


def test_host_bases_sample_against_the_python_sampler(host_ctx):
    """amsm_bases_sample: one 254-bit digest word and the direct square root together, against tests/sample_ref.py"""
    from accumulation_amd.engine import CommitterKey
    from accumulation_amd import ffi
    from tests import sample_ref as sr
    for first, n in ((0, 48), ((1 << 32) + 5, 16)):  # 64 indices
        ck = CommitterKey.sample(host_ctx, b"PC-DL-2020", n, ffi.AMSM_BASES_NO_PRECOMPUTE, first=first)
        xy, inf = ck.read()
        ck.free()
        want = sr.sample(BN254, b"PC-DL-2020", first, n)
        assert not inf.any() and np.array_equal(xy, sr.to_words(BN254, want))
        assert all(o.is_on_curve(BN254, pt) for pt in want) and len(set(want)) == n


def points_check_case(extra=0):
    """(xy, infinity bytes, expected statuses, index of the first bad point): the fixture's points and `extra + 10` copies of the
    generator, eight of them overwritten with non-canonical words, points off the curve and the identity's forms"""
    pts = _fixture_points()
    xy, _ = h.points_to_np(BN254, pts + [o.generator(BN254)] * (10 + extra))
    n = xy.shape[0]
    want = np.zeros(n, dtype=np.uint8)
    raw = lambda v: np.array(o.int_to_limbs(v, 4), dtype=np.uint64)  # noqa: E731
    k = len(pts)
    xy[k, :4], want[k] = raw(P), 1                          # x = p
    xy[k + 1, 4:], want[k + 1] = raw(P + 1), 1              # y = p + 1
    xy[k + 2, :4], want[k + 2] = raw((1 << 256) - 1), 1     # every bit set
    xy[k + 3, 4:], want[k + 3] = raw(P - 1), 2              # canonical words, off the curve
    xy[k + 4, :4], want[k + 4] = xy[k + 4, 4:], 2           # (y, y)
    xy[k + 5] = 0                                           # (0, 0): the identity
    xy[k + 6, 4:], want[k + 6] = 0, 2                       # (x, 0)
    inf = np.zeros(n, dtype=np.uint8)
    xy[k + 7, :4], inf[k + 7] = raw(P), 1                   # flagged infinite: the words are ignored
    xy[n - 1, 4:], want[n - 1] = raw(P), 1                  # the last point: y = p
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
    return BN254, host_ctx


def test_scheme_transcripts(env):
    """the four schemes on the host backend: every challenge the product squeezes equals the one the oracle derives from the
    public data alone (oracle/pyref_transcript.py over the BN254 Fq sponge)"""
    from tests import test_transcripts_vs_oracle as t
    t.test_hp_as_transcript(env, 2, 1, True)
    t.test_trivial_pc_as_transcript(env, 2, 0)
    t.test_r1cs_nark_as_transcript(env, 2, 1, True)
    t.test_ipa_pc_as_transcript(env, 1, 1, True)


@pytest.mark.parametrize("scheme,lg", [("hp_as", 6), ("r1cs_nark_as", 5), ("ipa_pc_as", 4), ("trivial_pc_as", 5)])
def test_profile_as_dump_equals_the_mirror(built_lib, tmp_path, scheme, lg):
    """`profile_as --curve 4 --dump` on the host backend, byte for byte against the Python mirror (tests/harness_mirror.py)"""
    from tests.test_profile_as_dump import compare
    compare(tmp_path, scheme, lg, "harness", "poseidon", -1, seed=6, curve=4)
