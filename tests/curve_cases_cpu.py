"""The cases without a GPU that Vesta, BN254 G1, Grumpkin and BLS12-377 G1 share, each written once: tests/test_<curve>_cpu.py takes
from here the fixtures and the cases its row of tests/curve_rows.py lists (Row.cpu_cases), under its own module name, and adds the
curve's own -- the facts its port rests on, the shape of its modulus, its encoding's flag bits.  Shared: the field tables compiled into
the HIP code, the host scalar-field helpers, the GLV set-up, the wire format, the Poseidon sponge, host linear combinations, MSMs over
the adversarial-point fixtures, the key streams, transparent keys, point validation and the four schemes on the library's host
backend, and the C++ drivers' dumps -- each against the big-int oracle with the `Curve` objects of tests/helpers.py (oracle/ knows
curves 0 and 1 only and is curve-generic)."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyref as o
from oracle import pyref_poseidon as pp
from oracle import pyref_ser as ser
from oracle import pyref_transcript as ot  # noqa: F401  (the transcript tests below run against it)
from tests import curve_rows as cr
from tests import helpers as h
from tests.curve_rows import CSRC, ROOT, _fixture_points, _tables

SHARED = ("row", "by_name", "host_ctx", "env")  # what every per-curve module takes beside its cases


@pytest.fixture(scope="module")
def row(request):
    return request.module.ROW


@pytest.fixture
def by_name(monkeypatch, row):
    """the curve-parametrised modules look curves up by name in the oracle's table: add the row's curve for the duration of one test"""
    monkeypatch.setitem(o.CURVES, row.curve.name, row.curve)
    monkeypatch.setitem(o.CURVES_BY_ID, row.curve.curve_id, row.curve)


@pytest.fixture
def host_ctx(built_lib, row):
    from accumulation_amd import Context, ffi
    ctx = Context(getattr(ffi, row.ffi), device=ffi.AMSM_DEVICE_HOST)
    yield ctx
    ctx.close()


# ---- the field tables ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", ["Fq", "Fr"])
def test_saturated_tables(row, field):
    src = open(os.path.join(CSRC, "fp.h")).read()
    name, m = (row.packs[0], row.P) if field == "Fq" else (row.packs[2], row.R)
    words = (m.bit_length() + 63) // 64 * 2
    blk, tab = _tables(src, name, words, 32)
    Rm = 1 << (32 * words)
    assert tab("mod") == m and tab("one") == Rm % m and tab("r2") == Rm * Rm % m
    assert int(re.search(r"INV = (0x[0-9a-f]+)u", blk).group(1), 16) == (-pow(m, -1, 1 << 32)) % (1 << 32)
    assert [int(x) for x in re.findall(r"int (?:L|W) = (\d+);", blk)] == [words, words]
    if row.twins:  # the tables of the other curve's other field
        _, ttab = _tables(src, row.twins[field == "Fr"], 8, 32)
        assert all(tab(t) == ttab(t) for t in ("mod", "one", "r2"))
    if row.dev_field:
        assert "struct DevField<" + row.packs[0] + ">" in src


def test_unsaturated_table(row):
    L, B = row.unsat
    W = 2 * row.curve.limbs
    blk, tab = _tables(open(os.path.join(CSRC, "fpu.h")).read(), row.packs[1], L, B)
    m, R_abi, R_dev = row.P, 1 << (32 * W), 1 << (L * B)
    assert [int(x) for x in re.findall(r"int (?:L|W|B) = (\d+);", blk)] == [L, W, B]
    assert tab("mod") == m and tab("one") == R_dev % m
    assert tab("k_import") == R_dev * R_dev * pow(R_abi, -1, m) % m and tab("k_export") == R_abi % m
    ninv = int(re.search(r"NINV = (0x[0-9a-f]+)u", blk).group(1), 16)
    assert ninv == (-pow(m, -1, 1 << B)) % (1 << B)
    assert (ninv == (1 << B) - 1) == (m % (1 << B) == 1)  # the p_0 = 1 reduction step (Vesta, BLS12-377), else the general one
    if row.dev_field:
        assert "using Sat = " + row.packs[0] + ";" in blk


def test_pack_names_stay_in_the_field_headers(row):
    """everything else follows through SatOf, DevField, CurveOf and the templates; the curve's unit names no pack of another curve"""
    fq, fqu, fr = row.packs
    unit_name = "kern_" + row.id + ".hip"
    for f in sorted(os.listdir(CSRC)):
        if f in ("fp.h", "fpu.h", "fp_mul_gfx950.h"):
            continue
        src = open(os.path.join(CSRC, f)).read()
        assert fqu not in src, f
        if f not in ("curves.h", unit_name, "kern_fr.hip", "api_types.h"):  # the table, the two units, the sponge's state tuple
            assert fq[:-1] not in src, f
    unit = open(os.path.join(CSRC, unit_name)).read()
    # the unit names the base field; the scalar field and the id it is built for are the curve table's (CurveOf<Fq>)
    assert "AMSM_EC_LAUNCHERS(" + fq + ")" in unit and fr not in unit
    table = open(os.path.join(CSRC, "curves.h")).read()
    assert re.search(r"using Fq = %s;\s+using Fr = %s;\s+static constexpr int id = %s;" % (fq, fr, row.ffi), table)
    assert re.search(r"struct CurveOf<%s> \{\s+using type = \w+;" % fq, table)
    assert not any(other.packs[0][:-2] in unit for other in cr.ROWS if other is not row) and "Bls12381" not in unit
    assert "AMSM_FR_LAUNCHERS(" + fr + ")" in open(os.path.join(CSRC, "kern_fr.hip")).read()
    from accumulation_amd import build
    assert unit_name in build.UNITS


def test_generated_multiplication_header_is_current(row):
    out = subprocess.run(["python3", os.path.join(ROOT, "tools", "gen_fp_asm.py")], capture_output=True, text=True, check=True).stdout
    assert out == open(os.path.join(CSRC, "fp_mul_gfx950.h")).read()
    fq, _, fr = row.packs
    for fn in ("fe_mul<%s>" % fq, "fe_mul<%s>" % fr) + (("fe_dot2<%s>" % fr, "fe_dot3<%s>" % fr) if row.fr_dots else ()):
        assert fn in out, fn
    if row.header_extra:
        row.header_extra(out)


# ---- the curve id ----------------------------------------------------------------------------------------------------------------------
def test_id_is_accepted_where_its_neighbours_are_refused(built_lib, row):
    from accumulation_amd import ffi
    from accumulation_amd.engine import Context
    C, cid = row.curve, row.curve.curve_id
    assert getattr(ffi, row.ffi) == cid
    a = np.ones(4, dtype=np.uint64)
    for bad in row.refused_ids:
        with pytest.raises(Exception):
            Context(bad, device=ffi.AMSM_DEVICE_HOST)
        assert built_lib.amsm_fr_to_mont(bad, a.ctypes.data, 1, a.ctypes.data) == ffi.AMSM_E_INVALID_ARG
        assert built_lib.amsm_point_serialized_size(bad, 1) == 0 and built_lib.amsm_fr_serialized_size(bad) == 0
    ctx = Context(cid, device=ffi.AMSM_DEVICE_HOST)
    assert ctx.curve == cid and ctx.fq_limbs == C.limbs
    ctx.close()
    assert built_lib.amsm_fr_to_mont(cid, a.ctypes.data, 1, a.ctypes.data) == ffi.AMSM_OK
    assert o.limbs_to_int([int(v) for v in a]) == o.fr_to_mont(C, 1 + (1 << 64) + (1 << 128) + (1 << 192))
    assert built_lib.amsm_fr_serialized_size(cid) == 32
    assert (built_lib.amsm_point_serialized_size(cid, 1), built_lib.amsm_point_serialized_size(cid, 0)) == row.wire


def test_python_tables(row):
    import accumulation_amd
    from accumulation_amd import ipa_pc
    from accumulation_amd.scalar_field import MODULI, Fr
    cid, R = row.curve.curve_id, row.R
    assert getattr(accumulation_amd, row.ffi) == cid and MODULI[cid] == R
    assert all(MODULI[other.curve.curve_id] == row.P for other in cr.ROWS if other.R == row.P)  # the cycle's other half
    assert ipa_pc.IPA_FOLD[cid] == ipa_pc.IPA_FOLD[row.ipa_fold_of] and (row.ipa_fold_of == 0 or ipa_pc.IPA_FOLD[cid] == (16, 15))  # BLS12-381's, unmeasured
    a, b = ipa_pc.IPA_FOLD[cid]
    hpp = open(os.path.join(ROOT, "include", "amsm.hpp")).read()
    assert re.search(r"case %s: return \{%d, %d, %d\};" % (row.ffi, row.curve.limbs, a, b), hpp)
    assert re.search(r"%s = %d," % (row.ffi, cid), open(os.path.join(ROOT, "include", "amsm.h")).read())
    fr = Fr(cid)
    assert fr.from_limbs(fr.to_limbs(R - 1)) == R - 1


# ---- host helpers ----------------------------------------------------------------------------------------------------------------------
def test_fr_helpers(built_lib, row):
    from tests import test_host_fr_cpu as t
    t.test_host_fr_helpers(built_lib, row.curve)
    t.test_host_fr_inverse_many(built_lib, row.curve)


def test_host_lincomb(built_lib, row):
    from tests import test_host_fr_cpu as t
    t.test_host_lincomb_vs_oracle(built_lib, row.curve)
    t.test_host_lincomb_batch_equals_single_calls_and_oracle(built_lib, row.curve)


def test_glv_pairing_and_split(row):
    """host_glv.h on the row's curve: lambda and beta pair up, [lambda] G = (beta Gx, Gy), and edge scalars split into short halves
    that give the same point (tests/cpp_host/curve_glv_check.cpp, compiled over the row's field packs)"""
    C, P, R = row.curve, row.P, row.R
    out = os.path.join(ROOT, "build", row.id + "_glv_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["hipcc", "-std=c++17", "-O2", "--offload-host-only", "--offload-arch=gfx950", "-x", "hip", "-w",
                           "-DGLV_FQ=" + row.packs[0], "-DGLV_FR=" + row.packs[2],
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp_host", "curve_glv_check.cpp"), "-o", out])
    res = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lam, beta = (int(x, 16) for x in re.search(r"lambda (\w+) beta (\w+)", res.stdout).groups())
    g = o.generator(C)
    assert 1 < lam < R and 1 < beta < P and pow(lam, 3, R) == 1 and pow(beta, 3, P) == 1
    assert o.mul(C, lam, g) == (beta * g[0] % P, g[1])
    assert "OK" in res.stdout


# ---- wire format -----------------------------------------------------------------------------------------------------------------------
def test_wire_format(built_lib, row, by_name):
    from tests import test_wire_format_cpu as t
    C, cid = row.curve, row.curve.curve_id
    t.test_scalars(built_lib, C.name)
    for compressed in (True, False):
        t.test_points(built_lib, C.name, compressed)
    t.test_rejections(built_lib, C.name)
    # the field's bits + 2 flag bits: 254 bits fill 32 bytes exactly (no 33rd byte as on the 255-bit curves), 377 take 48
    assert built_lib.amsm_fr_serialized_size(cid) == ser.fp_size(row.R) == 32
    assert built_lib.amsm_point_serialized_size(cid, 1) == ser.point_size(C, True) == row.wire[0]
    assert built_lib.amsm_point_serialized_size(cid, 0) == ser.point_size(C, False) == row.wire[1]


def test_generator_encoding_flag_bits_and_rejections(built_lib, row):
    """BN254 and Grumpkin: the generator is (1, y), 254 bits beside two flag bits"""
    from tests.test_wire_format_cpu import lib_points_deserialize, lib_points_serialize
    C, P, GY = row.curve, row.P, row.curve.gy
    g = o.generator(C)
    (blob,), sz = lib_points_serialize(built_lib, C, [g], True)
    # x = 1 little-endian; y (2, or Grumpkin's 195 bits) is the smaller root: no flag bit
    assert GY < P - GY
    assert sz == 32 and blob == (1).to_bytes(32, "little") == ser.point_serialize(C, g)
    rc, (back,) = lib_points_deserialize(built_lib, C, [blob], True)
    assert rc == 0 and back == g
    # -G: the larger root, bit 7 of the last byte -- beside the top bits of a 254-bit x in the same byte
    ng = o.neg(C, g)
    (nblob,), _ = lib_points_serialize(built_lib, C, [ng], True)
    assert nblob == b"\x01" + bytes(30) + b"\x80" == ser.point_serialize(C, ng)
    assert lib_points_deserialize(built_lib, C, [nblob], True) == (0, [ng])
    # a point whose x has bit 253 set keeps it under both flags' bits
    big = next(pt for kind in ("plain_x_at_p_minus_1",) for pt in _fixture_points(row, kind))
    for pt in (big, o.neg(C, big)):
        (b,), _ = lib_points_serialize(built_lib, C, [pt], True)
        assert b == ser.point_serialize(C, pt) and (b[31] & 0x3F) == (pt[0] >> 248) and lib_points_deserialize(built_lib, C, [b], True) == (0, [pt])
    # the identity: bit 6, x = 0; both flag bits: invalid
    (iblob,), _ = lib_points_serialize(built_lib, C, [None], True)
    assert iblob == bytes(31) + b"\x40" and lib_points_deserialize(built_lib, C, [iblob], True) == (0, [None])
    assert lib_points_deserialize(built_lib, C, [bytes(31) + b"\xc0"], True)[0] != 0
    # uncompressed: x without flags, y with the infinity bit only
    (ublob,), usz = lib_points_serialize(built_lib, C, [ng], False)
    assert usz == 64 and ublob == (1).to_bytes(32, "little") + (P - GY).to_bytes(32, "little") == ser.point_serialize(C, ng, False)
    assert lib_points_deserialize(built_lib, C, [ublob], False) == (0, [ng])
    assert lib_points_deserialize(built_lib, C, [(1).to_bytes(32, "little") + (GY + 1).to_bytes(32, "little")], False)[0] != 0  # off the curve
    # x >= p: p itself and the largest 254-bit integer (p < 2^254, so both fit beside the flags), compressed and uncompressed
    for x in (P, (1 << 254) - 1):
        assert lib_points_deserialize(built_lib, C, [x.to_bytes(32, "little")], True)[0] != 0
        assert lib_points_deserialize(built_lib, C, [x.to_bytes(32, "little") + GY.to_bytes(32, "little")], False)[0] != 0
    x = 1
    while ser._sqrt(x * x * x + C.b, P) is not None:  # an x with no point on the curve
        x += 1
    assert lib_points_deserialize(built_lib, C, [x.to_bytes(32, "little")], True)[0] != 0


# ---- Poseidon --------------------------------------------------------------------------------------------------------------------------
def test_poseidon(built_lib, row, by_name):
    from tests import test_poseidon_cpu as t
    t.test_round_constants_and_permutation(built_lib, row.curve.name)
    t.test_duplex_sequences(built_lib, row.curve.name)
    t.test_encodings_fork_and_challenges(built_lib, row.curve.name)
    # the sponge is its own: the other fields' round constants are over other moduli
    assert all(pp.PoseidonSponge(row.P).ark != pp.PoseidonSponge(q).ark for q in row.other_sponges)


# ---- host backend: MSMs over the adversarial points ---------------------------------------------------------------------------------------
def test_adversarial_fixture_is_what_it_claims(row):
    """BN254 and Grumpkin: the 9 x 29-bit fields' fixtures (BLS12-377's has its own kinds: tests/test_bls12_377_cpu.py)"""
    C, P, R = row.curve, row.P, row.R
    FIX = cr.fixture(row)
    assert FIX["internal_radix_bits"] == {C.name: 261}
    Rd, half = 1 << 261, (P - 1) // 2
    kinds = FIX["curves"][C.name]
    assert 40 <= sum(len(v) for v in kinds.values()) <= 60
    for kind, pts in kinds.items():
        radix, coord, name = kind.split("_", 2)
        for x, y in pts:
            pt = (int(x, 16), int(y, 16))
            assert o.is_on_curve(C, pt) and o.mul(C, R, pt) is None
            v = (pt[1] if coord == "y" else pt[0]) * (Rd if radix == "internal" else 1) % P
            target = {"at_0": 0, "at_1": 1, "at_p_minus_1": P - 1, "at_half_minus": half, "at_half_plus": half + 1,
                      "low_limbs_all_ones": (1 << 232) - 1, "top_limb_only": (P >> 232) << 232, "just_above_2p232": 1 << 232}[name]
            assert abs(v - target) < 64, kind  # (a coordinate gives a point with probability about 1 / 2 (x) or 1 / 3 (y))
    limbs = lambda v: [(v >> (29 * i)) & ((1 << 29) - 1) for i in range(9)]  # noqa: E731
    lo = limbs(int(kinds["internal_y_low_limbs_all_ones"][0][1], 16) * Rd % P)
    assert lo[8] == 0 and lo[1:8] == [(1 << 29) - 1] * 7
    hi = limbs(int(kinds["internal_y_top_limb_only"][0][1], 16) * Rd % P)
    assert hi[8] == limbs(P)[8] and hi[1:8] == [0] * 7
    l, r = cr.negated_doubling_pair(row)
    assert o.is_on_curve(C, l) and o.is_on_curve(C, r) and r[1] * Rd % P < 1 << 232


@pytest.mark.parametrize("flags", [1, 2], ids=["precomp", "plain"])
def test_host_msm_adversarial(host_ctx, row, flags):
    from tests.test_msm_gpu import run_msm
    C, (i, j) = row.curve, row.cancel_pair
    pts, sc = cr.adversarial(row, 21, row.host_adv_n)
    xy, inf = run_msm(host_ctx, C, pts, sc, flags)
    assert h.np_to_point(C, xy, inf) == o.msm_pippenger(C, pts, sc)
    # P + (-P) and an identity alone
    xy, inf = run_msm(host_ctx, C, [pts[i], pts[j]], [5, 5], flags)
    assert h.np_to_point(C, xy, inf) is None and pts[j] == o.neg(C, pts[i])


def test_host_bases_generate_matches_the_oracle_stream(host_ctx, row):
    """G_i = k_i G with the 254-bit multiplier stream taken over the integers: some k_i exceed r where r < 2^254, most where r < 2^253"""
    from accumulation_amd import CommitterKey, ffi
    C = row.curve
    assert sum(o.rng_scalar(99, i) >= row.R for i in range(64)) >= row.over_r[1]
    ck = CommitterKey.generate(host_ctx, 99, 64, ffi.AMSM_BASES_NO_PRECOMPUTE)
    xy, inf = ck.read()
    assert [h.np_to_point(C, xy[i], inf[i]) for i in range(64)] == o.rng_points(C, 99, 64)
    ck.free()


def test_host_vec_random_is_uniform_below_r(host_ctx, row):
    """amsm_vec_random over r: the rejection rule of pyref.rng_fr restated with the row's r (cref's version knows only curves 0 and 1);
    BN254's r and Grumpkin's fail 62 % of the candidates"""
    v = host_ctx.random_vector(7, 300, False)
    got = h.np_to_ints(v.download())
    assert got == [o.rng_fr(row.curve, 7, i) for i in range(300)] and all(x < row.R for x in got)
    if row.vec_top_bit:
        assert any(x >> (row.R.bit_length() - 1) for x in got)  # (the top bit of the field is reached)


def test_host_bases_sample_against_the_python_sampler(host_ctx, row, monkeypatch):
    """amsm_bases_sample against tests/sample_ref.py -- BN254: one 254-bit digest word and the direct square root together; Grumpkin:
    Tonelli-Shanks with 2-adicity 28 (h_sqrt), b = q - 17 reaching the sampler through curve_b_mont; BLS12-377: two digest words cut
    to 377 bits, Tonelli-Shanks with 2-adicity 46 on a 12-word field and the multiplication by the even cofactor"""
    from accumulation_amd.engine import CommitterKey
    from accumulation_amd import ffi
    from tests import sample_ref as sr
    C = row.curve
    if row.cofactor != 1:
        monkeypatch.setattr(sr, "cofactor", lambda c: row.cofactor if c.curve_id == C.curve_id else 1)
    for first, n in row.host_samples:
        ck = CommitterKey.sample(host_ctx, b"PC-DL-2020", n, ffi.AMSM_BASES_NO_PRECOMPUTE, first=first)
        xy, inf = ck.read()
        ck.free()
        want = sr.sample(C, b"PC-DL-2020", first, n)
        assert not inf.any() and np.array_equal(xy, sr.to_words(C, want))
        assert all(o.is_on_curve(C, pt) and o.mul(C, row.R, pt) is None for pt in want) and len(set(want)) == n


def test_host_points_check(host_ctx, row):
    """amsm_points_check: non-canonical words, points off the curve, the identity forms; status 3 is never reported where the cofactor
    is 1, and on BLS12-377 for (p - 1, 0), (0, 1), (2, 3) and four points [r]Q or Q outside the subgroup"""
    from accumulation_amd import CommitterKey, ffi
    from tests.test_points_check_cpu import report_of
    xy, inf, want, k = cr.points_check_case(row)
    assert (want == 3).sum() == row.off_subgroup and not want[:k].any()
    rep, st = host_ctx.check_points(xy, inf, want_status=True)
    assert np.array_equal(st, want) and rep == report_of(want) and rep["off_subgroup"] == row.off_subgroup and rep["first_bad"] == k
    with pytest.raises(ffi.AmsmError) as e:
        CommitterKey.load(host_ctx, xy, inf, flags=ffi.AMSM_BASES_CHECK | ffi.AMSM_BASES_NO_PRECOMPUTE)
    assert e.value.status == ffi.AMSM_E_INVALID_POINT
    ok = want == 0
    ck = CommitterKey.load(host_ctx, np.ascontiguousarray(xy[ok]), np.ascontiguousarray(inf[ok]), flags=ffi.AMSM_BASES_CHECK | ffi.AMSM_BASES_NO_PRECOMPUTE)
    assert len(ck) == int(ok.sum())
    ck.free()


# ---- the schemes ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def env(host_ctx, row):
    return row.curve, host_ctx


def test_scheme_transcripts(env):
    """the four schemes on the host backend: every challenge the product squeezes equals the one the oracle derives from the
    public data alone (oracle/pyref_transcript.py over the row's Fq sponge)"""
    from tests import test_transcripts_vs_oracle as t
    t.test_hp_as_transcript(env, 2, 1, True)
    t.test_trivial_pc_as_transcript(env, 2, 0)
    t.test_r1cs_nark_as_transcript(env, 2, 1, True)
    t.test_ipa_pc_as_transcript(env, 1, 1, True)


@pytest.mark.parametrize("scheme,lg", [("hp_as", 6), ("r1cs_nark_as", 5), ("ipa_pc_as", 4), ("trivial_pc_as", 5)])
def test_profile_as_dump_equals_the_mirror(built_lib, row, tmp_path, scheme, lg):
    """`profile_as --curve <id> --dump` on the host backend, byte for byte against the Python mirror (tests/harness_mirror.py); on
    BLS12-377 the harness stream's 254-bit integers take up to three subtractions of r"""
    from tests.test_profile_as_dump import compare
    compare(tmp_path, scheme, lg, "harness", "poseidon", -1, seed=6, curve=row.curve.curve_id)
