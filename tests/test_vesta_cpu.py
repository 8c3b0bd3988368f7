"""Vesta (AMSM_VESTA = 2, the other half of the Pasta cycle) without a GPU: the field tables compiled into the HIP code, the host
scalar-field helpers, the GLV set-up, the wire format, the Poseidon sponge, the host linear combinations, MSMs and the four schemes
on the library's host backend, and the C++ drivers' dumps -- each against the big-int oracle with a Vesta `Curve` built here
(Fq = Pallas's Fr, Fr = Pallas's Fq, y^2 = x^3 + 5, generator (-1, 2), cofactor 1)."""
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

PALLAS = o.PALLAS
VESTA = o.Curve("vesta", 2, p=PALLAS.r, r=PALLAS.p, b=5, gx=PALLAS.r - 1, gy=2, limbs=4)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "accumulation_amd", "csrc")


@pytest.fixture
def vesta_by_name(monkeypatch):
    """the curve-parametrised modules look curves up by name in the oracle's table: add Vesta for the duration of one test"""
    monkeypatch.setitem(o.CURVES, "vesta", VESTA)
    monkeypatch.setitem(o.CURVES_BY_ID, VESTA.curve_id, VESTA)


@pytest.fixture
def host_ctx(built_lib):
    from accumulation_amd import Context, ffi
    ctx = Context(ffi.AMSM_VESTA, device=ffi.AMSM_DEVICE_HOST)
    yield ctx
    ctx.close()


# ---- the constants ------------------------------------------------------------------------------------------------------------------
def test_curve_facts():
    g = o.generator(VESTA)
    assert o.is_on_curve(VESTA, g) and o.mul(VESTA, VESTA.r, g) is None  # prime order r_V (cofactor 1)
    assert VESTA.p % 3 == 1 and (VESTA.p - 1) % (1 << 32) == 0 and ((VESTA.p - 1) >> 32) % 2 == 1  # 2-adicity 32


def _tables(src, name, limbs, bits):
    blk = src[src.index("struct " + name + " {"):]
    blk = blk[:blk.index("};")]

    def tab(t):
        mm = re.search(r"AMSM_TABLE\(" + t + r", \d+, ([^)]*)\)", blk, re.S)
        vals = [int(x.strip().rstrip("u"), 16) for x in mm.group(1).replace("\n", " ").split(",")]
        assert len(vals) == limbs and all(v < (1 << bits) for v in vals)
        return sum(v << (bits * i) for i, v in enumerate(vals))
    return blk, tab


@pytest.mark.parametrize("name,m", [("VestaFq", PALLAS.r), ("VestaFr", PALLAS.p)])
def test_saturated_tables(name, m):
    blk, tab = _tables(open(os.path.join(CSRC, "fp.h")).read(), name, 8, 32)
    R = 1 << 256
    assert tab("mod") == m and tab("one") == R % m and tab("r2") == R * R % m
    assert int(re.search(r"INV = (0x[0-9a-f]+)u", blk).group(1), 16) == (-pow(m, -1, 1 << 32)) % (1 << 32)


def test_unsaturated_table():
    blk, tab = _tables(open(os.path.join(CSRC, "fpu.h")).read(), "VestaFqU", 9, 29)
    m, R_abi, R_dev = VESTA.p, 1 << 256, 1 << 261
    assert [int(x) for x in re.findall(r"int (?:L|W|B) = (\d+);", blk)] == [9, 8, 29]
    assert tab("mod") == m and tab("one") == R_dev % m
    assert tab("k_import") == R_dev * R_dev * pow(R_abi, -1, m) % m and tab("k_export") == R_abi % m
    assert int(re.search(r"NINV = (0x[0-9a-f]+)u", blk).group(1), 16) == (-pow(m, -1, 1 << 29)) % (1 << 29) == 0x1FFFFFFF
    # the shape the Pallas bound reasoning and zero-limb shortcuts rest on: p_0 = 1, limbs 5-7 zero, top limb 2^22, R' / p = 127
    limbs = [(m >> (29 * i)) & ((1 << 29) - 1) for i in range(9)]
    assert limbs == [0x1, 0x2375908, 0x052A3763, 0x0D31F813, 0x224, 0, 0, 0, 0x400000]
    assert R_dev // m == 127 and R_dev // PALLAS.p == 127


def test_generated_multiplication_header_is_current():
    out = subprocess.run(["python3", os.path.join(ROOT, "tools", "gen_fp_asm.py")], capture_output=True, text=True, check=True).stdout
    assert out == open(os.path.join(CSRC, "fp_mul_gfx950.h")).read()
    assert "fe_mul<VestaFq>" in out and "fe_mul<VestaFr>" in out


# ---- host helpers -----------------------------------------------------------------------------------------------------------------
def test_fr_helpers(built_lib):
    from tests import test_host_fr_cpu as t
    t.test_host_fr_helpers(built_lib, VESTA)
    t.test_host_fr_inverse_many(built_lib, VESTA)


def test_host_lincomb(built_lib):
    from tests import test_host_fr_cpu as t
    t.test_host_lincomb_vs_oracle(built_lib, VESTA)
    t.test_host_lincomb_batch_equals_single_calls_and_oracle(built_lib, VESTA)


def test_glv_pairing_and_split():
    """host_glv.h on Vesta: lambda and beta pair up, [lambda] G = (beta Gx, Gy) (tests/cpp_host/vesta_glv_check.cpp)"""
    out = os.path.join(ROOT, "build", "vesta_glv_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["hipcc", "-std=c++17", "-O2", "--offload-host-only", "--offload-arch=gfx950", "-x", "hip", "-w",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp_host", "vesta_glv_check.cpp"), "-o", out])
    res = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lam, beta = (int(x, 16) for x in re.search(r"lambda (\w+) beta (\w+)", res.stdout).groups())
    g = o.generator(VESTA)
    assert lam < VESTA.r and beta < VESTA.p and pow(lam, 3, VESTA.r) == 1 and pow(beta, 3, VESTA.p) == 1
    assert o.mul(VESTA, lam, g) == (beta * g[0] % VESTA.p, g[1])
    assert "OK" in res.stdout


# ---- wire format ---------------------------------------------------------------------------------------------------------------------
def test_wire_format(built_lib, vesta_by_name):
    from tests import test_wire_format_cpu as t
    t.test_scalars(built_lib, "vesta")
    for compressed in (True, False):
        t.test_points(built_lib, "vesta", compressed)
    t.test_rejections(built_lib, "vesta")
    assert built_lib.amsm_fr_serialized_size(2) == 32
    assert built_lib.amsm_point_serialized_size(2, 1) == ser.point_size(VESTA, True) == 33
    assert built_lib.amsm_point_serialized_size(2, 0) == ser.point_size(VESTA, False) == 65


def test_generator_encoding_and_rejections(built_lib):
    from tests.test_wire_format_cpu import lib_points_deserialize, lib_points_serialize
    g = o.generator(VESTA)
    (blob,), sz = lib_points_serialize(built_lib, VESTA, [g], True)
    # x = p - 1 little-endian; y = 2 is the smaller root: no flag bit
    assert sz == 33 and blob == (VESTA.p - 1).to_bytes(33, "little") == ser.point_serialize(VESTA, g)
    rc, (back,) = lib_points_deserialize(built_lib, VESTA, [blob], True)
    assert rc == 0 and back == g
    x = 1
    while ser._sqrt(x * x * x + VESTA.b, VESTA.p) is not None:  # an x with no point on Vesta
        x += 1
    assert lib_points_deserialize(built_lib, VESTA, [x.to_bytes(33, "little")], True)[0] != 0
    assert lib_points_deserialize(built_lib, VESTA, [VESTA.p.to_bytes(33, "little")], True)[0] != 0  # x = p


# ---- Poseidon --------------------------------------------------------------------------------------------------------------------------
def test_poseidon(built_lib, vesta_by_name):
    from tests import test_poseidon_cpu as t
    t.test_round_constants_and_permutation(built_lib, "vesta")
    t.test_duplex_sequences(built_lib, "vesta")
    t.test_encodings_fork_and_challenges(built_lib, "vesta")
    # the Vesta sponge is its own: Pallas's round constants are over another field
    assert pp.PoseidonSponge(VESTA.p).ark != pp.PoseidonSponge(PALLAS.p).ark


# ---- host backend ----------------------------------------------------------------------------------------------------------------------
def adversarial(seed, n):
    """n points with identities, duplicates and P / -P pairs, and scalars with 0, 1, r - 1 among them"""
    pts = o.rng_points(VESTA, seed, n)
    for i in range(0, n, 97):
        pts[i] = None
    for i in range(5, n, 61):
        pts[i] = pts[i - 3]
    for i in range(11, n, 53):
        pts[i] = o.neg(VESTA, pts[i - 1])
    sc = [o.rng_fr(VESTA, seed + 1, i) for i in range(n)]
    sc[1], sc[2], sc[3] = 0, 1, VESTA.r - 1
    return pts, sc


@pytest.mark.parametrize("flags", [1, 2], ids=["precomp", "plain"])
def test_host_msm_adversarial(host_ctx, flags):
    from tests.test_msm_gpu import run_msm
    pts, sc = adversarial(21, 1 << 10)
    xy, inf = run_msm(host_ctx, VESTA, pts, sc, flags)
    assert h.np_to_point(VESTA, xy, inf) == o.msm_pippenger(VESTA, pts, sc)
    # P + (-P) and an identity alone
    xy, inf = run_msm(host_ctx, VESTA, [pts[10], pts[11]], [5, 5], flags)
    assert h.np_to_point(VESTA, xy, inf) is None and pts[11] == o.neg(VESTA, pts[10])


def test_host_bases_generate_matches_the_oracle_stream(host_ctx):
    from accumulation_amd import CommitterKey, ffi
    ck = CommitterKey.generate(host_ctx, 99, 64, ffi.AMSM_BASES_NO_PRECOMPUTE)
    xy, inf = ck.read()
    assert [h.np_to_point(VESTA, xy[i], inf[i]) for i in range(64)] == o.rng_points(VESTA, 99, 64)
    ck.free()


def test_host_vec_random_is_uniform_below_r(host_ctx):
    """amsm_vec_random over r_V: the rejection rule of pyref.rng_fr restated with VESTA.r (cref's version knows only 0 and 1)"""
    v = host_ctx.random_vector(7, 300, False)
    assert h.np_to_ints(v.download()) == [o.rng_fr(VESTA, 7, i) for i in range(300)]


@pytest.fixture
def env(host_ctx):
    return VESTA, host_ctx


def test_scheme_transcripts(env):
    """the four schemes on the host backend: every challenge the product squeezes equals the one the oracle derives from the
    public data alone (oracle/pyref_transcript.py over the Vesta sponge)"""
    from tests import test_transcripts_vs_oracle as t
    t.test_hp_as_transcript(env, 2, 1, True)
    t.test_trivial_pc_as_transcript(env, 2, 0)
    t.test_r1cs_nark_as_transcript(env, 2, 1, True)
    t.test_ipa_pc_as_transcript(env, 1, 1, True)


@pytest.mark.parametrize("scheme,lg", [("hp_as", 6), ("r1cs_nark_as", 5), ("ipa_pc_as", 4), ("trivial_pc_as", 5)])
def test_profile_as_dump_equals_the_mirror(built_lib, tmp_path, scheme, lg):
    """`profile_as --curve 2 --dump` on the host backend, byte for byte against the Python mirror (tests/harness_mirror.py)"""
    from tests.test_profile_as_dump import compare
    compare(tmp_path, scheme, lg, "harness", "poseidon", -1, seed=6, curve=2)


def test_unknown_curve_is_refused(built_lib):
    from accumulation_amd import ffi
    from accumulation_amd.engine import Context
    with pytest.raises(Exception):
        Context(3, device=ffi.AMSM_DEVICE_HOST)
    a = np.zeros(4, dtype=np.uint64)
    assert built_lib.amsm_fr_to_mont(3, a.ctypes.data, 1, a.ctypes.data) == ffi.AMSM_E_INVALID_ARG
    assert built_lib.amsm_point_serialized_size(3, 1) == 0


def test_python_tables():
    from accumulation_amd import AMSM_VESTA, ipa_pc
    from accumulation_amd.scalar_field import MODULI, Fr
    assert AMSM_VESTA == 2 and MODULI[AMSM_VESTA] == VESTA.r
    assert ipa_pc.IPA_FOLD[AMSM_VESTA] == ipa_pc.IPA_FOLD[0]
    fr = Fr(AMSM_VESTA)
    assert fr.from_limbs(fr.to_limbs(VESTA.r - 1)) == VESTA.r - 1
