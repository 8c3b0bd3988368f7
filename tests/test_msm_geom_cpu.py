"""The geometry of an MSM -- accumulation_amd/csrc/msm_geom.h: window counts, the top digit, the chunk split of accumulate L0,
window-relative indices, and what each pipeline makes of a key, a range and a context -- at every rule edge, without a GPU:
tests/cpp_host/msm_geom_check.cpp is plain C++ over the header alone and its output is compared with tests/golden/msm_geom.txt.  The
golden was recorded from the functions as they stood in api_pipeline.inc (make_geom, bpl_geom_sets, bpl_geom, bps_geom and msm_plan's
chunked branch, cut over verbatim) before the repeated rules were stated once: a change of it is a change of a launch grid, of an
allocation or of a kernel's digit walk.  The check asserts the chunk split's invariants itself (exit status); the rule edges are
asserted below by name, so that the table cannot lose one unnoticed."""
import os
import subprocess

import pytest

from oracle import pyref as o
from tests import helpers as h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "accumulation_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp_host", "msm_geom_check.cpp")
EXE = os.path.join(ROOT, "build", "msm_geom_check")
GOLDEN = os.path.join(ROOT, "tests", "golden", "msm_geom.txt")
CURVES = ("pallas", "vesta", "bls12_381_g1", "bn254_g1", "grumpkin", "bls12_377_g1")
K0_MAX = 32


@pytest.fixture(scope="module")
def output():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", EXE])
    return subprocess.run([EXE], capture_output=True, text=True, check=True).stdout


@pytest.fixture(scope="module")
def rows(output):
    """(fn, case[, nv]) -> {field: value}: st and tail stay strings, l1 a pair, everything else an int"""
    out = {}
    for ln in output.splitlines():
        w = ln.split()
        if w[0] == "modulus":
            out[(w[0], w[1])] = {"hex": w[2]}
            continue
        rec = {}
        for k, v in (x.split("=") for x in w[2:]):
            rec[k] = v if k == "st" else tuple(v.split(",")) if k == "tail" else tuple(int(y) for y in v.split(",")) if k == "l1" else int(v)
        key = (w[0], w[1], rec["nv"]) if w[0] == "unit" else (w[0], w[1])
        assert key not in out, key
        out[key] = rec
    return out


def test_header_compiles_alone():
    """plain C++17 over msm_types.h, msm_select.h, prep_geom.h and include/amsm.h: no HIP, no context, no key"""
    src = os.path.join(ROOT, "build", "msm_geom_alone.cpp")
    os.makedirs(os.path.dirname(src), exist_ok=True)
    with open(src, "w") as f:
        f.write('#include "msm_geom.h"\nint main() { return amsm::windows_for(16) == 16 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, src])
    text = open(os.path.join(CSRC, "msm_geom.h")).read()
    incl = sorted(ln.split()[1].strip('"<>') for ln in text.splitlines() if ln.startswith("#include"))
    assert [i for i in incl if i.endswith(".h")] == ["../../include/amsm.h", "msm_select.h", "msm_types.h", "prep_geom.h"]


def test_output_matches_the_golden(output):
    want = open(GOLDEN).read()
    assert output.splitlines() == want.splitlines()
    assert len(want) < 256 * 1024


def test_moduli_are_the_oracle_s(rows):
    """the scalar fields the check walks are the oracle's (and those of csrc/curves.h: test_moduli_from_curves_h)"""
    curves = (o.PALLAS, h.VESTA, o.BLS12_381_G1, h.BN254, h.GRUMPKIN, h.BLS12_377)
    assert [rows[("modulus", cv)]["hex"] for cv in CURVES] == ["%064x" % c.r for c in curves]


def test_moduli_from_curves_h(output):
    """the same source over csrc/curves.h (the host side of a hipcc build): the same output, so the moduli written out in the check are
    the library's"""
    exe = EXE + "_curves_h"
    subprocess.check_call(["hipcc", "-std=c++17", "-O1", "--offload-host-only", "--offload-arch=gfx950", "-x", "hip", "-w",
                           "-DMSM_GEOM_MODULI_FROM_CURVES_H", "-I", CSRC, SRC, "-o", exe])
    assert subprocess.run([exe], capture_output=True, text=True, check=True, timeout=300).stdout == output


def test_window_and_limits(rows):
    ch, mk = (lambda c: rows[("chunked", c)]), (lambda c: rows[("make", c)])  # noqa: E731
    # W = floor(255 / c) + 1 windows, as many slots, 2^(c - 1) buckets; a plain key has a set per window
    for case in ("plain_n_1", "plain_n_255", "plain_n_2p8", "plain_n_2p10", "plain_n_2p16", "plain_n_2p18", "plain_n_2p20", "override_2",
                 "override_7", "override_8", "override_12", "override_24"):
        r = ch(case)
        assert r["st"] == "ok" and r["W"] == r["S"] == 255 // r["c"] + 1 and r["nb"] == 2 ** (r["c"] - 1), case
        assert r["n_sets"] == r["W"] and r["B"] == r["n_sets"] * r["nb"] and r["E"] == r["n"] * r["S"] and r["K1"] == 1024, case
        assert (r["groups"], r["precomp"], r["bpl"], r["idx_rel_bits"], r["top_split"], r["n_narrow"], r["top_shift"]) == (1, 0, 0, 0, 0, 0, 0)
    assert [ch("override_%d" % c)["c"] for c in (2, 7, 8, 12, 24)] == [2, 7, 8, 12, 24]
    assert ch("override_1")["st"] == ch("override_25")["st"] == "invalid_arg"
    # the short prep chain from 8-bit windows (32 slots) up; the rocPRIM sort below
    assert [ch(c)["short"] for c in ("override_2", "override_7", "override_8", "override_12", "plain_n_255", "plain_n_2p10")] == [0, 0, 1, 1, 0, 1]
    # entry words carry a 30-bit index
    assert mk("nS_2p30_minus_16")["st"] == "ok" and mk("nS_2p30_minus_16")["E"] == 2**30 - 16
    assert mk("nS_2p30")["st"] == "unsupported"
    assert mk("table_nW_2p30")["st"] == "unsupported" and mk("table_nW_2p30_minus_16")["st"] == "ok" and mk("plain_key_2p26")["st"] == "ok"
    # a plain key's bucket-per-lane walk
    assert mk("plain_c23_no_walk")["st"] == mk("plain_c17_no_walk")["st"] == "invalid_arg"
    assert [mk("plain_c16_top_sets_%d" % t)["st"] for t in (1, 2, 3, 4, 8, 16)] == ["invalid_arg", "ok", "invalid_arg", "ok", "ok", "invalid_arg"]
    for t in (2, 4, 8):
        r = mk("plain_c16_top_sets_%d" % t)
        assert (r["top_split"], r["n_sets"], r["n_narrow"]) == (t - 1, 16 + t - 1, 0)


def test_chunk_split(rows):
    """K0 / K0b / nA / T0 / n_chunks over the resident lanes (64 per wave slot), branch by branch; the check itself asserts that nA is a
    multiple of 256, the sizes multiples of 4 with K0b <= K0 <= K0_MAX + 4, and that chunk_of / chunk_start cover E and agree around T0"""
    for ws in (4, 2048, 3072, 4096):
        lanes, r = 64 * ws, lambda share: rows[("make", "chunks_ws%d_share_%s" % (ws, share))]  # noqa: E731
        for share in (1, 5, 11):  # small problems: one size of at least 12, phase A covers everything
            g = r(share)
            assert (g["K0"], g["K0b"]) == (12, 12) and g["n_chunks"] == -(-g["E"] // 12) and g["nA"] == -(-g["n_chunks"] // 256) * 256
        assert (r(12)["K0"], r(12)["K0b"], r(12)["nA"], r(12)["T0"], r(12)["n_chunks"]) == (16, 12, 0, 0, lanes)  # one round, not long
        assert (r(13)["K0"], r(13)["K0b"], r(13)["n_chunks"]) == (16, 16, -(-13 * lanes // 16))  # ra >= rounds: every round is long
        assert (r(33)["K0"], r(33)["K0b"], r(33)["nA"]) == (20, 16, lanes)  # 33 = 20 + 16 - 3: one long round of two
        assert (r(40)["K0"], r(40)["K0b"], r(40)["nA"], r(40)["n_chunks"]) == (24, 20, 0, 2 * lanes)
        assert (r(42)["K0"], r(42)["K0b"], r(42)["nA"], r(42)["T0"], r(42)["n_chunks"]) == (24, 20, lanes, 24 * lanes, lanes + -(-18 * lanes // 20))
        assert r("42_plus_1")["n_chunks"] in (r(42)["n_chunks"], r(42)["n_chunks"] + 1) and r("42_plus_1")["nA"] == lanes
        assert (r(47)["K0"], r(47)["K0b"]) == (24, 24) and r(47)["T0"] >= r(47)["E"]  # both rounds long: phase A covers everything
        assert (r(100)["K0"], r(100)["K0b"], r(100)["nA"], r(100)["n_chunks"]) == (28, 24, lanes, 4 * lanes)
        # phase A covers everything: whole chunks, and one entry into the next
        a, b = rows[("make", "chunks_ws%d_whole_chunks" % ws)], rows[("make", "chunks_ws%d_whole_chunks_plus_1" % ws)]
        assert a["K0"] == b["K0"] == 12 and a["E"] % 12 == 0 and b["E"] % 12 == 1
        assert (a["n_chunks"], b["n_chunks"]) == (a["E"] // 12, a["E"] // 12 + 2) and a["T0"] >= a["E"] and b["T0"] >= b["E"]
    n = 0
    for (fn, *_), g in rows.items():
        if fn in ("make", "chunked", "bpl", "bps") and g["st"] == "ok":
            assert g["nA"] % 256 == 0 and g["K0"] % 4 == 0 and g["K0b"] % 4 == 0 and 12 <= g["K0b"] <= g["K0"] <= K0_MAX + 4
            assert g["T0"] == g["nA"] * g["K0"] and g["n_chunks"] >= -(-g["E"] // g["K0"])
            n += 1
    assert n >= 250


def test_groups(rows):
    for gs, name in ((-1, "none"), (0, "0"), (1, "1"), (2, "2"), (3, "3"), (17, "17")):
        for fn, case in (("chunked", "table17"), ("chunked", "plain"), ("bps", "table17")):
            g = rows[(fn, "group_shift_%s_%s" % (name, case))]
            assert g["st"] == "ok" and (g["groups"], g["group_shift"]) == ((2, gs) if gs >= 0 else (1, 0))
            assert g["n_sets"] == g["groups"] * (1 if g["precomp"] else g["W"])


def test_window_relative_indices(rows):
    """idx_rel_bits = ceil log2 n where (W << b) - 1 is BELOW the largest absolute index, one group, a table; the three pipelines' follow-ups"""
    def want(g):
        b = max(1, (g["n"] - 1).bit_length())
        return b if g["precomp"] and g["groups"] == 1 and (g["W"] << b) - 1 < g["base_off"] + g["n"] - 1 + (g["W"] - 1) * g["table_stride"] else 0
    seen = set()
    for (fn, case, *_), g in rows.items():
        if case.startswith("rel") and g["st"] == "ok" and case != "rel_refused_c7_S37":
            assert g["idx_rel_bits"] == want(g), (fn, case)
            seen.add((fn, g["groups"], g["idx_rel_bits"] != 0, g["base_off"] != 0))
    for fn in ("chunked", "bpl", "bps"):
        assert {(fn, 1, True, False), (fn, 1, True, True)} <= seen, fn
    assert {("chunked", 1, False, False), ("bpl", 1, False, False)} <= seen
    whole = rows[("bps", "table17_n_2p17")]  # (bucket-split without the bits: the whole of a key)
    assert whole["n"] == whole["table_stride"] and whole["idx_rel_bits"] == want(whole) == 0
    assert {("chunked", 2, False, True), ("bpl", 2, False, True)} <= seen and not [s for s in seen if s[1] == 2 and s[2]]
    # the whole key: the relative word is as long as the absolute index, not shorter -- no bits (the comparison is <, not <=)
    assert rows[("chunked", "rel17_n_2p20_of_2p20")]["idx_rel_bits"] == rows[("bpl", "rel20_n_2p20_of_2p20")]["idx_rel_bits"] == 0
    assert rows[("chunked", "rel17_n_2p20_of_2p22")]["idx_rel_bits"] == rows[("bpl", "rel20_n_2p20_of_2p22")]["idx_rel_bits"] == 20
    assert rows[("chunked", "rel17_n_1_of_2p20")]["idx_rel_bits"] == 1 and rows[("chunked", "rel17_n_2p16_plus_1_of_2p20")]["idx_rel_bits"] == 17
    # two groups never carry them
    assert rows[("chunked", "rel17_n_2p20_of_2p22_groups2")]["idx_rel_bits"] == rows[("bpl", "rel20_n_2p20_of_2p22_groups2")]["idx_rel_bits"] == 0
    # chunked: kept only where the short prep chain takes the geometry
    r = rows[("chunked", "rel_refused_c7_S37")]
    assert want(r) == 10 and (r["idx_rel_bits"], r["short"], r["S"]) == (0, 0, 37)
    assert (rows[("chunked", "rel_kept_c8_S32")]["idx_rel_bits"], rows[("chunked", "rel_kept_c8_S32")]["short"]) == (10, 1)
    # bucket-split: a key without a table has no lane count, with the bits or without
    assert rows[("bps", "plain_key")]["st"] == "false"


def test_bucket_per_lane(rows):
    b = lambda c: rows[("bpl", c)]  # noqa: E731
    shifts = {}
    for cv in CURVES:
        for case, n, groups, off in (("n_2p18_plus_1", 2**18 + 1, 1, 0), ("n_2p20", 2**20, 1, 0), ("n_2p20_groups2", 2**20, 2, 0),
                                     ("n_2p20_of_2p22", 2**20, 1, 2**20)):
            g = b("%s_table20_%s" % (cv, case))
            assert g["st"] == "ok" and (g["n"], g["groups"], g["base_off"], g["bpl"], g["precomp"]) == (n, groups, off, 1, 1)
            assert (g["c"], g["W"], g["n_narrow"], g["n_sets"], g["top_split"]) == (20, 13, 4, groups, 0)
        shifts[cv] = b(cv + "_table20_n_2p20")["top_shift"]
        # part_max: W - 1 regular windows and the top one over its reach, halved (rounded up) for two groups
        one, two = b(cv + "_table20_n_2p20")["part_max"], b(cv + "_table20_n_2p20_groups2")["part_max"]
        assert two == (one + 1) // 2 and one >= 13 * 2**20 * 1024 // 2**19
        assert b(cv + "_table20_n_2p20_of_2p22")["idx_rel_bits"] == 20 and b(cv + "_table20_n_2p20")["idx_rel_bits"] == 0
        # a plain key: T = top_split + 1 sets for the top window -- the rule's smallest that fits, AMSM_TOP_SETS=2 two or none, 4 / 8 forced
        for n in ("n_2p18_plus_1", "n_2p20", "n_2p20_groups2"):
            rule, two_, four, eight = (b("%s_plain_c16_%s_top_sets_%d" % (cv, n, t)) for t in (0, 2, 4, 8))
            assert (four["st"], four["top_split"], eight["st"], eight["top_split"]) == ("ok", 3, "ok", 7), (cv, n)
            assert rule["st"] == "ok" and rule["top_split"] in (1, 3, 7)
            assert two_["st"] == ("ok" if rule["top_split"] == 1 else "false")
            for g in (rule, four, eight):
                assert g["n_sets"] == g["groups"] * (16 + g["top_split"]) and (g["c"], g["n_narrow"], g["precomp"], g["bpl"]) == (16, 0, 0, 1)
                assert g["part_max"] > 0 and g["idx_rel_bits"] == 0
        assert b(cv + "_plain_c16_n_2p21_too_long")["st"] == "false"
        g = b(cv + "_plain_c15_n_2p18")
        assert g["st"] == "ok" and (g["c"], g["W"], g["n_narrow"]) == (15, 18, 14)
    assert shifts["pallas"] == shifts["vesta"] == 1 and shifts["bls12_381_g1"] == 0  # (api_keys.inc: top_window_shift quotes them)
    # the rule takes more than two sets where the top window's reach is short
    assert b("bls12_377_g1_plain_c16_n_2p20_top_sets_0")["top_split"] > 1 and b("pallas_plain_c16_n_2p20_top_sets_0")["top_split"] == 1
    # forced 8 does not fit (5632 partitions), the rule's two do (4096)
    forced, rule = b("pallas_plain_c18_groups2_top_sets_8"), b("pallas_plain_c18_groups2_top_sets_0")
    assert forced == rule and (rule["st"], rule["top_split"], rule["B"] // 1024) == ("ok", 1, 4096)
    for case in ("pallas_plain_c23_no_walk", "pallas_plain_c23_no_walk_top_sets_8", "pallas_plain_no_window"):
        assert b(case)["st"] == "false", case


def test_bucket_split_and_units(rows):
    s = lambda c: rows[("bps", c)]  # noqa: E731
    assert [s("table%d_n_%s" % (c, n))["bps_log2_l"] for c in (16, 17) for n in ("2p16", "2p17")] == [2, 2, 1, 1]
    for c in (15, 16, 17):
        for n in ("2p16", "2p17"):
            g = s("table%d_n_%s" % (c, n))
            assert g["st"] == "ok" and (g["bpl"], g["n_sets"], g["precomp"]) == (2, 1, 1)
            # a unit: one bucket set per MSM and at most 16 slots
            assert rows[("unit_ok", "table%d_n_%s" % (c, n))]["st"] == ("ok" if g["S"] <= 16 else "false")
    assert (s("table15_n_2p16")["S"], s("table16_n_2p16")["S"]) == (18, 16)
    assert s("table17_n_2p17_groups2")["st"] == "ok" and s("table17_n_2p17_groups2")["n_sets"] == 2
    assert s("table12_n_2p19_no_lane_count")["st"] == "false"
    for c in (16, 17):
        g = s("table%d_n_2p16" % c)
        for nv in (2, 8):
            u = rows[("unit", "table%d_n_2p16" % c, nv)]
            assert (u["n_sets"], u["groups"], u["B"]) == (nv, nv, g["B"] * nv)
            assert {k: v for k, v in u.items() if k not in ("n_sets", "groups", "B", "nv", "tail")} == \
                   {k: v for k, v in g.items() if k not in ("n_sets", "groups", "B", "st", "tail")}


def test_l1_lanes(rows):
    l1 = lambda c: rows[("l1", c)]["l1"]  # noqa: E731  (hidden, exposed)
    assert l1("hidden_B_16383_avg_48") == (4, 4) and l1("hidden_B_16384_avg_48") == (4, 4) and l1("hidden_B_16384_below_48") == (1, 4)
    assert l1("B_4096_avg_24") == (16, 16) and l1("B_4096_below_24") == (4, 4) and l1("B_4097_avg_24") == (4, 4)
    assert l1("B_4096_avg_3") == (4, 4) and l1("B_4096_below_3") == (1, 1)
    assert l1("B_2p20_avg_3") == (1, 4) and l1("B_2p20_below_3") == (1, 1)
