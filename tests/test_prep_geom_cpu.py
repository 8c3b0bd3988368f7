"""The geometry of the prep chains -- accumulation_amd/csrc/prep_geom.h: partitions, index bits, LDS sizes, strides, what a chain
needs of a slot -- at every rule edge, without a GPU: tests/cpp_host/prep_geom_check.cpp is plain C++ over the header alone and its
output is compared with tests/golden/prep_geom.txt.  The golden was recorded from the expressions as they stood in kern_fr.hip and
api_pipeline.inc before they were stated once (PrepSmall, PrepNeeds, prep_index_bits): a change of it is a change of a launch or of
an allocation.  The rule edges themselves are asserted below, so that the table cannot lose one unnoticed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp_host", "prep_geom_check.cpp")
EXE = os.path.join(ROOT, "build", "prep_geom_check")
GOLDEN = os.path.join(ROOT, "tests", "golden", "prep_geom.txt")
KIB = 1024


@pytest.fixture(scope="module")
def output():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", EXE])
    return subprocess.run([EXE], capture_output=True, text=True, check=True).stdout


@pytest.fixture(scope="module")
def rows(output):
    """(kind, case[, l]) -> {field: int}; `needs` as a tuple of five"""
    out = {}
    for ln in output.splitlines():
        w = ln.split()
        kv = dict(x.split("=") for x in w[2:]) if w[0] != "small" else dict(x.split("=") for x in w[1:])
        rec = {k: (tuple(int(y) for y in v.split(",")) if k == "needs" else int(v)) for k, v in kv.items()}
        key = (w[0], rec["heavy_words"]) if w[0] == "small" else (w[0], w[1], rec["l"]) if w[0] == "bps_l" else (w[0], w[1])
        assert key not in out, key
        out[key] = rec
    return out


def test_output_matches_the_golden(output):
    want = open(GOLDEN).read()
    assert output.splitlines() == want.splitlines()


def test_short_chain_edges(rows):
    s = lambda c: rows[("short", c)]  # noqa: E731
    assert (s("plain_c8_S32")["supported"], s("plain_c8_S33")["supported"], s("plain_c7_S37")["supported"]) == (1, 0, 0)
    assert s("empty")["supported"] == 0
    # IB + SH <= 31: the partitions shrink to 8 buckets (4096 of them, PREP_MAX_P) and no further
    assert [(s(c)["IB"], s(c)["SH"], s(c)["P"], s(c)["supported"]) for c in ("table_2p24_W16", "table_2p25_W16", "table_2p26_W16")] == [
        (28, 3, 4096, 1), (29, 3, 4096, 0), (30, 3, 4096, 0)]
    assert (s("table_2p26_W16_rel16")["IB"], s("table_2p26_W16_rel16")["supported"]) == (20, 1)
    assert s("table_2p26_W16_rel16_off")["IB"] == 20  # window-relative: the offset into the key does not count
    # partitions
    assert [(s(c)["SH"], s(c)["P"]) for c in ("B_512x16", "B_512x16_plus_1", "B_512x1024", "B_512x1024_plus_1", "B_4096x1024",
                                              "B_4096x1024_plus_1")] == [(4, 512), (5, 257), (9, 1024), (9, 1025), (10, 4096), (11, 2049)]
    # the scatter's opt-in to more than 64 KiB of LDS
    assert s("scatter_lds_P1365")["scatter_lds"] == 64 * KIB - 4 and s("scatter_lds_P1366")["scatter_lds"] == 64 * KIB + 8
    assert (s("scatter_lds_P1366")["SPB"], s("scatter_lds_S32_P1366")["SPB"]) == (512, 256)
    for (kind, *_), r in rows.items():
        if kind in ("short", "bpl", "bps_l"):
            assert r["SPB"] in (256, 512)


def test_bucket_per_lane_edges(rows):
    b = lambda c: rows[("bpl", c)]  # noqa: E731
    for c in ("bpl_2p20_n_2p18_plus_1", "bpl_2p20_n_2p20", "bpl_2p22_n_2p20_off", "bpl_2p20_n_2p20_groups2", "bpl_plain_c16_top2",
              "bpl_plain_c16_top4", "bpl_plain_c16_top8", "bpl_plain_c16_top2_groups2", "bpl_plain_c8_S32", "bpl_B_516x1024"):
        r = b(c)
        assert r["supported"] == 1, c
        assert r["SH"] == 10 and r["P"] == r["partitions"] and r["groups_per_part"] == 17 and r["CAP"] == 37340
        assert r["FIX"] % 16 == 0 or r["FIX"] == r["CAP"]
        assert r["stride"] % 1024 == 0 and r["P"] * r["stride"] < 2**31
        assert r["local_lds"] == 160 * KIB and r["scatter_lds"] <= 160 * KIB
        assert r["part_entries"] == max(rows[("geom", c)]["E"], r["P"] * r["FIX"])
    assert (b("bpl_plain_c16_top2")["P"], b("bpl_plain_c16_top4")["P"], b("bpl_plain_c16_top8")["P"]) == (17 * 32, 19 * 32, 23 * 32)  # (W + T - 1) sets of 2^15
    assert (b("bpl_2p20_n_2p20")["P"], b("bpl_2p20_n_2p20_groups2")["P"]) == (512, 1024)
    assert (b("bpl_2p20_stage_fits")["supported"], b("bpl_2p20_stage_full")["supported"]) == (1, 0)
    for c in ("bpl_B_512x1024_plus_512", "bpl_B_513x1024", "bpl_B_2p15", "bpl_B_4100x1024"):
        assert b(c)["supported"] == 0, c


def test_bucket_split_edges(rows):
    ch = lambda c: rows[("bps", c)]["choose"]  # noqa: E731
    assert [ch(c) for c in ("bps_c16_n_2p16", "bps_c16_n_2p17", "bps_c17_n_2p16", "bps_c17_n_2p17")] == [2, 2, 1, 1]
    assert [ch(c) for c in ("bps_c18_l0", "bps_c17_n_2p16", "bps_c16_n_2p16", "bps_c15_l3", "bps_c14_l4", "bps_c13_l5", "bps_c12_l6")] == list(range(7))
    assert ch("bps_c11_l6_P64") == 6 and ch("bps_c17_n_2p19_wants_256") == 3
    for c in ("bps_c12_n_2p19_over_cap", "bps_c6_B_32", "bps_B_not_pow2", "bps_table_2p26_W16", "empty"):
        assert ch(c) == -1, c
    # the refusal for E / P + 1024 > CAP is that rule's and no other's
    r = rows[("bps_l", "bps_c12_n_2p19_over_cap", 6)]
    assert rows[("geom", "bps_c12_n_2p19_over_cap")]["E"] // r["P"] + 1024 > r["CAP"] and r["IB"] + r["SH"] <= 31 and r["P"] % 2 == 0
    for (kind, case, *l), r in rows.items():
        if kind == "bps_l" and ch(case) == l[0]:
            assert r["SH"] == 10 - l[0] and r["P"] == r["partitions"] and r["stride"] % 1024 == 0
            assert r["local_lds"] == 148 * KIB and r["IB"] + r["SH"] <= 31
            assert "needs" in r


def test_needs_are_the_sums_the_plans_allocate(rows):
    """vals_a / vals_b / bpl_grp / bpl_order / prep_small in bytes, each with its slack: the expressions msm_plan had"""
    for (kind, case, *l), r in rows.items():
        if "needs" not in r:
            continue
        g, small = rows[("geom", case)], 64 + rows[("short", case)]["small_words"] * 4 + 256
        if kind == "bpl":
            assert r["needs"] == (r["part_entries"] * 8 + 64, r["P"] * r["stride"] * 4 + 64, r["P"] * 17 * 8 + 64, r["P"] * 17 * 64 * 4 + 64, small)
        else:
            assert r["needs"] == (r["part_entries"] * 4 + 64, r["P"] * r["stride"] * 4 + 64, r["P"] * 16 * 8 + 64, g["B"] * 4 + 64, small)


def test_fill_is_whole_lines_inside_the_slot(rows):
    """PrepSmall's fill starts at the 16 flag words in front of d_small: a whole number of 256-byte lines, ending no later than the
    prep_small_words(g) words plus the 256 bytes of slack the slot reserves"""
    n = 0
    for (kind, case, *_), r in rows.items():
        if kind != "short":
            continue
        for fill in (r["fill"], r["fill_heavy"]):
            assert fill % 256 == 0
            assert fill - 16 * 4 <= r["small_words"] * 4 + 256, case
        n += 1
    assert n == len([k for k in rows if k[0] == "geom"]) >= 50
    a, b = rows[("small", 0)], rows[("small", 36928)]
    for s in (a, b):
        assert (s["part_total"], s["part_start"], s["part_cursor"], s["part_items"], s["hv_n"], s["hv_cnt"]) == (0, 4097, 8194, 12291, 16388, 16389)
        assert s["fill"] % 256 == 0 and s["block_words"] * 4 == a["fill"]
    assert a["hv_ids"] == a["hv_cur"] == a["hv_end"] == a["hv_cnt"] + 64
    assert (b["hv_ids"], b["hv_cur"], b["hv_end"]) == (b["hv_cnt"] + 36928, b["hv_cnt"] + 36928 + 4096, b["hv_cnt"] + 2 * 36928 + 4096)
    # the fill of the chain with heavy partitions covers hv.cnt, the one without ends behind the heavy count
    assert b["fill"] >= (16 + b["hv_cnt"] + 36928) * 4 and a["fill"] >= (16 + a["hv_cnt"]) * 4
