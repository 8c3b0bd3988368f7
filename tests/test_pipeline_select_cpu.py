"""Which pipeline an MSM takes -- accumulation_amd/csrc/msm_select.h, the ONE table-driven function behind every entry point --
at every threshold edge, without a GPU: tests/cpp_host/select_check.cpp is plain C++ over the header alone.
Edges: n = 2^k - 1, 2^k, 2^k + 1 for k = 15 .. 20, 2^21, 2^22; keys: a direct-sum key, 16-bit tables of 2^16 / 2^19 generators,
the 20-bit table (2^20 and 2^22 generators), a plain key; forms: plain, grouped (regular / irregular index classes), skewed.
The same program prints msel::tail_plan -- the form, grids and buffer needs of an MSM's tail -- at its rule edges and checks that what
msm_plan reserves before the Place is known covers every launch (it exits non-zero otherwise: the fixture's check=True)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp_host", "select_check.cpp")
EXE = os.path.join(ROOT, "build", "select_check")
P = lambda k: 1 << k  # noqa: E731


@pytest.fixture(scope="module")
def table():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", EXE])
    out = subprocess.run([EXE], capture_output=True, text=True, check=True).stdout.splitlines()
    rows, other = {}, []
    for ln in out:
        w = ln.split()
        if len(w) == 8 and w[4].startswith("twin="):
            rows[(w[0], int(w[1]), w[2])] = {"pipeline": w[3], "twin": int(w[4][5:]), "plain_window": int(w[5].split("=")[1]),
                                            "range": int(w[6].split("=")[1]), "probe": int(w[7].split("=")[1])}
        else:
            other.append(ln)
    return rows, other


def expect(table, key, n, form, pipeline, twin=0, plain_window=0, rng=0):
    got = table[0][(key, n, form)]
    assert (got["pipeline"], got["twin"], got["plain_window"], got["range"]) == (pipeline, twin, plain_window, rng), (key, n, form, got)


def test_direct_sum_keys(table):
    for n in (1, P(15) - 1, P(15)):
        expect(table, "direct_2p15", n, "plain", "direct_sum")
        expect(table, "direct_2p15", n, "grouped", "direct_sum")
        expect(table, "direct_2p15", n, "skewed", "direct_sum")  # no buckets: nothing to skew
        expect(table, "direct_2p15", n, "grouped_irregular", "chunked")  # index classes of unequal size: the windowed pipelines


@pytest.mark.parametrize("key", ["table_2p16", "table_2p19"])
def test_precomputed_keys_without_a_20_bit_table(table, key):
    top = P(16) if key == "table_2p16" else P(19)
    for n, want in ((1, "chunked"), (P(15), "chunked"), (P(15) + 1, "chunked"), (P(16) - 1, "chunked"), (P(16), "bucket_split"),
                    (P(16) + 1, "bucket_split"), (P(17) - 1, "bucket_split"), (P(17), "bucket_split"), (P(17) + 1, "chunked"),
                    (P(18), "chunked"), (P(19), "chunked")):
        if n > top:
            continue
        for form in ("plain", "grouped", "grouped_irregular"):
            expect(table, key, n, form, want)
        expect(table, key, n, "skewed", "chunked")
        assert table[0][(key, n, "plain")]["probe"] == (1 if want == "bucket_split" else 0)


@pytest.mark.parametrize("key", ["bpl_2p20", "bpl_2p22"])
def test_keys_with_the_20_bit_table(table, key):
    for n, want, twin in ((1, "chunked", 1), (P(15), "chunked", 1), (P(16) - 1, "chunked", 1), (P(16), "bucket_split", 1), (P(17), "bucket_split", 1),
                          (P(17) + 1, "chunked", 1), (P(18) - 1, "chunked", 1), (P(18), "chunked", 1), (P(18) + 1, "bucket_per_lane", 0),
                          (P(19), "bucket_per_lane", 0), (P(19) + 1, "bucket_per_lane", 0), (P(20) - 1, "bucket_per_lane", 0),
                          (P(20), "bucket_per_lane", 0)):
        for form in ("plain", "grouped", "grouped_irregular"):
            expect(table, key, n, form, want, twin)
        expect(table, key, n, "skewed", "chunked", 1)  # a skewed vector: chunked over the 17-bit twin
    # longer than the window: ranges of 2^20 (which share one bucket set)
    for n in ((P(20) + 1, P(21), P(22) - 1, P(22)) if key == "bpl_2p22" else ()):
        for form in ("plain", "skewed"):
            expect(table, key, n, form, "chunked", 0, 0, P(20))
        assert table[0][(key, n, "plain")]["probe"] == 1


def test_plain_keys(table):
    key = "plain_2p22"
    for n, want, c in ((1, "chunked", 0), (P(15), "chunked", 0), (P(16), "chunked", 0), (P(17) - 1, "chunked", 0), (P(17), "chunked", 0),
                       (P(17) + 1, "bucket_per_lane", 15), (P(18), "bucket_per_lane", 15), (P(18) + 1, "bucket_per_lane", 16),
                       (P(19), "bucket_per_lane", 16), (P(19) + 1, "bucket_per_lane", 16), (P(20), "bucket_per_lane", 16)):
        for form in ("plain", "grouped", "grouped_irregular"):
            expect(table, key, n, form, want, 0, c)
        expect(table, key, n, "skewed", "chunked")
        assert table[0][(key, n, "plain")]["probe"] == 0  # plain keys find out from the prep's overflow flag
    for n in (P(20) + 1, P(21), P(22)):
        expect(table, key, n, "plain", "chunked", 0, 0, P(20))


def test_switches_and_key_windows(table):
    other = table[1]
    assert "switch bpl=0 bpl_2p20 chunked" in other
    assert "switch bpl_plain=0 plain chunked range=0" in other
    assert "switch bps=0 table_2p16 chunked" in other
    assert "switch bps=1 table_2p16 plain chunked grouped bucket_split" in other
    assert "switch direct=0 direct_2p15 chunked" in other
    assert "switch window_override bpl_2p20 chunked twin=1 plain chunked" in other
    assert "split table_2p23 default range=2097152 off range=0 below range=0" in other
    win = {ln.split()[1]: [int(x.split("=")[1]) for x in ln.split()[2:]] for ln in other if ln.startswith("key_window")}
    # (precomputed, precomputed with AMSM_BPL=0, plain on the chunked pipeline)
    assert win == {"2p1": [8, 8, 4], "2p8": [8, 8, 4], "2p9": [8, 8, 8], "2p12": [8, 8, 8], "2p13": [10, 10, 8], "2p14": [10, 10, 8],
                   "2p15": [13, 13, 8], "2p16": [16, 16, 8], "2p17": [17, 17, 8], "2p18": [16, 16, 8], "2p19": [16, 16, 8],
                   "2p20": [20, 17, 13], "2p22": [20, 17, 16]}


def test_classification_of_probed_vectors(table):
    """msel::classify -- what a call makes of its vectors' two-valued probe words -- one case per rule"""
    got = {ln.split()[1]: ln.split()[2:] for ln in table[1] if ln.startswith("classify ")}
    want = {
        "two_valued": ["two_valued"],
        "mixed_flag_wins": ["regular"],
        # a canonical value of 2^255 or more stays with the windowed pipelines (they report it); in Montgomery form the stored
        # words say nothing about the value's size
        "value_2p255_canonical": ["regular"],
        "value_2p255_montgomery": ["two_valued"],
        "all_zero": ["all_zero"],
        "ones_7_samples": ["regular"],  # TV_ONES_MIN_SAMPLES = 8 of the 1024 samples
        "ones_8_samples": ["ones_apart"],
        "not_probed": ["regular"],
        "ones_over_20_bit_table": ["regular"],  # runs chunked over the 17-bit twin, where the ones cost little
        "ones_plain_key": ["ones_apart"],
        "ones_direct_sum": ["regular"],  # no buckets to skew
        "ones_direct_sum_off": ["ones_apart"],
        # tests/test_unit_scalars_gpu.py::test_views_that_share_memory_with_a_vector_that_keeps_its_ones
        "shared_memory_view": ["regular", "regular", "ones_apart"],
        "shared_memory_no_view": ["ones_apart", "ones_apart"],
        "shared_memory_adjacent": ["ones_apart", "regular"],  # touching is not sharing
        "shared_memory_unprobed_view": ["regular", "regular"],  # a vector too short to probe keeps its ones too
        "shared_memory_empty_view": ["ones_apart", "regular"],
        "shared_memory_two_valued_view": ["ones_apart", "two_valued"],  # a view that skips the pipelines keeps nothing in them
        "shared_memory_both_ones": ["ones_apart", "ones_apart"],
        "shared_memory_chain": ["regular", "regular", "regular"],
    }
    assert got == want


def tail_rows(table):
    rows = {}
    for ln in table[1]:
        w = ln.split()
        if w[0] == "tail":
            rows[(w[1], w[2])] = dict(kv.split("=") for kv in w[3:])
    return rows


def test_tail_plan_rule_edges(table):
    """msel::tail_plan, one line per rule edge and Place: (form, red_s, partial records per set, records of row / column scratch)"""
    rows = tail_rows(table)
    FQ, OL, R2 = "fused_quad", "one_lane", "red2"

    def expect_tail(case, lone, inner):
        # the two exposed places (a blocking call, the last MSM of a batch) always agree
        for place, want in (("lone", lone), ("batch_last", lone), ("batch_inner", inner)):
            r = rows[(case, place)]
            got = (r["form"], int(r["red_s"]), int(r["partials"]), int(r["rc"]))
            assert got == want, (case, place, r)
            quad = want[0] == FQ or (want[0] == R2 and place != "batch_inner")
            assert (int(r["quad"]), int(r["latency"]), int(r["ticket"])) == (int(quad), int(quad), int(want[0] == FQ)), (case, place, r)
            assert r["covered"] == "1"

    # a hidden tail stays on the quad kernels up to 2^17 buckets in all and 5 * 2^20 entries
    expect_tail("B_2p17", (FQ, 4, 128, 0), (FQ, 4, 128, 0))
    expect_tail("B_2p17_plus_1", (FQ, 4, 128, 0), (OL, 4, 32, 0))
    expect_tail("B_5_sets_of_2p15", (FQ, 4, 128, 0), (OL, 4, 32, 0))
    expect_tail("E_5_2p20", (FQ, 4, 128, 0), (FQ, 4, 128, 0))
    expect_tail("E_5_2p20_plus_1", (FQ, 4, 128, 0), (OL, 4, 32, 0))
    # row / column sums from 2^18 buckets per set, multiples of 1024 only: 256 + 1024 sums, a lane or a quad each
    expect_tail("nb_2p18_minus_1024", (FQ, 8, 510, 0), (OL, 8, 128, 0))
    expect_tail("nb_2p18", (R2, 8, 20, 1280), (R2, 8, 5, 1280))
    expect_tail("nb_2p18_plus_1", (FQ, 8, 512, 0), (OL, 8, 128, 0))
    # buckets per logical lane: 2 up to 256 buckets, 8 from 2^16, else 4; 32 behind the bucket-per-lane accumulation
    expect_tail("nb_256", (FQ, 2, 2, 0), (FQ, 2, 2, 0))
    expect_tail("nb_257", (FQ, 4, 1, 0), (FQ, 4, 1, 0))
    expect_tail("nb_65535", (FQ, 4, 256, 0), (FQ, 4, 256, 0))
    expect_tail("nb_65536", (FQ, 8, 128, 0), (FQ, 8, 128, 0))
    expect_tail("bpl_20_bit_table", (R2, 32, 24, 1536), (R2, 32, 6, 1536))
    expect_tail("bpl_off_2p19", (R2, 8, 24, 1536), (R2, 8, 6, 1536))
    expect_tail("bpl_plain_16_bit", (FQ, 32, 16, 0), (OL, 32, 4, 0))
    expect_tail("bpl_off_plain_16_bit", (FQ, 4, 128, 0), (OL, 4, 32, 0))
    expect_tail("two_sets_of_2p19", (R2, 32, 24, 3072), (R2, 32, 6, 3072))
    # the jump fold of an IPA opening: JUMP_NB = 256 buckets per set, two per logical lane
    expect_tail("jump_fold", (FQ, 2, 2, 0), (FQ, 2, 2, 0))
    assert rows[("jump_fold", "lone")]["red_threads"] == "128"


def test_tail_plan_of_the_gpu_shapes(table):
    """the shapes of tests/test_tail_forms_gpu.py: (a) one partial record per set, the first quad folds serially; (b) more than four,
    the workgroup tree; (c) a hidden tail over more than 2^17 buckets on the one-lane kernels, the batch's last on the fused one"""
    rows = tail_rows(table)
    a, b = rows[("gpu_a_plain_2p10", "lone")], rows[("gpu_b_table_2p15", "lone")]
    assert (a["form"], int(a["partials"])) == ("fused_quad", 1)
    assert b["form"] == "fused_quad" and int(b["partials"]) == 16 > 4
    c_in, c_last = rows[("gpu_c_plain_2p17_plus_64", "batch_inner")], rows[("gpu_c_plain_2p17_plus_64", "batch_last")]
    assert (c_in["form"], int(c_in["red_s"]), int(c_in["partials"])) == ("one_lane", 32, 2)
    assert (c_last["form"], int(c_last["partials"])) == ("fused_quad", 8)


def test_tail_plan_reservation_covers_every_launch(table):
    """every line: what tail_plan_any_place reserves holds what the launches of each Place write, and their grids reach every sum"""
    rows = tail_rows(table)
    assert len(rows) == 21 * 3
    assert all(r["covered"] == "1" for r in rows.values())
    # whole: the lanes' runs tile the set exactly -- true for every real geometry (nb is a power of two); the synthetic edges are not
    assert sorted({c for (c, _), r in rows.items() if r["whole"] == "0"}) == ["nb_257", "nb_2p18_plus_1", "nb_65535"]
