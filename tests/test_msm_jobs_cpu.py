"""The job list of a call -- accumulation_amd/csrc/msm_jobs.h: how the vectors of a call are cut into ranges, which ranges share one
bucket set, which bucket-split MSMs run as one unit, and what the host's sampling probes make of a slice -- at every rule edge,
without a GPU: tests/cpp_host/msm_jobs_check.cpp is plain C++ over the header alone and its output is compared with
tests/golden/msm_jobs.txt.  The golden was recorded from the two job loops as they stood in api_pipeline.inc (msm_multi_split_impl
for device vectors, msm_multi_host_xyzz for host slices, cut over verbatim side by side) before they were stated once with the
differences between the two forms as parameters: a change of it is a change of the path some call takes.  The check asserts the
shape of every plan itself (exit status); the rule edges are asserted below by name, so that the table cannot lose one unnoticed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "accumulation_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp_host", "msm_jobs_check.cpp")
EXE = os.path.join(ROOT, "build", "msm_jobs_check")
GOLDEN = os.path.join(ROOT, "tests", "golden", "msm_jobs.txt")
P = lambda k: 1 << k  # noqa: E731
B20 = P(19)  # buckets of a 20-bit key's one set


@pytest.fixture(scope="module")
def output():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", EXE])
    return subprocess.run([EXE], capture_output=True, text=True, check=True).stdout


@pytest.fixture(scope="module")
def rows(output):
    """(kind, case) -> {field: value}; r<i> / u<i> / j<i> are gathered in order into the lists "r", "u" and "j" of int tuples"""
    out = {}
    for ln in output.splitlines():
        w = ln.split()
        if w[0] in ("probe_min_len", "probe_wanted"):
            out[(w[0], "")] = {k: int(v) for k, v in (x.split("=") for x in w[1:])}
            continue
        rec = {"r": [], "u": [], "j": []}
        for k, v in (x.split("=") for x in w[2:]):
            if k[0] in "ruj" and k[1:].isdigit():
                assert int(k[1:]) == len(rec[k[0]]), ln
                rec[k[0]].append(tuple(int(y) for y in v.split(",")))
            else:
                rec[k] = tuple(int(y) for y in v.split(",")) if "," in v else int(v)
        assert (w[0], w[1]) not in out, ln
        out[(w[0], w[1])] = rec
    return out


def ranges(rows, case):
    """the plan of a case: its row, and its ranges as (vec, lo, n, over_twin, force_chunked, set, first, last, B)"""
    r = rows[("ranges", case)]
    assert r["n"] == len(r["r"])
    return r, r["r"]


def cut(n, step, vec=0, **kw):
    """n pairs in ranges of `step`, none in a set unless sets says so"""
    twin, forced = kw.get("twin", 0), kw.get("forced", 0)
    return [(vec, lo, min(step, n - lo), twin, forced, -1, 0, 0, 0) for lo in range(0, max(n, 1), step)]


def in_set(rs, count, set_id=0, buckets=B20):
    """the first `count` ranges of rs as one shared set"""
    return [r[:5] + (set_id, int(i == 0), int(i == count - 1), buckets) if i < count else r for i, r in enumerate(rs)]


def test_header_compiles_alone():
    """plain C++17 over msm_types.h, msm_select.h and msm_geom.h: no HIP, no context, no key, no device pointer"""
    src = os.path.join(ROOT, "build", "msm_jobs_alone.cpp")
    os.makedirs(os.path.dirname(src), exist_ok=True)
    with open(src, "w") as f:
        f.write('#include "msm_jobs.h"\nint main() { return amsm::mjobs::first_half(3) == 64 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, src])
    text = open(os.path.join(CSRC, "msm_jobs.h")).read()
    incl = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert sorted(i.strip('"') for i in incl if i.startswith('"')) == ["msm_geom.h", "msm_select.h", "msm_types.h"]
    assert all(i.startswith("<") and "/" not in i and "hip" not in i for i in incl if not i.startswith('"'))
    for word in ("amsm_ctx*", "amsm_bases*", "hipStream", "hipError", "__global__"):
        assert word not in text, word


def test_output_matches_the_golden(output):
    want = open(GOLDEN).read()
    assert output.splitlines() == want.splitlines()
    assert len(want) < 256 * 1024


def test_20_bit_key_device_vectors(rows):
    """ranges of 2^20; the leading ranges that take the bucket-per-lane pipeline (more than 2^18 pairs) in one set of 2^19 buckets"""
    rg = lambda c: ranges(rows, "dev20_n_" + c)[1]  # noqa: E731
    assert rg("2p20") == cut(P(20), P(20))  # one job, no set
    assert rg("2p20_plus_1") == cut(P(20) + 1, P(20))  # the second range is no bucket-per-lane MSM: one range alone is no set
    assert rg("2p21") == in_set(cut(P(21), P(20)), 2)
    # a last range of exactly 2^18 pairs is not bucket-per-lane: it stays outside the set ...
    assert rg("2p21_plus_2p18") == in_set(cut(P(21) + P(18), P(20)), 2) and rg("2p21_plus_2p18")[2][2] == P(18)
    # ... one pair more and it joins
    assert rg("2p21_plus_2p18_plus_1") == in_set(cut(P(21) + P(18) + 1, P(20)), 3)
    assert rg("2p22") == in_set(cut(P(22), P(20)), 4) == rg("2p22_off_2p20")
    assert rg("2p20_plus_2p18_only_first_bpl") == cut(P(20) + P(18), P(20))  # n_sh >= 2
    assert rg("2p22_share_off") == cut(P(22), P(20))
    assert rg("2p22_bpl_off") == cut(P(22), P(21))  # (no MSM takes the 20-bit table: the other keys' rule)
    # two vectors, two sets, numbered in order
    want = in_set(cut(P(21), P(20)), 2) + in_set(cut(P(21) + 1, P(20), vec=1), 2, set_id=1)
    assert ranges(rows, "dev20_two_sets")[1] == want and rows[("ranges", "dev20_two_sets")]["sets"] == 2


def test_20_bit_key_skewed_vectors(rows):
    """over the twin, cut by the twin's rule: no split below 2^22 pairs, ranges of 2^split_log2 from there"""
    for case, n, step in (("n_2p20_plus_1", P(20) + 1, P(22)), ("n_2p22_minus_1", P(22) - 1, P(22)), ("n_2p22", P(22), P(21)),
                          ("n_2p22_split_log2_20", P(22), P(20)), ("n_2p22_split_log2_0", P(22), P(23))):
        row, rs = ranges(rows, "dev20_skew_" + case)
        assert rs == cut(n, step, twin=1) and row["twin"] == 1 and row["sets"] == 0, case
    # a skewed and an unskewed vector in one call: each by its own key's rule
    row, rs = ranges(rows, "dev20_skew_and_not")
    assert rs == cut(P(21) + 1, P(22), twin=1) + in_set(cut(P(21) + 1, P(20), vec=1), 2) and row["twin"] == 1
    assert rows[("ranges", "dev20_n_2p22")]["twin"] == 0


def test_17_bit_key(rows):
    assert ranges(rows, "dev17_n_2p22_minus_1")[1] == cut(P(22) - 1, P(22))
    assert ranges(rows, "dev17_n_2p22")[1] == cut(P(22), P(21))
    # a skew verdict runs the vector chunked over the same key ...
    for form in ("dev17", "host17"):
        assert ranges(rows, form + "_skew_alone")[1] == cut(P(17), P(17), forced=1) + cut(P(17), P(17), vec=1)
        assert rows[("ranges", form + "_skew_alone")]["twin"] == 0
    # ... unless another vector of the call is cut: the device form forgets every verdict, the host form keeps them
    assert ranges(rows, "dev17_skew_beside_a_split")[1] == cut(P(17), P(17)) + cut(P(22), P(21), vec=1)
    assert ranges(rows, "host17_skew_beside_a_split")[1] == cut(P(17), P(17), forced=1) + cut(P(22), P(21), vec=1)
    assert ranges(rows, "dev17_skew_is_the_split")[1] == cut(P(22), P(21))
    assert ranges(rows, "host17_skew_is_the_split")[1] == cut(P(22), P(21), forced=1)


def test_plain_key(rows):
    for form in ("devplain", "hostplain"):
        assert ranges(rows, form + "_n_2p20")[1] == cut(P(20), P(20))
        assert ranges(rows, form + "_n_2p20_plus_1")[1] == cut(P(20) + 1, P(20))  # (no set: a plain key has one per window)
    for sw in ("bpl_plain_off", "window_override"):  # chunked: never cut
        assert ranges(rows, "devplain_n_2p20_" + sw)[1] == cut(P(20), P(20))
        assert ranges(rows, "devplain_n_2p20_plus_1_" + sw)[1] == cut(P(20) + 1, P(21))


def test_empty_vectors(rows):
    """the device form keeps an empty vector as one empty job, the host form drops it"""
    for case in ("empty", "empty_at_the_key_s_end"):
        assert ranges(rows, "dev20_" + case)[1] == [(0, 0, 0, 0, 0, -1, 0, 0, 0)]
        assert ranges(rows, "host20_" + case)[1] == []
    assert ranges(rows, "dev17_empty_between")[1] == cut(P(16), P(16)) + cut(0, 1, vec=1) + cut(P(16), P(16), vec=2)
    assert ranges(rows, "host17_empty_between")[1] == cut(P(16), P(16)) + cut(P(16), P(16), vec=2)


def test_host_halves_and_one_shot(rows):
    """the lone slice of [3 * 2^18, 2^20] pairs over a 20-bit key in two halves (the first a multiple of 64) over one set"""
    sizes = {"3x2p18_minus_1": 3 * P(18) - 1, "3x2p18": 3 * P(18), "3x2p18_plus_1": 3 * P(18) + 1, "2p20": P(20), "2p20_plus_1": P(20) + 1}
    for tag, n in sizes.items():
        case, whole = "host20_n_" + tag, cut(n, P(20))
        row, rs = ranges(rows, case)
        if 3 * P(18) <= n <= P(20):
            h1 = (((n + 1) // 2 + 63) // 64) * 64
            assert rs == in_set(cut(n, h1), 2) and row["sets"] == 1, case
            assert rows[("halves", case)] == {"r": [], "u": [], "j": [], "h1": h1, "B": B20}
            assert h1 % 64 == 0 and 0 <= h1 - (n - h1) < 128
        else:
            assert rs == whole and ("halves", case) not in rows, case
        # never: several slices, the re-run after an overflow, a skewed slice, a one-shot call, either switch off
        assert ranges(rows, case + "_k2")[1] == whole + [(1,) + r[1:] for r in whole]
        assert ranges(rows, case + "_no_halves")[1] == ranges(rows, case + "_host_halves_off")[1] == ranges(rows, case + "_share_off")[1] == whole
        assert ranges(rows, case + "_skew")[1] == cut(n, P(22), twin=1) and rows[("ranges", case + "_skew")]["twin"] == 1
        assert ranges(rows, case + "_oneshot_step_2p19")[1] == cut(n, P(19))
        assert ranges(rows, case + "_oneshot_no_step")[1] == whole
    assert rows[("halves", "host20_n_3x2p18_plus_1")]["h1"] == 3 * P(17) + 64  # odd: rounded up
    assert ranges(rows, "host17_n_2p20_no_halves_without_a_20_bit_table")[1] == cut(P(20), P(20))
    # a long slice is cut like a device vector, but the host form arms no set for its ranges
    assert ranges(rows, "host20_n_2p22")[1] == cut(P(22), P(20)) and ranges(rows, "dev20_n_2p22")[0]["sets"] == 1
    # the one-shot step: lengths 1, step, step + 1
    for tag, n in (("1", 1), ("2p18", P(18)), ("2p18_plus_1", P(18) + 1)):
        assert ranges(rows, "hostplain_oneshot_step_2p18_n_" + tag)[1] == cut(n, P(18))


def test_units(rows):
    """runs of equal bucket-split jobs in units of at most 8; the check asserts that the units cover the jobs in order, exactly once"""
    u = lambda c: rows[("units", c)]  # noqa: E731
    assert [u("run_of_%d" % n)["u"] for n in (1, 2, 8, 9, 17)] == [[(0, 1)], [(0, 2)], [(0, 8)], [(0, 8), (8, 1)], [(0, 8), (8, 8), (16, 1)]]
    assert all(j == (1, 0) for j in u("run_of_17")["j"])
    # a job that never joins a unit, between equal jobs: its geometry is not looked at, and nothing is inherited across it
    for between in ("skewed", "grouped", "shared"):
        r = u(between + "_between")
        assert r["u"] == [(0, 1), (1, 1), (2, 2)] and r["j"] == [(1, 0), (0, 0), (1, 0), (1, 0)], between
    assert u("skewed_first")["u"] == [(0, 1), (1, 2)] and u("skewed_first")["j"] == [(0, 0), (1, 0), (1, 0)]
    # equal but for the offset, the scalar form, the unit-scalar handling, the key
    assert u("differ_in_off")["u"] == [(0, 1), (1, 2), (3, 1)]
    assert u("differ_in_mont")["u"] == u("differ_in_skip_ones")["u"] == [(0, 1), (1, 1)]
    assert u("differ_in_key")["u"] == [(0, 1), (1, 2)] and u("differ_in_key")["j"] == [(1, 0), (1, 1), (1, 1)]
    assert u("not_bucket_split_2p15")["u"] == [(0, 1), (1, 1)] and u("not_bucket_split_2p15")["j"] == [(0, 0), (0, 0)]
    # AMSM_BPS_BATCH
    assert u("bps_batch_0")["u"] == u("bps_batch_1")["u"] == [(i, 1) for i in range(5)]
    assert u("bps_batch_2")["u"] == [(0, 2), (2, 2), (4, 1)]
    # a unit stays below 512 MiB of slot
    cap = u("slot_bytes_cap")
    fit = (512 << 20) // cap["slot_bytes"]
    assert 2 <= fit < 8 and cap["u"] == [(0, fit), (fit, 8 - fit)] and u("run_of_8")["slot_bytes"] * 8 < (512 << 20)
    # a 20-bit key's bucket-split MSMs run over its twin; without one they stay singles
    assert u("twin_present")["u"] == [(0, 3)] and u("twin_present")["j"] == [(1, 1)] * 3
    assert u("twin_absent")["u"] == [(0, 1), (1, 1), (2, 1)] and u("twin_absent")["j"] == [(0, 1)] * 3


def test_probes(rows):
    p = lambda c: (rows[("probe", c)]["verdict"], rows[("probe", c)]["loads"])  # noqa: E731
    assert rows[("probe_min_len", "")] == {"table17": P(16), "table20": P(18) + 1}
    assert rows[("probe_wanted", "")] == {"table17_n_2p16": 1, "table17_n_2p15": 0, "table20_n_2p19": 1, "plain_n_2p20": 0, "empty": 0}
    assert p("uniform_below_2p254") == p("uniform_over_the_20_bit_walk") == (0, 1024)
    assert p("constant") == p("constant_n_min_len") == (1, 1024)
    assert p("constant_n_min_len_minus_1") == (0, 0)  # false without looking
    assert p("samples_sharing_a_digit_23") == (0, 1024) and p("samples_sharing_a_digit_24") == (1, 1024)  # PROBE_LIMIT
    tv = lambda c: rows[("tv", c)]["looks"]  # noqa: E731
    assert (tv("distinct_0"), tv("distinct_1"), tv("distinct_2"), tv("distinct_2_between_samples")) == (1, 1, 0, 1)
    assert (rows[("ones", "samples_7")]["has"], rows[("ones", "samples_8")]["has"]) == (0, 1)  # TV_ONES_MIN_SAMPLES
    # the same pointer with another length is another vector; a chain of equals resolves to its first
    assert rows[("identical", "chain")]["first"] == (0, 1, 0, 3, 0, 3)
