"""How many bucket sets a plain key's top window owns on the bucket-per-lane pipeline, without a GPU: tests/cpp_host/top_sets_check.cpp is
plain C++ over csrc/msm_select.h (the rule, plain_top_sets) and csrc/msm_types.h (the prep's set routing, window_set; the top window's
shift and reach per curve).  The rule and the reach are restated here in Python and compared row by row; the figures DESIGN.md 4.1
quotes are pinned as literals."""
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp_host", "top_sets_check.cpp")
EXE = os.path.join(ROOT, "build", "top_sets_check")
CAP = 40960 - 3620  # kern_fr.hip: the LDS stage of k_prep_local_t, entries
MODULI = {  # the six scalar fields
    "pallas": 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001,
    "vesta": 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001,
    "bls12_381_g1": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
    "bn254_g1": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
    "grumpkin": 21888242871839275222246405745257275088696311157297823662689037894645226208583,
    "bls12_377_g1": 8444461749428370424248824938781546531375899335154063827935233455917409239041,
}


@pytest.fixture(scope="module")
def lines():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", EXE])
    return subprocess.run([EXE], capture_output=True, text=True, check=True).stdout.splitlines()  # (exit status 1: a check of its own failed)


def part_max(n, nb, reach, T, groups):
    per_win, per_top = -(-n * 1024 // nb), -(-n * 1024 // reach)
    pm = max(per_win, -(-2 * per_top // T))
    return (pm + 1) // 2 if groups == 2 else pm


def top_sets(n, nb, reach, W, groups=1, max_sets=8):
    """the rule, restated: the smallest T of 2, 4, 8 whose geometry meets both inequalities of prep_bpl_supported"""
    for T in (2, 4, 8):
        if T > max_sets:
            break
        P = (groups * (W + T) * nb) >> 10
        pm = part_max(n, nb, reach, T, groups)
        if n * W // P + 1024 <= CAP and pm + 5 * math.isqrt(pm) <= CAP:
            return T
    return 0


def test_rule_rows(lines):
    got = {}
    for ln in lines:
        w = ln.split()
        if w[0] == "rule":
            got[tuple(int(x) for x in w[1:6])] = int(w[6][2:])
    # (n, nb, reach, W, groups) -> T: BN254 / Grumpkin, BLS12-377, BLS12-381, Pallas / Vesta on 16-bit windows; the reach figures
    # that would need eight sets or more than eight; 15-bit windows
    want = {(786432, 32768, 24776, 16, 1): 2, (917504, 32768, 24776, 16, 1): 4, (1 << 20, 32768, 24776, 16, 1): 4,
            (1 << 19, 32768, 19116, 16, 1): 2, (786432, 32768, 19116, 16, 1): 4, (1 << 20, 32768, 19116, 16, 1): 4,
            (1 << 20, 32768, 29678, 16, 1): 2, (1 << 20, 32768, 32768, 16, 1): 2, ((1 << 18) + 1, 32768, 32768, 16, 1): 2,
            (1 << 20, 32768, 9560, 16, 1): 8, (1 << 20, 32768, 4000, 16, 1): 0, (1 << 18, 16384, 9560, 18, 1): 2,
            (1 << 18, 16384, 4780, 18, 1): 4}
    for k, T in want.items():
        assert got[k] == T, (k, got[k], T)
    for k, T in got.items():  # every printed row, the grouped ones included, against the restatement
        assert T == top_sets(*k), (k, T)
    # the part_max figures of the table the rule was specified with
    assert [part_max(786432, 32768, 24776, 2, 1), part_max(917504, 32768, 24776, 2, 1), part_max(1 << 20, 32768, 24776, 2, 1)] == [32504, 37921, 43338]
    assert [part_max(917504, 32768, 24776, 4, 1), part_max(1 << 20, 32768, 24776, 4, 1)] == [28672, 32768]
    assert [part_max(1 << 19, 32768, 19116, 2, 1), part_max(786432, 32768, 19116, 2, 1), part_max(1 << 20, 32768, 19116, 2, 1)] == [28085, 42128, 56170]
    assert [part_max(786432, 32768, 19116, 4, 1), part_max(1 << 20, 32768, 19116, 4, 1)] == [24576, 32768]
    assert part_max(1 << 20, 32768, 29678, 2, 1) == 36180 and 36180 + 5 * math.isqrt(36180) == 37130 <= CAP


def test_rule_edges(lines):
    """the largest n with two sets and the smallest with four, per reach, over n in (2^17, 2^20] on 16-bit windows"""
    got = {}
    for ln in lines:
        m = re.match(r"edge 32768 (\d+) last_T2=(\d+) first_T4=(\d+) last_T4=(\d+)", ln)
        if m:
            got[int(m.group(1))] = tuple(int(x) for x in m.groups()[1:])
    assert got[24776] == (880467, 880468, 1 << 20) and got[19116] == (679327, 679328, 1 << 20)
    assert got[9560][2] == got[19120][0]  # half the reach with four sets ends where two sets end
    for reach, (last2, first4, last4) in got.items():
        assert first4 == last2 + 1
        for n in (last2 - 1, last2, first4, first4 + 1, last4):
            assert top_sets(n, 32768, reach, 16) == (2 if n <= last2 else 4), (reach, n)
        assert last4 == 1 << 20 or top_sets(last4 + 1, 32768, reach, 16) == 8


def test_two_sets_exactly_where_two_fitted_before(lines):
    (ln,) = [x for x in lines if x.startswith("parent_equiv")]
    f = dict(kv.split("=") for kv in ln.split()[1:])
    assert int(f["cases"]) > 200000 and f["mismatches"] == f["over_two"] == f["bad_T"] == "0"
    # AMSM_TOP_SETS=2: two sets or none
    assert top_sets(1 << 20, 32768, 24776, 16, max_sets=2) == 0 and top_sets(786432, 32768, 24776, 16, max_sets=2) == 2


def test_group_bit_never_picks_the_top_set(lines):
    rows = [dict(kv.split("=") for kv in ln.split()[1:]) for ln in lines if ln.startswith("group_bit")]
    assert len(rows) == 3 * 2 * 5
    for r in rows:
        T, groups, shift = int(r["T"]), int(r["groups"]), int(r["shift"])
        per = (8192 if groups == 2 and shift >= 12 else 4096) // (groups * T)  # indices of one (group, top set) pair
        assert (int(r["min"]), int(r["max"])) == (per, per), r
        assert r["parent"] == ("1" if T == 2 else "-") and r["other_windows"] == "1", r


def reach_of(r, c):
    """top_window_shift and top_window_reach restated: (W, narrow windows, first bit, shift, largest raw digit, buckets reached)"""
    W = 255 // c + 1
    nn = W * c - 256
    lo = (W - nn) * c + (nn - 1) * (c - 1) if nn else (W - 1) * c
    cb = c - (1 if nn >= 2 else 0)  # width of the window below the top one
    top, below = (r - 1) >> lo, ((r - 1) >> (lo - cb)) & ((1 << cb) - 1)
    raw = top + (1 if below + 1 > (1 << (cb - 1)) else 0)
    narrow, s = (1 if nn else 0), 0
    while s + 1 < c and (raw << (narrow + s + 1)) <= (1 << (c - 1)):
        s += 1
    return W, nn, lo, s, raw, max(1024, min(1 << (c - 1), raw << (s + narrow)))


def test_top_window_reach_per_curve(lines):
    mods = {w[1]: int(w[2], 16) for w in (ln.split() for ln in lines) if w[0] == "modulus"}
    assert mods == MODULI
    got = {}
    for ln in lines:
        m = re.match(r"reach (\w+) c=(\d+) W=(\d+) narrow=(\d+) lo=(\d+) shift=(\d+) raw_max=(\d+) reach=(\d+)", ln)
        if m:
            got[(m.group(1), int(m.group(2)))] = tuple(int(x) for x in m.groups()[2:])
    assert len(got) == 18
    for (name, c), row in got.items():
        assert row == reach_of(MODULI[name], c), (name, c, row)
    # (shift, largest raw top digit, reach) on the plain keys' windows and the 20-bit table
    pin = {("pallas", 15): (1, 4096, 16384), ("pallas", 16): (1, 16384, 32768), ("pallas", 20): (1, 131072, 524288),
           ("bls12_381_g1", 15): (0, 7419, 14838), ("bls12_381_g1", 16): (0, 29678, 29678), ("bls12_381_g1", 20): (0, 237421, 474842),
           ("bn254_g1", 15): (1, 3097, 12388), ("bn254_g1", 16): (1, 12388, 24776), ("bn254_g1", 20): (1, 99106, 396424),
           # BLS12-377, r >> 240 = 0x12ab: shift TWO on every width -- 19 116 buckets on 16-bit windows, not 9560
           ("bls12_377_g1", 15): (2, 1195, 9560), ("bls12_377_g1", 16): (2, 4779, 19116), ("bls12_377_g1", 20): (2, 38235, 305880)}
    for k, v in pin.items():
        assert got[k][3:] == v, (k, got[k])
    for c in (15, 16, 20):
        assert got[("vesta", c)] == got[("pallas", c)] and got[("grumpkin", c)] == got[("bn254_g1", c)]


def test_tail_covers_eight_top_sets(lines):
    rows = [ln for ln in lines if ln.startswith("tail ")]
    assert len(rows) == 15 and all(ln.endswith("covered=1") for ln in rows)
