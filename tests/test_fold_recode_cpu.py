"""How the host recodes the scalar of a key fold -- accumulation_amd/csrc/fold_recode.h: the low bits, the non-adjacent form, the op
list of the table ladder and its refusals; csrc/host_glv.h: fold_digits, the GLV form of full-size scalars on all six curves -- without
a GPU and without libamsm.so.  tests/cpp_host/fold_recode_check.cpp prints the structures the fold kernels take as arguments for the
cases written below; the curve-independent half is plain C++ over fold_recode.h alone, the GLV half the host side of a hipcc build.

The output is compared with tests/golden/fold_recode.txt, which was recorded ONCE, from the recoding as it stood inside
launch_points_fold / launch_points_fold_tab of kern_ec.inc (cut out character for character) before the three non-adjacent forms and
the two low-bits loops were stated once: a change of it is a change of what a fold kernel is launched with.  Independently of the
golden, every printed structure is checked in Python integers: the digits give back the scalar, no two are adjacent, the GLV halves
recombine modulo r, the op list is ordered as the kernel walks it, and every refusal is one."""
import os
import subprocess

import pytest

from oracle import pyref as o
from tests import helpers as h
from tests.test_fold_gpu import _scalars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "accumulation_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp_host", "fold_recode_check.cpp")
BUILD = os.path.join(ROOT, "build")
GOLDEN = os.path.join(ROOT, "tests", "golden", "fold_recode.txt")
CURVES = {"pallas": o.PALLAS, "bls12_381": o.BLS12_381_G1, "vesta": h.VESTA, "bn254": h.BN254, "grumpkin": h.GRUMPKIN, "bls12_377": h.BLS12_377}
GLV_BITS = 140  # a masked scalar longer than this is split (host_glv.h: fold_digits)

_RND = [o.rng_scalar(0xF01D, i) for i in range(4)]
X140 = (1 << 139) | (_RND[1] % (1 << 139))  # exactly 140 bits: the longest scalar that stays plain
X141 = (1 << 140) | (_RND[2] % (1 << 140))  # exactly 141 bits: the shortest that is split
ALL_ONES = (1 << 255) - 1                    # every digit but the last a carry: the longest carry chain of the plain form

# the table geometries of the keys (c, W, n_narrow): 17- and 16-bit windows, the 20-bit table with four narrow windows, 8-bit windows;
# each with every level usable and with the top one left out (amsm_bases_fold: top_shift)
GEOMS = [(17, 16, 0), (16, 16, 0), (20, 13, 4), (8, 32, 0)]
# (c, W, n_narrow, levels, x, nbits, why): each must be refused
REFUSED = [
    (3, 16, 0, 16, 5, 255, "c = 3"),
    (31, 9, 0, 9, 5, 255, "c = 31"),
    (17, 16, 0, 0, 5, 255, "levels = 0"),
    (8, 40, 0, 33, 5, 255, "levels = 33"),
    (17, 16, 0, 17, 5, 255, "levels > W"),
    (20, 13, 13, 13, 5, 255, "n_narrow >= W"),
    (16, 16, 0, 15, 1 << 240, 255, "top bit of x beyond e_of(levels)"),
    (20, 13, 4, 12, 1 << 236, 255, "top bit of x beyond e_of(levels), narrow levels"),
    # nd > 31: the last level of a table that does not span the scalar takes every bit up to the top one
    (30, 2, 0, 2, 1 << 62, 255, "nd > 31: a top digit of 33 bits"),
    (30, 2, 0, 2, (1 << 61) - 1, 255, "nd > 31: a top digit of 31 ones, whose form is 2^31 - 1"),
]
# ... and their accepted neighbours
ACCEPTED = [(4, 64, 0, 32, 5, 255), (30, 9, 0, 9, 5, 255), (8, 40, 0, 32, 5, 255), (20, 13, 12, 13, 5, 255),
            (16, 16, 0, 15, (1 << 240) - 1, 255), (20, 13, 4, 12, (1 << 236) - 1, 255), (30, 2, 0, 2, 1 << 60, 255)]
# ops > 160 has no admissible input: a digit of b bits has at most (b + 2) / 2 non-zero positions, so 32 levels over 255 bits have at
# most (255 + 64) / 2 = 159 -- which 8-bit windows reach (five per digit, four in the 7-bit top one): the case below.  The check stays.
DENSEST = sum(171 << (8 * j) for j in range(32)) & ((1 << 255) - 1)  # 171 = 2^8 - 2^6 - 2^4 - 2^2 - 1


def _edges(c):
    k = c.r.bit_length() - 1
    return [c.r - 1, c.r - 2, (c.r - 1) // 2, (c.r + 1) // 2, 1 << k]


def _fold_cases(c):
    """(x, nbits) of one curve, all below r: the GPU fold test's scalars, the GLV check's edges, the threshold from both sides -- by the
    scalar's own length and by the mask --, and the three widths"""
    both = (1 << 139) | (1 << 140) | (_RND[3] % (1 << 139))
    out = _scalars(c) + [(x, 255) for x in _edges(c)] + [(X140, 255), (X141, 255), (both, 140), (both, 141)]
    out += [(c.r - 1, 128), (c.r - 1, 200), (_RND[0] % c.r, 200), (0, 128)]
    return list(dict.fromkeys(out))


def _plain_cases():
    out = [(0, 255), (1, 255), (2, 255), ((1 << 17) - 1, 255), (1 << 17, 255), ((1 << 128) - 1, 128), (_RND[0] % (1 << 128), 128),
           (X140, 255), (X141, 255), (ALL_ONES, 255), (ALL_ONES, 200), (ALL_ONES, 128), (0, 128)]
    for c in CURVES.values():
        out += [(x, 255) for x in _edges(c)] + [(_RND[1] % c.r, 255), (_RND[2] % c.r, 255)]
    out += [(o.PALLAS.r - 1, 128), (o.PALLAS.r - 1, 200), (_RND[3] % o.PALLAS.r, 200)]
    return list(dict.fromkeys(out))


def _tab_cases():
    c0, c1 = o.PALLAS, o.BLS12_381_G1
    sc = [(0, 255), (1, 255), (2, 255), ((1 << 17) - 1, 255), (1 << 17, 255), ((1 << 128) - 1, 128), (_RND[0] % (1 << 128), 128),
          (X140, 255), (X141, 255), (ALL_ONES, 255), (ALL_ONES, 200), (ALL_ONES, 128)]
    sc += [(x, 255) for x in _edges(c0)] + [(_RND[1] % c0.r, 255), (_RND[3] % c0.r, 200), (c1.r - 1, 255), (_RND[2] % c1.r, 255)]
    out = [(c, W, nn, lv, x, nb) for (c, W, nn) in GEOMS for lv in (W, W - 1) for x, nb in sc]
    out += [r[:6] for r in REFUSED] + ACCEPTED + [(8, 32, 0, 32, DENSEST, 255)]
    return list(dict.fromkeys(out))


def _case_file():
    lines = ["plain %d %x" % (nb, x) for x, nb in _plain_cases()]
    lines += ["tab %d %d %d %d %d %x" % (c, W, nn, lv, nb, x) for c, W, nn, lv, x, nb in _tab_cases()]
    for name, c in CURVES.items():
        lines += ["fold %s %d %x" % (name, nb, x) for x, nb in _fold_cases(c)]
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def output():
    os.makedirs(BUILD, exist_ok=True)
    cases, plain, glv = (os.path.join(BUILD, "fold_recode_" + n) for n in ("cases.txt", "check", "check_glv"))
    with open(cases, "w") as f:
        f.write(_case_file())
    builds = [subprocess.Popen(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", plain]),
              subprocess.Popen(["hipcc", "-std=c++17", "-O2", "--offload-host-only", "--offload-arch=gfx950", "-x", "hip", "-w",
                                "-DFOLD_RECODE_GLV", "-I", CSRC, SRC, "-o", glv])]
    assert [b.wait() for b in builds] == [0, 0]
    return "".join(subprocess.run([exe, cases], capture_output=True, text=True, check=True, timeout=300).stdout for exe in (plain, glv))


def _int(v):
    return int(v, 16)


@pytest.fixture(scope="module")
def rows(output):
    """kind -> [record]: the positional words under their names, the key=value words as they stand"""
    names = {"plain": ("nbits", "x"), "tab": ("c", "W", "nn", "levels", "nbits", "x"), "fold": ("curve", "nbits", "x"), "curve": ("curve",)}
    out = {k: [] for k in names}
    for ln in output.splitlines():
        w = ln.split()
        pos = [x for x in w[1:] if "=" not in x]
        rec = dict(zip(names[w[0]], pos))
        assert len(pos) == len(names[w[0]]), ln
        rec.update(x.split("=") for x in w[1:] if "=" in x)
        out[w[0]].append(rec)
    return out


def test_output_matches_the_golden(output):
    assert output.splitlines() == open(GOLDEN).read().splitlines()
    assert os.path.getsize(GOLDEN) < 128 * 1024


def test_every_case_is_answered(rows):
    assert [(_int(r["x"]), int(r["nbits"])) for r in rows["plain"]] == _plain_cases()
    assert [tuple(int(r[k]) for k in ("c", "W", "nn", "levels")) + (_int(r["x"]), int(r["nbits"])) for r in rows["tab"]] == _tab_cases()
    assert [r["curve"] for r in rows["curve"]] == list(CURVES)
    for name, c in CURVES.items():
        assert [(_int(r["x"]), int(r["nbits"])) for r in rows["fold"] if r["curve"] == name] == _fold_cases(c)
    assert all(x < 1 << 255 for x, _ in _plain_cases()) and all(t[4] < 1 << 255 for t in _tab_cases())
    assert all(x < c.r for c in CURVES.values() for x, _ in _fold_cases(c))
    # the threshold's two sides, and the longest carry chain, are among the cases
    assert (X140.bit_length(), X141.bit_length()) == (GLV_BITS, GLV_BITS + 1) and (ALL_ONES, 255) in _plain_cases()


def _signed(pos, neg, nd):
    """the value of a digit string, after checking that it is a non-adjacent form of nd positions"""
    assert pos & neg == 0
    nz = pos | neg
    assert nz & (nz >> 1) == 0, "adjacent non-zero digits"
    assert nd == nz.bit_length()
    return pos - neg


def _check_plain(r):
    x = _int(r["x"]) % (1 << int(r["nbits"]))
    assert _signed(_int(r["pos1"]), _int(r["neg1"]), int(r["nd"])) == x
    assert int(r["nd"]) in ((0,) if x == 0 else (x.bit_length(), x.bit_length() + 1))
    assert _int(r["pos2"]) == _int(r["neg2"]) == _int(r["beta"]) == 0


def test_plain_form(rows):
    for r in rows["plain"]:
        _check_plain(r)
        assert int(r["top"]) == (_int(r["x"]) % (1 << int(r["nbits"]))).bit_length()
    zero = [r for r in rows["plain"] if _int(r["x"]) == 0]
    assert zero and all(int(r["nd"]) == 0 and _int(r["pos1"]) == _int(r["neg1"]) == 0 for r in zero)
    ones = next(r for r in rows["plain"] if _int(r["x"]) == ALL_ONES and r["nbits"] == "255")
    assert (_int(ones["pos1"]), _int(ones["neg1"]), int(ones["nd"])) == (1 << 255, 1, 256)


def test_glv_form(rows):
    for info in rows["curve"]:
        c = CURVES[info["curve"]]
        lam, beta = _int(info["lambda"]), _int(info["beta"])
        assert 1 < lam < c.r and 1 < beta < c.p and pow(lam, 3, c.r) == 1 and pow(beta, 3, c.p) == 1
        mine = [r for r in rows["fold"] if r["curve"] == info["curve"]]
        split = 0
        for r in mine:
            x = _int(r["x"]) % (1 << int(r["nbits"]))
            assert int(r["glv"]) == (x.bit_length() > GLV_BITS), r
            if r["glv"] == "0":
                _check_plain(r)
                continue
            split += 1
            nd = int(r["nd"])
            halves = [(_int(r["pos" + i]), _int(r["neg" + i])) for i in "12"]
            k1, k2 = (_signed(p, n, (p | n).bit_length()) for p, n in halves)
            assert (k1 + k2 * lam - x) % c.r == 0
            assert nd == max((p | n).bit_length() for p, n in halves) and nd <= 160
            assert _int(r["beta"]) == beta * (1 << (64 * c.limbs)) % c.p  # the C ABI's Montgomery words
        assert split >= 10 and len(mine) - split >= 10


def _exponents(c, W, nn):
    """e_w of msm_types.h: window_exponent_of with no top shift: the window's first bit, one less for a narrow window"""
    reg = W - nn
    return [w * c if w < reg else reg * c + (w - reg) * (c - 1) - 1 for w in range(W)]


def _naf_weight_and_length(v):
    n = w = 0
    while v:
        if v & 1:
            v += 1 if v & 3 == 3 else -1
            w += 1
        v >>= 1
        n += 1
    return w, n


def _fits(c, W, nn, levels, x):
    """the rule of fold_tab_ops restated: the geometry is one, x ends below the first unusable level, every level's digit takes at
    most 31 positions and all of them at most 160 additions"""
    if not (4 <= c <= 30 and 1 <= levels <= 32 and levels <= W and nn < W):
        return False
    e = _exponents(c, W, nn) + [256]
    if levels < W and x.bit_length() > e[levels]:
        return False
    digits = [(x >> e[w]) & ((1 << (e[w + 1] - e[w])) - 1) if w + 1 < levels else x >> e[w] for w in range(levels)]
    forms = [_naf_weight_and_length(v) for v in digits]
    return sum(f[0] for f in forms) <= 160 and max(f[1] for f in forms) <= 31


def test_table_form(rows):
    accepted = 0
    for r in rows["tab"]:
        c, W, nn, levels, nbits = (int(r[k]) for k in ("c", "W", "nn", "levels", "nbits"))
        x = _int(r["x"]) % (1 << nbits)
        assert int(r["ok"]) == _fits(c, W, nn, levels, x), r
        if r["ok"] == "0":
            assert set(r) == {"c", "W", "nn", "levels", "nbits", "x", "ok"}  # (the checker itself ends the run unless the ops were left zeroed)
            continue
        accepted += 1
        e = [int(v) for v in r["e"].split(",")]
        assert e == _exponents(c, W, nn)[:levels]
        ops = [int(r["ops"][i:i + 4], 16) for i in range(0, len(r["ops"]), 4)]
        n_ops, nd = int(r["n_ops"]), int(r["nd"])
        assert len(ops) == n_ops <= 160 and nd <= 31
        where = [(op & 31, (op >> 5) & 31) for op in ops]  # (position, level)
        assert all(op & 0x7C00 == 0 for op in ops) and all(lv < levels for _, lv in where)
        assert sum((-1 if op >> 15 else 1) << (p + e[lv]) for op, (p, lv) in zip(ops, where)) == x
        # as the kernel walks it: positions never rise, and within one position the levels keep the order they were recoded in
        assert all(a[0] > b[0] or (a[0] == b[0] and a[1] < b[1]) for a, b in zip(where, where[1:]))
        assert nd == (max(p for p, _ in where) + 1 if ops else 0)
        for lv in range(levels):  # every level's digit is a non-adjacent form
            nz = sum(1 << p for p, l in where if l == lv)
            assert nz & (nz >> 1) == 0
    assert accepted >= 100
    for c, W, nn, levels, x, nbits, why in REFUSED:
        assert not _fits(c, W, nn, levels, x % (1 << nbits)), why
    assert all(_fits(*t[:4], t[4] % (1 << t[5])) for t in ACCEPTED)
    # a key's top level left out: a full-size scalar does not fit and the fold takes the plain ladder
    assert not _fits(16, 16, 0, 15, o.PALLAS.r - 1) and _fits(16, 16, 0, 16, o.PALLAS.r - 1)
    dense = next(r for r in rows["tab"] if _int(r["x"]) == DENSEST)
    assert (dense["ok"], dense["n_ops"]) == ("1", "159")
