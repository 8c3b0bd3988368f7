"""Exact-integer model of the CONTRACTS of the device's field primitives and group law (csrc/fpu.h, fp.h, ec.h), for the
field probe (tests/hip/field_probe.hip).  Python integers only.

For every probed function the model gives
  * a predicate for the documented Needs (limb widths, value bounds) -- no generated case may violate it;
  * the expected residue class, or the exact value where the contract is exact;
  * the documented Gives: tightness, limb widths and the value bound.
It checks contracts, not the algorithm: a result is right if it is tight, lies in the documented range and is congruent
to the right value.  Nothing here is a copy of u_columns.

The packs are parametrised by (p, L, B): p from the oracle's curves (oracle/pyref.py, tests/helpers.py), the limb shape
from the width of p (9 x 29 bits up to 256 bits, 14 x 28 bits above); tests/test_field_probe_cpu.py compares the derived
constants with the tables compiled into csrc/fpu.h.

A curve of even order (BLS12-377) has a point T = (x, 0) of order 2.  Its doubling is the identity, and on an unsaturated
field the formulas reach that identity as a NON-ZERO multiple of p unless the doubling tests Y = 0 mod p first (csrc/ec.h,
fp.h: HasTwoTorsion).  For such a pack the group-law cases also hold T with Y written as every multiple of p its invariant
admits, and the small-order points around it (SMALL_ORDER, _two_torsion_cases).
"""
from __future__ import annotations

import functools
import json
import math
import os
import random
import re
from dataclasses import dataclass
from typing import Optional

from oracle import pyref as o
from tests import helpers as h

HERE = os.path.dirname(os.path.abspath(__file__))
STRIDE, N_IN, N_OUT = 16, 8, 4  # words per slot, operand slots, result slots (field_probe.hip)
MAX_CASES = 512

# the operation table: same names, same order as PROBE_OPS in tests/hip/field_probe.hip
OPS = ["mul", "sqr",
       "mul_sub_k4", "mul_sub_k9", "mul_sub_k10", "mul_sub_k13", "mul_sub_k14",
       "sqr_sub_bcc_k4", "sqr_sub_bcc_k10",
       "mul_sub_mul_k2", "mul_sub_mul_k4", "mul_sub_mul_k16",
       "sub_k2", "sub_k4", "sub_k8", "sub_k12",
       "sub_bcc_k4", "dbl", "triple", "neg_lazy", "neg_lazy_tight",
       "is_zero_mod4", "is_zero_mod8", "is_zero_mod16",
       "canon2", "canon4", "canon8",
       "import", "export", "from_words", "store",
       "xyzz_dbl", "xyzz_dbl_affine", "xyzz_madd", "xyzz_add", "affine_neg_if",
       "jac_dbl", "jac_madd", "xyzz_from_jac", "xyzz_dbl_quad", "xyzz_add_quad",
       "sat_mul", "sat_dot2", "sat_dot3", "sat_add", "sat_sub", "sat_neg", "sat_inv"]
OP_ID = {n: i for i, n in enumerate(OPS)}
FIELD_OPS = OPS[:OPS.index("xyzz_dbl")]
GROUP_OPS = OPS[OPS.index("xyzz_dbl"):OPS.index("sat_mul")]
SAT_OPS = OPS[OPS.index("sat_mul"):]
QUAD_OPS = ("xyzz_dbl_quad", "xyzz_add_quad")  # every case replicated over an aligned quad of lanes
_SPLIT = re.compile(r"^(mul_sub_k|sqr_sub_bcc_k|mul_sub_mul_k|sub_k|sub_bcc_k|is_zero_mod|canon)(\d+)$")


def split_op(op):
    m = _SPLIT.match(op)
    return (m.group(1), int(m.group(2))) if m else (op, 0)


@dataclass(frozen=True)
class Pack:
    name: str          # the struct in csrc/fpu.h / fp.h
    pid: int           # pack id of field_probe.hip
    p: int
    L: int             # register limbs
    B: int             # bits per limb
    W: int             # 32-bit words in memory
    unsat: bool
    curve: Optional[o.Curve] = None  # the curve this is the base field of (group-law layer)
    other: Optional[int] = None      # pack id of the same field with CHAIN flipped
    dots: bool = False               # fp_mul_gfx950.h generates fe_dot2 / fe_dot3 for it

    @property
    def two_torsion(self):  # the curve has even order: csrc/fp.h specialises HasTwoTorsion for this pack
        return self.curve is not None and self.curve.name in SMALL_ORDER

    @property
    def Rp(self):  # the radix the registers compute in: R' = 2^(B L)
        return 1 << (self.B * self.L)

    @property
    def R(self):   # the C ABI's radix
        return 1 << (32 * self.W)

    @property
    def M(self):
        return (1 << self.B) - 1

    @property
    def top_shift(self):
        return self.B * (self.L - 1)

    @property
    def ninv(self):
        return (-pow(self.p, -1, 1 << self.B)) % (1 << self.B)

    @property
    def one(self):
        return self.Rp % self.p

    @property
    def k_import(self):  # mont_mul(x R, k) = x R'
        return self.Rp * self.Rp * pow(self.R, -1, self.p) % self.p

    @property
    def k_export(self):  # mont_mul(x R', k) = x R
        return self.R % self.p

    def limbs(self, v):
        """v as limbs 0..L-2 of B bits and the rest in the top limb"""
        assert v >= 0
        out = [(v >> (self.B * i)) & self.M for i in range(self.L - 1)] + [v >> self.top_shift]
        assert out[-1] < (1 << 32), "does not fit the registers"
        return out

    def value(self, limbs):
        return sum(int(x) << (self.B * i) for i, x in enumerate(limbs))

    def is_tight(self, limbs):
        return len(limbs) == self.L and all(0 <= x <= self.M for x in limbs)

    def is_lazy(self, limbs):
        return len(limbs) == self.L and all(0 <= x < (1 << (self.B + 1)) for x in limbs)

    def to_m(self, x):
        return x * self.Rp % self.p

    def from_m(self, v):
        return v * pow(self.Rp, -1, self.p) % self.p

    def kp_bp(self, K, S):
        """UKpBp<K, S>: K p in the redundant form whose limbs 0..L-2 are >= S (2^B - 1)"""
        t = self.limbs(K * self.p)
        return [t[0] + (S << self.B)] + [x + (S << self.B) - S for x in t[1:-1]] + [t[-1] - S]

    def neg_lazy_limbs(self, y):
        """the limbs of u_neg_lazy(y) = u_kp_minus_lazy<2>(y): 2p - y, lazy"""
        return [c - x for c, x in zip(self.kp_bp(2, 1), self.limbs(y))]

    def sub_limit(self, K):
        """the largest y whose K p - y can be formed limb-wise without a carry pass"""
        return K * self.p - (1 << self.top_shift) - 1


def _unsat(name, pid, curve, other=None):
    L, B, W = (9, 29, 8) if curve.p.bit_length() <= 256 else (14, 28, 12)
    return Pack(name, pid, curve.p, L, B, W, True, curve, other)


def _sat(name, pid, m, dots=False):
    W = 8 if m.bit_length() <= 256 else 12
    return Pack(name, pid, m, W, 32, W, False, None, None, dots)


# the small-order points of the curves of even order: T of order 2 (y = 0), S of order 6 (3 S = T), U of order 3 with x = 0
SMALL_ORDER = {"bls12_377_g1": {"T": (h.BLS12_377_P - 1, 0), "S": (2, 3), "U": (0, 1)}}

UNSAT_PACKS = [_unsat("PallasFqU", 0, o.PALLAS, 5), _unsat("Bls12381FqU", 1, o.BLS12_381_G1), _unsat("VestaFqU", 2, h.VESTA, 6),
               _unsat("Bn254FqU", 3, h.BN254, 7), _unsat("GrumpkinFqU", 4, h.GRUMPKIN, 8),
               _unsat("Bls12377FqU", 9, h.BLS12_377, 20)]
SAT_PACKS = [_sat("PallasFq", 10, o.PALLAS.p), _sat("PallasFr", 11, o.PALLAS.r, True), _sat("Bls12381Fq", 12, o.BLS12_381_G1.p),
             _sat("Bls12381Fr", 13, o.BLS12_381_G1.r, True), _sat("VestaFq", 14, h.VESTA.p), _sat("VestaFr", 15, h.VESTA.r),
             _sat("Bn254Fq", 16, h.BN254.p), _sat("Bn254Fr", 17, h.BN254.r, True), _sat("GrumpkinFq", 18, h.GRUMPKIN.p),
             _sat("GrumpkinFr", 19, h.GRUMPKIN.r, True), _sat("Bls12377Fq", 21, h.BLS12_377.p), _sat("Bls12377Fr", 22, h.BLS12_377.r, True)]


@dataclass
class Want:
    form: str                      # 'tight' | 'lazy' | 'bool' | 'words'
    exact: Optional[int] = None    # the integer value where the contract is exact
    residue: Optional[int] = None  # else the residue class ...
    below: Optional[int] = None    # ... and the bound as a fraction over R': value * R' < below


# ------------------------------------------------------------------------------------------------------------------
# Field layer: Needs and Gives, from the comments of csrc/fpu.h and fp.h
# ------------------------------------------------------------------------------------------------------------------
def field_contract(pk, op, ins):
    """-> (needs_hold, Want) for one case; ins are raw limb lists"""
    base, K = split_op(op)
    p, Rp = pk.p, pk.Rp
    T, Z = pk.is_tight, pk.is_lazy
    inv = pow(Rp, -1, p)
    if base == "from_words":
        w = ins[0]
        ok = len(w) == pk.W and all(0 <= x < (1 << 32) for x in w)
        return ok, Want("tight", exact=sum(x << (32 * i) for i, x in enumerate(w)))
    v = [pk.value(a) for a in ins]
    edge = pk.sub_limit(K)
    if base == "mul":  # one operand may be lazy; the result is tight only if its bound p + a b / R' fits the registers
        a, b = ins
        prod = v[0] * v[1]
        ok = ((Z(a) and T(b)) or (T(a) and Z(b))) and p * Rp + prod <= Rp * Rp
        return ok, Want("tight", residue=prod * inv % p, below=p * Rp + prod)
    if base == "sqr":
        ok = T(ins[0]) and p * Rp + v[0] * v[0] <= Rp * Rp
        return ok, Want("tight", residue=v[0] * v[0] * inv % p, below=p * Rp + v[0] * v[0])
    if base == "mul_sub_k":  # a b / R' + (K p - c): the subtrahend rides in the upper columns
        a, b, c = ins
        prod = v[0] * v[1]
        ok = ((Z(a) and T(b)) or (T(a) and Z(b))) and T(c) and v[2] <= edge and (p + K * p) * Rp + prod <= Rp * Rp
        return ok, Want("tight", residue=(prod * inv - v[2]) % p, below=(p + K * p - v[2]) * Rp + prod)
    if base == "sqr_sub_bcc_k":  # a^2 / R' + (K p - b - 2c)
        s = v[1] + 2 * v[2]
        ok = all(T(x) for x in ins) and s <= edge and (p + K * p) * Rp + v[0] * v[0] <= Rp * Rp
        return ok, Want("tight", residue=(v[0] * v[0] * inv - s) % p, below=(p + K * p - s) * Rp + v[0] * v[0])
    if base == "mul_sub_mul_k":  # (a b + (K p - c) d) / R' with one reduction; a and K p - c are the lazy operands
        a, b, c, d = ins
        total = v[0] * v[1] + (K * p - v[2]) * v[3]
        ok = Z(a) and T(b) and T(c) and T(d) and v[2] <= edge and p * Rp + total <= Rp * Rp
        return ok, Want("tight", residue=(v[0] * v[1] - v[2] * v[3]) * inv % p, below=p * Rp + total)
    if base == "sub_k":
        r = v[0] - v[1] + K * p
        return T(ins[0]) and T(ins[1]) and v[1] < K * p and r < Rp, Want("tight", exact=r)
    if base == "sub_bcc_k":
        r = v[0] - v[1] - 2 * v[2] + K * p
        return all(T(x) for x in ins) and v[1] + 2 * v[2] < K * p and r < Rp, Want("tight", exact=r)
    if base in ("dbl", "triple"):
        r = v[0] * (2 if base == "dbl" else 3)
        return T(ins[0]) and r < Rp, Want("tight", exact=r)
    if base == "neg_lazy":
        return T(ins[0]) and v[0] < p, Want("lazy", exact=2 * p - v[0])
    if base == "neg_lazy_tight":
        return T(ins[0]) and v[0] < p, Want("tight", exact=2 * p - v[0])
    if base == "is_zero_mod":
        return T(ins[0]) and v[0] < K * p, Want("bool", exact=int(v[0] % p == 0))
    if base == "canon":
        return T(ins[0]) and v[0] < K * p, Want("tight", exact=v[0] % p)
    if base == "import":  # any W-word value in; below 2p and congruent to a R' / R out
        t = v[0] * pk.k_import
        return T(ins[0]) and v[0] < pk.R, Want("tight", residue=t * inv % p, below=min(p * Rp + t, 2 * p * Rp))
    if base == "export":  # tight, below 8p in; the canonical a R / R' out
        return T(ins[0]) and v[0] < 8 * p, Want("tight", exact=v[0] * pk.k_export * inv % p)
    if base == "store":   # tight, below 8p in; canonical packed words out
        return T(ins[0]) and v[0] < 8 * p, Want("words", exact=v[0] % p)
    raise KeyError(op)


def check_field(pk, want, slot):
    """slot: the STRIDE words of result slot 0 -> None, or what is wrong"""
    if want.form == "bool":
        return None if slot[0] == want.exact else f"predicate gave {slot[0]}, expected {want.exact}"
    if want.form == "words":
        got = sum(int(x) << (32 * i) for i, x in enumerate(slot[:pk.W]))
        return None if got == want.exact else f"stored {got:#x}, expected the canonical {want.exact:#x}"
    limbs = [int(x) for x in slot[:pk.L]]
    width = pk.B + (1 if want.form == "lazy" else 0)
    if any(x >> width for x in limbs):
        return f"limbs wider than {width} bits: {[hex(x) for x in limbs]}"
    got = pk.value(limbs)
    if want.exact is not None:
        return None if got == want.exact else f"value {got:#x}, expected exactly {want.exact:#x}"
    if got % pk.p != want.residue:
        return f"value {got:#x} is not congruent to {want.residue:#x}"
    if got * pk.Rp >= want.below:
        return f"value {got:#x} = {got / pk.p:.3f} p leaves its bound {want.below / pk.Rp / pk.p:.3f} p"
    return None


# ------------------------------------------------------------------------------------------------------------------
# Value classes
# ------------------------------------------------------------------------------------------------------------------
def clip_top(pk, limbs, vmax):
    """the limb vector with its top limb lowered until the value is <= vmax (None if the low limbs alone exceed it)"""
    low = pk.value(limbs[:-1])
    if low > vmax:
        return None
    return list(limbs[:-1]) + [min(limbs[-1], (vmax - low) >> pk.top_shift)]


def tight_classes(pk, vmax, rng, all_limbs=False):
    """named tight operands with value <= vmax: the value classes of the probe, clipped to what the caller's Needs admit"""
    p = pk.p
    tiny = 1 << pk.top_shift
    out = {}
    for name, v in (("0", 0), ("1", 1), ("p-1", p - 1), ("p", p), ("p+1", p + 1), ("max", vmax), ("tiny_max", tiny - 1),
                    ("tiny_rand", rng.randrange(tiny)), ("rand", rng.randrange(vmax + 1)), ("rand_c", rng.randrange(min(vmax, p - 1) + 1))):
        if 0 <= v <= vmax:
            out[name] = pk.limbs(v)
    ones = clip_top(pk, [pk.M] * pk.L, vmax)
    if ones is not None:
        out["ones"] = ones
    for i in (range(pk.L) if all_limbs else (1, pk.L // 2, pk.L - 1)):
        if (1 << (pk.B * i)) <= vmax:
            out[f"limb{i}"] = pk.limbs(1 << (pk.B * i))
    return out


def lazy_classes(pk, rng):
    """operands only a multiplication may take: limbs below 2^(B+1)"""
    wide = (1 << (pk.B + 1)) - 1
    return {"lazy_ones": [wide] * pk.L,
            "lazy_rand": [rng.randrange(wide + 1) for _ in range(pk.L)],
            "lazy_neg_tiny": pk.neg_lazy_limbs(rng.randrange(1 << pk.top_shift)),
            "lazy_neg_0": pk.neg_lazy_limbs(0)}


def _b_max(pk, a_val, reserve):
    """the largest tight b with p + a b / R' + reserve <= R'"""
    budget = (pk.Rp - pk.p - reserve) * pk.Rp
    return pk.Rp - 1 if a_val == 0 else min(pk.Rp - 1, budget // a_val)


def _with_largest_partner(pk, a, reserve):
    """a against the largest value, and the largest all-ones limb pattern, that the product bound admits"""
    bm = _b_max(pk, pk.value(a), reserve)
    out = [("bmax", pk.limbs(bm))]
    ones = clip_top(pk, [pk.M] * pk.L, bm)
    if ones is not None:
        out.append(("ones_clipped", ones))
    return out


def ab_pairs(pk, reserve, rng):
    """a dozen (a, b) products for the functions that take a product and more: tight and lazy, m_k at 0 and at 2^B - 1, the
    largest products the bound admits"""
    tc, lc = tight_classes(pk, pk.Rp - 1, rng), lazy_classes(pk, rng)
    pairs = [("1*1", tc["1"], tc["1"]), ("p-1*p-1", tc["p-1"], tc["p-1"]), ("p*1:m_k=2^B-1", tc["p"], tc["1"]),
             ("0*rand:m_k=0", tc["0"], tc["rand"]), ("rand*rand_c", tc["rand_c"], tc["rand_c"]),
             (f"limb{pk.L // 2}*ones_clipped", tc[f"limb{pk.L // 2}"], _with_largest_partner(pk, tc[f"limb{pk.L // 2}"], reserve)[-1][1]),
             ("lazy_rand*rand_c", lc["lazy_rand"], tc["rand_c"]), ("lazy_neg_tiny*rand_c", lc["lazy_neg_tiny"], tc["rand_c"])]
    for name in ("lazy_ones", "lazy_rand"):
        for pn, partner in _with_largest_partner(pk, lc[name], reserve):
            pairs.append((f"{name}*{pn}", lc[name], partner))
    for pn, partner in _with_largest_partner(pk, tc["ones"], reserve):
        pairs.append((f"ones*{pn}", tc["ones"], partner))
    pairs.append(("tiny_max*bmax", tc["tiny_max"], pk.limbs(_b_max(pk, pk.value(tc["tiny_max"]), reserve))))
    return pairs


def _bc_pairs(pk, lim, rng):
    """(b, c) with b + 2c up to lim and down to 0"""
    p, tiny = pk.p, 1 << pk.top_shift
    c_r = rng.randrange(lim // 2 + 1)
    vals = [(0, 0), (lim, 0), (lim & 1, lim // 2), (lim - 2 * c_r, c_r), (1, 1), (p - 1, (lim - p + 1) // 2), (tiny - 1, tiny - 1),
            (rng.randrange(lim // 3), rng.randrange(lim // 3)), (p, p), (p + 1, p - 1)]
    out = [(f"b={b:#x},c={c:#x}"[:60], pk.limbs(b), pk.limbs(c)) for b, c in vals if b >= 0 and c >= 0 and b + 2 * c <= lim]
    ob = clip_top(pk, [pk.M] * pk.L, lim)
    oc = clip_top(pk, [pk.M] * pk.L, lim // 2)
    out.append(("b=ones,c=0", ob, pk.limbs(0)))
    out.append(("b=rest,c=ones", pk.limbs(lim - 2 * pk.value(oc)), oc))
    return out


def reduction_multipliers(pk, a, b):
    """the limbs m_0 .. m_(L-1) the Montgomery reduction of a b multiplies p by: the one m < R' with a b + m p = 0 mod R'"""
    return pk.limbs((-pk.value(a) * pk.value(b) * pow(pk.p, -1, pk.Rp)) % pk.Rp)


def chosen_m_patterns(pk):
    """named multiplier patterns for the reduction, column by column: alternating 0 / 2^B - 1 from either start, a single 1 and a
    single 2^B - 1 in each column, all ones, one random pattern (its own seed: the streams of the older cases stay as they were)"""
    L, M = pk.L, pk.M
    rng = random.Random(f"chosen_m:{pk.name}")
    pats = [("alt:0,M", [M * (i & 1) for i in range(L)]), ("alt:M,0", [M * (1 - (i & 1)) for i in range(L)])]
    pats += [(f"one@{k}", [int(i == k) for i in range(L)]) for k in range(L)]
    pats += [(f"M@{k}", [M * int(i == k) for i in range(L)]) for k in range(L)]
    pats += [("all:1", [1] * L), ("rand", [rng.randrange(M + 1) for _ in range(L)])]
    return pats


def chosen_m_cases(pk):
    """(tag, [a, 1]) with a = -m p mod R': a is tight, a * 1 is inside the Needs of the multiplication, and the reduction's
    multipliers are exactly the limbs of m"""
    one = pk.limbs(1)
    out = []
    for tag, m in chosen_m_patterns(pk):
        a = pk.limbs((-pk.value(m) * pk.p) % pk.Rp)
        assert pk.is_tight(a) and reduction_multipliers(pk, a, one) == m
        out.append((f"m={tag}", [a, one]))
    return out


def _kp_plus(pk, KMAX, rs):
    return [(f"{k}p+{r:#x}"[:40], pk.limbs(k * pk.p + r)) for k in range(KMAX) for r in rs]


@functools.lru_cache(maxsize=None)
def field_cases(pid, op):
    """[(tag, ins)] for one unsaturated pack and one field operation: every case within the Needs, at most MAX_CASES"""
    pk = PACK_BY_ID[pid]
    rng = random.Random(f"field:{pk.name}:{op}")
    base, K = split_op(op)
    p, Rp = pk.p, pk.Rp
    cand = []
    if base == "mul":
        tc, lc = tight_classes(pk, Rp - 1, rng), lazy_classes(pk, rng)
        for an, a in tc.items():
            for bn, b in tc.items():
                cand.append((f"{an}*{bn}", [a, b]))
        for zn, z in lc.items():
            for bn, b in tc.items():
                cand += [(f"{zn}*{bn}", [z, b]), (f"{bn}*{zn}", [b, z])]
        for i in range(pk.L):
            for xn in ("1", "rand_c", "p-1"):
                cand += [(f"limb{i}*{xn}", [pk.limbs(1 << (pk.B * i)), tc[xn]]), (f"{xn}*limb{i}", [tc[xn], pk.limbs(1 << (pk.B * i))])]
        for an, a in list(tc.items()) + list(lc.items()):
            for pn, b in _with_largest_partner(pk, a, 0):
                cand += [(f"{an}*{pn}", [a, b]), (f"{pn}*{an}", [b, a])]
        cand += chosen_m_cases(pk)  # appended: the cases before them are what they were
    elif base == "sqr":
        for an, a in tight_classes(pk, math.isqrt((Rp - p) * Rp), rng, all_limbs=True).items():
            cand.append((an, [a]))
        cand += [(f"rand{i}", [pk.limbs(rng.randrange(p))]) for i in range(8)]
    elif base == "mul_sub_k":
        cs = tight_classes(pk, pk.sub_limit(K), rng)
        cs["(K-1)p"] = pk.limbs((K - 1) * p)
        for pn, a, b in ab_pairs(pk, K * p, rng):
            for cn, c in cs.items():
                cand.append((f"{pn}-{cn}", [a, b, c]))
                if pk.is_lazy(a) and not pk.is_tight(a) and cn in ("max", "0", "ones"):
                    cand.append((f"swapped:{pn}-{cn}", [b, a, c]))
    elif base == "sqr_sub_bcc_k":
        ac = tight_classes(pk, math.isqrt((Rp - p - K * p) * Rp), rng)
        for an in ("0", "1", "p-1", "max", "ones", "rand", "tiny_max", f"limb{pk.L // 2}"):
            for bcn, b, c in _bc_pairs(pk, pk.sub_limit(K), rng):
                cand.append((f"{an}^2-{bcn}", [ac.get(an), b, c]))
    elif base == "mul_sub_mul_k":
        cs = tight_classes(pk, pk.sub_limit(K), rng)
        ds = tight_classes(pk, Rp - 1, rng)
        for pn, a, b in ab_pairs(pk, K * p, rng):
            if not pk.is_tight(b):
                continue
            for cn in ("0", "1", "p-1", "p", "max", "ones", "tiny_max", "rand"):
                if cn not in cs:
                    continue
                for dn in ("0", "1", "ones", "rand", "max"):
                    cand.append((f"{pn}-{cn}*{dn}", [a, b, cs[cn], ds[dn]]))
    elif base == "sub_k":
        bs = tight_classes(pk, K * p - 1, rng)
        for an, a in tight_classes(pk, Rp - 1 - K * p, rng).items():
            for bn, b in bs.items():
                cand.append((f"{an}-{bn}", [a, b]))
        for bn, b in bs.items():  # the largest a: the result is 2^(B L) - 1
            cand.append((f"top-{bn}", [pk.limbs(Rp - 1 - K * p + pk.value(b)), b]))
    elif base == "sub_bcc_k":
        ac = tight_classes(pk, Rp - 1 - K * p, rng)
        for bcn, b, c in _bc_pairs(pk, K * p - 1, rng):
            for an in ("0", "1", "p-1", "max", "ones", "rand", "tiny_max"):
                cand.append((f"{an}-{bcn}", [ac.get(an), b, c]))
            cand.append((f"top-{bcn}", [pk.limbs(Rp - 1 - K * p + pk.value(b) + 2 * pk.value(c)), b, c]))
    elif base in ("dbl", "triple"):
        for an, a in tight_classes(pk, (Rp - 1) // (2 if base == "dbl" else 3), rng, all_limbs=True).items():
            cand.append((an, [a]))
    elif base in ("neg_lazy", "neg_lazy_tight"):
        for an, a in tight_classes(pk, p - 1, rng, all_limbs=True).items():
            cand.append((an, [a]))
        cand += [(f"rand{i}", [pk.limbs(rng.randrange(p))]) for i in range(8)]
    elif base == "is_zero_mod":
        for k in range(K):
            cand.append((f"{k}p", [pk.limbs(k * p)]))
            for d in (1, -1):
                if 0 <= k * p + d:
                    cand.append((f"{k}p{d:+d}", [pk.limbs(k * p + d)]))
            for j in (1, 2, pk.M, rng.randrange(1, 1 << (pk.top_shift - pk.B))):  # the same low limb, not zero
                if k * p + (j << pk.B) < K * p:
                    cand.append((f"{k}p+{j:#x}*2^B"[:40], [pk.limbs(k * p + (j << pk.B))]))
        cand += [(f"rand{i}", [pk.limbs(rng.randrange(K * p))]) for i in range(32)]
        cand.append(("ones", [clip_top(pk, [pk.M] * pk.L, K * p - 1)]))
    elif base == "canon":
        cand += [(t, [a]) for t, a in _kp_plus(pk, K, (0, 1, p - 1, rng.randrange(p), rng.randrange(1 << pk.top_shift)))]
        cand.append(("ones", [clip_top(pk, [pk.M] * pk.L, K * p - 1)]))
    elif base == "import":
        for an, a in tight_classes(pk, pk.R - 1, rng, all_limbs=True).items():
            cand.append((an, [a]))
        cand += [(f"rand{i}", [pk.limbs(rng.randrange(pk.R))]) for i in range(16)]
    elif base in ("export", "store"):
        for an, a in tight_classes(pk, 8 * p - 1, rng, all_limbs=True).items():
            cand.append((an, [a]))
        cand += [(t, [a]) for t, a in _kp_plus(pk, 8, (0, 1, p - 1, rng.randrange(p)))]
    elif base == "from_words":
        ones = (1 << 32) - 1
        cand += [("all_ones", [[ones] * pk.W]), ("zero", [[0] * pk.W]), ("alternating", [[0xAAAAAAAA, 0x55555555] * (pk.W // 2)])]
        cand += [(f"word{i}", [[ones if j == i else 0 for j in range(pk.W)]]) for i in range(pk.W)]
        cand += [(f"bit{32 * i + 31}", [[(1 << 31) if j == i else 0 for j in range(pk.W)]]) for i in range(pk.W)]
        cand += [(f"rand{i}", [[rng.randrange(1 << 32) for _ in range(pk.W)]]) for i in range(16)]
    else:
        raise KeyError(op)
    out, seen = [], set()
    for tag, ins in cand:
        if any(x is None for x in ins):
            continue
        key = tuple(tuple(x) for x in ins)
        if key in seen or not field_contract(pk, op, ins)[0]:
            continue
        seen.add(key)
        out.append((tag, ins))
    assert 0 < len(out) <= MAX_CASES, (pk.name, op, len(out))
    return out


# ------------------------------------------------------------------------------------------------------------------
# Saturated layer (csrc/fp.h, fp_mul_gfx950.h): canonical values in, canonical values out, everything exact
# ------------------------------------------------------------------------------------------------------------------
def sat_classes(pk, rng):
    m = pk.p
    out = {"0": 0, "1": 1, "m-1": m - 1, "m-2": m - 2, "R": pk.R % m}
    top = m >> (32 * (pk.W - 1))
    if top:  # the largest canonical value whose lower limbs are all-ones
        out["ones"] = ((top - 1) << (32 * (pk.W - 1))) | ((1 << (32 * (pk.W - 1))) - 1)
    for i in range(4):
        out[f"rand{i}"] = rng.randrange(m)
    assert all(v < m for v in out.values())
    return out


def sat_expected(pk, op, vals):
    m, Ri = pk.p, pow(pk.R, -1, pk.p)
    if op == "sat_mul":
        return vals[0] * vals[1] * Ri % m
    if op in ("sat_dot2", "sat_dot3"):
        return sum(vals[2 * i] * vals[2 * i + 1] for i in range(len(vals) // 2)) * Ri % m
    if op == "sat_add":
        return (vals[0] + vals[1]) % m
    if op == "sat_sub":
        return (vals[0] - vals[1]) % m
    if op == "sat_neg":
        return (-vals[0]) % m
    if op == "sat_inv":  # Montgomery forms: (x R)^-1 R^2 = x^-1 R; fe_inv(0) = 0
        return pow(vals[0], -1, m) * pk.R * pk.R % m if vals[0] else 0
    raise KeyError(op)


@functools.lru_cache(maxsize=None)
def sat_cases(pid, op):
    """[(tag, values)]: canonical integers (the limbs are pk.limbs(value))"""
    pk = PACK_BY_ID[pid]
    rng = random.Random(f"sat:{pk.name}:{op}")
    sc = sat_classes(pk, rng)
    # products whose canonical results sit at m - 1, so that the unreduced sums of fe_dot2 / fe_dot3 are 2m - 2 and 3m - 3
    prods = [("m-1*R", sc["m-1"], sc["R"]), ("R*m-1", sc["R"], sc["m-1"]), ("m-1*m-1", sc["m-1"], sc["m-1"]), ("0*rand", 0, sc["rand0"]),
             ("ones*ones", sc.get("ones", 1), sc.get("ones", 1)), ("rand*rand", sc["rand1"], sc["rand2"]), ("1*m-2", 1, sc["m-2"]),
             ("m-2*R", sc["m-2"], sc["R"])]
    if op in ("sat_mul", "sat_add", "sat_sub"):
        out = [(f"{an},{bn}", (a, b)) for an, a in sc.items() for bn, b in sc.items()]
    elif op in ("sat_neg", "sat_inv"):
        out = [(an, (a,)) for an, a in sc.items()]
    elif op == "sat_dot2":
        out = [(f"{x[0]}+{y[0]}", (x[1], x[2], y[1], y[2])) for x in prods for y in prods]
    elif op == "sat_dot3":
        ps = prods[:6]
        out = [(f"{x[0]}+{y[0]}+{z[0]}", (x[1], x[2], y[1], y[2], z[1], z[2])) for x in ps for y in ps for z in ps]
    else:
        raise KeyError(op)
    assert 0 < len(out) <= MAX_CASES
    return out


# ------------------------------------------------------------------------------------------------------------------
# Group-law layer (csrc/ec.h): real curve points, every coordinate lifted to the smallest, the largest and a random
# representative under the invariant of its representation
# ------------------------------------------------------------------------------------------------------------------
XYZZ_BOUND = (8, 3, 2, 2)   # X < 8p, Y < 3p, ZZ, ZZZ < 2p
JAC_BOUND = (12, 13, 3)     # X < 12p, Y < 13p, Z < 3p
MODES = ("min", "max", "rand")


def _fixture_points(curve):
    name = {"pallas": "adversarial_points.json", "bls12_381_g1": "adversarial_points.json", "vesta": "adversarial_points.json",
            "bn254_g1": "bn254_adversarial_points.json", "grumpkin": "grumpkin_adversarial_points.json",
            "bls12_377_g1": "bls12_377_adversarial_points.json"}[curve.name]
    fx = json.load(open(os.path.join(HERE, "golden", name)))
    kinds = {k: [(int(x, 16), int(y, 16)) for x, y in v] for k, v in fx["curves"][curve.name].items()}
    if "negated_doubling_pair" in fx:
        kinds["negated_doubling_pair"] = [tuple(int(v, 16) for v in fx["negated_doubling_pair"][k]) for k in ("l", "r")]
    return kinds


@functools.lru_cache(maxsize=None)
def probe_points(pid):
    """-> (points, tiny): a dozen points of the curve -- the fixtures' tiny-y and near-p entries first -- and those among them and
    their negatives whose y, in the internal radix, is below 2^(B (L - 1)) (the class the K = 2 top-limb borrow needed)"""
    pk = PACK_BY_ID[pid]
    c = pk.curve
    kinds = _fixture_points(c)
    everything = [P for pts in kinds.values() for P in pts]
    assert all(o.is_on_curve(c, P) for P in everything)
    lim = 1 << pk.top_shift
    tiny = []
    for P in everything:
        for Q in (P, o.neg(c, P)):
            if pk.to_m(Q[1]) < lim and Q not in tiny:
                tiny.append(Q)
    pts = tiny[:3] + [o.neg(c, P) for P in tiny[:2]]
    for k, v in kinds.items():  # one point of every kind
        if v[0] not in pts and len(pts) < 11:
            pts.append(v[0])
    g = o.generator(c)
    pts += [g, o.mul(c, 0xABCDEF, g)]
    return pts, tiny


def lift(pk, v, bound, mode, rng):
    """v canonical -> the smallest, the largest or a random representative below bound * p"""
    k = {"min": 0, "max": bound - 1, "rand": rng.randrange(bound)}[mode]
    return pk.limbs(v + k * pk.p)


def xyzz_rep(pk, A, mode, rng):
    if A is None:
        return [[0] * pk.L] * 4
    p = pk.p
    z = rng.randrange(1, p)
    vals = (A[0] * z * z % p, A[1] * z * z * z % p, z * z % p, z * z * z % p)
    return [lift(pk, pk.to_m(v), b, mode, rng) for v, b in zip(vals, XYZZ_BOUND)]


def jac_rep(pk, A, mode, rng):
    if A is None:
        return [[0] * pk.L] * 3
    p = pk.p
    z = rng.randrange(1, p)
    vals = (A[0] * z * z % p, A[1] * z * z * z % p, z)
    return [lift(pk, pk.to_m(v), b, mode, rng) for v, b in zip(vals, JAC_BOUND)]


def affine_rep(pk, Q, lazy):
    """q of xyzz_madd / jac_madd: x canonical; y plain, or the lazily negated limbs (2p - (-y)) that affine_neg_if hands over"""
    if Q is None:
        return [[0] * pk.L] * 2
    y = pk.to_m(Q[1])
    return [pk.limbs(pk.to_m(Q[0])), pk.neg_lazy_limbs(pk.p - y) if lazy else pk.limbs(y)]


def _under(pk, limbs, bounds):
    return all(pk.is_tight(a) and pk.value(a) < b * pk.p for a, b in zip(limbs, bounds))


def group_needs(pk, op, ins):
    """the register invariants and operand forms ec.h states for the inputs"""
    def q_ok(x, y):
        return pk.is_tight(x) and pk.value(x) < pk.p and ((pk.is_tight(y) and pk.value(y) < pk.p) or (pk.is_lazy(y) and pk.value(y) <= 2 * pk.p))
    if op in ("xyzz_dbl", "xyzz_dbl_quad"):
        return _under(pk, ins[0:4], XYZZ_BOUND)
    if op == "xyzz_dbl_affine":
        return pk.is_tight(ins[0]) and pk.value(ins[0]) < 2 * pk.p and pk.is_tight(ins[1]) and pk.value(ins[1]) <= 2 * pk.p
    if op == "xyzz_madd":
        return _under(pk, ins[0:4], XYZZ_BOUND) and q_ok(ins[4], ins[5])
    if op in ("xyzz_add", "xyzz_add_quad"):
        return _under(pk, ins[0:4], XYZZ_BOUND) and _under(pk, ins[4:8], XYZZ_BOUND)
    if op == "affine_neg_if":
        return _under(pk, ins[0:2], (1, 1)) and ins[2][0] in (0, 1)
    if op in ("jac_dbl", "xyzz_from_jac"):
        return _under(pk, ins[0:3], JAC_BOUND)
    if op == "jac_madd":
        return _under(pk, ins[0:3], JAC_BOUND) and q_ok(ins[4], ins[5])
    raise KeyError(op)


def _pairs(pk):
    """(tag, acc, q) over the probe points: generic, q = acc, q = -acc, acc infinite, q infinite, the doubling of a negated tiny-y
    point among the q = acc"""
    c = pk.curve
    pts, tiny = probe_points(pk.pid)
    n = len(pts)
    out = [("generic", pts[i], pts[(i + 3) % n]) for i in range(n)]
    out += [("q=acc", P, P) for P in pts]
    out += [("q=acc:negated_tiny_y", o.neg(c, P), o.neg(c, P)) for P in tiny[:4] if o.neg(c, P) not in pts]
    out += [("q=-acc", P, o.neg(c, P)) for P in pts[:7]]
    out += [("acc=inf", None, P) for P in (pts[0], pts[3], pts[-1])]
    out += [("q=inf", P, None) for P in (pts[0], pts[-1])] + [("both=inf", None, None)]
    return out


@functools.lru_cache(maxsize=None)
def small_order_points(pid):
    """-> {T, S, U, 2S} for a pack whose curve has even order, each checked to be on the curve and of the order claimed"""
    pk = PACK_BY_ID[pid]
    c = pk.curve
    pts = dict(SMALL_ORDER[c.name])
    for name, order in (("T", 2), ("S", 6), ("U", 3)):
        P = pts[name]
        assert o.is_on_curve(c, P) and o.mul(c, order, P) is None and all(o.mul(c, d, P) is not None for d in range(1, order)), name
    assert pts["T"][1] == 0 and pts["U"][0] == 0 and o.mul(c, 3, pts["S"]) == pts["T"]
    pts["2S"] = o.mul(c, 2, pts["S"])
    assert o.is_on_curve(c, pts["2S"]) and o.mul(c, 3, pts["2S"]) is None and pts["2S"] is not None  # (on BLS12-377 it is U itself)
    return pts


def _with_y(limbs, pk, ky):
    """a representation of T = (x, 0) with its second coordinate rewritten as ky p"""
    return [limbs[0], pk.limbs(ky * pk.p)] + list(limbs[2:])


def _two_torsion_cases(pk, op):
    """[(tag, ins, expected)] for a pack whose curve has even order: the point T of order 2 with Y (or y) written as every multiple
    of p that the operand's invariant admits -- the representatives the HasTwoTorsion guards of csrc/ec.h exist for -- and the points
    of order 6 and 3 around it.  Own seed; appended to the cases every pack has."""
    c, p = pk.curve, pk.p
    so = small_order_points(pk.pid)
    T, S, U, S2 = so["T"], so["S"], so["U"], so["2S"]
    rng = random.Random(f"two_torsion:{pk.name}:{op}")
    zero = [0] * pk.L
    quad = op in QUAD_OPS
    out = []
    if op in ("xyzz_dbl", "xyzz_dbl_quad", "jac_dbl"):
        rep, bound = (jac_rep, JAC_BOUND[1]) if op == "jac_dbl" else (xyzz_rep, XYZZ_BOUND[1])
        for ky in range(bound):  # Y < 3p (XYZZ), Y < 13p (Jacobian)
            for mode in MODES:
                out.append((f"T:Y={ky}p:{mode}", _with_y(rep(pk, T, mode, rng), pk, ky), None))
        for tag, P in (("S", S), ("2S", S2)):
            for mode in MODES:
                out.append((f"{tag}:{mode}", rep(pk, P, mode, rng), o.add(c, P, P)))
    elif op == "xyzz_dbl_affine":  # y <= 2p is inside the stated Needs: 2p is what a lazily negated 0 would be
        x = pk.to_m(T[0])
        for kx in (0, 1):
            for ky in (0, 1, 2):
                out.append((f"T:x+{kx}p,y={ky}p", [pk.limbs(x + kx * p), pk.limbs(ky * p)], None))
    elif op in ("xyzz_madd", "jac_madd"):
        rep, bound = (xyzz_rep, XYZZ_BOUND[1]) if op == "xyzz_madd" else (jac_rep, JAC_BOUND[1])
        qx = pk.limbs(pk.to_m(T[0]))
        qys = [("y=0", zero), ("y=p:tight", pk.limbs(p)), ("y=p:lazy", pk.kp_bp(1, 1)), ("y=2p:tight", pk.limbs(2 * p)),
               ("y=2p:lazy", pk.kp_bp(2, 1))]

        def case(tag, acc, qy, want):
            out.append((tag, acc + [zero] * (4 - len(acc)) + [qx, qy], want))
        for ky in range(bound):
            for qi, (qn, qy) in enumerate(qys):
                for mode in (MODES if ky < 3 else (MODES[(ky + qi) % 3],)):
                    case(f"q=acc=T:Y={ky}p:{mode}:{qn}", _with_y(rep(pk, T, mode, rng), pk, ky), qy, None)
        for qn, qy in qys:
            for mode in MODES:  # T reached as 3 S, in whatever representative the lift gives Y
                case(f"acc=3S,q=T:{mode}:{qn}", rep(pk, o.mul(c, 3, S), mode, rng), qy, None)
                case(f"acc=S,q=T:{mode}:{qn}", rep(pk, S, mode, rng), qy, o.add(c, S, T))
            case(f"acc=inf,q=T:{qn}", rep(pk, None, "min", rng), qy, T)
    elif op in ("xyzz_add", "xyzz_add_quad"):
        n = 0
        for k1 in range(XYZZ_BOUND[1]):
            for k2 in range(XYZZ_BOUND[1]):
                for mode in ((MODES[n % 3],) if quad else MODES):
                    ins = _with_y(xyzz_rep(pk, T, mode, rng), pk, k1) + _with_y(xyzz_rep(pk, T, mode, rng), pk, k2)
                    out.append((f"T+T:Y={k1}p,{k2}p:{mode}", ins, None))
                n += 1
        for tag, A, Q in (("S+2S", S, S2), ("T+U", T, U), ("U+T", U, T)):
            for mode in MODES:
                out.append((f"{tag}:{mode}", xyzz_rep(pk, A, mode, rng) + xyzz_rep(pk, Q, mode, rng), o.add(c, A, Q)))
    return out


@functools.lru_cache(maxsize=None)
def group_cases(pid, op):
    """[(tag, ins, expected)]: expected is the oracle's affine point (None = infinity), or for affine_neg_if the (x, y) values"""
    pk = PACK_BY_ID[pid]
    c = pk.curve
    rng = random.Random(f"group:{pk.name}:{op}")
    pts, tiny = probe_points(pid)
    singles = [("P", P) for P in pts] + [("negated_tiny_y", o.neg(c, P)) for P in tiny[:4] if o.neg(c, P) not in pts] + [("inf", None)]
    zero = [0] * pk.L
    out = []
    if op in ("xyzz_dbl", "xyzz_dbl_quad"):
        for tag, P in singles:
            for mode in MODES:
                for rep in range(1 if op == "xyzz_dbl_quad" else 2):
                    out.append((f"{tag}:{mode}", xyzz_rep(pk, P, mode, rng), o.add(c, P, P)))
    elif op == "xyzz_dbl_affine":  # x below 2p, y up to 2p: the negated tiny-y point arrives as 2p - y
        for tag, P in singles[:-1]:
            x, y = pk.to_m(P[0]), pk.to_m(P[1])
            for kx in (0, 1):
                for ky in (0, 1):
                    out.append((f"{tag}:x+{kx}p,y+{ky}p", [pk.limbs(x + kx * pk.p), pk.limbs(y + ky * pk.p)], o.add(c, P, P)))
    elif op in ("xyzz_madd", "jac_madd"):
        rep = xyzz_rep if op == "xyzz_madd" else jac_rep
        for tag, A, Q in _pairs(pk):
            for mode in MODES:
                for lazy in ((False, True) if Q is not None else (False,)):
                    acc = rep(pk, A, mode, rng)
                    ins = acc + [zero] * (4 - len(acc)) + affine_rep(pk, Q, lazy)
                    out.append((f"{tag}:{mode}:{'lazy' if lazy else 'plain'}", ins, o.add(c, A, Q)))
    elif op in ("xyzz_add", "xyzz_add_quad"):
        for tag, A, Q in _pairs(pk):
            for mode in MODES:
                out.append((f"{tag}:{mode}", xyzz_rep(pk, A, mode, rng) + xyzz_rep(pk, Q, mode, rng), o.add(c, A, Q)))
            if op == "xyzz_add":
                out.append((f"{tag}:max+min", xyzz_rep(pk, A, "max", rng) + xyzz_rep(pk, Q, "min", rng), o.add(c, A, Q)))
    elif op == "affine_neg_if":
        vals = [(pk.to_m(P[0]), pk.to_m(P[1])) for P in pts[:8]] + [(0, 0), (1, 0), (0, 1), (pk.p - 1, pk.p - 1)]
        for x, y in vals:
            for flag in (0, 1):
                out.append((f"flag={flag}", [pk.limbs(x), pk.limbs(y), [flag] + [0] * (pk.L - 1)], (x, 2 * pk.p - y if flag and y else y)))
    elif op in ("jac_dbl", "xyzz_from_jac"):
        for tag, P in singles:
            for mode in MODES:
                for rep in range(2):
                    out.append((f"{tag}:{mode}", jac_rep(pk, P, mode, rng), o.add(c, P, P) if op == "jac_dbl" else P))
    else:
        raise KeyError(op)
    extra = _two_torsion_cases(pk, op) if pk.two_torsion else []
    if op in QUAD_OPS:  # a quarter of the launch; the two-torsion class, where there is one, takes its room from the tail of the others
        out = out[:MAX_CASES // 4 - len(extra)]
    out += extra
    assert 0 < len(out) <= MAX_CASES, (pk.name, op, len(out))
    return out


def _decode(pk, limbs, bounds, what):
    """tight and within the invariant of the representation -> the values, or raise"""
    vals = []
    for name, a, b in zip(what, limbs, bounds):
        a = [int(x) for x in a[:pk.L]]
        if not pk.is_tight(a):
            raise AssertionError(f"{name} is not tight: {[hex(x) for x in a]}")
        v = pk.value(a)
        if v >= b * pk.p:
            raise AssertionError(f"{name} = {v / pk.p:.3f} p leaves its invariant {name} < {b} p")
        vals.append(v)
    return vals


def check_group(pk, op, ins, slots, expected):
    """slots: the N_OUT result slots of one case -> None, or what is wrong"""
    p = pk.p
    try:
        if op == "affine_neg_if":
            x = [int(v) for v in slots[0][:pk.L]]
            y = [int(v) for v in slots[1][:pk.L]]
            if x != ins[0]:
                return "x changed"
            if not pk.is_lazy(y) or pk.value(y) != expected[1]:
                return f"y = {pk.value(y):#x} (limbs {[hex(v) for v in y]}), expected {expected[1]:#x} in limbs below 2^(B+1)"
            return None
        if op in ("jac_dbl", "jac_madd"):
            X, Y, Z = _decode(pk, slots[:3], JAC_BOUND, ("X", "Y", "Z"))
            if Z == 0:
                got = None
            else:
                if Z % p == 0:
                    return "Z is a non-zero multiple of p"
                z = pk.from_m(Z)
                zi = pow(z, -1, p)
                got = (pk.from_m(X) * zi * zi % p, pk.from_m(Y) * zi * zi * zi % p)
        else:
            X, Y, ZZ, ZZZ = _decode(pk, slots[:4], XYZZ_BOUND, ("X", "Y", "ZZ", "ZZZ"))
            if ZZ == 0:
                got = None
            else:
                zz, zzz = pk.from_m(ZZ), pk.from_m(ZZZ)
                if zz == 0 or pow(zz, 3, p) != zzz * zzz % p:
                    return "ZZ^3 != ZZZ^2"
                got = (pk.from_m(X) * pow(zz, -1, p) % p, pk.from_m(Y) * pow(zzz, -1, p) % p)
    except AssertionError as e:
        return str(e)
    if got != expected:
        return f"affine image {got} differs from the oracle's {expected}"
    return None


PACK_BY_ID = {pk.pid: pk for pk in UNSAT_PACKS + SAT_PACKS}
