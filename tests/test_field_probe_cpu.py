"""The field probe without a GPU: the model's constants against the tables compiled into csrc/fpu.h, every generated case against
the Needs of its function, the probe's cross-compilation, and the two operation tables against each other."""
import os
import re

import pytest

from oracle import pyref as o
from tests import field_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPU_H = os.path.join(ROOT, "accumulation_amd", "csrc", "fpu.h")
PROBE_SRC = os.path.join(ROOT, "tests", "hip", "field_probe.hip")


def _ids(pk):
    return pk.name


@pytest.mark.parametrize("pk", fm.UNSAT_PACKS, ids=_ids)
def test_model_constants_match_the_device_tables(pk):
    """R', NINV, k_import, k_export (and p, one, the limb shape) as the model derives them from the oracle's modulus == csrc/fpu.h"""
    src = open(FPU_H).read()
    blk = src[src.index("struct " + pk.name + " {"):]
    blk = blk[:blk.index("};")]
    assert (pk.L, pk.B, pk.W) == tuple(int(re.search(rf"int {n} = (\d+);", blk).group(1)) for n in "LBW")

    def tab(t):
        vals = [int(x.strip().rstrip("u"), 16) for x in re.search(r"AMSM_TABLE\(" + t + r", \d+, ([^)]*)\)", blk, re.S).group(1).split(",")]
        assert len(vals) == pk.L and all(v <= pk.M for v in vals)
        return pk.value(vals)

    assert pk.p == pk.curve.p and tab("mod") == pk.p
    assert pk.Rp == 1 << (pk.B * pk.L) and tab("one") == pk.Rp % pk.p == pk.one
    assert tab("k_import") == pk.k_import == pk.Rp * pk.Rp * pow(1 << (64 * pk.curve.limbs), -1, pk.p) % pk.p
    assert tab("k_export") == pk.k_export == o.mont_constants(pk.p, pk.curve.limbs)["R"]
    assert int(re.search(r"NINV = (0x[0-9a-f]+)u", blk).group(1), 16) == pk.ninv
    assert pk.ninv * pk.p % (1 << pk.B) == (1 << pk.B) - 1
    assert o.is_on_curve(pk.curve, o.generator(pk.curve))


@pytest.mark.parametrize("pk", fm.SAT_PACKS, ids=_ids)
def test_saturated_packs_are_the_fields_of_the_curves(pk):
    src = open(os.path.join(ROOT, "accumulation_amd", "csrc", "fp.h")).read()
    blk = src[src.index("struct " + pk.name + " {"):]
    blk = blk[:blk.index("};")]
    vals = [int(x.strip().rstrip("u"), 16) for x in re.search(r"AMSM_TABLE\(mod, \d+, ([^)]*)\)", blk, re.S).group(1).split(",")]
    assert len(vals) == pk.L == pk.W and pk.value(vals) == pk.p
    gen = open(os.path.join(ROOT, "accumulation_amd", "csrc", "fp_mul_gfx950.h")).read()
    assert f"fe_mul<{pk.name}>" in gen                        # every saturated pack has a generated (or shared) schedule
    assert (f"fe_dot2<{pk.name}>" in gen) == pk.dots == (f"fe_dot3<{pk.name}>" in gen)


@pytest.mark.parametrize("op", fm.FIELD_OPS)
@pytest.mark.parametrize("pk", fm.UNSAT_PACKS, ids=_ids)
def test_every_field_case_is_inside_the_needs(pk, op):
    cases = fm.field_cases(pk.pid, op)
    assert len(cases) <= fm.MAX_CASES
    for tag, ins in cases:
        assert fm.field_contract(pk, op, ins)[0], (pk.name, op, tag)
        assert all(0 <= x < (1 << 32) for a in ins for x in a)


@pytest.mark.parametrize("pk", fm.UNSAT_PACKS, ids=_ids)
def test_field_cases_reach_the_edges_the_issue_names(pk):
    """the value classes are there after clipping: the exact subtrahend limit and 0, all-ones lazy limbs in a column sum, m_k at 0
    and at 2^B - 1 (in all columns at once, and in each column beside a neighbour of the other kind), every k p below KMAX p and
    its neighbours"""
    p, wide = pk.p, (1 << (pk.B + 1)) - 1
    for op in fm.FIELD_OPS:
        base, K = fm.split_op(op)
        vals = [[pk.value(a) for a in ins] for _, ins in fm.field_cases(pk.pid, op)]
        raw = [ins for _, ins in fm.field_cases(pk.pid, op)]
        if base in ("mul_sub_k", "mul_sub_mul_k"):
            assert {v[2] for v in vals} >= {0, pk.sub_limit(K)}, op
            assert any(ins[2][:-1] == [pk.M] * (pk.L - 1) for ins in raw), op
        if base == "sqr_sub_bcc_k":
            assert {v[1] + 2 * v[2] for v in vals} >= {0, pk.sub_limit(K)}, op
        if base in ("mul", "mul_sub_k", "mul_sub_mul_k"):
            assert any(ins[0][:-1] == [wide] * (pk.L - 1) for ins in raw), op           # lazy limbs all at 2^(B+1) - 1 (top limb clipped)
            assert any(v[0] * v[1] == p for v in vals) and any(v[0] * v[1] == 0 for v in vals), op  # every m_k = 2^B - 1; every m_k = 0
        if base == "mul":
            assert any(ins[1][:-1] == [wide] * (pk.L - 1) for ins in raw), op
            assert all([1 << (pk.B * i), 1] in vals for i in range(pk.L)), op
            m0 = lambda v: ((v[0] * v[1]) % (1 << pk.B)) * pk.ninv % (1 << pk.B)  # noqa: E731
            assert {m0(v) for v in vals} >= {0, pk.M}, op
        if base == "mul":  # the reduction column by column: m_k = 0 beside m_(k+1) != 0, and the other way round, at every column
            ms = [fm.reduction_multipliers(pk, *ins) for ins in raw]
            for k in range(pk.L - 1):
                assert any(m[k] == 0 and m[k + 1] != 0 for m in ms) and any(m[k] != 0 and m[k + 1] == 0 for m in ms), (op, k)
            assert [pk.M * (i & 1) for i in range(pk.L)] in ms and [pk.M * (1 - (i & 1)) for i in range(pk.L)] in ms and [1] * pk.L in ms
            for k in range(pk.L):
                assert [int(i == k) for i in range(pk.L)] in ms and [pk.M * int(i == k) for i in range(pk.L)] in ms, (op, k)
        if base == "is_zero_mod":
            flat = {v[0] for v in vals}
            assert flat >= {k * p for k in range(K)} | {k * p + 1 for k in range(K)} | {k * p - 1 for k in range(1, K)}, op
            assert flat >= {k * p + (1 << pk.B) for k in range(K)}, op
        if base == "canon":
            assert {v[0] for v in vals} >= {k * p + r for k in range(K) for r in (0, 1, p - 1)}, op
        if base == "import":
            assert pk.R - 1 in {v[0] for v in vals}
        if base in ("export", "store"):
            assert 8 * p - 1 in {v[0] for v in vals}
        if base == "from_words":
            assert [(1 << 32) - 1] * pk.W in [ins[0] for ins in raw]


@pytest.mark.parametrize("op", fm.GROUP_OPS)
@pytest.mark.parametrize("pk", fm.UNSAT_PACKS, ids=_ids)
def test_every_group_case_is_inside_the_invariants(pk, op):
    cases = fm.group_cases(pk.pid, op)
    assert len(cases) * (4 if op in fm.QUAD_OPS else 1) <= fm.MAX_CASES
    for tag, ins, _ in cases:
        assert fm.group_needs(pk, op, ins), (pk.name, op, tag)


@pytest.mark.parametrize("pk", fm.UNSAT_PACKS, ids=_ids)
def test_group_cases_hold_the_tiny_y_class_and_the_bound_edges(pk):
    """points whose internal y is below 2^(B (L - 1)), their negatives doubled through a lazily negated q.y (the K = 2 top-limb
    borrow of xyzz_dbl_affine), and accumulators with Y just under 3p"""
    pts, tiny = fm.probe_points(pk.pid)
    assert len(tiny) >= 2 and all(pk.to_m(P[1]) < (1 << pk.top_shift) for P in tiny)
    edge = 2 * pk.p - (1 << pk.top_shift)
    madd = fm.group_cases(pk.pid, "xyzz_madd")
    assert any(tag.startswith("q=acc") and pk.value(ins[5]) > edge and not pk.is_tight(ins[5]) for tag, ins, _ in madd)
    assert any(pk.value(ins[1]) >= 2 * pk.p and pk.value(ins[0]) >= 7 * pk.p for _, ins, _ in madd)
    assert any(pk.value(ins[1]) > edge for _, ins, _ in fm.group_cases(pk.pid, "xyzz_dbl_affine"))
    assert any(pk.value(ins[5]) > edge for tag, ins, _ in fm.group_cases(pk.pid, "jac_madd") if tag.startswith("q=acc"))
    for op in ("xyzz_madd", "xyzz_add", "jac_madd"):
        tags = {tag.split(":")[0] for tag, _, _ in fm.group_cases(pk.pid, op)}
        assert tags >= {"generic", "q=acc", "q=-acc", "acc=inf", "q=inf"}, op


def test_chosen_multipliers_are_what_the_reduction_computes():
    """a = -m p mod R' against b = 1: a word-by-word Montgomery reduction in radix 2^B, written out here, multiplies p by exactly the
    limbs of m -- on the p_0 = 1 branch (m_k = -lo) and on the general one (m_k = lo NINV mod 2^B) alike"""
    for pk in fm.UNSAT_PACKS:
        pats = dict(fm.chosen_m_patterns(pk))
        assert len(pats) == 2 * pk.L + 4
        present = [ins for _, ins in fm.field_cases(pk.pid, "mul")]  # (an operand pair an older case already holds keeps that tag)
        for (tag, ins), m in zip(fm.chosen_m_cases(pk), pats.values()):
            acc, got = pk.value(ins[0]) * pk.value(ins[1]), []
            for _ in range(pk.L):
                got.append((acc & pk.M) * pk.ninv & pk.M)
                acc = (acc + got[-1] * pk.p) >> pk.B
            assert got == m == fm.reduction_multipliers(pk, *ins), (pk.name, tag)
            assert pk.is_tight(ins[0]) and fm.field_contract(pk, "mul", ins)[0] and ins in present, (pk.name, tag)
    assert {pk.name for pk in fm.UNSAT_PACKS if pk.ninv == pk.M} == {"PallasFqU", "VestaFqU", "Bls12377FqU"}  # the p_0 = 1 branch


def test_two_torsion_flag_is_the_headers():
    """Pack.two_torsion <=> csrc/fp.h specialises HasTwoTorsion for the pack <=> the curve has a point with y = 0 (x^3 = -b has a
    root: -b is a cube, p = 1 mod 3 for every curve here) -- and the flipped pack of the probe inherits the specialisation"""
    src = open(os.path.join(ROOT, "accumulation_amd", "csrc", "fp.h")).read()
    special = set(re.findall(r"struct HasTwoTorsion<(\w+)> \{\s*static constexpr bool value = true;", src))
    for pk in fm.UNSAT_PACKS:
        c = pk.curve
        assert c.p % 3 == 1
        even = pow(-c.b % c.p, (c.p - 1) // 3, c.p) == 1
        assert pk.two_torsion == even == (pk.name in special), pk.name
        if even:
            so = fm.small_order_points(pk.pid)
            assert so["T"][1] == 0 and o.add(c, so["T"], so["T"]) is None and o.add(c, so["S"], so["2S"]) == so["T"]
            assert f"struct HasTwoTorsion<{pk.name}Other> : HasTwoTorsion<{pk.name}> {{}};" in open(PROBE_SRC).read()
    assert special == {"Bls12377Fq", "Bls12377FqU"}


@pytest.mark.parametrize("pk", [pk for pk in fm.UNSAT_PACKS if pk.two_torsion], ids=_ids)
def test_group_cases_hold_the_two_torsion_class(pk):
    """for a curve of even order: the point of order 2 with Y (y) written as a NON-ZERO multiple of p -- the representatives the
    HasTwoTorsion guards exist for -- reaches each of the three guarded doublings, xyzz_dbl_affine, and the q = acc branch of both
    mixed additions and of both full additions; every such case is inside the invariants and expects the identity"""
    p = pk.p
    T = fm.small_order_points(pk.pid)["T"]
    xT = pk.to_m(T[0])

    def kp(limbs):  # k if the limbs are k p with k != 0, else 0
        v = pk.value(limbs)
        return v // p if v and v % p == 0 else 0

    for op, bound in (("xyzz_dbl", 3), ("xyzz_dbl_quad", 3), ("jac_dbl", 13)):
        hit = [ins for _, ins, want in fm.group_cases(pk.pid, op) if kp(ins[1]) and pk.value(ins[0]) % p != 0 and want is None]
        assert {kp(ins[1]) for ins in hit} == set(range(1, bound)) and all(fm.group_needs(pk, op, ins) for ins in hit), op
        assert any(pk.value(ins[1]) == 0 and pk.value(ins[2]) != 0 and want is None for _, ins, want in fm.group_cases(pk.pid, op)), op
    hit = [ins for _, ins, want in fm.group_cases(pk.pid, "xyzz_dbl_affine") if kp(ins[1]) and want is None]
    assert {(pk.value(ins[0]), kp(ins[1])) for ins in hit} == {(xT + kx * p, ky) for kx in (0, 1) for ky in (1, 2)}
    assert all(fm.group_needs(pk, "xyzz_dbl_affine", ins) for ins in hit)
    for op, bound in (("xyzz_madd", 3), ("jac_madd", 13)):
        cases = fm.group_cases(pk.pid, op)
        hit = [ins for tag, ins, want in cases if tag.startswith("q=acc=T") and want is None]
        assert all(pk.value(ins[4]) == xT and pk.value(ins[5]) % p == 0 and fm.group_needs(pk, op, ins) for ins in hit), op
        assert {(kp(ins[1]), kp(ins[5]), pk.is_tight(ins[5])) for ins in hit} >= \
            {(ky, kq, t) for ky in range(bound) for kq in (1, 2) for t in (False, True)}, op   # lazy and tight limbs of p and of 2p
        assert {kp(ins[1]) for ins in hit if pk.value(ins[5]) == 0} == set(range(bound)), op    # and the plain y = 0
        tags = {tag.split(":")[0] for tag, _, _ in cases}
        assert tags >= {"acc=3S,q=T", "acc=S,q=T", "acc=inf,q=T"}, op
    for op in ("xyzz_add", "xyzz_add_quad"):
        cases = fm.group_cases(pk.pid, op)
        hit = [ins for tag, ins, want in cases if tag.startswith("T+T") and want is None]
        assert {(kp(ins[1]), kp(ins[5])) for ins in hit} == {(a, b) for a in range(3) for b in range(3)}, op
        assert all(fm.group_needs(pk, op, ins) for ins in hit), op
        want = {tag.split(":")[0]: w for tag, _, w in cases}
        assert want["S+2S"] == T and want["T+U"] is not None and want["T+U"] == want["U+T"], op
        assert len(cases) * (4 if op in fm.QUAD_OPS else 1) <= fm.MAX_CASES


@pytest.mark.parametrize("pk", fm.SAT_PACKS, ids=_ids)
def test_saturated_cases_are_canonical_and_reach_the_unreduced_sums(pk):
    m, Ri = pk.p, pow(pk.R, -1, pk.p)
    for op in fm.SAT_OPS:
        cases = fm.sat_cases(pk.pid, op)
        assert len(cases) <= fm.MAX_CASES and all(0 <= v < m for _, vals in cases for v in vals)
    for op, k in (("sat_dot2", 2), ("sat_dot3", 3)):  # the sum of the canonical products just below k m
        sums = {sum(vals[2 * i] * vals[2 * i + 1] * Ri % m for i in range(k)) for _, vals in fm.sat_cases(pk.pid, op)}
        assert k * m - k in sums, op


def test_operation_tables_agree():
    """PROBE_OPS of field_probe.hip and OPS of field_model.py: the same names in the same order; the pack ids too"""
    src = open(PROBE_SRC).read()
    body = src[src.index("#define PROBE_OPS(X)"):src.index("enum ProbeOp")]
    assert re.findall(r"X\((\w+)\)", body) == fm.OPS
    packs = src[src.index("#define PROBE_PACKS(X)"):src.index("#ifdef PROBE_PACK")]
    got = {int(i): n for i, n in re.findall(r"X\((\d+), (\w+)\)", packs)}
    want = {pk.pid: pk.name for pk in fm.UNSAT_PACKS + fm.SAT_PACKS}
    want.update({pk.other: pk.name + "Other" for pk in fm.UNSAT_PACKS if pk.other is not None})
    assert got == want
    from accumulation_amd import build
    assert sorted(got) == build.PROBE_PACKS


def test_probe_is_not_part_of_the_library():
    from accumulation_amd import build
    assert not any("probe" in u for u in build.UNITS)
    assert os.path.dirname(build.PROBE_LIB) == os.path.dirname(PROBE_SRC) and build.PROBE_LIB.endswith(".so")


def test_probe_cross_compiles_for_gfx950():
    """builds it if it is missing or stale (as the GPU module's fixture does) and finds the one entry point"""
    import ctypes

    from accumulation_amd import build
    path = build.build_probe(verbose=False)
    assert os.path.exists(path) and not build.probe_stale()
    lib = ctypes.CDLL(path)
    assert lib.field_probe_op_count() == len(fm.OPS)
    assert hasattr(lib, "field_probe_run")
