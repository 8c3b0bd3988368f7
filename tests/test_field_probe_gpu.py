"""The base-field primitives and the group law, one function at a time, at the edges of their stated bounds.

tests/hip/field_probe.hip applies ONE function of csrc/fpu.h / fp.h / ec.h per launch to raw register limbs; tests/field_model.py
holds the documented contract of each (Needs, residue class or exact value, Gives) in Python integers.  A result passes if it
has the documented limb widths, lies in the documented range and is congruent (or equal) to the right value; the group law's
results must map to the oracle's affine sum and stay inside the register invariant of their representation.  No case
leaves a function's Needs (tests/test_field_probe_cpu.py asserts that without a GPU), so nothing here is meant to fault.

The probe compiles the force-inlined templates into its own kernels: it pins the source-level semantics on the hardware, not
the register allocation of the MSM kernels."""
import pytest

from tests import field_model as fm
from tests import field_probe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    return field_probe.load()


def _ids(pk):
    return pk.name


def _fail(pk, op, errors, n):
    lines = "\n".join(f"  [{tag}] {err}" for tag, err in errors[:12])
    pytest.fail(f"{pk.name} {op}: {len(errors)} of {n} cases break the contract\n{lines}", pytrace=False)


@pytest.mark.parametrize("op", fm.FIELD_OPS)
@pytest.mark.parametrize("pk", fm.UNSAT_PACKS, ids=_ids)
def test_field_primitive_keeps_its_contract(probe, pk, op):
    cases = fm.field_cases(pk.pid, op)
    out = field_probe.run(probe, pk.pid, op, [ins for _, ins in cases])
    if pk.other is not None:  # the other CHAIN setting is the same function: bit-identical limbs
        assert (field_probe.run(probe, pk.other, op, [ins for _, ins in cases]) == out).all(), "CHAIN changes the limbs"
    errors = []
    for (tag, ins), res in zip(cases, out):
        ok, want = fm.field_contract(pk, op, ins)
        assert ok, (tag, "the case is outside the function's Needs")
        err = fm.check_field(pk, want, res[0][0])
        if err:
            errors.append((tag, err))
    if errors:
        _fail(pk, op, errors, len(cases))


@pytest.mark.parametrize("op", fm.GROUP_OPS)
@pytest.mark.parametrize("pk", fm.UNSAT_PACKS, ids=_ids)
def test_group_law_matches_oracle_inside_its_invariants(probe, pk, op):
    cases = fm.group_cases(pk.pid, op)
    rep = 4 if op in fm.QUAD_OPS else 1
    out = field_probe.run(probe, pk.pid, op, [ins for _, ins, _ in cases], replicate=rep)
    if pk.other is not None:
        assert (field_probe.run(probe, pk.other, op, [ins for _, ins, _ in cases], replicate=rep) == out).all(), "CHAIN changes the limbs"
    errors = []
    for (tag, ins, expected), res in zip(cases, out):
        assert fm.group_needs(pk, op, ins), (tag, "the case is outside the register invariants")
        if not (res == res[0]).all():
            errors.append((tag, "the four lanes of the quad disagree"))
            continue
        err = fm.check_group(pk, op, ins, res[0], expected)
        if err:
            errors.append((tag, err))
    if errors:
        _fail(pk, op, errors, len(cases))


SAT = [(pk, op) for pk in fm.SAT_PACKS for op in fm.SAT_OPS if pk.dots or op not in ("sat_dot2", "sat_dot3")]


@pytest.mark.parametrize("pk,op", SAT, ids=[f"{pk.name}-{op}" for pk, op in SAT])
def test_saturated_field_is_exact(probe, pk, op):
    """fe_mul is a b / R mod m and bit-identical to fe_mul_ref of the same launch; fe_dot2 / fe_dot3 (where generated) are the
    canonical sum, with unreduced sums just below 2m and 3m among the cases; fe_add, fe_sub, fe_neg, fe_inv are exact"""
    cases = fm.sat_cases(pk.pid, op)
    out = field_probe.run(probe, pk.pid, op, [[pk.limbs(v) for v in vals] for _, vals in cases])
    errors = []
    for (tag, vals), res in zip(cases, out):
        want = fm.sat_expected(pk, op, vals)
        got = pk.value(res[0][0][:pk.L])
        if got != want:
            errors.append((tag, f"{got:#x}, expected {want:#x}"))
        elif op == "sat_mul" and pk.value(res[0][1][:pk.L]) != got:
            errors.append((tag, "the generated schedule differs from fe_mul_ref"))
    if errors:
        _fail(pk, op, errors, len(cases))
