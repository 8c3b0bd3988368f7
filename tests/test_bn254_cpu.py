"""BN254 G1 (AMSM_BN254_G1 = 4: y^2 = x^3 + 3, generator (1, 2), cofactor 1; the first 9 x 29-bit field on the general reduction)
without a GPU: the cases its row of tests/curve_rows.py lists (Row.cpu_cases), whose bodies
tests/curve_cases_cpu.py holds once for all four curves, and behind them the curve's own."""
import math

import pytest

pytest.register_assert_rewrite("tests.curve_cases_cpu")
from oracle import pyref as o  # noqa: E402
from tests import curve_cases_cpu as cases  # noqa: E402
from tests import curve_rows as cr  # noqa: E402
from tests import helpers as h  # noqa: E402

BN254 = h.BN254
ROW = cr.BN254
globals().update(cr.take(cases, ROW.cpu_cases, ROW.aliases))


P_LIMBS_29 = [0x187CFD47, 0x010460B6, 0x1C72A34F, 0x02D522D0, 0x1585D978, 0x02DB40C0, 0x00A6E141, 0x0E5C2634, 0x0030644E]


def test_curve_facts():
    P, R = BN254.p, BN254.r
    assert P == 21888242871839275222246405745257275088696311157297823662689037894645226208583
    assert R == 21888242871839275222246405745257275088548364400416034343698204186575808495617
    g = o.generator(BN254)
    assert g == (1, 2) and o.is_on_curve(BN254, g) and o.mul(BN254, R, g) is None  # prime order r (cofactor 1)
    assert P.bit_length() == R.bit_length() == 254
    assert P % 4 == 3  # the direct square root
    assert P % 3 == 1 and R % 3 == 1  # cube roots of unity in both fields: GLV (j = 0)
    assert (R - 1) % (1 << 28) == 0 and ((R - 1) >> 28) % 2 == 1  # 2-adicity 28
    assert math.gcd(17, P - 1) == 1 and math.gcd(17, R - 1) == 1  # the sponge's alpha = 17 permutes
    assert (1 << 261) // P == 169 and (1 << 261) // o.PALLAS.p == 127  # head-room of a tight value
    assert R < (1 << 254) and abs(R / (1 << 255) - 0.378) < 0.001  # the scalar stream's acceptance rate per candidate
    assert 0.622 ** 64 < 1e-13  # its fallback


def test_modulus_shape_in_radix_2p29():
    """no zero limb, p_0 != 1, no power-of-two limb: none of the Pallas shortcuts of csrc/fpu.h applies, and the column sums still fit"""
    P = BN254.p
    limbs = [(P >> (29 * i)) & ((1 << 29) - 1) for i in range(9)]
    assert limbs == P_LIMBS_29
    assert all(v != 0 and v & (v - 1) != 0 for v in limbs) and limbs[0] != 1
    lazy, tight = (1 << 30) - 1, (1 << 29) - 1
    carry = 1 << 35
    assert 9 * lazy * tight + 9 * tight * tight + carry < 1 << 63  # one product, one lazy operand
    assert 18 * lazy * tight + 9 * tight * tight + carry + (1 << 32) < 1 << 64  # u_mul_add_mul, an addend riding along
    assert (4 * 9 + 9) * tight * tight + carry < 1 << 64  # four tight products under one reduction (the removed u_dot<4>)
