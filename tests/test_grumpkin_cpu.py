"""Grumpkin (AMSM_GRUMPKIN = 6: base field BN254's r, order BN254's p, y^2 = x^3 - 17, generator (1, sqrt(-16)), cofactor 1)
without a GPU: the cases its row of tests/curve_rows.py lists (Row.cpu_cases), whose bodies
tests/curve_cases_cpu.py holds once for all four curves, and behind them the curve's own."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest

pytest.register_assert_rewrite("tests.curve_cases_cpu")
from oracle import pyref as o  # noqa: E402
from oracle import pyref_ser as ser  # noqa: E402
from tests import curve_cases_cpu as cases  # noqa: E402
from tests import curve_rows as cr  # noqa: E402
from tests import helpers as h  # noqa: E402
from tests.curve_rows import ROOT  # noqa: E402

BN254, GRUMPKIN = h.BN254, h.GRUMPKIN
ROW = cr.GRUMPKIN
globals().update(cr.take(cases, ROW.cpu_cases, ROW.aliases))


Q_LIMBS_29 = [0x10000001, 0x1F0FAC9F, 0x0E5C2450, 0x07D090F3, 0x1585D283, 0x02DB40C0, 0x00A6E141, 0x0E5C2634, 0x0030644E]


def test_curve_facts():
    P, R, GY = GRUMPKIN.p, GRUMPKIN.r, GRUMPKIN.gy
    assert (P, R) == (BN254.r, BN254.p)  # Grumpkin's base field (coordinates) and scalar field (group order): BN254's, swapped
    assert P == 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
    assert R == 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
    g = o.generator(GRUMPKIN)
    assert GY == 0x2CF135E7506A45D632D270D45F1181294833FC48D823F272C and GY * GY % P == P - 16
    assert g == (1, GY) and o.is_on_curve(GRUMPKIN, g) and o.mul(GRUMPKIN, R, g) is None  # order p_BN, prime: cofactor 1
    assert GRUMPKIN.b == P - 17 and P.bit_length() == R.bit_length() == 254
    assert P % 4 == 1 and (P - 1) % (1 << 28) == 0 and ((P - 1) >> 28) % 2 == 1  # Tonelli-Shanks, 2-adicity 28
    assert P % 3 == 1 and R % 3 == 1  # cube roots of unity in both fields: GLV (j = 0)
    assert math.gcd(17, P - 1) == 1  # the sponge's alpha = 17 permutes Fq
    assert (1 << 261) // P == 169 and abs((1 << 261) / P - 169.28) < 0.01  # head-room of a tight value: BN254's
    assert R < (1 << 254) and abs(R / (1 << 255) - 0.378) < 0.001  # the scalar stream's acceptance rate per candidate
    assert R >> 240 == 0x3064  # the top 16-bit window of a scalar: BN254's, so a plain 2^20 MSM takes BN254's pipeline
    assert ser.point_size(GRUMPKIN, True) == 32 and ser.point_size(GRUMPKIN, False) == 64  # 254 + 2 flag bits


def test_modulus_shape_in_radix_2p29():
    """no zero limb, no power-of-two limb above limb 0, q_0 = 2^28 + 1 and NINV = 2^28 - 1: the general reduction branch of
    csrc/fpu.h, and the column sums of the nine-limb general shape still fit"""
    P = GRUMPKIN.p
    limbs = [(P >> (29 * i)) & ((1 << 29) - 1) for i in range(9)]
    assert limbs == Q_LIMBS_29 and limbs[0] == (1 << 28) + 1
    assert all(v != 0 for v in limbs) and all(v & (v - 1) != 0 for v in limbs[1:])
    ninv = (-pow(P, -1, 1 << 29)) % (1 << 29)
    assert ninv == 0x0FFFFFFF and ninv != (1 << 29) - 1
    lazy, tight = (1 << 30) - 1, (1 << 29) - 1
    carry = 1 << 35
    assert 9 * lazy * tight + 9 * tight * tight + carry < 1 << 63  # one product, one lazy operand
    assert 18 * lazy * tight + 9 * tight * tight + carry + (1 << 32) < 1 << 64  # u_mul_add_mul, an addend riding along
    assert (4 * 9 + 9) * tight * tight + carry < 1 << 64  # four tight products under one reduction (the removed u_dot<4>)


def test_curve_b_is_q_minus_17(host_ctx, row, built_lib):
    """curve_b_mont through amsm_points_check on the host backend, and through the uncompressed encoding"""
    from tests.test_points_check_cpu import report_of
    from tests.test_wire_format_cpu import lib_points_deserialize
    pts, want = cr.grumpkin_b_cases()
    rep, st = host_ctx.check_points(cr.raw_points(GRUMPKIN, pts), np.zeros(len(pts), dtype=np.uint8), want_status=True)
    assert list(st) == want and rep == report_of(np.array(want, dtype=np.uint8)) and rep["first_bad"] == 2
    wx, wy = cr.old_cast_point()  # on the curve the old cast of b described, not on this one
    assert lib_points_deserialize(built_lib, GRUMPKIN, [wx.to_bytes(32, "little") + wy.to_bytes(32, "little")], False)[0] != 0


def test_fixture_generator_reproduces_both_fixtures(tmp_path):
    """tools/gen_bn254_adversarial_points.py --curve: the committed Grumpkin fixture, and BN254's byte for byte as before"""
    P, R = GRUMPKIN.p, GRUMPKIN.r
    spec = importlib.util.spec_from_file_location("gen_adv", os.path.join(ROOT, "tools", "gen_bn254_adversarial_points.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for name, fname in (("grumpkin", "grumpkin_adversarial_points.json"), ("bn254_g1", "bn254_adversarial_points.json")):
        c, _, f = gen.CURVES[name]
        assert f == fname and (c.p, c.r, c.b) == ((P, R, P - 17) if name == "grumpkin" else (R, P, 3))
        committed = json.load(open(os.path.join(ROOT, "tests", "golden", fname)))
        kinds = gen.build(c)
        assert committed["curves"][c.name] == {k: [[hex(pt[0]), hex(pt[1])] for pt in v] for k, v in kinds.items()}


def test_the_cycle_closes(built_lib, host_ctx, row):
    from accumulation_amd import Context, ffi
    bn = Context(ffi.AMSM_BN254_G1, device=ffi.AMSM_DEVICE_HOST)
    try:
        cr.cycle_closes(bn, BN254, host_ctx, GRUMPKIN, 41)  # BN254 commitments' coordinates, committed to on Grumpkin
        cr.cycle_closes(host_ctx, GRUMPKIN, bn, BN254, 43)  # and the other way round
    finally:
        bn.close()
