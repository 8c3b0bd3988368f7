"""Vesta (AMSM_VESTA = 2, the other half of the Pasta cycle: Fq = Pallas's Fr, Fr = Pallas's Fq, y^2 = x^3 + 5, generator (-1, 2),
cofactor 1) without a GPU: the cases its row of tests/curve_rows.py lists (Row.cpu_cases), whose bodies
tests/curve_cases_cpu.py holds once for all four curves, and behind them the curve's own."""

import numpy as np
import pytest

pytest.register_assert_rewrite("tests.curve_cases_cpu")
from oracle import pyref as o  # noqa: E402
from oracle import pyref_ser as ser  # noqa: E402
from tests import curve_cases_cpu as cases  # noqa: E402
from tests import curve_rows as cr  # noqa: E402
from tests import helpers as h  # noqa: E402

VESTA = h.VESTA
ROW = cr.VESTA
globals().update(cr.take(cases, ROW.cpu_cases, ROW.aliases))


def test_curve_facts():
    g = o.generator(VESTA)
    assert o.is_on_curve(VESTA, g) and o.mul(VESTA, VESTA.r, g) is None  # prime order r_V (cofactor 1)
    assert VESTA.p % 3 == 1 and (VESTA.p - 1) % (1 << 32) == 0 and ((VESTA.p - 1) >> 32) % 2 == 1  # 2-adicity 32
    # the shape the Pallas bound reasoning and zero-limb shortcuts rest on: p_0 = 1 (NINV all ones), limbs 5-7 zero, top limb 2^22,
    # R' / p = 127
    m, R_dev = VESTA.p, 1 << 261
    assert (-pow(m, -1, 1 << 29)) % (1 << 29) == 0x1FFFFFFF
    limbs = [(m >> (29 * i)) & ((1 << 29) - 1) for i in range(9)]
    assert limbs == [0x1, 0x2375908, 0x052A3763, 0x0D31F813, 0x224, 0, 0, 0, 0x400000]
    assert R_dev // m == 127 and R_dev // o.PALLAS.p == 127


def test_generator_encoding_and_rejections(built_lib):
    from tests.test_wire_format_cpu import lib_points_deserialize, lib_points_serialize
    g = o.generator(VESTA)
    (blob,), sz = lib_points_serialize(built_lib, VESTA, [g], True)
    # x = p - 1 little-endian; y = 2 is the smaller root: no flag bit
    assert sz == 33 and blob == (VESTA.p - 1).to_bytes(33, "little") == ser.point_serialize(VESTA, g)
    rc, (back,) = lib_points_deserialize(built_lib, VESTA, [blob], True)
    assert rc == 0 and back == g
    x = 1
    while ser._sqrt(x * x * x + VESTA.b, VESTA.p) is not None:  # an x with no point on Vesta
        x += 1
    assert lib_points_deserialize(built_lib, VESTA, [x.to_bytes(33, "little")], True)[0] != 0
    assert lib_points_deserialize(built_lib, VESTA, [VESTA.p.to_bytes(33, "little")], True)[0] != 0  # x = p


def test_unknown_curve_is_refused(built_lib):
    from accumulation_amd import ffi
    from accumulation_amd.engine import Context
    with pytest.raises(Exception):
        Context(3, device=ffi.AMSM_DEVICE_HOST)
    a = np.zeros(4, dtype=np.uint64)
    assert built_lib.amsm_fr_to_mont(3, a.ctypes.data, 1, a.ctypes.data) == ffi.AMSM_E_INVALID_ARG
    assert built_lib.amsm_point_serialized_size(3, 1) == 0
