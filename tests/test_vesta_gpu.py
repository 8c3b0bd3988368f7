"""Vesta (AMSM_VESTA = 2) on the GPU: the cases its row of tests/curve_rows.py lists (Row.gpu_cases), whose bodies tests/curve_cases_gpu.py holds once
for all four curves, with this module's own context, host-backend context and 20-bit key."""
import pytest

pytest.register_assert_rewrite("tests.curve_cases_gpu")
from tests import curve_cases_gpu as cases  # noqa: E402
from tests import curve_rows as cr  # noqa: E402

pytestmark = pytest.mark.gpu
ROW = cr.VESTA
globals().update(cr.take(cases, ROW.gpu_cases, ROW.aliases))
