"""test_points_check_gpu.py on the host backend (conftest.py of this directory; test_host_context_cpu.py says why).  The sizes above
2^HOST_MAX_LOG (= 2^16) of that file are skipped here, its _size_guard: the host backend multiplies every BLS12-381 point by the
255-bit group order, and 2^20 of those would take minutes; what is skipped is the 2^20 run alone, which the GPU suite covers."""
from tests.test_points_check_gpu import *  # noqa: F401,F403
pytestmark = []  # (the star import brought the GPU module's `gpu` mark along: these run on the host backend, without one)
