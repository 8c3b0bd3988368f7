"""test_trivial_pc_as_device_gpu.py on the host backend (conftest.py of this directory; test_host_context_cpu.py says why).  The
2^20 harness of that file (above 2^HOST_MAX_LOG = 2^18) is skipped here."""
from tests.test_trivial_pc_as_device_gpu import *  # noqa: F401,F403
pytestmark = []  # (the star import brought the GPU module's `gpu` mark along: these run on the host backend, without one)
