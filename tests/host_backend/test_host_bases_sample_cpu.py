"""test_bases_sample_gpu.py on the host backend (conftest.py of this directory; test_host_context_cpu.py says why).  The sizes above
2^HOST_MAX_LOG (= 2^18) of that file are skipped here: its _size_guard."""
from tests.test_bases_sample_gpu import *  # noqa: F401,F403
pytestmark = []  # (the star import brought the GPU module's `gpu` mark along: these run on the host backend, without one)
