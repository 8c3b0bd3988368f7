"""tests/cpp/sample_check.cpp: transparent keys (amsm_bases_sample) from C++ through include/amsm.hpp and the scheme headers'
setup_transparent -- on the host backend without a GPU, and on the GPU with the same values printed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sample_check.cpp")
EXE = os.path.join(ROOT, "build", "sample_check")


def build():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    libdir = os.path.join(ROOT, "accumulation_amd")
    tmp = EXE + f".{os.getpid()}"  # (compiled beside the target and moved into place: pytest -n workers may build it at once)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-o", tmp,
                           "-L", libdir, "-l:libamsm.so", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"])
    os.replace(tmp, EXE)


def run(device):
    build()
    out = subprocess.run([EXE], capture_output=True, text=True, env=dict(os.environ, AMSM_CHECK_DEVICE=str(device)), timeout=600)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "done", out.stdout + out.stderr
    return out.stdout


def test_cpp_sample_on_the_host_backend(built_lib):
    assert run(-1).count("value ") == 12  # three generators and a commitment per curve


@pytest.mark.gpu
def test_cpp_sample_on_the_gpu_prints_the_host_backend_values(built_lib):
    assert run(0) == run(-1)
