"""The out-of-memory sweep from C++ (tests/cpp/oom_sweep.cpp: the C ABI of include/amsm.h and the four gate wrappers of
amsm::Context): builds as plain C++17 and runs on the library's host backend -- keys, a matrix and the MSM entry points, each with
every allocation request refused once."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "oom_sweep.cpp")
EXE = os.path.join(ROOT, "build", "oom_sweep")

FAMILIES = ["amsm_bases_generate", "amsm_bases_load|CHECK", "amsm_bases_from_device", "amsm_bases_sample", "amsm_bases_fold", "amsm_matrix_load",
            "amsm_msm_device", "amsm_msm", "amsm_msm_oneshot"]


def build():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    libdir = os.path.join(ROOT, "accumulation_amd")
    tmp = EXE + f".{os.getpid()}"  # (compiled beside the target and moved into place: parallel workers build and run the same program)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-o", tmp,
                           "-L", libdir, "-l:libamsm.so", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"])
    os.replace(tmp, EXE)


def test_cpp_oom_sweep_on_the_host_backend(built_lib):
    build()
    out = subprocess.run([EXE], capture_output=True, text=True, env=dict(os.environ, AMSM_CHECK_DEVICE="-1"), timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines()]
    assert ["done"] in lines
    fams = {ln[1]: dict(zip(ln[2::2], map(int, ln[3::2]))) for ln in lines if ln[0] == "family"}
    assert list(fams) == FAMILIES, fams
    # every creator's memory passes the gate on the host backend: each sweep saw at least one AMSM_E_OOM (the matrix: its three arrays)
    for name in FAMILIES[:6] + ["amsm_msm_oneshot"]:
        assert fams[name]["oom"] >= 1, (name, fams[name])
    assert fams["amsm_matrix_load"]["oom"] == 3
