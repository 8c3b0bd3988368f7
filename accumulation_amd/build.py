"""Build libamsm.so in-tree with hipcc for gfx950 (one object per translation unit, in parallel).

    python -m accumulation_amd.build [--force]

hipcc cross-compiles without a GPU.  The objects land in build/obj/, the library next to this file so
that it travels with the repo snapshot to the GPU box (it is git-ignored, not gpurun-ignored).
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(ROOT, "build", "obj")
LIB = os.path.join(HERE, "libamsm.so")
ARCH = "gfx950"
UNITS = ["api.hip", "kern_pallas.hip", "kern_bls12_381.hip", "kern_vesta.hip", "kern_bn254.hip", "kern_grumpkin.hip",
         "kern_bls12_377.hip", "kern_fr.hip"]
FLAGS = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-Wno-unused-result", "-Wno-pass-failed",
         "-Rpass-analysis=kernel-resource-usage"]


def _deps():
    out = [os.path.join(ROOT, "include", "amsm.h")]
    for f in os.listdir(CSRC):
        out.append(os.path.join(CSRC, f))
    return out


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _unit_deps(unit: str, all_deps):
    """The files a unit really includes (the depfile hipcc wrote on its last compile: -MD), else everything."""
    dep = os.path.join(OBJ, unit.replace(".hip", ".d"))
    if not os.path.exists(dep):
        return all_deps
    try:
        words = open(dep).read().replace("\\\n", " ").split()
    except OSError:
        return all_deps
    files = [w for w in words[1:] if not w.endswith(":") and (w.startswith(ROOT) or not os.path.isabs(w))]
    files = [f if os.path.isabs(f) else os.path.join(ROOT, f) for f in files]
    return [f for f in files if os.path.exists(f)] or all_deps


def _compile(unit: str) -> str:
    src = os.path.join(CSRC, unit)
    obj = os.path.join(OBJ, unit.replace(".hip", ".o"))
    log = obj + ".log"
    extra = os.environ.get("AMSM_EXTRA_FLAGS", "").split()  # (sanitizer / debug builds of the host side)
    cmd = ["hipcc", *FLAGS, *extra, "-MD", "-MF", obj[:-2] + ".d", "-c", src, "-o", obj]
    with open(log, "w") as lf:
        rc = subprocess.call(cmd, stdout=lf, stderr=subprocess.STDOUT)
    if rc != 0:
        sys.stderr.write(open(log).read()[-6000:])
        raise RuntimeError(f"hipcc failed on {unit} (log: {log})")
    return obj


def build_lib(force: bool = False, verbose: bool = True) -> str:
    os.makedirs(OBJ, exist_ok=True)
    deps = _deps()
    todo = [u for u in UNITS if force or _stale(os.path.join(OBJ, u.replace(".hip", ".o")), _unit_deps(u, deps))]
    if todo and verbose:
        print(f"[accumulation_amd.build] hipcc --offload-arch={ARCH}: {', '.join(todo)}", flush=True)
    with ThreadPoolExecutor(max_workers=8) as ex:  # one worker per unit
        list(ex.map(_compile, todo))
    objs = [os.path.join(OBJ, u.replace(".hip", ".o")) for u in UNITS]
    if todo or not os.path.exists(LIB):
        subprocess.check_call(["hipcc", "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", LIB, *objs])
    return LIB


# The field probe (tests/hip/field_probe.hip): a test-only device unit, NOT part of libamsm.so.  One source, one object per
# pack (-DPROBE_PACK=<id>) plus the dispatcher, compiled in parallel with the library's flags and linked next to the source.
PROBE_SRC = os.path.join(ROOT, "tests", "hip", "field_probe.hip")
PROBE_LIB = os.path.join(ROOT, "tests", "hip", "libfield_probe.so")
PROBE_OBJ = os.path.join(ROOT, "build", "obj", "probe")
PROBE_PACKS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22]  # field_probe.hip: PROBE_PACKS


def probe_stale() -> bool:
    return _stale(PROBE_LIB, [PROBE_SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC)])


def _compile_probe(pack) -> str:
    tag = "dispatch" if pack is None else f"pack{pack}"
    obj = os.path.join(PROBE_OBJ, f"field_probe_{tag}.o")
    log = obj + ".log"
    flags = [f for f in FLAGS if not f.startswith("-Rpass")]
    define = [] if pack is None else [f"-DPROBE_PACK={pack}"]
    cmd = ["hipcc", *flags, *define, "-I", CSRC, "-c", PROBE_SRC, "-o", obj]
    with open(log, "w") as lf:
        rc = subprocess.call(cmd, stdout=lf, stderr=subprocess.STDOUT)
    if rc != 0:
        sys.stderr.write(open(log).read()[-6000:])
        raise RuntimeError(f"hipcc failed on field_probe.hip ({tag}; log: {log})")
    return obj


def build_probe(force: bool = False, verbose: bool = True) -> str:
    """tests/hip/libfield_probe.so, rebuilt when it is missing or older than its source or anything under csrc/."""
    if not force and not probe_stale():
        return PROBE_LIB
    os.makedirs(PROBE_OBJ, exist_ok=True)
    if verbose:
        print(f"[accumulation_amd.build] hipcc --offload-arch={ARCH}: tests/hip/field_probe.hip ({len(PROBE_PACKS)} packs)", flush=True)
    jobs = min(16, os.cpu_count() or 1)
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        objs = list(ex.map(_compile_probe, [None] + PROBE_PACKS))
    subprocess.check_call(["hipcc", "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", PROBE_LIB, *objs])
    return PROBE_LIB


if __name__ == "__main__":
    if "--probe" in sys.argv:
        print(build_probe(force="--force" in sys.argv))
    else:
        print(build_lib(force="--force" in sys.argv))
