"""Loader and launcher of the field probe (tests/hip/field_probe.hip -> tests/hip/libfield_probe.so)."""
import ctypes
import os

import numpy as np

from tests import field_model as fm


def load():
    """Build the probe if it is missing or stale, then load it.  AMSM_FIELD_PROBE_LIB names another build of it (a probe compiled
    against a deliberately broken copy of csrc/, to see the tests fail)."""
    from accumulation_amd import build
    path = os.environ.get("AMSM_FIELD_PROBE_LIB") or build.build_probe(verbose=False)
    lib = ctypes.CDLL(path)
    lib.field_probe_run.restype = ctypes.c_int
    lib.field_probe_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    lib.field_probe_op_count.restype = ctypes.c_int
    assert lib.field_probe_op_count() == len(fm.OPS)
    return lib


def run(lib, pid, op, cases, replicate=1):
    """cases: per case a list of up to N_IN operands (lists of words) -> uint32 array (len(cases), replicate, N_OUT, STRIDE).
    The launch is padded to whole quads with copies of case 0."""
    n = len(cases) * replicate
    n_pad = (n + 3) & ~3
    buf = np.zeros((n_pad, fm.N_IN, fm.STRIDE), dtype=np.uint32)
    for i, ins in enumerate(cases):
        assert len(ins) <= fm.N_IN
        for j, a in enumerate(ins):
            assert len(a) <= fm.STRIDE
            buf[i * replicate:(i + 1) * replicate, j, :len(a)] = np.array(a, dtype=np.uint64).astype(np.uint32)
    buf[n:] = buf[0]
    out = np.zeros((n_pad, fm.N_OUT, fm.STRIDE), dtype=np.uint32)
    rc = lib.field_probe_run(pid, fm.OP_ID[op], buf.ctypes.data, out.ctypes.data, n_pad)
    assert rc == 0, f"field_probe_run(pack {pid}, {op}) returned HIP status {rc}"
    return out[:n].reshape(len(cases), replicate, fm.N_OUT, fm.STRIDE)
