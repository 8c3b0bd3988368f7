"""The three forms of an MSM's tail (csrc/msm_select.h: tail_plan; kernels k_bucket_reduce<QUAD, FUSED> / k_fold<QUAD>) that no other
GPU test pins down by name -- the row / column form, the direct sum's fold, the two-valued sums and the jump fold are reached by
test_bpl_gpu.py, test_direct_sum_gpu.py, test_two_valued_gpu.py and test_ipa_jump_gpu.py:
  (a) fused_quad with ONE partial record per set (the first quad folds serially): a plain key, 2^10 pairs, a blocking call --
      8-bit windows, 32 sets of 128 buckets, one workgroup per set
  (b) fused_quad with more than four records per set (the workgroup tree): a precomputed key of 2^15 generators without the
      direct-sum table, 2^12 pairs, blocking -- 13-bit windows, one set of 4096 buckets, 16 records (a key of 2^12 generators has 8-bit
      windows and ONE record per set: the CPU table, tests/test_pipeline_select_cpu.py::test_tail_plan_of_the_gpu_shapes, names these
      shapes); Pallas and BLS12-381 (12-word records: other LDS sizes)
  (c) one_lane: a device batch of two MSMs of 2^17 + 64 pairs over a plain key -- 15-bit windows, 19 sets of 2^14 buckets > 2^17 in
      all, so the first MSM's hidden tail runs on the one-lane kernels and the second's, which the caller waits for, on the fused one
One child process runs them with AMSM_DEBUG=1 (the library names each tail's form on stderr); every result equals oracle/ark_msm.c
bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyref as o

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_C = (1 << 17) + 64


@pytest.fixture(scope="module")
def child(cref, tmp_path_factory):
    d = tmp_path_factory.mktemp("tail_forms")
    data = {}
    for c, tag, n in ((o.PALLAS, "pallas", N_C), (o.BLS12_381_G1, "bls12_381", 1 << 15)):
        data[tag + "_xy"] = cref.rng_points(c.curve_id, 0x7A11, n, threads=16)
        data[tag + "_frs"] = np.stack([cref.rng_frs(c.curve_id, 0x7A20 + j, n if tag == "pallas" else 1 << 12) for j in range(2)])
    inputs, results = str(d / "inputs.npz"), str(d / "results.npz")
    np.savez(inputs, **data)
    env = dict(os.environ, AMSM_DEBUG="1")
    run = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tests", "tail_forms_child.py"), inputs, results],
                         cwd=ROOT, env=env, capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr[-3000:])
    forms, case = {}, None
    for ln in run.stderr.splitlines():
        if ln.startswith("== "):
            case = ln[3:]
            forms[case] = []
        elif case and ln.startswith("[amsm] tail "):
            w = ln.split()
            forms[case].append(w[2])
            assert w[-1] == "success" or "no error" in ln, ln  # (hipGetErrorString(hipSuccess))
    return data, dict(np.load(results)), forms


def same(cref, c, got_xy, got_inf, xy, frs):
    ref, rinf = cref.msm(c.curve_id, xy, frs, threads=16)
    return bool(got_inf) == bool(rinf) and np.array_equal(got_xy, ref)


def test_fused_quad_one_record_per_set(cref, child):
    data, res, forms = child
    assert forms["a"] == ["fused_quad"]
    assert same(cref, o.PALLAS, res["a_xy"][0], res["a_inf"][0], data["pallas_xy"][:1 << 10], data["pallas_frs"][0, :1 << 10])


@pytest.mark.parametrize("c,tag", [(o.PALLAS, "pallas"), (o.BLS12_381_G1, "bls12_381")], ids=["pallas", "bls12_381"])
def test_fused_quad_workgroup_tree(cref, child, c, tag):
    data, res, forms = child
    assert forms["b_" + tag] == ["fused_quad"]
    assert same(cref, c, res["b_%s_xy" % tag][0], res["b_%s_inf" % tag][0], data[tag + "_xy"][:1 << 12], data[tag + "_frs"][0, :1 << 12])


def test_one_lane_hidden_tail_then_fused_quad(cref, child):
    data, res, forms = child
    assert forms["c"] == ["one_lane", "fused_quad"]
    for j in range(2):
        assert same(cref, o.PALLAS, res["c_xy"][j], res["c_inf"][j], data["pallas_xy"], data["pallas_frs"][j]), j
