"""The allocation gate on the GPU: the out-of-memory sweep (tests/oom_sweep.py) over every family of entry points, one test per family
so that a failure names its family, and the memory limit.  Every refusal here is the gate's own (the test hook, or a limit below
1 GiB): nothing allocates against the real capacity of the device.  An iteration is one call of at most 2^17 + 64 pairs plus a trim.

A refusal is a return code.  A sweep that ends in anything else -- another status, a wrong point from the probe MSM, bytes still held
-- raises oom_sweep.Refused and nothing more runs on that context."""
import os
import subprocess
import sys

import numpy as np
import pytest

from accumulation_amd import CommitterKey, Context, VariableBaseMSM, ffi
from tests import oom_sweep as sw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20
K10, K12, K16, K17 = 0x6B10, 0x6B12, 0x6B16, 0x6B17  # key seeds
N17 = (1 << 17) + 64


class Env:
    def __init__(self):
        self.ctx = Context(ffi.AMSM_PALLAS)
        self.probe = sw.Probe(self.ctx)
        self._keys = {}

    def key(self, seed, n, flags):
        if seed not in self._keys:
            self._keys[seed] = CommitterKey.generate(self.ctx, seed, n, flags)
        return self._keys[seed]

    @property
    def k10(self):  # a small key with its direct-sum table
        return self.key(K10, 1 << 10, ffi.AMSM_BASES_DEFAULT)

    @property
    def k12(self):  # plain
        return self.key(K12, 1 << 12, ffi.AMSM_BASES_NO_PRECOMPUTE)

    @property
    def k16(self):  # precomputed, no direct-sum table at this size
        return self.key(K16, 1 << 16, ffi.AMSM_BASES_PRECOMPUTE)

    @property
    def k17(self):  # plain and long: the bucket-per-lane pipeline over a plain key
        return self.key(K17, N17, ffi.AMSM_BASES_NO_PRECOMPUTE)


@pytest.fixture(scope="module")
def env(built_lib, cref):
    e = Env()
    yield e
    e.ctx.close()


# ---- key creation --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [10, 16])
@pytest.mark.parametrize("creator", ["generate", "load_check", "sample", "from_device"])
def test_sweep_key_creation(env, creator, log_n):
    """2^10: window table, direct-sum table (tolerated: a key without one), scratch; 2^16: no direct-sum table.  amsm_bases_from_device
    makes a plain key unless told otherwise (its keys are the IPA's one-shot round keys): nothing optional there"""
    r = sw.key_family(env.ctx, env.probe, creator, 1 << log_n, abi_copy=(creator == "generate" and log_n == 10))
    assert r["oom"] >= 1, r
    if log_n == 10 and creator != "from_device":
        assert r["tolerated"] >= 1, r  # the direct-sum table (and the default key's window table) can be done without


def test_sweep_key_abi_copy_refused_is_a_null_pointer(env):
    """amsm_bases_device_ptr makes the key's C-ABI copy on first use, on the books of the context that holds the key's table: a
    refusal is a null pointer and nothing else -- the next call makes the copy"""
    from accumulation_amd.engine import _ptr
    import ctypes as C
    ctx, lib, n = env.ctx, env.ctx._lib, 1 << 10
    want = sw.key_points(ctx.curve, K10, n)
    refused = 0
    for k in range(sw.CAP):
        key = CommitterKey.generate(ctx, K10, n, ffi.AMSM_BASES_NO_PRECOMPUTE)
        held, before = ctx.memory_held()[0], ctx.alloc_stats()
        ctx.fail_alloc_after(k)
        p = lib.amsm_bases_device_ptr(key._h)
        ctx.fail_alloc_after(-1)
        fired = ctx.alloc_stats()[2] > before[2]
        if fired:
            refused += 1
            assert not p and ctx.memory_held()[0] == held and key.tables()["abi_copy"] == 0
            env.probe.run(f"amsm_bases_device_ptr, request {k}")
            p = lib.amsm_bases_device_ptr(key._h)
        assert p
        back = np.empty_like(want)
        ffi.check(lib.amsm_dev_download(ctx._h, _ptr(back), C.c_void_p(p), back.nbytes), "amsm_dev_download")
        assert np.array_equal(back, want)
        made = key.tables()["abi_copy"]
        assert ctx.memory_held()[0] == held + made  # the copy is on this context's books ...
        key.free()
        assert ctx.memory_held()[0] == held - n * 64  # ... and leaves them with the key
        if not fired:
            assert refused == (1 if made else 0), (refused, made)
            return
    raise AssertionError("still refusing")


def test_sweep_key_precompute_flag_is_an_error_where_default_degrades(env):
    assert sw.precompute_vs_default(env.ctx, env.probe)


def test_sweep_key_load_check_bls12_381(built_lib, cref):
    ctx = Context(ffi.AMSM_BLS12_381_G1)
    try:
        r = sw.key_family(ctx, sw.Probe(ctx, ffi.AMSM_BLS12_381_G1), "load_check", 1 << 10, curve=ffi.AMSM_BLS12_381_G1)
        assert r["oom"] >= 1, r
    finally:
        ctx.close()


def test_sweep_bases_fold(env):
    assert sw.fold_family(env.ctx, env.probe)["oom"] >= 1


def test_sweep_points_check(env):
    assert sw.points_check_family(env.ctx, env.probe)["oom"] >= 1


def test_sweep_matrix_load(env):
    assert sw.matrix_family(env.ctx, env.probe)["oom"] == 3  # three arrays, each refused once


# ---- MSM pipelines -------------------------------------------------------------------------------------------------------------
def test_sweep_msm_direct_sum(env):
    ctx = env.ctx
    assert env.k10.tables()["direct_sum_table"] > 0
    r = sw.msm_family(ctx, env.probe, env.k10, K10, 0xD1, 1 << 10, name="direct sum", counter=lambda: ctx.pipeline_stats()["direct_sum"])
    assert r["oom"] >= 1, r


def test_sweep_msm_chunked(env):
    assert sw.msm_family(env.ctx, env.probe, env.k12, K12, 0xD2, 1 << 12, name="chunked pipeline")["oom"] >= 1


def test_sweep_msm_bucket_split(env):
    ctx = env.ctx
    r = sw.msm_family(ctx, env.probe, env.k16, K16, 0xD3, 1 << 16, name="bucket-split pipeline",
                      counter=lambda: ctx.pipeline_stats()["bucket_split"])
    assert r["oom"] >= 1, r


def test_sweep_msm_unit_of_three(env):
    """three 2^16-pair vectors in one amsm_msm_batch_device run as ONE unit; a refusal inside the unit's plan is tolerated: AMSM_OK,
    the right points, and no unit counted for that call"""
    ctx, key, n = env.ctx, env.k16, 1 << 16
    vecs = [ctx.random_vector(0xBA7C + v, n, mont=False) for v in range(3)]
    want = [sw.msm_expected(ctx.curve, K16, n, 0, 0xBA7C + v, n) for v in range(3)]
    units = lambda: ctx.pipeline_stats()["bucket_split_units"]  # noqa: E731
    log = []

    def call():
        u0 = units()
        st, res = sw.status_of(lambda: VariableBaseMSM.multi_scalar_mul_batch(key, vecs, mont=False))
        log.append((st, units() - u0))
        return st, res

    def check(got, fired):
        xy, inf = got
        for v in range(3):
            assert sw.same_point((xy[v], inf[v]), want[v]), f"unit: MSM {v} differs from the oracle"
        log[-1] += (fired,)

    r = sw.sweep(ctx, env.probe, call, check, name="unit of three bucket-split MSMs")
    assert r["oom"] >= 1, r
    ok = [e for e in log if e[0] == ffi.AMSM_OK]
    assert ok[-1][1] == 1 and not ok[-1][2], log  # the clean call: one unit
    assert any(e[2] and e[1] == 0 for e in ok), f"no tolerated refusal ran the unit's MSMs singly: {log}"


def test_sweep_msm_bucket_per_lane_plain(env):
    ctx = env.ctx
    r = sw.msm_family(ctx, env.probe, env.k17, K17, 0xD4, N17, name="bucket-per-lane over a plain key",
                      counter=lambda: ctx.pipeline_stats()["bucket_per_lane"])
    assert r["oom"] >= 1, r


def test_sweep_msm_two_valued(env):
    assert sw.two_valued_family(env.ctx, env.probe, env.k16, K16)["oom"] >= 1


def test_sweep_msm_grouped(env):
    assert sw.grouped_family(env.ctx, env.probe, env.k16, K16, 1 << 16, 15)["oom"] >= 1


def test_sweep_msm_host_slices(env):
    assert sw.host_msm_family(env.ctx, env.probe, env.k12, K12)["oom"] >= 1


def test_sweep_msm_oneshot(env):
    assert sw.oneshot_family(env.ctx, env.probe)["oom"] >= 1


def test_sweep_msm_multi_mid_batch(env):
    """four different-length MSMs: the later jobs ask for more than the earlier ones left, so a refusal finds MSMs in flight"""
    r = sw.multi_family(env.ctx, env.probe, env.k16, K16, [1 << 12, 1 << 14, 1 << 16, 3 << 14], name="amsm_msm_multi_device")
    assert r["oom"] >= 3, r


# ---- the schemes' entry points -------------------------------------------------------------------------------------------------
def test_sweep_ipa_round_fused(env):
    assert sw.ipa_round_family(env.ctx, env.probe, env.k16, 16, 1)["oom"] >= 1


def test_sweep_ipa_jump_fold(env):
    assert sw.jump_fold_family(env.ctx, env.probe, env.k16, 16, 10)["oom"] >= 1


def test_jump_fold_with_too_many_bucket_sets_is_unsupported(env):
    """(log_key 16, j 1): 2 * 2^15 bucket sets would be the reduction's gridDim.y -- past HIP's 65535.  AMSM_E_UNSUPPORTED, decided before
    any allocation: the drivers keep such rounds on the device"""
    from accumulation_amd.engine import _ptr
    from accumulation_amd.scalar_field import Fr
    ctx = env.ctx
    xi = np.ascontiguousarray(Fr(ctx.curve).to_limbs(0x77AA55), dtype=np.uint64).reshape(1, 4)
    xy = np.zeros((1 << 15, 2 * ctx.fq_limbs), dtype=np.uint64)
    inf = np.zeros(1 << 15, dtype=np.uint8)
    before = ctx.alloc_stats()
    assert ctx._lib.amsm_ipa_jump_fold(ctx._h, env.k16._h, 16, _ptr(xi), 1, _ptr(xy), _ptr(inf)) == ffi.AMSM_E_UNSUPPORTED
    assert ctx.alloc_stats() == before
    env.probe.run("jump fold (16, 1)")


# ---- vector and polynomial entry points ----------------------------------------------------------------------------------------
def test_sweep_hp_t_vecs(env):
    assert sw.t_vecs_family(env.ctx, env.probe)["oom"] >= 1


def test_sweep_poly_div_and_evaluate(env):
    r = sw.poly_family(env.ctx, env.probe)
    assert r["div"]["oom"] >= 1 and r["eval"]["oom"] >= 1, r


def test_sweep_dev_alloc(env):
    assert sw.dev_alloc_family(env.ctx, env.probe)["oom"] == 1


# ---- a driver ------------------------------------------------------------------------------------------------------------------
def test_sweep_hp_as_prove(env):
    assert sw.hp_prove_family(env.ctx, env.probe)["oom"] >= 1


# ---- the limit -----------------------------------------------------------------------------------------------------------------
def test_limit_refuses_an_msm_and_raising_it_gives_the_exact_result(built_lib, cref):
    ctx = Context(ffi.AMSM_PALLAS)
    try:
        n = 1 << 16
        key = CommitterKey.generate(ctx, K16, n, ffi.AMSM_BASES_PRECOMPUTE)
        vec = ctx.random_vector(0xD3, n, mont=False)
        ctx.trim()
        held = ctx.memory_held()[0]
        limit = held + MIB
        ctx.set_memory_limit(limit)
        with pytest.raises(ffi.AmsmError) as e:
            VariableBaseMSM.multi_scalar_mul(key, vec, mont=False)
        assert e.value.status == ffi.AMSM_E_OOM
        h = ctx.memory_held()
        assert h[2] == limit and h[1] <= limit and h[0] <= limit, h
        assert ctx.alloc_stats()[1] >= 1 and ctx.alloc_stats()[3] == 0
        ctx.set_memory_limit(0)
        assert sw.same_point(VariableBaseMSM.multi_scalar_mul(key, vec, mont=False), sw.msm_expected(ctx.curve, K16, n, 0, 0xD3, n))
    finally:
        ctx.close()


def test_limit_denies_the_direct_sum_table_and_says_so(built_lib, cref):
    ctx = Context(ffi.AMSM_PALLAS)
    try:
        n = 1 << 10  # direct-sum table: 512 points per generator = 32 MiB; the window table and its scratch fit in 16 MiB
        ctx.set_memory_limit(ctx.memory_held()[0] + 16 * MIB)
        denied = ctx.tables_denied()
        key = CommitterKey.generate(ctx, K10, n)
        t = key.tables()
        assert key.precomputed and t["direct_sum_table"] == 0 and t["direct_sum_table_denied"] == "allocation failed", t
        assert ctx.tables_denied() == denied + 1
        assert ctx.memory_held()[1] <= ctx.memory_held()[2]
        vec = ctx.random_vector(0xD1, n, mont=False)
        assert sw.same_point(VariableBaseMSM.multi_scalar_mul(key, vec, mont=False), sw.msm_expected(ctx.curve, K10, n, 0, 0xD1, n))
    finally:
        ctx.close()


def test_limit_from_the_environment_is_read_at_creation(built_lib):
    code = ("from accumulation_amd import Context, ffi\n"
            "ctx = Context(ffi.AMSM_PALLAS)\n"
            "assert ctx.memory_held()[2] == 8 << 20, ctx.memory_held()\n"
            "try:\n"
            "    ctx.vector(1 << 19)\n"  # 16 MiB
            "    raise SystemExit('not refused')\n"
            "except ffi.AmsmError as e:\n"
            "    assert e.status == ffi.AMSM_E_OOM\n"
            "ctx.vector(1 << 10)\n"
            "assert ctx.alloc_stats()[1] == 1\n"
            "from accumulation_amd import MultiContext\n"  # a multi-device context ignores the variable (no limit it could not change)
            "m = MultiContext(ffi.AMSM_PALLAS, devices=(0, 0))\n"
            "assert m.memory_held()[2] == 0 and m.shard(1).memory_held()[2] == 0\n"
            "print('limit ok')\n")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, AMSM_MEM_LIMIT_MB="8"),
                       timeout=120)
    assert p.returncode == 0 and "limit ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-2000:])


def test_a_key_outlives_its_context(built_lib, cref):
    """a GPU context destroyed before a key it made: the key still serves another context on the device, stays off that context's
    books, and its later free is a plain free"""
    maker, user = Context(ffi.AMSM_PALLAS), Context(ffi.AMSM_PALLAS)
    try:
        n = 1 << 10
        key = CommitterKey.generate(maker, K10, n)
        assert maker.memory_held()[0] >= key.tables()["window_table"] + key.tables()["direct_sum_table"] > 0
        h, key._h = key._h, None
        maker.close()
        borrowed = CommitterKey(user, h)
        vec = user.random_vector(0xD1, n, mont=False)
        user.trim()
        held = user.memory_held()[0]
        assert sw.same_point(VariableBaseMSM.multi_scalar_mul(borrowed, vec, mont=False), sw.msm_expected(user.curve, K10, n, 0, 0xD1, n))
        user.trim()
        borrowed.free()
        assert user.memory_held()[0] == held
    finally:
        user.close()


def test_multi_device_context_refuses_the_setters(built_lib):
    from accumulation_amd import MultiContext
    ctx = MultiContext(ffi.AMSM_PALLAS, devices=(0, 0))
    try:
        assert ctx._lib.amsm_ctx_set_memory_limit(ctx._h, 1 << 30) == ffi.AMSM_E_UNSUPPORTED
        assert ctx._lib.amsm_ctx_fail_alloc_after(ctx._h, 0) == ffi.AMSM_E_UNSUPPORTED
        assert len(ctx.memory_held()) == 4 and len(ctx.alloc_stats()) == 4
    finally:
        ctx.close()
