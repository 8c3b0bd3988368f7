"""The allocation gate on the HOST backend (no GPU needed): the memory limit, the books, and the out-of-memory sweep
(tests/oom_sweep.py) over every family whose memory passes the gate there -- keys, vectors, matrices (cpu::h_alloc before the gate).
The host backend's MSMs and scheme entry points compute in std::vector scratch that the gate does not cover (include/amsm.h): their
sweeps make no request of their own, so they only show that an armed hook harms nothing (require_oom off, said where it is)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from accumulation_amd import CommitterKey, Context, ffi
from tests import oom_sweep as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20


@pytest.fixture(scope="module")
def env(built_lib, cref):
    ctx = Context(ffi.AMSM_PALLAS, device=ffi.AMSM_DEVICE_HOST)
    yield ctx, sw.Probe(ctx)
    ctx.close()


# ---- the four entry points -----------------------------------------------------------------------------------------------------
def test_books_follow_keys_vectors_and_matrices(built_lib):
    ctx = Context(ffi.AMSM_PALLAS, device=ffi.AMSM_DEVICE_HOST)
    assert ctx.memory_held() == (0, 0, 0, 0) and ctx.alloc_stats() == (0, 0, 0, 0)
    key = CommitterKey.generate(ctx, 1, 1 << 10)
    assert ctx.memory_held()[0] == (1 << 10) * 64  # 2^10 affine Pallas points
    v = ctx.vector(1000)
    held = ctx.memory_held()
    assert held[0] == (1 << 10) * 64 + 32000 and held[1] == held[0] and ctx.alloc_stats() == (2, 0, 0, 0)
    key.free()  # amsm_bases_free takes no context: the owner is credited all the same
    assert ctx.memory_held()[0] == 32000 and ctx.memory_held()[1] == held[1]
    v.free()
    ctx.trim()
    assert ctx.memory_held()[0] == 0
    ctx.close()


def test_a_key_outlives_its_context(built_lib):
    """a key stays on the books of the context that made it -- not on those of the context that uses it --, and a context destroyed
    first is forgotten: the later free is a plain free that touches nobody's books"""
    maker = Context(ffi.AMSM_PALLAS, device=ffi.AMSM_DEVICE_HOST)
    user = Context(ffi.AMSM_PALLAS, device=ffi.AMSM_DEVICE_HOST)
    key = CommitterKey.generate(maker, 1, 64)
    assert maker.memory_held()[0] == 64 * 64 and user.memory_held()[0] == 0
    want = key.read()[0]
    h, key._h = key._h, None
    lib = maker._lib
    maker.close()
    back = np.empty_like(want)
    inf = np.empty(64, dtype=np.uint8)
    from accumulation_amd.engine import _ptr
    assert lib.amsm_bases_read(user._h, h, 0, 64, _ptr(back), _ptr(inf)) == ffi.AMSM_OK and np.array_equal(back, want)
    before = (user.memory_held(), user.alloc_stats())
    lib.amsm_bases_free(h)
    assert (user.memory_held(), user.alloc_stats()) == before
    user.close()


def test_hook_refuses_exactly_one_request(env):
    ctx, _ = env
    ctx.trim()
    ctx.fail_alloc_after(1)
    a = ctx.vector(10)
    with pytest.raises(ffi.AmsmError) as e:
        ctx.vector(11)
    assert e.value.status == ffi.AMSM_E_OOM
    b = ctx.vector(11)  # once
    s0 = ctx.alloc_stats()
    ctx.fail_alloc_after(0)
    ctx.fail_alloc_after(-1)  # disarmed
    c = ctx.vector(12)
    assert ctx.alloc_stats()[2] == s0[2]
    for v in (a, b, c):
        v.free()


def test_null_and_multi_device_arguments(built_lib):
    lib = built_lib
    assert lib.amsm_ctx_set_memory_limit(None, 0) == ffi.AMSM_E_INVALID_ARG
    assert lib.amsm_ctx_fail_alloc_after(None, 0) == ffi.AMSM_E_INVALID_ARG
    assert lib.amsm_ctx_memory_held(None, None) == ffi.AMSM_E_INVALID_ARG
    assert lib.amsm_ctx_alloc_stats(None, None) == ffi.AMSM_E_INVALID_ARG


# ---- the limit -----------------------------------------------------------------------------------------------------------------
def test_limit_refuses_then_raising_it_gives_the_same_result(built_lib, cref):
    ctx = Context(ffi.AMSM_PALLAS, device=ffi.AMSM_DEVICE_HOST)
    keep = ctx.vector(1000)
    held = ctx.memory_held()[0]
    ctx.set_memory_limit(held + MIB)
    assert ctx.memory_held()[2] == held + MIB
    with pytest.raises(ffi.AmsmError) as e:
        CommitterKey.generate(ctx, 7, 1 << 15)  # 2 MiB of points
    assert e.value.status == ffi.AMSM_E_OOM
    assert ctx.alloc_stats()[1] == 1 and ctx.memory_held()[0] == held
    small = CommitterKey.generate(ctx, 7, 1 << 10)  # 64 KiB: fits
    assert ctx.memory_held()[1] <= held + MIB
    small.free()
    ctx.set_memory_limit(0)
    key = CommitterKey.generate(ctx, 7, 1 << 15)
    assert np.array_equal(key.read()[0], cref.rng_points(ffi.AMSM_PALLAS, 7, 1 << 15))
    keep.free()
    ctx.close()


def test_limit_from_the_environment_is_read_at_creation(built_lib):
    code = ("from accumulation_amd import Context, ffi\n"
            "ctx = Context(ffi.AMSM_PALLAS, device=ffi.AMSM_DEVICE_HOST)\n"
            "assert ctx.memory_held()[2] == 3 << 20, ctx.memory_held()\n"
            "try:\n"
            "    ctx.vector(1 << 17)\n"  # 4 MiB
            "    raise SystemExit('not refused')\n"
            "except ffi.AmsmError as e:\n"
            "    assert e.status == ffi.AMSM_E_OOM\n"
            "ctx.vector(1 << 10)\n"
            "print('limit ok')\n")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, AMSM_MEM_LIMIT_MB="3"),
                       timeout=120)
    assert p.returncode == 0 and "limit ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-2000:])


# ---- the sweep -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("creator", ["generate", "load_check", "sample", "from_device"])
def test_sweep_key_creation(env, creator):
    ctx, probe = env
    r = sw.key_family(ctx, probe, creator, 1 << 10)
    assert r["oom"] >= 1, r


def test_sweep_key_load_check_bls12_381(built_lib, cref):
    ctx = Context(ffi.AMSM_BLS12_381_G1, device=ffi.AMSM_DEVICE_HOST)
    try:
        r = sw.key_family(ctx, sw.Probe(ctx, ffi.AMSM_BLS12_381_G1), "load_check", 1 << 8, curve=ffi.AMSM_BLS12_381_G1)
        assert r["oom"] >= 1, r
    finally:
        ctx.close()


def test_sweep_bases_fold(env):
    assert sw.fold_family(*env)["oom"] >= 1


def test_sweep_points_check_makes_no_request_on_the_host(env):
    ctx, probe = env
    xy = sw.key_points(ctx.curve, 0xC4EC, 1 << 10)
    s0 = ctx.alloc_stats()
    ctx.fail_alloc_after(0)
    assert ctx.check_points(xy)["first_bad"] == 1 << 10
    ctx.fail_alloc_after(-1)
    assert ctx.alloc_stats() == s0  # (the host check works in place: nothing to refuse)


def test_sweep_matrix_load(env):
    r = sw.matrix_family(*env)
    assert r["oom"] == 3, r  # the three arrays, each refused once; the earlier ones are given back


def test_sweep_dev_alloc(env):
    assert sw.dev_alloc_family(*env)["oom"] == 1


def test_sweep_hp_t_vecs(env):
    assert sw.t_vecs_family(*env)["oom"] >= 1  # (the output vectors: amsm_dev_alloc)


def test_sweep_poly(env):
    r = sw.poly_family(*env, require_oom_eval=False)
    assert r["div"]["oom"] >= 1  # (the quotients: amsm_dev_alloc); the evaluation allocates nothing on the host
    assert r["eval"]["iterations"] >= 1


def test_sweep_msm_and_oneshot(env):
    """the host MSM's scratch is not gated; amsm_msm_oneshot makes its temporary key through the gate"""
    ctx, probe = env
    r = sw.oneshot_family(ctx, probe, 1 << 10)
    assert r["oom"] == 1, r


def test_sweep_scheme_entry_points(env):
    """amsm_ipa_round_fused / amsm_ipa_jump_fold on the host backend work in ungated scratch: the armed hook must harm nothing
    (the results equal a clean run's, d_coeffs / d_z included)"""
    ctx, probe = env
    key = CommitterKey.generate(ctx, 0x1A00, 1 << 12)
    sw.ipa_round_family(ctx, probe, key, log_key=12, j=1)
    sw.jump_fold_family(ctx, probe, key, log_key=12, j=6)


def test_sweep_hp_as_prove(env):
    r = sw.hp_prove_family(*env)
    assert r["oom"] >= 1, r
