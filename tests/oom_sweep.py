"""The out-of-memory sweep (include/amsm.h: "the contract after AMSM_E_OOM") and the families it is run over.

sweep(ctx, probe, call, check) runs, for k = 0, 1, 2, ...: trim, fail_alloc_after(k), the call, alloc_stats -- the k-th allocation
request of the call is refused by the gate's test hook, so every allocation of the call fails exactly once, one per iteration:
  * refused and AMSM_E_OOM: no handle, memory_held after a trim as before the call, and a probe MSM on the same context (64 pairs over
    a 64-generator key made beforehand) gives AMSM_OK and the known point;
  * refused and AMSM_OK (the call can do without that buffer): the result is checked like a clean one;
  * not refused: the result is checked and the sweep ends.
Any other status fails at once; so does the 200th iteration.

The families below are written once for both backends (a GPU context, a host-backend context): tests/test_oom_gpu.py and
tests/test_oom_host_cpu.py choose.  Expected values come from oracle/cref (cref.msm over cref.rng_points / the downloaded scalars),
computed once per shape and shared; the scheme entry points without an oracle form are compared bit for bit with a clean run of the
same call on the same context (point 4 of the contract).
"""
import ctypes as C
import functools

import numpy as np

from accumulation_amd import CommitterKey, Context, PedersenCommitment, VariableBaseMSM, ffi
from accumulation_amd.engine import PointVector, _ptr
from oracle import cref

CURVE = ffi.AMSM_PALLAS
CAP = 200
SENTINEL = 0x5E7712E15E7712E0  # what *out holds before a creator is called


class Refused(Exception):
    """a sweep found something other than AMSM_OK / AMSM_E_OOM, or broke the contract: nothing more runs on that context"""


def stop_if_device_error(status, where):
    """AMSM_E_HIP on a GPU context may be a device fault: the whole session ends there -- no later test starts anything on that device"""
    if status == ffi.AMSM_E_HIP:
        import pytest
        pytest.exit(f"{where}: AMSM_E_HIP -- a finding about the cleanup path; nothing more is run", returncode=3)


# ---- oracle values, computed once --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def key_points(curve, seed, n):
    """the generators of amsm_bases_generate(seed, n) by the oracle's own derivation"""
    return cref.rng_points(curve, seed, n)


@functools.lru_cache(maxsize=None)
def scalars(curve, seed, n):
    """the canonical scalars of amsm_vec_random(seed, n, mont = 0)"""
    return cref.rng_frs(curve, seed, n)


@functools.lru_cache(maxsize=None)
def msm_expected(curve, key_seed, key_n, off, scalar_seed, n):
    xy, inf = cref.msm(curve, key_points(curve, key_seed, key_n)[off:off + n], scalars(curve, scalar_seed, n))
    return xy.copy(), bool(inf)


def same_point(got, want):
    (gxy, ginf), (wxy, winf) = got, want
    return bool(ginf) == bool(winf) and (bool(winf) or np.array_equal(np.asarray(gxy).reshape(-1), np.asarray(wxy).reshape(-1)))


# ---- the probe ---------------------------------------------------------------------------------------------------------------
class Probe:
    """a 64-pair MSM over a 64-generator key, both made before any sweep: the context still works"""

    def __init__(self, ctx, curve=CURVE):
        self.ctx = ctx
        self.key = CommitterKey.generate(ctx, 0x9B0BE, 64)
        self.vec = ctx.random_vector(0x9B0BF, 64, mont=False)
        self.want = msm_expected(curve, 0x9B0BE, 64, 0, 0x9B0BF, 64)

    def run(self, where):
        try:
            got = VariableBaseMSM.multi_scalar_mul(self.key, self.vec, mont=False)
        except ffi.AmsmError as e:
            stop_if_device_error(e.status, where + " (probe)")
            raise Refused(f"{where}: the probe MSM returned {e.status} -- the context is not reusable") from e
        if not same_point(got, self.want):
            raise Refused(f"{where}: the probe MSM gave a wrong point")


def status_of(fn):
    """(status, result) of a call through the Python wrappers"""
    try:
        return ffi.AMSM_OK, fn()
    except ffi.AmsmError as e:
        return e.status, None


def sweep(ctx, probe, call, check, *, name, require_oom=True, after_oom=None, release=None):
    """call() -> (status, result); check(result, fired) asserts a result that came with AMSM_OK; release(result) gives back what an
    AMSM_OK call produced (a handle), so that the next iteration starts from the same books; after_oom(k): further checks behind a
    refusal (point 3 of the contract).  Returns {"oom": .., "tolerated": .., "iterations": ..}."""
    n_oom = n_tolerated = 0
    for k in range(CAP):
        ctx.trim()
        held = ctx.memory_held()[0]
        before = ctx.alloc_stats()
        ctx.fail_alloc_after(k)
        status, result = call()
        ctx.fail_alloc_after(-1)
        after = ctx.alloc_stats()
        fired = after[2] > before[2]
        where = f"{name}, request {k}"
        if status not in (ffi.AMSM_OK, ffi.AMSM_E_OOM):
            stop_if_device_error(status, where)
            raise Refused(f"{where}: status {status} ({ffi.load().amsm_strerror(status).decode()})")
        if after[1] != before[1] or after[3] != before[3]:
            raise Refused(f"{where}: a refusal that was not the hook's (alloc_stats {before} -> {after})")
        if status == ffi.AMSM_E_OOM:
            if not fired:
                raise Refused(f"{where}: AMSM_E_OOM without a refused request")
            if result is not None:
                raise Refused(f"{where}: AMSM_E_OOM and a result")
            n_oom += 1
            ctx.trim()
            now = ctx.memory_held()[0]
            if now != held:
                raise Refused(f"{where}: {now - held} bytes still held after AMSM_E_OOM and a trim")
            if after_oom:
                after_oom(k)
            probe.run(where)
            continue
        try:
            check(result, fired)
        finally:
            if release:
                release(result)
        if not fired:
            assert after[0] - before[0] <= k, (where, before, after)  # the call made fewer requests than the countdown
            if require_oom and not n_oom:
                raise Refused(f"{name}: no iteration returned AMSM_E_OOM -- the hook reaches no required allocation of this call")
            probe.run(where)
            return {"oom": n_oom, "tolerated": n_tolerated, "iterations": k + 1}
        n_tolerated += 1
    raise Refused(f"{name}: still refusing after {CAP} iterations")


# ---- key creation ------------------------------------------------------------------------------------------------------------
def _creator_call(lib, fn):
    """a creator through the raw ABI with *out holding a sentinel: (status, handle or None), the sentinel checked behind a failure"""
    h = C.c_void_p(SENTINEL)
    rc = fn(C.byref(h))
    if rc != ffi.AMSM_OK:
        if h.value != SENTINEL:
            raise Refused(f"a failing creator (status {rc}) wrote *out")
        return rc, None
    assert h.value not in (None, SENTINEL)
    return rc, h


def key_family(ctx, probe, creator, n, *, curve=CURVE, flags=ffi.AMSM_BASES_DEFAULT, name=None, abi_copy=False):
    """creator: "generate" | "load_check" | "sample" | "from_device".  A key that comes to be is read back, compared with the oracle's
    points and used for one MSM (which pipeline it takes depends on the tables it got -- the tolerated refusals)."""
    lib = ctx._lib
    seed = 0x6E11 + n
    L2 = 2 * ctx.fq_limbs
    want_xy = key_points(curve, seed, n) if creator != "sample" else None
    src = None
    if creator == "from_device":
        src = PointVector(ctx, n)
        ffi.check(lib.amsm_dev_upload(ctx._h, src.ptr, _ptr(want_xy), want_xy.nbytes), "amsm_dev_upload")
    if creator == "sample":  # (no independent derivation of the sampled points here: a clean key is the reference)
        ref = CommitterKey.sample(ctx, b"oom-sweep", n, flags)
        want_xy = ref.read()[0]
        ref.free()
    m = min(n, 1 << 10)
    vec = ctx.random_vector(0x5CA1 + n, m, mont=False)
    want_msm = cref.msm(curve, want_xy[:m], scalars(curve, 0x5CA1 + n, m))

    def call():
        if creator == "generate":
            return _creator_call(lib, lambda out: lib.amsm_bases_generate(ctx._h, seed, n, flags, out))
        if creator == "load_check":
            return _creator_call(lib, lambda out: lib.amsm_bases_load(ctx._h, _ptr(want_xy), None, n, flags | ffi.AMSM_BASES_CHECK, out))
        if creator == "sample":
            return _creator_call(lib, lambda out: lib.amsm_bases_sample(ctx._h, b"oom-sweep", 9, 0, n, flags, out))
        return _creator_call(lib, lambda out: lib.amsm_bases_from_device(ctx._h, src.ptr, n, flags | ffi.AMSM_BASES_CHECK, out))

    def check(h, fired):
        key = CommitterKey(ctx, h)
        try:
            got_xy, got_inf = key.read()
            assert not got_inf.any() and np.array_equal(got_xy, want_xy), f"{creator} {n}: the key's points differ from the oracle's"
            assert same_point(VariableBaseMSM.multi_scalar_mul(key, vec, mont=False), want_msm), f"{creator} {n}: MSM over the new key"
            if abi_copy and not ctx.is_host:  # the C-ABI copy: tolerated, a refusal is a null pointer and nothing else
                p = lib.amsm_bases_device_ptr(key._h)
                if p:
                    back = np.empty((n, L2), dtype=np.uint64)
                    ffi.check(lib.amsm_dev_download(ctx._h, _ptr(back), C.c_void_p(p), back.nbytes), "amsm_dev_download")
                    assert np.array_equal(back, want_xy)
                else:
                    assert fired, "amsm_bases_device_ptr returned NULL without a refusal"
        finally:
            key._h = None  # (released by the sweep)

    def release(h):
        lib.amsm_bases_free(h)

    return sweep(ctx, probe, call, check, name=name or f"amsm_bases_{creator} 2^{n.bit_length() - 1}", release=release)


def precompute_vs_default(ctx, probe, n=1 << 10):
    """AMSM_BASES_PRECOMPUTE must give AMSM_E_OOM where AMSM_BASES_DEFAULT gives a plain key: the request the default key tolerates
    (its window table) is found by the sweep, then the same countdown is run with the explicit flag."""
    lib = ctx._lib
    seed = 0x6E11 + n
    plain_at, k_seen = [], []

    def call_counting():
        k_seen.append(len(k_seen))  # (the sweep's k: one call per iteration)
        return _creator_call(lib, lambda out: lib.amsm_bases_generate(ctx._h, seed, n, ffi.AMSM_BASES_DEFAULT, out))

    def check_k(h, fired):
        if fired and not lib.amsm_bases_precomputed(h):
            plain_at.append(k_seen[-1])

    sweep(ctx, probe, call_counting, check_k, name="amsm_bases_generate DEFAULT", release=lambda h: lib.amsm_bases_free(h))
    assert plain_at, "no refusal left AMSM_BASES_DEFAULT with a plain key"
    for k in plain_at:
        ctx.trim()
        ctx.fail_alloc_after(k)
        rc, h = _creator_call(lib, lambda out: lib.amsm_bases_generate(ctx._h, seed, n, ffi.AMSM_BASES_PRECOMPUTE, out))
        ctx.fail_alloc_after(-1)
        assert rc == ffi.AMSM_E_OOM and h is None, f"AMSM_BASES_PRECOMPUTE with request {k} refused: status {rc}"
        probe.run(f"AMSM_BASES_PRECOMPUTE, request {k}")
    return plain_at


def fold_family(ctx, probe, n_half=1 << 10):
    from accumulation_amd.scalar_field import Fr
    lib = ctx._lib
    fr = Fr(ctx.curve)
    seed = 0xF01D
    key = CommitterKey.generate(ctx, seed, 2 * n_half, ffi.AMSM_BASES_NO_PRECOMPUTE)
    x = 0xDEADBEEF12345
    xl = np.ascontiguousarray(fr.to_limbs(x), dtype=np.uint64)
    pts = key_points(ctx.curve, seed, 2 * n_half)
    want = cref.points_fold(ctx.curve, pts[:n_half], pts[n_half:], x)

    def call():
        return _creator_call(lib, lambda out: lib.amsm_bases_fold(ctx._h, key._h, n_half, _ptr(xl), 64, out))

    def check(h, fired):
        k2 = CommitterKey(ctx, h)
        try:
            assert np.array_equal(k2.read()[0], want), "folded key differs from the oracle's fold"
        finally:
            k2._h = None

    return sweep(ctx, probe, call, check, name="amsm_bases_fold", release=lambda h: lib.amsm_bases_free(h))


def points_check_family(ctx, probe, n=1 << 10):
    xy = key_points(ctx.curve, 0xC4EC, n).copy()
    xy[n // 3, 0] ^= 1  # one point off the curve (or non-canonical): the report must name it

    def check(rep, fired):
        assert rep["first_bad"] == n // 3 and rep["non_canonical"] + rep["off_curve"] + rep["off_subgroup"] == 1, rep

    return sweep(ctx, probe, lambda: status_of(lambda: ctx.check_points(xy)), check, name="amsm_points_check")


def matrix_family(ctx, probe, n_rows=1 << 10):
    from accumulation_amd.scalar_field import Fr
    lib = ctx._lib
    fr = Fr(ctx.curve)
    rng = np.random.default_rng(5)
    n_in, n_w = 16, 48
    per = 3
    row_ptr = (np.arange(n_rows + 1, dtype=np.uint32) * per).astype(np.uint32)
    col = rng.integers(0, n_in + n_w, size=n_rows * per, dtype=np.uint32)
    vals = np.ascontiguousarray(np.stack([fr.to_limbs(int(v)) for v in rng.integers(1, 1 << 30, size=n_rows * per)]), dtype=np.uint64)
    inp = ctx.random_vector(71, n_in, mont=True)
    wit = ctx.random_vector(72, n_w, mont=True)
    want = cref.fr_spmv(ctx.curve, row_ptr, col, vals, inp.download(), wit.download())

    def call():
        return _creator_call(lib, lambda out: lib.amsm_matrix_load(ctx._h, _ptr(row_ptr), _ptr(col), _ptr(vals), n_rows, n_rows * per, out))

    def check(h, fired):
        out = ctx.vector(n_rows)
        ffi.check(lib.amsm_matrix_vec_mul(ctx._h, h, inp.ptr, n_in, wit.ptr, n_w, out.ptr), "amsm_matrix_vec_mul")
        assert np.array_equal(out.download(), want), "A z differs from the oracle's"

    return sweep(ctx, probe, call, check, name="amsm_matrix_load", release=lambda h: lib.amsm_matrix_free(h))


# ---- MSM pipelines -----------------------------------------------------------------------------------------------------------
def make_key(ctx, seed, n, flags):
    return CommitterKey.generate(ctx, seed, n, flags)


def msm_family(ctx, probe, key, key_seed, vec_seed, n, *, name, off=0, counter=None):
    """one amsm_msm_device of n pairs; counter(): a pipeline counter that must have moved on the clean iteration"""
    vec = ctx.random_vector(vec_seed, n, mont=False)
    want = msm_expected(ctx.curve, key_seed, len(key), off, vec_seed, n)
    c0 = counter() if counter else None

    def check(got, fired):
        assert same_point(got, want), f"{name}: the MSM differs from the oracle"

    r = sweep(ctx, probe, lambda: status_of(lambda: VariableBaseMSM.multi_scalar_mul(key, vec, base_off=off, mont=False)), check, name=name)
    if counter:
        assert counter() > c0, f"{name}: the pipeline this family is about never ran"
    return r


def batch_family(ctx, probe, key, key_seed, n, n_vecs, *, name, check_stats=None):
    vecs = [ctx.random_vector(0xBA7C + v, n, mont=False) for v in range(n_vecs)]
    want = [msm_expected(ctx.curve, key_seed, len(key), 0, 0xBA7C + v, n) for v in range(n_vecs)]

    def check(got, fired):
        xy, inf = got
        for v in range(n_vecs):
            assert same_point((xy[v], inf[v]), want[v]), f"{name}: MSM {v} differs from the oracle"
        if check_stats:
            check_stats(fired)

    return sweep(ctx, probe, lambda: status_of(lambda: VariableBaseMSM.multi_scalar_mul_batch(key, vecs, mont=False)), check, name=name)


def multi_family(ctx, probe, key, key_seed, lens, *, name):
    """different-length MSMs in one amsm_msm_multi_device: a refusal at a later job finds earlier ones enqueued"""
    vecs = [ctx.random_vector(0x3017 + i, n, mont=False) for i, n in enumerate(lens)]
    want = [msm_expected(ctx.curve, key_seed, len(key), 0, 0x3017 + i, n) for i, n in enumerate(lens)]

    def check(got, fired):
        xy, inf = got
        for v in range(len(lens)):
            assert same_point((xy[v], inf[v]), want[v]), f"{name}: MSM {v} differs from the oracle"

    return sweep(ctx, probe, lambda: status_of(lambda: VariableBaseMSM.multi_scalar_mul_multi(key, [(0, v) for v in vecs], mont=False)), check,
                 name=name)


def two_valued_family(ctx, probe, key, key_seed, n=1 << 14):
    """constant vectors in one amsm_msm_batch_device (the form the provers' commits take): each is v * (sum of the generators)"""
    vals = [0x1234567 << 100 | 77, 5]
    canon = [np.ascontiguousarray(np.array([(v >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)) for v in vals]
    vecs = [ctx.fill(c, n) for c in canon]  # (the words as given: canonical scalars, mont = 0 below)
    pts = key_points(ctx.curve, key_seed, len(key))[:n]
    want = [cref.msm(ctx.curve, pts, np.tile(c, (n, 1))) for c in canon]
    c0 = ctx.two_valued_msms()

    def check(got, fired):
        xy, inf = got
        for v in range(len(vals)):
            assert same_point((xy[v], inf[v]), want[v]), "two-valued MSM differs from the oracle"

    r = sweep(ctx, probe, lambda: status_of(lambda: VariableBaseMSM.multi_scalar_mul_batch(key, vecs, mont=False)), check, name="two-valued MSMs")
    if not ctx.is_host:
        assert ctx.two_valued_msms() > c0, "the two-valued form never ran"
    return r


def grouped_family(ctx, probe, key, key_seed, n, shift):
    vec = ctx.random_vector(0x6209, n, mont=False)
    s = scalars(ctx.curve, 0x6209, n)
    pts = key_points(ctx.curve, key_seed, len(key))[:n]
    idx = (np.arange(n) >> shift) & 1
    want = [cref.msm(ctx.curve, pts, np.where((idx == g)[:, None], s, 0).astype(np.uint64)) for g in range(2)]

    def check(got, fired):
        xy, inf = got
        for g in range(2):
            assert same_point((xy[g], inf[g]), want[g]), f"grouped MSM, class {g}"

    return sweep(ctx, probe, lambda: status_of(lambda: VariableBaseMSM.multi_scalar_mul_grouped(key, vec, shift, mont=False)), check,
                 name="amsm_msm_grouped_device")


def host_msm_family(ctx, probe, key, key_seed, n=1 << 12):
    s = scalars(ctx.curve, 0x4057, n)
    want = msm_expected(ctx.curve, key_seed, len(key), 0, 0x4057, n)

    def check(got, fired):
        assert same_point(got, want), "amsm_msm differs from the oracle"

    return sweep(ctx, probe, lambda: status_of(lambda: VariableBaseMSM.multi_scalar_mul(key, s, mont=False)), check, name="amsm_msm (host slices)")


def oneshot_family(ctx, probe, n=1 << 12):
    pts = key_points(ctx.curve, 0x0A57, n)
    s = scalars(ctx.curve, 0x0A58, n)
    want = msm_expected(ctx.curve, 0x0A57, n, 0, 0x0A58, n)

    def check(got, fired):
        assert same_point(got, want), "amsm_msm_oneshot differs from the oracle"

    return sweep(ctx, probe, lambda: status_of(lambda: VariableBaseMSM.multi_scalar_mul_oneshot(ctx, pts, s, mont=False)), check,
                 name="amsm_msm_oneshot")


# ---- the schemes' entry points -----------------------------------------------------------------------------------------------
def ipa_round_family(ctx, probe, key, log_key=16, j=1):
    """amsm_ipa_round_fused at round j with the previous round's fold pending: d_coeffs / d_z hold what was uploaded behind every
    AMSM_E_OOM.  Expected outputs: the same call on clean copies (the round's arithmetic has its oracle tests elsewhere)."""
    from accumulation_amd.scalar_field import Fr
    lib = ctx._lib
    fr = Fr(ctx.curve)
    cur = 1 << (log_key - j)  # the vectors' logical length at round j; the fold halves 2 * cur entries first
    up_c = cref.rng_frs(ctx.curve, 0x1A01, 2 * cur)
    up_z = cref.rng_frs(ctx.curve, 0x1A02, 2 * cur)
    up_c, up_z = cref.fr_to_mont(ctx.curve, up_c), cref.fr_to_mont(ctx.curve, up_z)
    xi = np.ascontiguousarray(np.stack([fr.to_limbs(0xABCDEF0123 + 7 * r) for r in range(j)]), dtype=np.uint64)
    fold_x = np.ascontiguousarray(fr.to_limbs(0x51515151517), dtype=np.uint64)
    hp = np.ascontiguousarray(key_points(ctx.curve, 0x1A03, 1)[0], dtype=np.uint64)
    d_c, d_z, d_u = ctx.vector(2 * cur), ctx.vector(2 * cur), ctx.vector(1 << log_key)

    def upload():
        for d, h in ((d_c, up_c), (d_z, up_z)):
            ffi.check(lib.amsm_dev_upload(ctx._h, d.ptr, _ptr(h), h.nbytes), "amsm_dev_upload")

    def call():
        upload()
        lr = np.zeros((2, 2 * ctx.fq_limbs), dtype=np.uint64)
        lr_inf = np.zeros(2, dtype=np.uint8)
        ip = np.zeros((2, 4), dtype=np.uint64)
        rc = lib.amsm_ipa_round_fused(ctx._h, key._h, _ptr(xi), j, log_key, d_c.ptr, d_z.ptr, _ptr(fold_x), _ptr(hp), d_u.ptr, _ptr(lr),
                                      _ptr(lr_inf), _ptr(ip))
        return rc, (None if rc != ffi.AMSM_OK else (lr, lr_inf, ip, d_c.download()[:cur].copy(), d_z.download()[:cur].copy()))

    rc, clean = call()
    assert rc == ffi.AMSM_OK, rc

    def after_oom(k):
        assert np.array_equal(d_c.download(), up_c) and np.array_equal(d_z.download(), up_z), \
            f"amsm_ipa_round_fused, request {k}: AMSM_E_OOM and d_coeffs / d_z were touched"

    def check(got, fired):
        for a, b in zip(got, clean):
            assert np.array_equal(a, b), "amsm_ipa_round_fused differs from the clean run"

    return sweep(ctx, probe, call, check, name="amsm_ipa_round_fused", after_oom=after_oom, require_oom=not ctx.is_host)


def jump_fold_family(ctx, probe, key, log_key=16, j=10):
    from accumulation_amd.scalar_field import Fr
    lib = ctx._lib
    fr = Fr(ctx.curve)
    m0 = 1 << (log_key - j)
    xi = np.ascontiguousarray(np.stack([fr.to_limbs(0x77AA55 + 13 * r) for r in range(j)]), dtype=np.uint64)

    def call():
        xy = np.zeros((m0, 2 * ctx.fq_limbs), dtype=np.uint64)
        inf = np.zeros(m0, dtype=np.uint8)
        rc = lib.amsm_ipa_jump_fold(ctx._h, key._h, log_key, _ptr(xi), j, _ptr(xy), _ptr(inf))
        return rc, (None if rc != ffi.AMSM_OK else (xy, inf))

    rc, clean = call()
    assert rc == ffi.AMSM_OK, rc

    def check(got, fired):
        assert np.array_equal(got[0], clean[0]) and np.array_equal(got[1], clean[1]), "amsm_ipa_jump_fold differs from the clean run"

    return sweep(ctx, probe, call, check, name="amsm_ipa_jump_fold", require_oom=not ctx.is_host)


# ---- vector and polynomial entry points --------------------------------------------------------------------------------------
def t_vecs_family(ctx, probe, n=1 << 10, require_oom=True):
    from accumulation_amd.hp_as import compute_t_vecs
    from accumulation_amd.scalar_field import Fr
    fr = Fr(ctx.curve)
    a = [ctx.random_vector(10 + i, n - 7 * i, mont=True) for i in range(3)]
    b = [ctx.random_vector(20 + i, n - 5 * i, mont=True) for i in range(3)]
    mu = np.stack([fr.to_limbs(x) for x in (1, 0x1234567, (1 << 127) + 3)])
    want = cref.fr_t_vecs(ctx.curve, [v.download() for v in a], [v.download() for v in b], mu, n)

    def check(got, fired):
        for t, w in zip(got, want):
            assert np.array_equal(t.download(), w), "t-vectors differ from the oracle"

    return sweep(ctx, probe, lambda: status_of(lambda: compute_t_vecs(ctx, a, b, mu, n)), check, name="amsm_hp_t_vecs",
                 require_oom=require_oom)


def poly_family(ctx, probe, n=1 << 12, require_oom=True, require_oom_eval=True):
    from accumulation_amd.scalar_field import Fr
    fr = Fr(ctx.curve)
    polys = [ctx.random_vector(0x9017 + i, n - 3 * i, mont=True) for i in range(2)]
    z = 0x1234567890ABCDEF1234567
    zs = np.stack([fr.to_limbs(z), fr.to_limbs(z + 1)])
    host = [[fr.from_limbs(c) for c in p.download()] for p in polys]

    def horner(cs, x):
        acc = 0
        for c in reversed(cs):
            acc = (acc * x + c) % fr.r
        return acc

    want_rem = [horner(host[0], z), horner(host[1], z + 1)]
    out = {}

    def check_div(got, fired):
        quots, rem = got
        for i in range(2):
            assert fr.from_limbs(rem[i]) == want_rem[i], "remainder differs from the host evaluation"
            q = [fr.from_limbs(c) for c in quots[i].download()]
            x = 3 + i  # q(x) (x - z_i) + rem == p(x)
            assert (horner(q, x) * (x - (z + i)) + want_rem[i]) % fr.r == horner(host[i], x), "quotient differs"

    out["div"] = sweep(ctx, probe, lambda: status_of(lambda: ctx.poly_div_linear(polys, zs)), check_div, name="amsm_poly_div_linear_batch",
                       require_oom=require_oom)

    def check_eval(got, fired):
        for i in range(2):
            assert fr.from_limbs(got[i]) == horner(host[i], z), "evaluation differs from the host's"

    out["eval"] = sweep(ctx, probe, lambda: status_of(lambda: ctx.poly_evaluate(polys, zs[0])), check_eval, name="amsm_poly_evaluate_batch",
                        require_oom=require_oom_eval)
    return out


def dev_alloc_family(ctx, probe):
    lib = ctx._lib

    def call():
        p = C.c_void_p(SENTINEL)
        rc = lib.amsm_dev_alloc(ctx._h, 12345 * 32, C.byref(p))
        if rc != ffi.AMSM_OK:
            if p.value != SENTINEL:
                raise Refused(f"a failing amsm_dev_alloc (status {rc}) wrote *d_ptr")
            return rc, None
        return rc, p

    def check(p, fired):
        data = np.arange(12345 * 4, dtype=np.uint64)
        back = np.empty_like(data)
        ffi.check(lib.amsm_dev_upload(ctx._h, p, _ptr(data), data.nbytes), "amsm_dev_upload")
        ffi.check(lib.amsm_dev_download(ctx._h, _ptr(back), p, back.nbytes), "amsm_dev_download")
        assert np.array_equal(back, data)

    return sweep(ctx, probe, call, check, name="amsm_dev_alloc", release=lambda p: lib.amsm_dev_free(ctx._h, p))


# ---- a driver ----------------------------------------------------------------------------------------------------------------
class DriverRng:
    """deterministic scalars for the drivers' zk randomness (`.field()`), re-seeded per prove"""

    def __init__(self, seed):
        self.seed, self.i = seed, 0

    def field(self):
        import hashlib
        self.i += 1
        return int.from_bytes(hashlib.sha256(f"{self.seed}/{self.i}".encode()).digest(), "little") & ((1 << 250) - 1)


def hp_inputs(ctx, ck, n, num):
    from accumulation_amd.hp_as import Accumulator, InputInstance, InputWitness, InputWitnessRandomness, compute_hp
    from accumulation_amd.scalar_field import Fr
    fr = Fr(ctx.curve)
    rng = DriverRng(0xC0FFEE)
    out = []
    for i in range(num):
        a, b = ctx.random_vector(100 + i, n, mont=True), ctx.random_vector(200 + i, n, mont=True)
        rnd = InputWitnessRandomness(rng.field(), rng.field(), rng.field())
        c = [PedersenCommitment.commit(ck, v, fr.to_limbs(r)) for v, r in ((a, rnd.rand_1), (b, rnd.rand_2), (compute_hp(ctx, a, b), rnd.rand_3))]
        out.append(Accumulator(InputInstance(*c), InputWitness(a, b, rnd)))
    return out


def accumulator_words(acc, proof):
    """everything a prove produced, as arrays that compare bit for bit"""
    inst = acc.instance
    pts = [inst.comm_1, inst.comm_2, inst.comm_3] + list(proof.product_poly_comm.low) + list(proof.product_poly_comm.high)
    out = [np.asarray(p[0]).copy() for p in pts] + [np.array([bool(p[1]) for p in pts])]
    return out + [acc.witness.a_vec.download(), acc.witness.b_vec.download()]


def hp_prove_family(ctx, probe, n=600):
    """ASForHadamardProducts.prove, zk on: every failing iteration raises AmsmError with AMSM_E_OOM and nothing else; the first clean
    iteration's accumulator equals the one a FRESH context makes from the same inputs"""
    from accumulation_amd.hp_as import ASForHadamardProducts as AS

    def clean(c):
        ck = PedersenCommitment.setup(c, n, seed=4242)
        pk, _, _ = AS.index(ck)
        inputs = hp_inputs(c, ck, n, 3)
        return ck, pk, inputs

    fresh = Context(ctx.curve, device=ctx.device)
    try:
        _, fpk, finputs = clean(fresh)
        acc1, _ = AS.prove(fpk, finputs[:1], [], DriverRng(7), None)
        want = accumulator_words(*AS.prove(fpk, finputs[1:], [acc1], DriverRng(8), None))
        del acc1, finputs, fpk
    finally:
        fresh.close()
    ck, pk, inputs = clean(ctx)
    old, _ = AS.prove(pk, inputs[:1], [], DriverRng(7), None)

    def call():
        try:
            return ffi.AMSM_OK, AS.prove(pk, inputs[1:], [old], DriverRng(8), None)
        except ffi.AmsmError as e:
            return e.status, None
        # (anything else -- an assertion inside the driver, a TypeError over a half-made object -- is the test's failure)

    def check(got, fired):
        for a, b in zip(accumulator_words(*got), want):
            assert np.array_equal(a, b), "the accumulator differs from a fresh context's"

    return sweep(ctx, probe, call, check, name="ASForHadamardProducts.prove")
