"""amsm_points_check / amsm_points_check_device / AMSM_BASES_CHECK on the library's host backend, without a GPU: the fixture
tests/golden/points_check_v1.json (written by tools/gen_points_check_golden.py from the big-integer oracle; its statuses are derived
here a second time from the definition), mutated generated keys with exact counts, first index and status arrays, the checked key
load and its error return, and the edge cases (n = 0, no infinity bytes, no status array, a multi-context host run)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import pyref as o
from tests import sample_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "points_check_v1.json")
NAMES = ["pallas", "vesta", "bls12_381"]
BAD_CLASSES = {1: "non_canonical", 2: "off_curve", 3: "off_subgroup"}


def curve_ids():
    from accumulation_amd import ffi
    return {"pallas": ffi.AMSM_PALLAS, "bls12_381": ffi.AMSM_BLS12_381_G1, "vesta": ffi.AMSM_VESTA}


def fixture(name, classes=None):
    """-> (xy words (n, 2 limbs) uint64, infinity bytes, expected statuses, classes) of the fixture's points of curve `name`"""
    c = sr.CURVES[name]
    rows = [e for e in json.load(open(GOLDEN))["curves"][name] if classes is None or e["class"] in classes]
    xy = np.array([o.int_to_limbs(int(e["x"], 16), c.limbs) + o.int_to_limbs(int(e["y"], 16), c.limbs) for e in rows], dtype=np.uint64)
    inf = np.array([e["inf"] for e in rows], dtype=np.uint8)
    return xy.reshape(-1, 2 * c.limbs), inf, np.array([e["status"] for e in rows], dtype=np.uint8), [e["class"] for e in rows]


def status_by_definition(c, name, x_raw, y_raw, inf):
    if inf or (x_raw == 0 and y_raw == 0):
        return 0
    if x_raw >= c.p or y_raw >= c.p:
        return 1
    P = (o.fq_from_mont(c, x_raw), o.fq_from_mont(c, y_raw))
    if not o.is_on_curve(c, P):
        return 2
    if name == "bls12_381" and o.mul(c, c.r, P) is not None:
        return 3
    return 0


def report_of(status):
    bad = np.nonzero(status)[0]
    return {"non_canonical": int((status == 1).sum()), "off_curve": int((status == 2).sum()), "off_subgroup": int((status == 3).sum()),
            "first_bad": int(bad[0]) if len(bad) else len(status)}


def check_host_slices(ctx, xy, inf):
    rep, st = ctx.check_points(xy, inf, want_status=True)
    assert ctx.check_points(xy, inf) == rep  # (no status array)
    return rep, st


def check_device(ctx, xy):
    """through amsm_points_check_device: the points uploaded as they are ((0, 0) = identity; no infinity bytes there)"""
    from accumulation_amd import ffi
    from accumulation_amd.engine import PointVector, _ptr
    v = PointVector(ctx, xy.shape[0])
    if v.n:
        ffi.check(ctx._lib.amsm_dev_upload(ctx._h, v.ptr, _ptr(np.ascontiguousarray(xy)), xy.nbytes), "amsm_dev_upload")
    rep, st = v.check(want_status=True)
    assert v.check() == rep
    v.free()
    return rep, st


def mutated_key(ctx, name, log_n, n_bad, seed):
    """a generated key of 2^log_n points read back, n_bad seeded positions (0 and n - 1 among them) overwritten with the fixture's bad
    points of every class in turn -> (xy, expected statuses).  The untouched points are multiples of the generator: status 0."""
    from accumulation_amd import ffi
    from accumulation_amd.engine import CommitterKey
    n = 1 << log_n
    ck = CommitterKey.generate(ctx, 0xC0FFEE + log_n, n, ffi.AMSM_BASES_NO_PRECOMPUTE)
    xy, _ = ck.read()
    ck.free()
    fxy, finf, fst, _ = fixture(name)
    pool = [i for i in range(len(fst)) if fst[i] != 0 and not finf[i]]
    rng = np.random.default_rng(seed)
    pos = np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), size=n_bad - 2, replace=False)])
    want = np.zeros(n, dtype=np.uint8)
    for k, at in enumerate(pos):
        src = pool[k % len(pool)]
        xy[at] = fxy[src]
        want[at] = fst[src]
    return xy, want


@pytest.fixture(scope="module")
def ctxs(built_lib):
    from accumulation_amd import Context, ffi
    out = {name: Context(cid, device=ffi.AMSM_DEVICE_HOST) for name, cid in curve_ids().items()}
    yield out
    for c in out.values():
        c.close()


@pytest.mark.parametrize("name", NAMES)
def test_fixture_statuses_follow_from_the_definition(name):
    c = sr.CURVES[name]
    rows = json.load(open(GOLDEN))["curves"][name]
    assert 40 <= len(rows) <= 80
    for e in rows:
        assert status_by_definition(c, name, int(e["x"], 16), int(e["y"], 16), e["inf"]) == e["status"], e["class"]
    want = {0, 1, 2, 3} if name == "bls12_381" else {0, 1, 2}
    assert {e["status"] for e in rows} == want


@pytest.mark.parametrize("name", NAMES)
def test_golden_fixture(ctxs, name):
    xy, inf, want, _ = fixture(name)
    rep, st = check_host_slices(ctxs[name], xy, inf)
    assert np.array_equal(st, want) and rep == report_of(want)
    # the device-pointer variant has no infinity bytes: the flagged points are given as the identity they stand for
    xy0 = xy.copy()
    xy0[inf != 0] = 0
    rep, st = check_device(ctxs[name], xy0)
    assert np.array_equal(st, want) and rep == report_of(want)


@pytest.mark.parametrize("name", NAMES)
def test_mutated_generated_key(ctxs, name):
    xy, want = mutated_key(ctxs[name], name, 12, 32, seed=7)
    assert want[0] and want[-1] and int((want != 0).sum()) == 32
    for rep, st in (check_host_slices(ctxs[name], xy, None), check_device(ctxs[name], xy)):
        assert np.array_equal(st, want) and rep == report_of(want) and rep["first_bad"] == 0
    xy[0] = 0  # the first bad point moves
    want[0] = 0
    rep, st = check_host_slices(ctxs[name], xy, None)
    assert np.array_equal(st, want) and rep == report_of(want) and rep["first_bad"] > 0


def checked_load_cases(ctx, name, n=600):
    from accumulation_amd import ffi
    from accumulation_amd.engine import CommitterKey, PointVector, VariableBaseMSM, _ptr
    lib = ctx._lib
    c = sr.CURVES[name]
    ck = CommitterKey.generate(ctx, 0xBA5E5, n, ffi.AMSM_BASES_NO_PRECOMPUTE)
    xy, _ = ck.read()
    ck.free()
    xy[5] = 0  # an identity among them is valid
    inf = np.zeros(n, dtype=np.uint8)
    inf[9] = 1
    scalars = np.array([o.int_to_limbs(o.rng_scalar(3, i) % c.r, 4) for i in range(n)], dtype=np.uint64)
    for flags in (ffi.AMSM_BASES_NO_PRECOMPUTE, ffi.AMSM_BASES_DEFAULT):
        plain = CommitterKey.load(ctx, xy, inf, flags=flags)
        checked = CommitterKey.load(ctx, xy, inf, flags=flags | ffi.AMSM_BASES_CHECK)
        assert plain.precomputed == checked.precomputed
        (a, ai), (b, bi) = plain.read(), checked.read()
        assert np.array_equal(a, b) and np.array_equal(ai, bi)
        (r0, i0), (r1, i1) = VariableBaseMSM.multi_scalar_mul(plain, scalars), VariableBaseMSM.multi_scalar_mul(checked, scalars)
        assert i0 == i1 and np.array_equal(r0, r1)
        plain.free()
        checked.free()
    fxy, finf, fst, _ = fixture(name)
    ctx.synchronize()
    for status in sorted(set(int(s) for s in fst) - {0}):
        bad = xy.copy()
        bad[n - 3] = fxy[[i for i in range(len(fst)) if fst[i] == status and not finf[i]][0]]
        dev = PointVector(ctx, n)
        ffi.check(lib.amsm_dev_upload(ctx._h, dev.ptr, _ptr(bad), bad.nbytes), "amsm_dev_upload")
        before = ctx.memory()
        h = C.c_void_p(0x1234)  # the handle variable must come back untouched
        assert lib.amsm_bases_load(ctx._h, _ptr(bad), None, n, ffi.AMSM_BASES_CHECK, C.byref(h)) == ffi.AMSM_E_INVALID_POINT
        assert h.value == 0x1234
        assert lib.amsm_bases_from_device(ctx._h, dev.ptr, n, ffi.AMSM_BASES_CHECK, C.byref(h)) == ffi.AMSM_E_INVALID_POINT
        assert h.value == 0x1234
        assert ctx.memory() == before
        with pytest.raises(ffi.AmsmError) as e:
            CommitterKey.load(ctx, bad, flags=ffi.AMSM_BASES_CHECK | ffi.AMSM_BASES_NO_PRECOMPUTE)
        assert e.value.status == ffi.AMSM_E_INVALID_POINT and "invalid point" in str(e.value)
        # without the flag the same calls build a key, as before
        k = CommitterKey.from_device(ctx, dev)
        assert len(k) == n
        k.free()
        bad_inf = np.zeros(n, dtype=np.uint8)
        bad_inf[n - 3] = 1  # ... and the infinity byte hides the point's words
        k = CommitterKey.load(ctx, bad, bad_inf, flags=ffi.AMSM_BASES_CHECK | ffi.AMSM_BASES_NO_PRECOMPUTE)
        k.free()
        good = PointVector(ctx, n)
        ffi.check(lib.amsm_dev_upload(ctx._h, good.ptr, _ptr(xy), xy.nbytes), "amsm_dev_upload")
        k0, k1 = CommitterKey.from_device(ctx, good), CommitterKey.from_device(ctx, good, flags=ffi.AMSM_BASES_CHECK)
        assert k0.precomputed == k1.precomputed and np.array_equal(k0.read()[0], k1.read()[0])
        for v in (k0, k1, dev, good):
            v.free()
    g = C.c_void_p()
    assert lib.amsm_bases_generate(ctx._h, 1, 4, ffi.AMSM_BASES_CHECK, C.byref(g)) == ffi.AMSM_E_INVALID_ARG and not g.value


@pytest.mark.parametrize("name", NAMES)
def test_checked_load(ctxs, name):
    checked_load_cases(ctxs[name], name)


def edge_cases(ctx, name):
    from accumulation_amd import ffi
    lib = ctx._lib
    report = np.full(4, 77, dtype=np.uint64)
    rp = report.ctypes.data_as(C.c_void_p)
    assert lib.amsm_points_check(ctx._h, None, None, 0, rp, None) == ffi.AMSM_OK and not report.any()
    report[:] = 77
    assert lib.amsm_points_check_device(ctx._h, None, 0, rp, None) == ffi.AMSM_OK and not report.any()
    assert lib.amsm_points_check(ctx._h, None, None, 3, rp, None) == ffi.AMSM_E_INVALID_ARG
    assert lib.amsm_points_check(None, None, None, 0, rp, None) == ffi.AMSM_E_INVALID_ARG
    assert lib.amsm_points_check(ctx._h, None, None, 0, None, None) == ffi.AMSM_E_INVALID_ARG
    assert lib.amsm_points_check_device(ctx._h, None, 3, rp, None) == ffi.AMSM_E_INVALID_ARG
    assert lib.amsm_points_check_device(ctx._h, None, 0, None, None) == ffi.AMSM_E_INVALID_ARG
    assert b"invalid point" in lib.amsm_strerror(ffi.AMSM_E_INVALID_POINT)
    xy, inf, want, _ = fixture(name)
    keep = inf == 0  # NULL is_inf: nothing is flagged
    rep = ctx.check_points(xy[keep])
    assert rep == report_of(want[keep])


@pytest.mark.parametrize("name", NAMES)
def test_edge_cases(ctxs, name):
    edge_cases(ctxs[name], name)


def test_multi_context_host_run(built_lib):
    """amsm_ctx_create_multi with n_dev = 0 is the host backend: the same calls, the same answers"""
    from accumulation_amd import ffi
    lib = built_lib
    h = C.c_void_p()
    assert lib.amsm_ctx_create_multi(C.byref(h), ffi.AMSM_BLS12_381_G1, None, 0) == ffi.AMSM_OK and lib.amsm_ctx_is_host(h) == 1
    xy, inf, want, _ = fixture("bls12_381")
    report, status = np.zeros(4, dtype=np.uint64), np.zeros(len(want), dtype=np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.amsm_points_check(h, vp(xy), vp(inf), len(want), vp(report), vp(status)) == ffi.AMSM_OK
    assert np.array_equal(status, want) and list(report) == list(report_of(want).values())
    k = C.c_void_p()
    assert lib.amsm_bases_load(h, vp(xy), vp(inf), len(want), ffi.AMSM_BASES_CHECK, C.byref(k)) == ffi.AMSM_E_INVALID_POINT and not k.value
    ok = np.ascontiguousarray(xy[want == 0])
    assert lib.amsm_bases_load(h, vp(ok), vp(np.ascontiguousarray(inf[want == 0])), len(ok), ffi.AMSM_BASES_CHECK, C.byref(k)) == ffi.AMSM_OK
    assert lib.amsm_bases_len(k) == len(ok)
    lib.amsm_bases_free(k)
    lib.amsm_ctx_destroy(h)
