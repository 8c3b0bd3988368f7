"""amsm_points_check / amsm_points_check_device / AMSM_BASES_CHECK on the GPU: the kernels of
accumulation_amd/csrc/points_check_kernels.h against the fixture tests/golden/points_check_v1.json, byte for byte against the
library's host backend (which runs the definition itself: on_curve and a multiplication by r), at 2^20 points through the piecewise
upload of the host-slice entry point with the expectation taken from the construction, the checked key load (plain and precomputed
keys, sharded and replicated keys of a three-"device" context), and the small-order inputs that make the BLS12-381 ladder's
intermediates hit the identity and +-P.

HOST_MAX_LOG: the host-backend re-collection of this file (tests/host_backend/test_host_points_check_cpu.py) skips the sizes above
2^HOST_MAX_LOG -- there every BLS12-381 point costs a 255-bit multiplication on the host; the GPU run covers all of them."""
import numpy as np
import pytest

from tests import test_points_check_cpu as pc

pytestmark = pytest.mark.gpu

HOST_MAX_LOG = 16
NAMES = pc.NAMES


@pytest.fixture(scope="module")
def ctxs(built_lib):
    """per curve: (the context under test -- the GPU's, or the host backend's in the re-collection -- and a host-backend context)"""
    from accumulation_amd import Context, ffi
    out = {name: (Context(cid), Context(cid, device=ffi.AMSM_DEVICE_HOST)) for name, cid in pc.curve_ids().items()}
    yield out
    for a, b in out.values():
        a.close()
        b.close()


def _size_guard(ctx, log_n):
    if ctx.is_host and log_n > HOST_MAX_LOG:
        pytest.skip(f"host backend: sizes above 2^{HOST_MAX_LOG} run on the GPU only")


@pytest.mark.parametrize("name", NAMES)
def test_golden_fixture_on_the_kernels(ctxs, name):
    dev, _ = ctxs[name]
    xy, inf, want, _ = pc.fixture(name)
    rep, st = pc.check_host_slices(dev, xy, inf)
    assert np.array_equal(st, want) and rep == pc.report_of(want)
    xy0 = xy.copy()
    xy0[inf != 0] = 0
    rep, st = pc.check_device(dev, xy0)
    assert np.array_equal(st, want) and rep == pc.report_of(want)


@pytest.mark.parametrize("name", NAMES)
def test_device_and_host_backend_agree_byte_for_byte(ctxs, name):
    dev, host = ctxs[name]
    xy, want = pc.mutated_key(dev, name, 16, 64, seed=11)
    got = [pc.check_host_slices(dev, xy, None), pc.check_device(dev, xy), pc.check_host_slices(host, xy, None)]
    for rep, st in got:
        assert np.array_equal(st, got[2][1]) and rep == got[2][0]
    assert np.array_equal(got[0][1], want) and got[0][0] == pc.report_of(want)


@pytest.mark.parametrize("name", ["pallas", "bls12_381"])
def test_a_million_points_through_the_piecewise_upload(ctxs, name):
    dev, _ = ctxs[name]
    _size_guard(dev, 20)
    n = 1 << 20
    xy, want = pc.mutated_key(dev, name, 20, 252, seed=13)
    fxy, finf, fst, _ = pc.fixture(name)
    pool = [i for i in range(len(fst)) if fst[i] != 0 and not finf[i]]
    for k, at in enumerate(((1 << 19) - 1, (1 << 19) + 1, (1 << 18), (1 << 18) - 1)):  # around the pieces' boundaries
        xy[at] = fxy[pool[k]]
        want[at] = fst[pool[k]]
    assert int((want != 0).sum()) == 256 and want[0] and want[n - 1]
    rep, st = dev.check_points(xy, None, want_status=True)
    assert np.array_equal(st, want) and rep == pc.report_of(want)
    xy[0] = 0  # the first bad point now lies in a later position
    want[0] = 0
    rep = dev.check_points(xy)
    assert rep == pc.report_of(want) and rep["first_bad"] > 0
    inf = np.zeros(n, dtype=np.uint8)
    inf[want != 0] = 1  # every bad point flagged infinite: a valid key
    assert dev.check_points(xy, inf) == {"non_canonical": 0, "off_curve": 0, "off_subgroup": 0, "first_bad": n}


@pytest.mark.parametrize("name", NAMES)
def test_checked_load(ctxs, name):
    pc.checked_load_cases(ctxs[name][0], name)
    pc.edge_cases(ctxs[name][0], name)


@pytest.mark.parametrize("name", ["pallas", "bls12_381"])
def test_checked_load_of_a_precomputed_key(ctxs, name):
    from accumulation_amd import ffi
    from accumulation_amd.engine import CommitterKey
    dev, _ = ctxs[name]
    n = 1 << 13
    ck = CommitterKey.generate(dev, 5, n, ffi.AMSM_BASES_NO_PRECOMPUTE)
    xy, _ = ck.read()
    ck.free()
    a = CommitterKey.load(dev, xy, flags=ffi.AMSM_BASES_PRECOMPUTE)
    b = CommitterKey.load(dev, xy, flags=ffi.AMSM_BASES_PRECOMPUTE | ffi.AMSM_BASES_CHECK)
    assert (dev.is_host or a.precomputed) and a.precomputed == b.precomputed and a.tables() == b.tables() and np.array_equal(a.read()[0], b.read()[0])
    scalars = dev.random_vector(0xA11CE, n, False)
    from accumulation_amd.engine import VariableBaseMSM
    (r0, i0), (r1, i1) = VariableBaseMSM.multi_scalar_mul(a, scalars), VariableBaseMSM.multi_scalar_mul(b, scalars)
    assert i0 == i1 and np.array_equal(r0, r1)
    fxy, finf, fst, _ = pc.fixture(name)
    xy[n // 2] = fxy[[i for i in range(len(fst)) if fst[i] == 2][0]]
    with pytest.raises(ffi.AmsmError) as e:
        CommitterKey.load(dev, xy, flags=ffi.AMSM_BASES_PRECOMPUTE | ffi.AMSM_BASES_CHECK)
    assert e.value.status == ffi.AMSM_E_INVALID_POINT


@pytest.mark.parametrize("replicate", [False, True])
def test_checked_load_on_three_devices(ctxs, replicate):
    from accumulation_amd import ffi
    from accumulation_amd.engine import CommitterKey, MultiContext
    dev, _ = ctxs["bls12_381"]
    if dev.is_host:
        pytest.skip("multi-device contexts are a GPU matter")
    n = 3000
    ck = CommitterKey.generate(dev, 9, n, ffi.AMSM_BASES_NO_PRECOMPUTE)
    xy, _ = ck.read()
    ck.free()
    multi = MultiContext(ffi.AMSM_BLS12_381_G1, devices=(0, 0, 0))
    flags = ffi.AMSM_BASES_NO_PRECOMPUTE | (ffi.AMSM_BASES_REPLICATE if replicate else 0)
    good = CommitterKey.load(multi, xy, flags=flags | ffi.AMSM_BASES_CHECK)
    assert (replicate or good.num_shards == 3) and np.array_equal(good.read()[0], xy)
    good.free()
    fxy, finf, fst, _ = pc.fixture("bls12_381")
    for status in (1, 2, 3):
        bad = xy.copy()
        bad[n - 2] = fxy[[i for i in range(len(fst)) if fst[i] == status and not finf[i]][0]]  # in the last shard
        mem = [multi.shard(g).memory() for g in range(3)]
        with pytest.raises(ffi.AmsmError) as e:
            CommitterKey.load(multi, bad, flags=flags | ffi.AMSM_BASES_CHECK)
        assert e.value.status == ffi.AMSM_E_INVALID_POINT
        assert [multi.shard(g).memory() for g in range(3)] == mem
        rep = multi.check_points(bad)  # the check calls run on the primary device
        assert rep["first_bad"] == n - 2 and sum(rep[k] for k in ("non_canonical", "off_curve", "off_subgroup")) == 1
    multi.close()


def test_small_order_inputs_to_the_subgroup_ladder(ctxs):
    """order 3 ((0, +-2)), 11 and 10177, with their negatives: intermediates of the ladder are the identity and +-P"""
    dev, host = ctxs["bls12_381"]
    xy, inf, want, classes = pc.fixture("bls12_381", classes={"order_3", "order_11", "order_10177"})
    assert len(want) >= 2 + 4 + 4 and not inf.any() and (want == 3).all()
    c = pc.sr.BLS
    pts = {pc.o.point_from_mont_limbs(c, [int(w) for w in row], 0) for row in xy}
    assert (0, 2) in pts and (0, c.p - 2) in pts and all(pc.o.neg(c, P) in pts for P in pts)
    for rep, st in (pc.check_host_slices(dev, xy, None), pc.check_device(dev, xy), pc.check_host_slices(host, xy, None)):
        assert (st == 3).all() and rep == pc.report_of(want)
