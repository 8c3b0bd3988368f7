"""amsm_bases_sample on the GPU: the sampling kernels (accumulation_amd/csrc/sample_kernels.h) against the big-integer sampler of
tests/sample_ref.py and, bit for bit, against the library's host backend; sampled keys as ordinary keys (MSMs through the windowed
pipelines and the direct-sum table equal those over the same points loaded); sharded sampling on a multi-device context.

HOST_MAX_LOG: the host-backend re-collection of this file (tests/host_backend/test_host_bases_sample_cpu.py) skips the sizes above
2^HOST_MAX_LOG; the GPU run covers all of them."""
import numpy as np
import pytest

from tests import sample_ref as sr

pytestmark = pytest.mark.gpu

HOST_MAX_LOG = 18
DOMAIN = b"PC-DL-2020"
NAMES = ["pallas", "vesta", "bls12_381"]


def _ids():
    from accumulation_amd import ffi
    return {"pallas": ffi.AMSM_PALLAS, "bls12_381": ffi.AMSM_BLS12_381_G1, "vesta": ffi.AMSM_VESTA}


@pytest.fixture(scope="module")
def ctxs(built_lib):
    """per curve: (the context under test -- the GPU's, or the host backend's in the re-collection -- and a host-backend context)"""
    from accumulation_amd import Context, ffi
    out = {name: (Context(cid), Context(cid, device=ffi.AMSM_DEVICE_HOST)) for name, cid in _ids().items()}
    yield out
    for a, b in out.values():
        a.close()
        b.close()


def _size_guard(ctx, n):
    if ctx.is_host and n > (1 << HOST_MAX_LOG):
        pytest.skip(f"host backend: sizes above 2^{HOST_MAX_LOG} run on the GPU only")


def _sample(ctx, n, first=0, flags=None, domain=DOMAIN):
    from accumulation_amd import ffi
    from accumulation_amd.engine import CommitterKey
    ck = CommitterKey.sample(ctx, domain, n, ffi.AMSM_BASES_NO_PRECOMPUTE if flags is None else flags, first=first)
    xy, inf = ck.read()
    ck.free()
    assert not inf.any()
    return xy


@pytest.mark.parametrize("name,log_n", [("pallas", 12), ("vesta", 12), ("bls12_381", 9)])
def test_against_the_python_sampler(ctxs, name, log_n):
    c = sr.CURVES[name]
    n = 1 << log_n
    assert np.array_equal(_sample(ctxs[name][0], n), sr.to_words(c, sr.sample(c, DOMAIN, 0, n)))
    far = (1 << 32) + 5
    assert np.array_equal(_sample(ctxs[name][0], 64, first=far), sr.to_words(c, sr.sample(c, DOMAIN, far, 64)))


@pytest.mark.parametrize("name", NAMES)
def test_device_and_host_backend_are_bit_identical(ctxs, name):
    dev, host = ctxs[name]
    n = 1 << 16
    assert np.array_equal(_sample(dev, n), _sample(host, n))
    assert np.array_equal(_sample(dev, 1000, first=(1 << 40) + 1, domain=b""), _sample(host, 1000, first=(1 << 40) + 1, domain=b""))


def test_windows_of_a_large_key(ctxs):
    dev, host = ctxs["pallas"]
    n = 1 << 20
    _size_guard(dev, n)
    xy = _sample(dev, n)
    for lo, hi in ((0, 256), ((1 << 19) - 128, (1 << 19) + 128), (n - 256, n)):
        assert np.array_equal(xy[lo:hi], _sample(host, hi - lo, first=lo)), (lo, hi)


@pytest.mark.parametrize("log_n", [16, 12])  # 2^16: the windowed pipelines; 2^12: the direct-sum table
def test_a_sampled_key_gives_the_msm_of_the_same_points_loaded(ctxs, log_n):
    from accumulation_amd import ffi
    from accumulation_amd.engine import CommitterKey, VariableBaseMSM
    dev, _ = ctxs["pallas"]
    n = 1 << log_n
    sampled = CommitterKey.sample(dev, DOMAIN, n)  # default flags: the key builds its tables
    xy, inf = sampled.read()
    loaded = CommitterKey.load(dev, xy)
    ts, tl = sampled.tables(), loaded.tables()
    assert sampled.precomputed == loaded.precomputed and all(ts[k] == tl[k] for k in ("window_table", "direct_sum_table", "levels"))
    if log_n == 12 and not dev.is_host:
        assert sampled.tables()["direct_sum_table"] > 0
    scalars = dev.random_vector(0xA11CE, n, False)
    a, ainf = VariableBaseMSM.multi_scalar_mul(sampled, scalars)
    b, binf = VariableBaseMSM.multi_scalar_mul(loaded, scalars)
    assert ainf == binf and not ainf and np.array_equal(a, b)
    plain = CommitterKey.load(dev, xy, flags=ffi.AMSM_BASES_NO_PRECOMPUTE)
    c, cinf = VariableBaseMSM.multi_scalar_mul(plain, scalars)
    assert cinf == ainf and np.array_equal(a, c)


def test_eight_shards_sample_their_own_index_ranges(ctxs):
    from accumulation_amd import ffi
    from accumulation_amd.engine import CommitterKey, MultiContext
    dev, _ = ctxs["pallas"]
    if dev.is_host:
        pytest.skip("multi-device contexts are a GPU matter")
    n = 1 << 16
    single = _sample(dev, n)
    multi = MultiContext(ffi.AMSM_PALLAS, devices=(0,) * 8)
    ck = CommitterKey.sample(multi, DOMAIN, n, ffi.AMSM_BASES_NO_PRECOMPUTE)
    assert ck.num_shards == 8
    covered = 0
    for g in range(8):
        lo, hi = multi.shard_range(ck, g)
        assert lo == covered and hi > lo
        xy, inf = ck.read(lo, hi - lo)
        assert not inf.any() and np.array_equal(xy, single[lo:hi]), g
        covered = hi
    assert covered == n
    ck.free()
    multi.close()
