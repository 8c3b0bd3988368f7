"""The grid-stride loops of the scalar-field vector kernels, past their first pass.

k_vec_hadamard, k_vec_combine<NV> and k_hp_t_vecs<N> prefetch element i + stride before they multiply and store element i, then
rotate their registers; k_vec_inner_product, k_vec_inner_product_pair and k_ipa_fold_ip accumulate over a strided loop.  With the
grids that ship a lane takes a second element only above 2^22 (streaming) / 2^18 (reductions) elements, so here every curve's
context is capped at CAP workgroups (amsm_ctx_set_vec_grid_max): L = 1024 lanes, and sizes a little above L, 2 L, 3 L, ... put
the prefetch, the rotation, the second evaluation of the ragged-length predicates and the second store to work.  Every test
first asks amsm_ctx_vec_grid whether its size really exceeds the lanes of its launch: a test that would not enter the loop fails.

The reference is Python integers on the Montgomery limbs (oracle/pyref.py) for all six curves, bit-exact over the whole output.
The last tests run the grids that ship, uncapped, at the first sizes where they loop (Pallas only)."""
import numpy as np
import pytest

from oracle import pyref as o
from tests import helpers as h
from tests.test_vec_gpu import edge_value_pass

pytestmark = pytest.mark.gpu

CAP = 4
L = CAP * 256  # lanes of a capped launch
ALL = [o.PALLAS, h.VESTA, o.BLS12_381_G1, h.BN254, h.GRUMPKIN, h.BLS12_377]
FEW = [o.PALLAS, h.BLS12_377]
cid = lambda c: c.name  # noqa: E731

HADAMARD_NS = [L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 5 * L + 257]
COMBINE_N = 3 * L + 77
COMBINE_LENS = [COMBINE_N, L - 1, L, L + 1, 2 * L + 5, 1]  # straddle the iteration boundaries; repeated as needed
COMBINE_HIDING = [None, 2 * L + 3, L - 5]
TVEC_LEN = 2 * L + 77
IP_NS = [L + 1, 4 * L + 300]
IPA_LOG_KEY = 13
IPA_HALF = 1 << (IPA_LOG_KEY - 1)  # round j = 0: 4096 = 4 L
EDGE_PAIRS_MIN = 1600  # the edge-value pass feeds m^2 pairs; m = 41 distinct values on every curve today
STREAM_NS = HADAMARD_NS + [COMBINE_N, TVEC_LEN, EDGE_PAIRS_MIN]
REDUCE_NS = IP_NS + [IPA_HALF, EDGE_PAIRS_MIN]

POOL_N = 2 * (1 << IPA_LOG_KEY) + 64  # the longest vector (the 2 x 2^13 elements a fused round folds) and room for offsets


@pytest.fixture(scope="module")
def capped():
    """one context per curve with every grid-stride Fr launch held to CAP workgroups"""
    from accumulation_amd import Context
    out = {}
    for c in ALL:
        ctx = Context(c.curve_id)
        ctx.set_vec_grid_max(CAP)
        for n in STREAM_NS:
            assert ctx.vec_grid(n)[0] * 256 < n, (c.name, n)
        for n in REDUCE_NS:
            assert ctx.vec_grid(n)[1] * 256 < n, (c.name, n)
        out[c.name] = ctx
    yield out
    for ctx in out.values():
        ctx.close()


def loops(ctx, n, reduce=False):
    """does an n-element launch of this context give some lane a second element?"""
    return ctx.vec_grid(n)[1 if reduce else 0] * 256 < n


_pools = {}


def pool(c):
    """POOL_N field elements uniform in [0, r), as canonical integers and as Montgomery limbs: made once per curve, read-only"""
    if c.name not in _pools:
        vals = o.rng_frs(c, 0x57A1DE + c.curve_id, POOL_N)
        mont = h.fr_mont_np(c, vals)
        mont.setflags(write=False)
        _pools[c.name] = (vals, mont)
    return _pools[c.name]


def vec(ctx, c, k, n):
    """vector number k (distinct offsets into the pool), n elements: (canonical ints, device vector)"""
    vals, mont = pool(c)
    off = 37 * k
    assert off + n <= POOL_N
    return vals[off:off + n], ctx.upload(mont[off:off + n])


def test_cap_is_a_further_bound_and_zero_restores_the_built_in_grids(capped):
    """amsm_ctx_vec_grid with the cap at 0 is min(ceil(n / 256), 64 CUs) / min(ceil(n / 256), 1024); a positive cap only lowers"""
    import torch
    ctx = capped["pallas"]
    cus = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    sizes = [1, 255, 256, 257, L, L + 1, 1 << 18, (1 << 18) + 257, cus * 64 * 256, cus * 64 * 256 + 257, (1 << 32) - 256]
    try:
        ctx.set_vec_grid_max(0)
        for n in sizes:
            assert ctx.vec_grid(n) == (min(-(-n // 256), cus * 64), min(-(-n // 256), 1024)), n
        ctx.set_vec_grid_max(7)
        for n in sizes:
            assert ctx.vec_grid(n) == (min(-(-n // 256), cus * 64, 7), min(-(-n // 256), 1024, 7)), n
    finally:
        ctx.set_vec_grid_max(CAP)
    assert ctx.vec_grid(L + 1) == (CAP, CAP)


@pytest.mark.parametrize("c", ALL, ids=cid)
@pytest.mark.parametrize("n", HADAMARD_NS)
def test_hadamard_past_the_first_pass(capped, c, n):
    from accumulation_amd.hp_as import compute_hp
    ctx = capped[c.name]
    assert loops(ctx, n)
    a, da = vec(ctx, c, 0, n)
    b, db = vec(ctx, c, 1, n + 3)  # zip truncates to the shorter
    got = compute_hp(ctx, da, db)
    assert got.n == n
    assert h.fr_from_mont_np(c, got.download()) == o.compute_hp(c, a, b)


@pytest.mark.parametrize("c", ALL, ids=cid)
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 8, 9, 17])
def test_combine_past_the_first_pass(capped, c, k):
    """every instantiation k_vec_combine<1..8>, and k = 9, 17: groups of eight whose running sum is re-read from `out` (the plain
    store in place of the non-temporal one).  Ragged operands, three hiding settings, the unit-first-coefficient branch
    (fe_dot_n<NV - 1>) and the general one (fe_dot_n<NV>)."""
    from accumulation_amd.hp_as import combine_vectors
    ctx = capped[c.name]
    n = COMBINE_N
    assert loops(ctx, n)
    lens = [COMBINE_LENS[j % len(COMBINE_LENS)] for j in range(k)]
    hv, dv = zip(*[vec(ctx, c, 2 + j, ln) for j, ln in enumerate(lens)])
    for unit in (True, False):
        ch = [x or 1 for x in o.rng_frs(c, 0xC0EF + k, k)]
        if unit:
            ch[0] = 1
            if k == 9:
                ch[8] = 1  # the second group's only coefficient: the unit branch on the in-place launch
        else:
            assert ch[0] != 1
        if k == 17:
            ch[9] = 1
        ch_np = h.fr_mont_np(c, ch)
        for hl in COMBINE_HIDING:
            hid, dh = vec(ctx, c, 30, hl) if hl else (None, None)
            got = combine_vectors(ctx, dv, ch_np, dh)
            assert got.n == n
            assert h.fr_from_mont_np(c, got.download()) == o.combine_vectors(c, hv, ch, hid), (unit, hl)


def tvec_curves(n_in):
    return ALL if n_in in (2, 3, 4, 9) else FEW


@pytest.mark.parametrize("zk", [False, True], ids=["plain", "hiding"])
@pytest.mark.parametrize("c,n_in", [(c, n_in) for n_in in (1, 2, 3, 4, 5, 6, 7, 8, 9, 17) for c in tvec_curves(n_in)],
                         ids=lambda v: v.name if isinstance(v, o.Curve) else str(v))
def test_t_vecs_past_the_first_pass(capped, c, n_in, zk):
    """every instantiation k_hp_t_vecs<1..8>, and n_in = 9, 17: t_vecs_blocked, whose add_into hands its destination to the
    combination kernel both as an operand and as the output, and whose Hadamard products go through a scratch vector.  mu_0 is
    the unit without hiding (the schemes' case) and a general element with it, so both branches of the kernel loop."""
    from accumulation_amd.hp_as import compute_t_vecs
    ctx = capped[c.name]
    ln = TVEC_LEN
    assert loops(ctx, ln)
    a_short, b_short = (1, n_in - 1) if n_in > 1 else (0, None)
    a_lens = [(L + 3 if n_in > 1 else 2 * L + 5) if j == a_short else ln for j in range(n_in)]
    b_lens = [L - 1 if j == b_short else ln for j in range(n_in)]
    a, da = zip(*[vec(ctx, c, j, a_lens[j]) for j in range(n_in)])
    b, db = zip(*[vec(ctx, c, 20 + j, b_lens[j]) for j in range(n_in)])
    mu = [x or 1 for x in o.rng_frs(c, 0x3000 + n_in, n_in + 1)]  # n_in + 1 challenges (the last only used with hiding)
    hiding = dh = None
    if zk:
        (ha, dha), (hb, dhb) = vec(ctx, c, 40, ln), vec(ctx, c, 41, L + 1)
        hiding, dh = (ha, hb), (dha, dhb)
    else:
        mu[0] = 1
    exp = o.compute_t_vecs(c, a, b, mu, ln, hiding)
    got = compute_t_vecs(ctx, da, db, h.fr_mont_np(c, mu), ln, dh)
    assert len(got) == 2 * n_in - 1
    full = [g.download() for g in got]
    for k in range(2 * n_in - 1):
        assert h.fr_from_mont_np(c, full[k]) == exp[k], k
    # the committed subset only (coefficient n_in - 1 is never committed, src/hp_as/mod.rs:373-375)
    got2 = compute_t_vecs(ctx, da, db, h.fr_mont_np(c, mu), ln, dh, skip_uncommitted=True)
    assert got2[n_in - 1] is None
    for k in range(2 * n_in - 1):
        if k != n_in - 1:
            assert np.array_equal(got2[k].download(), full[k]), k


def inner_product(ctx, da, db, n):
    from accumulation_amd import ffi
    from accumulation_amd.engine import _ptr
    ip = np.zeros(4, dtype=np.uint64)
    ffi.check(ctx._lib.amsm_vec_inner_product(ctx._h, da.ptr, db.ptr, n, _ptr(ip)), "amsm_vec_inner_product")
    return ip


@pytest.mark.parametrize("c", ALL, ids=cid)
@pytest.mark.parametrize("n", IP_NS)
def test_inner_product_past_the_first_pass(capped, c, n):
    ctx = capped[c.name]
    assert loops(ctx, n, reduce=True)
    a, da = vec(ctx, c, 3, n)
    b, db = vec(ctx, c, 5, n)
    got = h.fr_from_mont_np(c, inner_product(ctx, da, db, n).reshape(1, 4))[0]
    assert got == sum(x * y for x, y in zip(a, b)) % c.r


@pytest.mark.parametrize("c", FEW, ids=cid)
def test_ipa_round_past_the_first_pass(capped, c):
    """amsm_ipa_round and amsm_ipa_round_fused (with and without the pending fold, with and without h') at half = 4 L: both inner
    products and the folded vectors against Python integers, the upper halves untouched, and the two points bit-identical to
    the same call with the grids that ship (that path is pinned to the oracle at 64 generators in tests/test_ipa_gpu.py)."""
    from accumulation_amd import PedersenCommitment, ffi
    from accumulation_amd.engine import _ptr
    ctx = capped[c.name]
    r, m, half = c.r, 1 << IPA_LOG_KEY, IPA_HALF
    assert loops(ctx, half, reduce=True)
    key = PedersenCommitment.setup(ctx, m, seed=0x1FA)
    h_prime = np.ascontiguousarray(key.read(5, 1)[0][0])
    x = o.rng_scalar(0x2FA, 0) % (1 << 128) or 1
    xinv = pow(x, -1, r)
    x_np = h.fr_mont_np(c, [x])[0]
    vals, mont = pool(c)
    u = ctx.vector(m)

    def run(fused, with_fold, with_h, cap):
        pre = 2 * m if with_fold else m
        d_c, d_z = ctx.upload(mont[0:pre]), ctx.upload(mont[32:32 + pre])
        xy = np.zeros((2, 2 * ctx.fq_limbs), dtype=np.uint64)
        inf = np.zeros((2,), dtype=np.uint8)
        ips = np.zeros((2, 4), dtype=np.uint64)
        try:
            ctx.set_vec_grid_max(cap)
            assert loops(ctx, half, reduce=True) == (cap != 0)
            if fused:
                ffi.check(ctx._lib.amsm_ipa_round_fused(ctx._h, key._h, None, 0, IPA_LOG_KEY, d_c.ptr, d_z.ptr,
                                                        _ptr(x_np) if with_fold else None, _ptr(h_prime) if with_h else None, u.ptr,
                                                        _ptr(xy), _ptr(inf), _ptr(ips)), "amsm_ipa_round_fused")
            else:
                ffi.check(ctx._lib.amsm_ipa_round(ctx._h, key._h, None, 0, IPA_LOG_KEY, d_c.ptr, d_z.ptr, u.ptr, _ptr(xy), _ptr(inf),
                                                  _ptr(ips)), "amsm_ipa_round")
        finally:
            ctx.set_vec_grid_max(CAP)
        return xy, inf, ips, d_c.download(), d_z.download()

    for fused, with_fold, with_h in ((False, False, False), (True, False, False), (True, False, True), (True, True, False),
                                     (True, True, True)):
        tag = (fused, with_fold, with_h)
        xy, inf, ips, cv, zv = run(fused, with_fold, with_h, CAP)
        cs, zs = vals[0:2 * m], vals[32:32 + 2 * m]
        if with_fold:
            cf = [(cs[i] + xinv * cs[m + i]) % r for i in range(m)]
            zf = [(zs[i] + x * zs[m + i]) % r for i in range(m)]
            assert h.fr_from_mont_np(c, cv[:m]) == cf and h.fr_from_mont_np(c, zv[:m]) == zf, tag
            assert np.array_equal(cv[m:], mont[m:2 * m]) and np.array_equal(zv[m:], mont[32 + m:32 + 2 * m]), tag
        else:
            cf, zf = cs[:m], zs[:m]
            assert np.array_equal(cv, mont[0:m]) and np.array_equal(zv, mont[32:32 + m]), tag
        got = h.fr_from_mont_np(c, ips)
        assert got[0] == sum(cf[half + i] * zf[i] for i in range(half)) % r, tag  # <c_r, z_l>
        assert got[1] == sum(cf[i] * zf[half + i] for i in range(half)) % r, tag  # <c_l, z_r>
        xy0, inf0, ips0, cv0, zv0 = run(fused, with_fold, with_h, 0)
        assert np.array_equal(xy, xy0) and np.array_equal(inf, inf0) and np.array_equal(ips, ips0), tag
        assert np.array_equal(cv, cv0) and np.array_equal(zv, zv0), tag
    key.free()


@pytest.mark.parametrize("c", ALL, ids=cid)
def test_edge_values_past_the_first_pass(capped, c):
    """tests/test_vec_gpu.py's pass over the carry-chain edge values, on the capped context: more pairs than lanes, so the
    operands just below r, 2 r and 3 r also meet the prefetch and the rotation of every kernel in that pass"""
    ctx = capped[c.name]
    n = edge_value_pass(ctx, c)
    assert n >= EDGE_PAIRS_MIN and loops(ctx, n) and loops(ctx, n, reduce=True)


# ---- the grids that ship: no cap, the first sizes at which they loop ---------------------------------------------------------

@pytest.fixture(scope="module")
def shipped():
    """An uncapped Pallas context and two random vectors of n = 64 CUs x 256 + 257 elements, born on the device
    (amsm_vec_random), with their host copies.  About 0.65 GiB of device memory at the peak (two inputs and three outputs)."""
    import torch
    from accumulation_amd import Context
    c = o.PALLAS
    ctx = Context(c.curve_id)
    cus = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    n = cus * 64 * 256 + 257
    assert ctx.vec_grid(n)[0] == cus * 64 and loops(ctx, n)
    x, y = ctx.random_vector(0x51, n, mont=True), ctx.random_vector(0x52, n, mont=True)
    yield ctx, c, n, x, y, x.download(), y.download()
    x.free()
    y.free()
    ctx.close()


def windows(n):
    """first lanes, the lanes whose second element is the vector's tail, the last lanes' first element and the tail itself"""
    w = list(range(0, 300)) + list(range(257 - 5, 257 + 5)) + list(range(n - 262 - 5, n)) + [n - 1]
    return sorted(set(w))


def test_shipped_grid_hadamard(shipped, cref):
    """Reference used: BOTH.  The whole output against the C restatement (cref.fr_hadamard: 4.2 M Montgomery products, measured
    at 0.6 s on one busy core of a build machine; the whole test takes under 0.2 s beside an MI355X, so it is quick enough) and
    the windows of the lanes around the loop's edges against Python integers, which ties the comparison to a second,
    independent reference."""
    from accumulation_amd.hp_as import compute_hp
    ctx, c, n, x, y, hx, hy = shipped
    out = compute_hp(ctx, x, y)
    got = out.download()
    out.free()
    assert np.array_equal(got, cref.fr_hadamard(c.curve_id, hx, hy))
    w = windows(n)
    assert h.fr_from_mont_np(c, got[w]) == o.compute_hp(c, h.fr_from_mont_np(c, hx[w]), h.fr_from_mont_np(c, hy[w]))


def test_shipped_grid_combine(shipped, cref):
    """a 2-vector combination with a unit first coefficient and a hiding vector shorter than n.  Reference used: BOTH, as for the
    Hadamard product (cref.fr_combine over 4.2 M elements: measured at 1.0 s on one busy core of a build machine; the whole test
    takes 0.35 s beside an MI355X)."""
    from accumulation_amd.hp_as import combine_vectors
    ctx, c, n, x, y, hx, hy = shipped
    hl = n - 300  # the hiding addend ends inside the second pass
    ch = [1, o.rng_fr(c, 0x53, 0) or 2]
    out = combine_vectors(ctx, [x, y], h.fr_mont_np(c, ch), y.view(0, hl))
    got = out.download()
    out.free()
    assert np.array_equal(got, cref.fr_combine(c.curve_id, [hx, hy], h.fr_mont_np(c, ch), hiding=hy[:hl]))
    w = windows(n)
    xs, ys = h.fr_from_mont_np(c, hx[w]), h.fr_from_mont_np(c, hy[w])
    exp = [(xv + ch[1] * yv + (yv if i < hl else 0)) % c.r for i, xv, yv in zip(w, xs, ys)]
    assert h.fr_from_mont_np(c, got[w]) == exp


def test_shipped_grid_t_vecs(shipped, cref):
    """a 2-input compute_t_vecs.  Reference used: BOTH (cref.fr_t_vecs over 4.2 M elements: measured at 3.3 s on one busy core
    of a build machine; the whole test takes 0.9 s beside an MI355X)."""
    from accumulation_amd.hp_as import compute_t_vecs
    ctx, c, n, x, y, hx, hy = shipped
    mu = [1, o.rng_fr(c, 0x54, 0) or 2]
    mu_np = h.fr_mont_np(c, mu)
    outs = compute_t_vecs(ctx, [x, y], [y, x], mu_np, n)
    got = [t.download() for t in outs]
    for t in outs:
        t.free()
    exp = cref.fr_t_vecs(c.curve_id, [hx, hy], [hy, hx], mu_np, n)
    for k in range(3):
        assert np.array_equal(got[k], exp[k]), k
    w = windows(n)
    xs, ys = h.fr_from_mont_np(c, hx[w]), h.fr_from_mont_np(c, hy[w])
    pexp = o.compute_t_vecs(c, [xs, ys], [ys, xs], mu, len(w), None)
    for k in range(3):
        assert h.fr_from_mont_np(c, got[k][w]) == pexp[k], k


def test_shipped_grid_inner_product(shipped):
    """amsm_vec_inner_product at n = 2^18 + 257, the first size past its 1024 workgroups, against Python integers"""
    ctx, c, _, x, y, hx, hy = shipped
    n = (1 << 18) + 257
    assert ctx.vec_grid(n)[1] == 1024 and loops(ctx, n, reduce=True)
    got = h.np_to_ints(inner_product(ctx, x, y, n).reshape(1, 4))[0]
    # the limbs as Python integers, A = a R and B = b R: the kernel's Montgomery sum is sum(A B) R^-1 mod r
    raw = lambda v: [int.from_bytes(v[i].tobytes(), "little") for i in range(n)]  # noqa: E731
    assert got == sum(p * q for p, q in zip(raw(hx), raw(hy))) * pow(1 << 256, -1, c.r) % c.r
