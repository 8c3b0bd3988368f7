"""The five device entry points of the IPA opening -- amsm_ipa_check_poly_coeffs, amsm_ipa_round_scalars, amsm_ipa_round,
amsm_ipa_round_fused, amsm_ipa_jump_fold -- against Python integers, on all six curves.

The reference (tests/curve_rows.py): a generated key has G_i = k_i G with k_i = mults(seed, i), so every sum of points the opening
forms is ONE scalar multiplication of the generator, `expect(C, mult, scalars)`; every field result is converted from Montgomery form
(and checked to be canonical) before it is compared.  The library's own other entry points serve as a reference in two places only,
both as a SECOND check beside the integers: the jump fold against CommitterKey.fold one challenge at a time (k_points_fold, another
kernel), and the untouched output classes of a degenerate key against the same jump over the generated key.

  A  check polynomial (k = 0, 1, 8, 9, 13: one coefficient, one workgroup exactly, the first second workgroup) and the round scalars
     (log_n = 1, 8, 9, every j, two vectors and one), whole outputs, the exact zeros included
  B  amsm_ipa_round and the four forms of amsm_ipa_round_fused over four kinds of key (the form each takes is read off
     csrc/msm_select.h kPipeline, pinned by tests/test_pipeline_select_cpu.py, and asserted from Context.pipeline_stats()), every round
     of the small keys, the last round (one lane, group_shift 0) of every key, and a round whose L is the identity
  C  the jump fold at all four table widths of csrc/msm_select.h kPrecomputedWindow that a key of up to 2^16 generators gets: 8, 10
     (a digit straddles two 64-bit words of S_t), 13 and 16 bits; lists cut into several pieces (`piece_rule` restates
     api_schemes.inc: ipa_jump_fold_impl over this module's own recoding, and a case that would not get there fails); gridDim.y = 2;
     keys with duplicate generators, P / -P runs and identities

Measured on the 10- and 13-bit cases (the rule is deterministic: the same on every curve up to the challenges' digits): n_rep = 6.

Teeth -- libraries built with one line of arithmetic or selection changed (none touches an address, a length or a loop bound), and
the cases of this module that go red with each, on every curve:
  the word-straddle OR removed from the jump's recoding   the 10- and 13-bit jumps (the older IPA modules stay green)
  hi doubled 7 times instead of 8                         the jumps at every width above 8 bits
  the host sums piece p = 0 only                          every jump with n_rep >= 2, the degenerate keys
  the kernel ignores an entry's sign bit                  every jump but the all-ones one (no negative digit there)
  k_ipa_round_scalars swaps idx and h + idx               the round scalars, the rounds, the identity round
  k_ipa_fold_ip folds z with xinv                         the rounds (their pending-fold variants)
  k_check_poly_coeffs reads bit i - 1                     the check polynomial at k = 8, 9, 13 (k = 0, 1: the same bit)
  ipa_round_impl adds hterm[1 - k]                        the rounds (their h' variants), the identity round"""
import numpy as np
import pytest

from oracle import pyref as o
from tests import helpers as h
from tests.curve_rows import ints, mults
from tests.test_vec_stride_gpu import ALL

pytestmark = pytest.mark.gpu
cid = lambda c: c.name  # noqa: E731

JUMP_NB = 256  # api_schemes.inc: values of a digit's byte, buckets per set


# ---- conversions ----------------------------------------------------------------------------------------------------------------------
def rinv(c):
    return pow(1 << 256, -1, c.r)


def to_mont(c, vals):
    """canonical integers -> (n, 4) uint64 Montgomery limbs"""
    if not len(vals):
        return np.zeros((0, 4), dtype=np.uint64)
    buf = b"".join((((int(v) % c.r) << 256) % c.r).to_bytes(32, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u8").reshape(-1, 4).astype(np.uint64)


def from_mont(c, a):
    """(n, 4) limbs -> canonical integers; the limbs themselves must be below r"""
    raw = ints(a)
    assert all(v < c.r for v in raw)
    ri = rinv(c)
    return [v * ri % c.r for v in raw]


def point_of(c, xy, inf):
    """the affine point of an output (None: the identity, whose words must be zero); coordinates canonical"""
    words = [int(v) for v in np.asarray(xy).reshape(-1)]
    if inf:
        assert not any(words)
        return None
    assert o.limbs_to_int(words[:c.limbs]) < c.p and o.limbs_to_int(words[c.limbs:]) < c.p
    pt = h.np_to_point(c, xy, inf)
    assert o.is_on_curve(c, pt)
    return pt


def times_g(c, m):
    return o.mul(c, m % c.r, o.generator(c))


def challenge(seed, i):
    return o.rng_scalar(seed, i) % (1 << 128) or 1


def challenges(c, seed, j):
    """j round challenges of 128 bits; from three on, one r - 1 and one 1 among them -- never in the last place, whose challenge the
    pending fold uses (1 and r - 1 are their own inverses: a fold could not tell x from 1 / x)"""
    xs = [challenge(seed, i) for i in range(j)]
    if j >= 2:
        xs[0] = c.r - 1
    if j >= 3:
        xs[1] = 1
    return xs


def products(c, xs):
    """S_t, t < 2^len(xs): the product of the challenges the bits of t pick, the first challenge by the TOP bit"""
    s = [1]
    for x in xs:
        s = [v for t in s for v in (t, t * x % c.r)]
    return s


# ---- one context per curve, pools of uniform field elements ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctxs():
    from accumulation_amd import Context
    out = {c.name: Context(c.curve_id) for c in ALL}
    yield out
    for ctx in out.values():
        ctx.close()


_pools = {}


def pool(ctx, c, n):
    """two vectors of at least n elements uniform below r (amsm_vec_random, as tests/test_skew_gpu.py takes them), as canonical
    integers and as the Montgomery limbs that were downloaded: made once per curve and size class, read-only"""
    size = 4096 if n <= 4096 else (1 << 17) + 1024
    assert n <= size
    if (c.name, size) not in _pools:
        out = []
        for k in (0, 1):
            v = ctx.random_vector(0x1A0 + 2 * c.curve_id + k + size, size, mont=True)
            mont = v.download()
            v.free()
            mont.setflags(write=False)
            out.append((from_mont(c, mont), mont))
        _pools[(c.name, size)] = out
    return _pools[(c.name, size)]


# ======================================================================================================================================
# A. the check polynomial and the round scalars
# ======================================================================================================================================
@pytest.mark.parametrize("c", ALL, ids=cid)
@pytest.mark.parametrize("k", [0, 1, 8, 9, 13])
def test_check_poly_coeffs(ctxs, c, k):
    """coefficient p of prod_i (1 + xi_i X^(2^(k - i))) is the product of the xi_i whose bit (k - i) is set in p"""
    from accumulation_amd import ffi
    from accumulation_amd.engine import _ptr
    ctx = ctxs[c.name]
    xs = [challenge(0x2A0 + k, i) for i in range(k)]
    if k == 1:
        xs[0] = o.rng_fr(c, 0x2A1, 0) % c.r or 2  # a full-size value
    if k >= 8:
        xs[1], xs[k // 2], xs[k - 1] = 1, o.rng_fr(c, 0x2A1, 1) % c.r or 2, c.r - 1
    want = []
    for p in range(1 << k):
        v = 1
        for i in range(1, k + 1):
            if (p >> (k - i)) & 1:
                v = v * xs[i - 1] % c.r
        want.append(v)
    out = ctx.upload(pool(ctx, c, 4096)[0][1][:1 << k] if k < 13 else np.tile(pool(ctx, c, 4096)[0][1], (2, 1)))  # no zeros, no ones
    assert out.n == 1 << k
    xi = to_mont(c, xs) if k else None
    ffi.check(ctx._lib.amsm_ipa_check_poly_coeffs(ctx._h, _ptr(xi), k, out.ptr), "amsm_ipa_check_poly_coeffs")
    assert from_mont(c, out.download()) == want
    assert len(want) == 1 << k and want[0] == 1
    out.free()


def test_check_poly_refuses_more_than_30_challenges(ctxs):
    """include/amsm.h: k <= 30.  The refusal comes before any launch; the output is untouched"""
    from accumulation_amd import ffi
    from accumulation_amd.engine import _ptr
    c = o.PALLAS
    ctx = ctxs[c.name]
    seen = pool(ctx, c, 4096)[0][1][:4]
    out = ctx.upload(seen)
    xi = to_mont(c, [challenge(0x2B0, i) for i in range(31)])
    assert ctx._lib.amsm_ipa_check_poly_coeffs(ctx._h, _ptr(xi), 31, out.ptr) == ffi.AMSM_E_INVALID_ARG
    assert np.array_equal(out.download(), seen)
    out.free()


@pytest.mark.parametrize("c", ALL, ids=cid)
@pytest.mark.parametrize("log_n", [1, 8, 9])
def test_round_scalars(ctxs, c, log_n):
    """vec_kernels.h k_ipa_round_scalars in integers: with h = n / 2^(j + 1) and s_j(k) the product of the challenges x_t (t < j)
    whose bit (log n - 1 - t) is set in k,
        u[k] = c[h + (k mod h)] s_j(k)   where bit (log n - 1 - j) of k is clear  (L's class)
        u[k] = c[k mod h] s_j(k)         where it is set                          (R's class)
    one vector: u; two vectors: out_l = u on L's class and exact zeros elsewhere, out_r likewise.  log_n = 1: h = 1."""
    from accumulation_amd import ffi
    from accumulation_amd.engine import _ptr
    ctx = ctxs[c.name]
    n = 1 << log_n
    (vals, mont), (_, junk) = pool(ctx, c, 4096)
    for j in range(log_n):
        m = n >> j
        hh = m // 2
        xs = challenges(c, 0x2C0 + log_n, j)
        s = products(c, xs)
        off = 29 * j
        cv = vals[off:off + m]
        u, right = [], []
        for k in range(n):
            g = (k >> (log_n - 1 - j)) & 1
            idx = k & (hh - 1)
            u.append((cv[idx] if g else cv[hh + idx]) * s[k >> (log_n - j)] % c.r)
            right.append(g)
        assert sum(right) == n // 2
        d_c = ctx.upload(mont[off:off + m])
        xi = to_mont(c, xs) if j else None
        out_l, out_r = ctx.upload(junk[:n]), ctx.upload(junk[7:7 + n])  # the zeros below are written, not left over
        ffi.check(ctx._lib.amsm_ipa_round_scalars(ctx._h, _ptr(xi), j, log_n, d_c.ptr, out_l.ptr, out_r.ptr), "amsm_ipa_round_scalars")
        got_l, got_r = out_l.download(), out_r.download()
        assert from_mont(c, got_l) == [0 if g else v for v, g in zip(u, right)], j
        assert from_mont(c, got_r) == [v if g else 0 for v, g in zip(u, right)], j
        assert not got_l[np.array(right, dtype=bool)].any() and not got_r[~np.array(right, dtype=bool)].any(), j  # zero WORDS
        one = ctx.upload(junk[:n])
        ffi.check(ctx._lib.amsm_ipa_round_scalars(ctx._h, _ptr(xi), j, log_n, d_c.ptr, one.ptr, None), "amsm_ipa_round_scalars (one vector)")
        assert from_mont(c, one.download()) == u, j
        assert np.array_equal(d_c.download(), mont[off:off + m]), j
        for v in (d_c, out_l, out_r, one):
            v.free()


# ======================================================================================================================================
# B. amsm_ipa_round and amsm_ipa_round_fused
# ======================================================================================================================================
# (log_key, key flags, rounds, the counter of Context.pipeline_stats() every round's grouped MSM must move -- None: the chunked
# pipeline, which has none, so no counter may move).  From csrc/msm_select.h kPipeline, first matching row:
#   direct     a default key of 2^6 generators carries the direct-sum table: KEY_DIRECT, (0, 2^15] pairs -> DIRECT_SUM (a round's index
#              classes are regular for every group_shift: n is a multiple of 2 << group_shift)
#   table      PRECOMPUTE | NO_DIRECT_TABLE, 2^10: KEY_TABLE below BPS_MIN_PAIRS = 2^16 -> CHUNKED, 8-bit windows (kPrecomputedWindow)
#   plain      NO_PRECOMPUTE, 2^10: KEY_PLAIN up to 2^17 pairs -> CHUNKED
#   bps        a default key of 2^16 generators has no direct-sum table (DIRECT_MAX_LOG2 = 15): KEY_TABLE, 2^16 pairs in
#              (2^16 - 1, 2^17] -> BUCKET_SPLIT, 16-bit windows
KEYS = {
    "direct": (6, "default", range(6), "direct_sum"),
    "table": (10, "table", range(10), None),
    "plain": (10, "plain", range(10), None),
    "bps": (16, "default", (0, 1, 9, 15), "bucket_split"),
}
COUNTERS = ("direct_sum", "bucket_split", "bucket_per_lane", "fallbacks", "bucket_split_fallbacks")
VARIANTS = ((False, False, False), (True, False, False), (True, False, True), (True, True, False), (True, True, True))  # fused, fold, h'
H_MULT = 0x5EED0A11CE  # h' = H_MULT G


def key_flags(name):
    from accumulation_amd import ffi
    return {"default": ffi.AMSM_BASES_DEFAULT, "table": ffi.AMSM_BASES_PRECOMPUTE | ffi.AMSM_BASES_NO_DIRECT_TABLE,
            "plain": ffi.AMSM_BASES_NO_PRECOMPUTE}[name]


def call_round(ctx, c, key, log_key, j, xs, c_mont, z_mont, fused, fold_x, h_xy):
    """one call on fresh device copies of the vectors -> (points, infinity flags, inner products, c and z as the call left them)"""
    from accumulation_amd import ffi
    from accumulation_amd.engine import _ptr
    d_c, d_z, u = ctx.upload(c_mont), ctx.upload(z_mont), ctx.vector(1 << log_key)
    xy = np.full((2, 2 * ctx.fq_limbs), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    inf = np.full((2,), 7, dtype=np.uint8)
    ips = np.zeros((2, 4), dtype=np.uint64)
    xi = to_mont(c, xs) if j else None
    if fused:
        fx = to_mont(c, [fold_x])[0] if fold_x is not None else None
        ffi.check(ctx._lib.amsm_ipa_round_fused(ctx._h, key._h, _ptr(xi), j, log_key, d_c.ptr, d_z.ptr, _ptr(fx), _ptr(h_xy), u.ptr,
                                                _ptr(xy), _ptr(inf), _ptr(ips)), "amsm_ipa_round_fused")
    else:
        assert fold_x is None and h_xy is None
        ffi.check(ctx._lib.amsm_ipa_round(ctx._h, key._h, _ptr(xi), j, log_key, d_c.ptr, d_z.ptr, u.ptr, _ptr(xy), _ptr(inf), _ptr(ips)),
                  "amsm_ipa_round")
    out = xy, inf, ips, d_c.download(), d_z.download()
    for v in (d_c, d_z, u):
        v.free()
    return out


def round_in_integers(c, mult, log_key, j, xs, cf, zf):
    """(<c_r, z_l>, <c_l, z_r>, multiplier of L_j, multiplier of R_j) of round j over the current vectors cf, zf (2 h elements):
    L_j = sum over k with bit (log n - 1 - j) clear of c[h + (k mod h)] s_j(k) k_k G, R_j over the others with c[k mod h];
    k = 2 h t + h g + i with t the top j bits (s_j(k) = S_t), g the class and i < h"""
    r, hh = c.r, 1 << (log_key - 1 - j)
    assert len(cf) == len(zf) == 2 * hh
    cl, cr, zl, zr = cf[:hh], cf[hh:], zf[:hh], zf[hh:]
    ip0, ip1 = sum(a * b for a, b in zip(cr, zl)) % r, sum(a * b for a, b in zip(cl, zr)) % r
    lm = rm = 0
    for t, s in enumerate(products(c, xs)):
        at = 2 * hh * t
        lm += s * sum(a * b for a, b in zip(cr, mult[at:at + hh]))
        rm += s * sum(a * b for a, b in zip(cl, mult[at + hh:at + 2 * hh]))
    return ip0, ip1, lm % r, rm % r


def h_prime(c):
    xy, _ = h.points_to_np(c, [times_g(c, H_MULT)])
    return np.ascontiguousarray(xy[0])


def check_round(ctx, c, key, mult, log_key, j, xs, cs, c_mont, zs, z_mont, tag, variants=VARIANTS):
    """every variant of round j over vectors whose first 2 m elements are given (m = 2^(log_key - j): the round's length; a pending
    fold takes all 2 m, the other variants the first m): inner products, folded vectors, untouched upper halves and both points"""
    r, m = c.r, 1 << (log_key - j)
    fold_x = xs[j - 1] if j else challenge(0x3F0, log_key)
    assert fold_x not in (1, r - 1)
    xinv = pow(fold_x, -1, r)
    folded = ([(cs[i] + xinv * cs[m + i]) % r for i in range(m)], [(zs[i] + fold_x * zs[m + i]) % r for i in range(m)])
    want = {False: round_in_integers(c, mult, log_key, j, xs, cs[:m], zs[:m]),
            True: round_in_integers(c, mult, log_key, j, xs, *folded)}
    points = {}
    for fused, fold, with_h in variants:
        t = tag + (fused, fold, with_h)
        n_in = 2 * m if fold else m
        xy, inf, ips, cv, zv = call_round(ctx, c, key, log_key, j, xs, c_mont[:n_in], z_mont[:n_in], fused, fold_x if fold else None,
                                          h_prime(c) if with_h else None)
        ip0, ip1, lm, rm = want[fold]
        assert from_mont(c, ips) == [ip0, ip1], t
        if fold:
            assert from_mont(c, cv[:m]) == folded[0] and from_mont(c, zv[:m]) == folded[1], t
            assert np.array_equal(cv[m:], c_mont[m:2 * m]) and np.array_equal(zv[m:], z_mont[m:2 * m]), t
        else:
            assert np.array_equal(cv, c_mont[:m]) and np.array_equal(zv, z_mont[:m]), t
        for g, (pm, ip) in enumerate(((lm, ip0), (rm, ip1))):
            k = (pm + ip * H_MULT) % r if with_h else pm
            if (g, k) not in points:
                points[(g, k)] = times_g(c, k)
            assert point_of(c, xy[g], inf[g]) == points[(g, k)], t + (g,)
        assert all(v in (0, 1) for v in inf), t


@pytest.mark.parametrize("c", ALL, ids=cid)
@pytest.mark.parametrize("kind", list(KEYS))
def test_rounds_against_integers(ctxs, c, kind):
    from accumulation_amd import CommitterKey
    ctx = ctxs[c.name]
    log_key, flags, rounds, counter = KEYS[kind]
    n, seed = 1 << log_key, 0x3A00 + 16 * c.curve_id + log_key
    assert log_key - 1 in rounds
    key = CommitterKey.generate(ctx, seed, n, key_flags(flags))
    assert key.precomputed == (kind != "plain") and (kind == "direct" or key.window_bits == {"table": 8, "plain": 0, "bps": 16}[kind])
    assert (key.tables()["direct_sum_table"] > 0) == (kind == "direct")
    mult = [v % c.r for v in mults(seed, n)]
    (cs, c_mont), (zs, z_mont) = pool(ctx, c, 2 * n)
    before = ctx.pipeline_stats()
    for j in rounds:
        off = 37 * j
        m2 = 2 * (n >> j)
        check_round(ctx, c, key, mult, log_key, j, challenges(c, 0x3B0 + log_key, j), cs[off:off + m2], c_mont[off:off + m2],
                    zs[off:off + m2], z_mont[off:off + m2], (kind, j))
    after = ctx.pipeline_stats()
    moved = {k: after[k] - before[k] for k in COUNTERS if after[k] != before[k]}
    assert moved == ({counter: len(rounds) * len(VARIANTS)} if counter else {}), moved
    key.free()


@pytest.mark.parametrize("c", ALL, ids=cid)
def test_round_whose_l_is_the_identity(ctxs, c):
    """c_r = 0: every scalar of L's class is zero, <c_r, z_l> = 0, so L_j is the identity with and without h' while R_j is finite --
    the batched normalisation with an identity among its inputs; out_lr_inf reads [1, 0]"""
    from accumulation_amd import CommitterKey
    ctx = ctxs[c.name]
    log_key, j = 10, 2
    n, m, seed = 1 << log_key, 1 << (log_key - j), 0x3C00 + c.curve_id
    key = CommitterKey.generate(ctx, seed, n, key_flags("table"))
    mult = [v % c.r for v in mults(seed, n)]
    (cs, c_mont), (zs, z_mont) = pool(ctx, c, 4096)
    cs, c_mont, zs, z_mont = list(cs[100:100 + m]), c_mont[100:100 + m].copy(), zs[100:100 + m], z_mont[100:100 + m]
    cs[m // 2:] = [0] * (m // 2)
    c_mont[m // 2:] = 0
    xs = challenges(c, 0x3C1, j)
    ip0, ip1, lm, rm = round_in_integers(c, mult, log_key, j, xs, cs, zs)
    assert (ip0, lm) == (0, 0) and ip1 and rm
    for fused, with_h in ((False, False), (True, False), (True, True)):
        xy, inf, ips, _, _ = call_round(ctx, c, key, log_key, j, xs, c_mont, z_mont, fused, None, h_prime(c) if with_h else None)
        assert list(inf) == [1, 0] and not xy[0].any(), (fused, with_h)
        assert from_mont(c, ips) == [0, ip1] and not ips[0].any(), (fused, with_h)
        assert point_of(c, xy[1], inf[1]) == times_g(c, rm + ip1 * H_MULT if with_h else rm), (fused, with_h)
    key.free()


# ======================================================================================================================================
# C. amsm_ipa_jump_fold
# ======================================================================================================================================
def jump_recode(s, cbits):
    """api_schemes.inc ipa_jump_fold_impl over integers: the signed cbits-bit digits of s, lowest first (a raw window above
    2^(cbits - 1) becomes raw - 2^cbits and carries), over 255 // cbits + 1 windows"""
    out, carry = [], 0
    for w in range(255 // cbits + 1):
        raw = ((s >> (cbits * w)) & ((1 << cbits) - 1)) + carry
        carry = 1 if raw > (1 << (cbits - 1)) else 0
        out.append(raw - (carry << cbits))
    assert carry == 0 and s >> (cbits * len(out)) == 0
    return out


def jump_lists(S, cbits):
    """entries per list: list (half, v) holds the (t, w) whose |digit| has byte `half` equal to v + 1 -- checked to add up to S_t"""
    counts = [0] * (2 * JUMP_NB)
    for s in S:
        back = 0
        for w, d in enumerate(jump_recode(s, cbits)):
            lo, hi = abs(d) & 255, abs(d) >> 8
            assert hi < JUMP_NB
            if lo:
                counts[lo - 1] += 1
            if hi:
                counts[JUMP_NB + hi - 1] += 1
            back += (-1 if d < 0 else 1) * (lo + (hi << 8)) << (cbits * w)
        assert back == s
    return counts


def piece_rule(counts):
    """(piece, n_rep) of ipa_jump_fold_impl: pieces of at least 32 entries and about 700 in all, at most 6 per list, a multiple of 4,
    grown until at most 720 pieces remain; n_rep = the pieces of the longest list"""
    total, longest = sum(counts), max(counts)
    piece = max(32, (total + 699) // 700)
    piece = max(piece, (longest + 5) // 6)
    piece = (piece + 3) // 4 * 4
    while sum((x + piece - 1) // piece for x in counts) > 720 and piece < 4096:
        piece += 4
    return piece, max(1, (longest + piece - 1) // piece)


def jump(ctx, c, ck, log_key, xs):
    from accumulation_amd.engine import _ptr
    j = len(xs)
    m0 = (1 << log_key) >> j
    xy = np.zeros((m0, 2 * ctx.fq_limbs), dtype=np.uint64)
    inf = np.full((m0,), 7, dtype=np.uint8)
    rc = ctx._lib.amsm_ipa_jump_fold(ctx._h, ck._h, log_key, _ptr(to_mont(c, xs)), j, _ptr(xy), _ptr(inf))
    return rc, xy, inf


def sampled(m0):
    """outputs 0, 1, 31, 32, 63 and the last of every 64 (lane 0 and 63 of a wave, the halves' edge, every gridDim.y block)"""
    return sorted({0, 1, 31, 32, 63} | {k for k in range(63, m0, 64)} | ({64} if m0 > 64 else set()))


# (log_key, j, window bits of the key's table, every challenge 1, least n_rep)
JUMPS = [(12, 6, 8, False, 1), (13, 7, 10, False, 2), (15, 9, 13, False, 2), (16, 10, 16, False, 2), (13, 6, 10, False, 2),
         (12, 6, 8, True, 2)]


@pytest.mark.parametrize("c", ALL, ids=cid)
@pytest.mark.parametrize("log_key,j,cbits,ones,min_rep", JUMPS, ids=["%d_%d_%dbit%s" % (a, b, w, "_ones" if u else "") for a, b, w, u, _ in JUMPS])
def test_jump_fold_across_table_widths(ctxs, c, log_key, j, cbits, ones, min_rep):
    """B_k = (sum_t S_t k_(t m0 + k)) G at the sampled outputs, and all m0 outputs bit for bit equal to the key folded physically one
    challenge at a time.  These shapes qualify by the rule above ipa_jump_fold_impl (a single-device precomputed key without the
    direct-sum table, equal-width windows covering 256 bits, m0 a multiple of 64): AMSM_OK, never a refusal"""
    from accumulation_amd import CommitterKey, ffi
    ctx = ctxs[c.name]
    n, m0, seed = 1 << log_key, (1 << log_key) >> j, 0x4A00 + 16 * c.curve_id + log_key
    xs = [1] * j if ones else [challenge(0x4B0 + log_key + j, i) for i in range(j)]
    S = products(c, xs)
    counts = jump_lists(S, cbits)  # (on the CPU, before the launch: the digits add up to S_t)
    piece, n_rep = piece_rule(counts)
    assert n_rep >= min_rep, (piece, n_rep)  # a case that would not cut its lists fails
    if ones:
        assert (piece, n_rep, counts[0], sum(counts)) == (32, 2, 1 << j, 1 << j)
    ck = CommitterKey.generate(ctx, seed, n, ffi.AMSM_BASES_PRECOMPUTE | ffi.AMSM_BASES_NO_DIRECT_TABLE)
    assert ck.window_bits == cbits and ck.tables()["direct_sum_table"] == 0
    rc, xy, inf = jump(ctx, c, ck, log_key, xs)
    assert rc == ffi.AMSM_OK
    mult = mults(seed, n)
    for k in sampled(m0):
        assert point_of(c, xy[k], inf[k]) == times_g(c, sum(s * mult[t * m0 + k] for t, s in enumerate(S))), k
    key, half = ck, n // 2
    for x in xs:
        nxt = key.fold(half, to_mont(c, [x])[0], 128)
        if key is not ck:
            key.free()
        key, half = nxt, half // 2
    fxy, finf = key.read()
    key.free()
    ck.free()
    assert np.array_equal(xy, fxy) and np.array_equal(inf, finf)


@pytest.mark.parametrize("c", ALL, ids=cid)
def test_jump_fold_over_degenerate_keys(ctxs, c):
    """A generated key of 2^12 points read back and three of its 64 output classes overwritten (j = 6, m0 = 64):
      k0   every G_(t m0 + k0) the same point P: the madd of k_ipa_jump_accum doubles, and so does the add of its LDS tree
      k1   P, -P, P, -P, ...: a wave's entries t, t + 4, .. are all P or all -P, the tree first doubles and then cancels
      k2   identities, the even t by the infinity flag (coordinates left in place) and the odd t as (0, 0)
    With every challenge 1 (one list of 64 entries, two pieces): B_k0 = 2^j P, B_k1 = B_k2 = the identity with its flag, every other
    class bit for bit what the generated key gives (itself compared with integers at the sampled outputs).  With random challenges:
    the integer formula over the adjusted multipliers.  P = k_k0 G, k_k1 G: points of the prime-order subgroup on every curve"""
    from accumulation_amd import CommitterKey, ffi
    ctx = ctxs[c.name]
    log_key, j, r = 12, 6, c.r
    n, m0, T, seed = 1 << log_key, 64, 64, 0x4C00 + c.curve_id
    k0, k1, k2 = 5, 32, 63
    flags = ffi.AMSM_BASES_PRECOMPUTE | ffi.AMSM_BASES_NO_DIRECT_TABLE
    gen = CommitterKey.generate(ctx, seed, n, flags)
    gxy, ginf = gen.read()
    assert not ginf.any()
    mult = [v % r for v in mults(seed, n)]
    xy, inf, adj = gxy.copy(), ginf.copy(), list(mult)
    p1 = point_of(c, gxy[k1], 0)
    assert p1 == times_g(c, mult[k1]) and point_of(c, gxy[k0], 0) == times_g(c, mult[k0])
    neg_xy = h.points_to_np(c, [o.neg(c, p1)])[0][0]
    for t in range(T):
        xy[t * m0 + k0], adj[t * m0 + k0] = gxy[k0], mult[k0]
        xy[t * m0 + k1], adj[t * m0 + k1] = (gxy[k1], mult[k1]) if t % 2 == 0 else (neg_xy, r - mult[k1])
        adj[t * m0 + k2] = 0
        if t % 2 == 0:
            inf[t * m0 + k2] = 1
        else:
            xy[t * m0 + k2] = 0
    deg = CommitterKey.load(ctx, xy, inf, flags)
    assert deg.window_bits == 8 and deg.tables()["direct_sum_table"] == 0
    ones = [1] * j
    assert piece_rule(jump_lists(products(c, ones), 8)) == (32, 2)
    rc, bxy, binf = jump(ctx, c, gen, log_key, ones)
    assert rc == ffi.AMSM_OK
    rc, dxy, dinf = jump(ctx, c, deg, log_key, ones)
    assert rc == ffi.AMSM_OK
    assert point_of(c, dxy[k0], dinf[k0]) == times_g(c, (1 << j) * mult[k0])
    assert point_of(c, dxy[k1], dinf[k1]) is None and point_of(c, dxy[k2], dinf[k2]) is None and dinf[k1] == 1 and dinf[k2] == 1
    rest = [k for k in range(m0) if k not in (k0, k1, k2)]
    assert np.array_equal(dxy[rest], bxy[rest]) and np.array_equal(dinf[rest], binf[rest])
    for k in sampled(m0):
        assert point_of(c, bxy[k], binf[k]) == times_g(c, sum(mult[t * m0 + k] for t in range(T))), k
    xs = [challenge(0x4C1, i) for i in range(j)]
    S = products(c, xs)
    jump_lists(S, 8)
    rc, rxy, rinf = jump(ctx, c, deg, log_key, xs)
    assert rc == ffi.AMSM_OK
    for k in sorted(set(sampled(m0)) | {k0, k1, k2}):
        want = times_g(c, sum(s * adj[t * m0 + k] for t, s in enumerate(S)))
        assert point_of(c, rxy[k], rinf[k]) == want, k
        assert (want is None) == (k == k2)
    gen.free()
    deg.free()
