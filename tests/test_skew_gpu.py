"""The paths an MSM takes because of its scalars' VALUES, on all six curves (every point-side kernel among them is a template over
the base field; until now only Pallas, and partly BLS12-381, ran them with real work):
  heavy buckets      more than tune::K1 = 1024 partial records in one bucket: k_accum_l1's heavy list, k_accum_l2a, k_accum_l2b
  heavy partitions   more than PrepGeom::HEAVY (>= 2^17) entries in one partition: k_prep_heavy_count / k_prep_heavy_place
  two-valued form    k_tv_probe / k_tv_sum with up to TV_EXC_MAX = 8 exceptions (Pallas and BLS12-381: tests/test_two_valued_gpu.py)
  overflow flag      a bucket-per-lane or bucket-split prep that overflows sends the MSM to the chunked re-run
  hidden tails       the inner MSM of a batch: one_lane (k_bucket_reduce<Fq, false, false> + k_fold<false>) and red2 with
                     k_red2_weighted<Fq, false>, named by the library under AMSM_DEBUG=1 (tests/tail_forms_child.py, one child per curve)

Oracle: keys are generated (G_i = m_i G, the multiplier stream of tests/curve_rows.py), so the expected point of every MSM is ONE scalar
multiplication of the generator by sum s_i m_i mod r, in Python integers.  Every comparison is bit-exact.

Reach: Context.heavy_buckets() (amsm_ctx_heavy_buckets) counts the buckets k_accum_l1 listed as heavy.  `recode` below restates the
signed-digit walk of csrc/vec_kernels.h (digit_step, equal c-bit windows: every key here but the 20-bit one) and `populations` gives
the entries per bucket of a vector.  A chunk of the accumulation holds at most K0_MAX = 32 entries, so a bucket of more than
32 * 1024 entries has more than K1 partial records and MUST be heavy; a bucket of at most 1024 entries has at most 1024 and cannot
be.  The vectors are chosen so that no bucket lies between the two bounds (asserted), which makes the expected counter delta exact.
Heavy partitions have no counter (the prep's count stays on the device): they are reached by construction, a partition whose
population by `populations` exceeds the HEAVY of csrc/prep_geom.h restated in `prep_heavy`.

Teeth (libraries built with one kernel changed, each change in bounds; red tests of this module, the same on every curve):
  k_accum_l2a ends its loop over heavy buckets after one pass    test_heavy_buckets[three_values] (the older skew tests stay green)
  k_accum_l2a skips slice 31                                     every case that reaches a heavy bucket: all but test_hidden_tails
  k_accum_l1 takes `>=` for `>`                                  none: no bucket here holds exactly K1 partial records
  k_prep_heavy_place misplaces its last slice                    test_heavy_partitions, test_constant_vectors_reach_the_buckets[table]
  k_tv_sum drops the last exception's scalar                     test_two_valued_form
  one-lane k_bucket_reduce / k_red2_weighted drop their last lane  test_hidden_tails[plain] / [table20] (no older test reaches the latter)"""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyref as o
from tests import helpers as h
from tests.curve_rows import expect, got, ints, mults

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CURVES = {"pallas": o.PALLAS, "bls12_381_g1": o.BLS12_381_G1, "vesta": h.VESTA, "bn254_g1": h.BN254, "grumpkin": h.GRUMPKIN,
          "bls12_377_g1": h.BLS12_377}
K0_MAX, K1, TV_MIN_PAIRS, TV_EXC_MAX = 32, 1024, 1 << 14, 8  # csrc/launch.h tune::, api_pipeline.inc, vec_kernels.h
N = 1 << 17                # heavy buckets: a plain key's MSM of 2^17 pairs is chunked, 32 windows of 8 bits (msm_select.h: kPipeline, kPlainChunkedWindow)
N_KEY = (1 << 17) + (1 << 12)  # heavy partitions: more than 2^17 equal scalars and a uniform rest
N_BPL = (1 << 17) + 1      # the shortest plain-key MSM on the bucket-per-lane pipeline (15-bit windows)
N_BPS = 1 << 16            # the shortest bucket-split MSM
C_PLAIN, C_TABLE = 8, 16   # window widths: plain keys of 2^9 .. 2^19 pairs chunked; a precomputed key of 2^17 + 2^12 generators


# ---- the recoding and the prep geometry, restated -------------------------------------------------------------------------------------
def recode(s, c):
    """the signed digits of s over 255 // c + 1 windows of c bits, lowest first: a raw window above 2^(c - 1) becomes raw - 2^c and
    carries one into the next (vec_kernels.h: digit_step without narrow windows or a top shift)"""
    out, carry = [], 0
    for _ in range(255 // c + 1):
        raw = (s & ((1 << c) - 1)) + carry
        s >>= c
        carry = 1 if raw > (1 << (c - 1)) else 0
        out.append(raw - (carry << c))
    assert s == 0 and carry == 0  # (a scalar below 2^255 fits the windows)
    return out


def populations(scalars, c, plain, group_shift=None):
    """entries per bucket of the vector: {(group, bucket index): entries} -- a plain key has one bucket set per window, a precomputed
    one a single set for all windows; digits d and -d share bucket |d| - 1"""
    nb = 1 << (c - 1)
    groups = [0] * len(scalars) if group_shift is None else [(i >> group_shift) & 1 for i in range(len(scalars))]
    pops = collections.Counter()
    for (g, s), m in collections.Counter(zip(groups, scalars)).items():
        for w, d in enumerate(recode(s, c)):
            if d:
                pops[(g, (w * nb if plain else 0) + abs(d) - 1)] += m
    return pops


def heavy_expected(pops):
    """the exact number of heavy buckets: no population may leave it open"""
    between = {k: v for k, v in pops.items() if K1 < v <= K0_MAX * K1}
    assert not between, between
    return sum(1 for v in pops.values() if v > K0_MAX * K1)


def prep_heavy(n, c, plain):
    """(log2 buckets per partition, PrepGeom::HEAVY) of the chunked pipeline's prep for one group of n pairs (csrc/prep_geom.h: prep_geom;
    the index bits leave the partition size alone at these shapes)"""
    W, nb = 255 // c + 1, 1 << (c - 1)
    B, E = (W if plain else 1) * nb, n * W
    sh = 4
    while ((B + (1 << sh) - 1) >> sh) > 512 and sh < 10:
        sh += 1
    P = (B + (1 << sh) - 1) >> sh
    return sh, max(4 * (E // P + 1), 1 << 17)


def test_recoding_restatement():
    """the digits give the scalar back, a raw window of exactly 2^(c - 1) stays positive, one above it goes negative and carries"""
    for c in (C_PLAIN, 15, C_TABLE, 17):
        for C in CURVES.values():
            for s in (0, 1, 2, C.r - 1, C.r - 2, (1 << c) - 1, 1 << (c - 1), (1 << (c - 1)) + 1, o.rng_scalar(7, c) % C.r):
                d = recode(s, c)
                assert sum(x << (c * w) for w, x in enumerate(d)) == s and all(-(1 << (c - 1)) < x <= (1 << (c - 1)) for x in d)
        assert recode(1 << (c - 1), c)[:2] == [1 << (c - 1), 0] and recode((1 << (c - 1)) + 1, c)[:2] == [1 - (1 << (c - 1)), 1]
        assert recode((1 << c) - 1, c)[:2] == [-1, 1]


# ---- one context and key set per curve ------------------------------------------------------------------------------------------------
def to_np(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype="<u8").reshape(-1, 4).astype(np.uint64)


class Env:
    """the default context, one without the two-valued form and one without the skew probe (a context reads its switches when it is
    made), each with the SAME generated plain and precomputed key of N_KEY generators"""

    def __init__(self, name, monkeypatch):
        from accumulation_amd import CommitterKey, Context, ffi
        self.name, self.C = name, CURVES[name]
        self.seed = 0x5EED5000 + self.C.curve_id
        self.mult = mults(self.seed, N_KEY)
        self.ctx, self.keys = {}, {}
        for tag, var in (("default", None), ("no_tv", "AMSM_TWO_VALUED"), ("no_probe", "AMSM_BPL_PROBE")):
            with monkeypatch.context() as m:
                if var:
                    m.setenv(var, "0")
                self.ctx[tag] = Context(self.C.curve_id)
            self.keys[tag] = {
                "plain": CommitterKey.generate(self.ctx[tag], self.seed, N_KEY, ffi.AMSM_BASES_NO_PRECOMPUTE),
                "table": CommitterKey.generate(self.ctx[tag], self.seed, N_KEY, ffi.AMSM_BASES_PRECOMPUTE | ffi.AMSM_BASES_NO_DIRECT_TABLE)}
            assert not self.keys[tag]["plain"].precomputed and self.keys[tag]["table"].window_bits == C_TABLE
        v = self.ctx["default"].random_vector(self.seed + 1, N_KEY, False)  # uniform below r
        self.uniform = ints(v.download())
        v.free()
        assert all(0 < s < self.C.r for s in self.uniform[:3]) and len(set(self.uniform[:3])) == 3

    def close(self):
        for tag, c in self.ctx.items():
            for k in self.keys[tag].values():
                k.free()
            c.close()

    def msm(self, tag, key, scalars, mont=False, group_shift=None):
        """the MSM of a device vector over the first len(scalars) generators of the key; -> (the affine point(s), the counters that
        moved: heavy buckets, two-valued MSMs and those of pipeline_stats())"""
        from accumulation_amd import VariableBaseMSM
        ctx, ck, r = self.ctx[tag], self.keys[tag][key], self.C.r
        vec = ctx.upload(to_np([(s << 256) % r for s in scalars] if mont else scalars))
        before = dict(ctx.pipeline_stats(), heavy=ctx.heavy_buckets(), two_valued=ctx.two_valued_msms())
        if group_shift is None:
            res = got(self.C, *VariableBaseMSM.multi_scalar_mul(ck, vec, mont=mont))
        else:
            out, inf = VariableBaseMSM.multi_scalar_mul_grouped(ck, vec, group_shift, mont=mont)
            res = [got(self.C, out[g], inf[g]) for g in (0, 1)]
        after = dict(ctx.pipeline_stats(), heavy=ctx.heavy_buckets(), two_valued=ctx.two_valued_msms())
        vec.free()
        return res, {k: after[k] - before[k] for k in after if after[k] != before[k]}

    def want(self, scalars):
        return expect(self.C, self.mult, scalars)  # (zip stops at the vector's length)


@pytest.fixture(scope="module", params=list(CURVES))
def env(request, built_lib):
    mp = pytest.MonkeyPatch()
    e = Env(request.param, mp)
    yield e
    e.close()
    mp.undo()


def skewed(e, n, k):
    """the value x on every scalar but each k-th, which stays uniform"""
    sc = [e.uniform[0]] * n
    sc[::k] = e.uniform[:n:k]
    return sc


# ---- case 1: heavy buckets through k_accum_l1's list, k_accum_l2a and k_accum_l2b -----------------------------------------------------
@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])
@pytest.mark.parametrize("shape", ["two_values", "three_values", "one_value_and_a_uniform_tenth"])
def test_heavy_buckets(env, shape, mont):
    """2^17 pairs over the plain key: chunked, 32 bucket sets of 128 buckets.  Two values alternating: two buckets of 2^16 entries per
    window, about 64 heavy buckets -- one pass of k_accum_l2a's grid of (32 slices, 64); three values cycling: about 96, so its second
    pass runs (the LDS reused behind the trailing barrier); one value with a uniform tenth: heavy and ordinary buckets in one set.
    The counter moves by exactly what the restated recoding says (digit coincidences and zero digits included), and no vector is
    taken by the two-valued form"""
    x, y, z = env.uniform[:3]
    sc = {"two_values": [x, y] * (N // 2), "three_values": ([x, y, z] * (N // 3 + 1))[:N], "one_value_and_a_uniform_tenth": skewed(env, N, 10)}[shape]
    n_heavy = heavy_expected(populations(sc, C_PLAIN, True))
    lo, hi = {"two_values": (40, 64), "three_values": (65, 96), "one_value_and_a_uniform_tenth": (20, 33)}[shape]
    assert lo <= n_heavy <= hi, n_heavy  # (more than 64: k_accum_l2a's loop over gridDim.y goes round again)
    res, moved = env.msm("default", "plain", sc, mont=mont)
    assert moved == {"heavy": n_heavy}, (env.name, shape, moved)
    assert res == env.want(sc), (env.name, shape)


def test_heavy_buckets_grouped(env):
    """the same skewed vector as two sums by bit 16 of the index (amsm_msm_grouped_device): 64 bucket sets, each group's x-buckets heavy"""
    sc = skewed(env, N, 10)
    n_heavy = heavy_expected(populations(sc, C_PLAIN, True, group_shift=16))
    assert 40 <= n_heavy <= 64
    res, moved = env.msm("default", "plain", sc, group_shift=16)
    assert moved == {"heavy": n_heavy}, (env.name, moved)
    for g in (0, 1):
        assert res[g] == expect(env.C, env.mult, [s if (i >> 16) & 1 == g else 0 for i, s in enumerate(sc)]), (env.name, g)


# ---- case 2: the reference harness's constant vectors, with the two-valued form switched off -------------------------------------------
@pytest.mark.parametrize("key", ["plain", "table"])
def test_constant_vectors_reach_the_buckets(env, key):
    """vec![x; n], vec![r - 1; n], vec![1; n] and a few values whose digits sit at the recoding's edges, 2^17 pairs each, in a context
    with AMSM_TWO_VALUED=0: every non-zero digit is a bucket of 2^17 entries (a precomputed key's windows share one set, so equal
    digits of different windows share a bucket).  The counter equals the restated digits' count for every value -- the check of
    `recode` against the device's walk --, and nothing sums the unit scalars apart (that probe is the two-valued one)"""
    c, plain = (C_PLAIN, True) if key == "plain" else (C_TABLE, False)
    r = env.C.r
    for name, s in (("x", env.uniform[0]), ("r_minus_1", r - 1), ("one", 1), ("half_window", 1 << (c - 1)), ("half_window_plus_1", (1 << (c - 1)) + 1),
                    ("window_of_ones", (1 << c) - 1), ("ones_up_to_the_top", (1 << (r.bit_length() - 1)) - 1)):
        n_heavy = heavy_expected(populations([s] * N, c, plain))
        assert n_heavy == len({abs(d) if not plain else (w, d) for w, d in enumerate(recode(s, c)) if d}) >= 1
        res, moved = env.msm("no_tv", key, [s] * N)
        if key == "table":  # sent chunked by the skew probe: no other pipeline is counted
            assert moved == {"heavy": n_heavy}, (env.name, name, moved)
        assert moved["heavy"] == n_heavy and "two_valued" not in moved and "unit_scalar_sums" not in moved, (env.name, name, moved)
        assert res == env.want([s] * N), (env.name, name)


# ---- case 3: heavy partitions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,key", [("default", "plain"), ("no_probe", "plain"), ("default", "table")])
def test_heavy_partitions(env, tag, key):
    """2^17 + 2^12 pairs, every 32nd scalar uniform and the rest equal: more than 2^17 entries in one bucket, so its partition exceeds
    PrepGeom::HEAVY = 2^17 and is split over 64 workgroups.  Over the plain key the MSM is first tried on the bucket-per-lane
    pipeline, whose prep overflows (plain keys are not probed): the chunked re-run is the one that meets the heavy partitions"""
    c, plain = (C_PLAIN, True) if key == "plain" else (C_TABLE, False)
    sc = skewed(env, N_KEY, 32)
    pops = populations(sc, c, plain)
    sh, heavy = prep_heavy(N_KEY, c, plain)
    parts = collections.Counter()
    for (_, b), m in pops.items():
        parts[b >> sh] += m
    assert heavy == 1 << 17 and sum(1 for m in parts.values() if m > heavy) >= 1
    res, moved = env.msm(tag, key, sc)
    assert moved.pop("heavy") == heavy_expected(pops), (env.name, moved)
    assert moved in ({}, {"bucket_per_lane": 1, "fallbacks": 1}) and (key == "plain" or moved == {}), (env.name, moved)
    assert res == env.want(sc), env.name


# ---- case 4: the two-valued form, the four later curves included ------------------------------------------------------------------------------
def two_valued_vectors(e, n):
    """[(name, scalars, taken)]: for v in {a stream value, r - 1, 2} the constant vector, one with zeros, one exception at index 0, one at
    index n - 1 (the value r - 1, or a stream value where v is r - 1), eight exceptions (both ends among them, zeros as the other value)
    and nine"""
    r, u = e.C.r, e.uniform
    out = []
    for vn, v in (("stream", u[0]), ("r_minus_1", r - 1), ("two", 2)):
        edge = r - 1 if v != r - 1 else u[1]
        out.append((vn + "_constant", [v] * n, True))
        zeros = [0 if i % 3 == 0 else v for i in range(n)]
        out.append((vn + "_and_zeros", zeros, True))
        first = [v] * n
        first[0] = u[2]
        out.append((vn + "_exception_first", first, True))
        last = [v] * n
        last[n - 1] = edge
        out.append((vn + "_exception_last", last, True))
        eight = list(zeros)
        pos = (0, 70, 4099, n // 3 + 1, n // 3 + 2, n // 2 + 17, n - 2000, n - 1)
        for j, p in enumerate(pos):
            eight[p] = u[10 + j]
        eight[n - 1] = edge
        assert sum(1 for s in eight if s not in (0, v)) == TV_EXC_MAX
        out.append((vn + "_eight_exceptions", eight, True))
        nine = list(eight)
        nine[n // 5] = u[30]
        assert sum(1 for s in nine if s not in (0, v)) == TV_EXC_MAX + 1
        out.append((vn + "_nine_exceptions", nine, False))
    return out


@pytest.mark.parametrize("key", ["table", "plain"])
@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])
def test_two_valued_form(env, mont, key):
    """(the four later curves had one such vector, on Vesta; Pallas and BLS12-381 also have tests/test_two_valued_gpu.py) a batch of 2^14-pair vectors (TV_MIN_PAIRS): every vector with at most eight exceptions takes k_tv_probe / k_tv_sum, the ones with
    nine do not; the same vectors one pair shorter are below the probe's minimum and none takes it.  All results exact"""
    from accumulation_amd import VariableBaseMSM
    ctx, ck, r = env.ctx["default"], env.keys["default"][key], env.C.r
    n = TV_MIN_PAIRS
    vecs = two_valued_vectors(env, n)
    up = [ctx.upload(to_np([(s << 256) % r for s in sc] if mont else sc)) for _, sc, _ in vecs]
    for m in (n, n - 1):
        before = ctx.two_valued_msms()
        out, inf = VariableBaseMSM.multi_scalar_mul_batch(ck, [v.view(0, m) for v in up], mont=mont)
        taken = ctx.two_valued_msms() - before
        assert taken == (sum(1 for _, _, t in vecs if t) if m == n else 0), (env.name, m, taken)
        for j, (name, sc, _) in enumerate(vecs):
            assert got(env.C, out[j], inf[j]) == env.want(sc[:m]), (env.name, name, m)
    for v in up:
        v.free()


# ---- case 5: overflow re-runs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,n,attempt,fell", [("plain", N_BPL, "bucket_per_lane", "fallbacks"), ("table", N_BPS, "bucket_split", "bucket_split_fallbacks")])
def test_overflowing_prep_is_run_again_chunked(env, key, n, attempt, fell):
    """AMSM_BPL_PROBE=0: a uniform vector whose lowest 16 bits are 5 on every third scalar -- one digit of the lowest window, 15 or 16
    bits wide, for a third of the scalars -- is tried on the bucket-per-lane pipeline (a plain key, 2^17 + 1 pairs) or the
    bucket-split one (a precomputed key, 2^16 pairs); that bucket's partition overflows its fixed share, the flag sends the MSM to the
    chunked re-run, and the result is exact.  (Where the top window's reach differs -- BLS12-377, BN254 -- the partition loads and a
    plain key's top sets differ.)"""
    sc = list(env.uniform[:n])
    sc[::3] = [(s >> 16 << 16) | 5 for s in sc[::3]]
    assert all(s < env.C.r for s in sc)
    res, moved = env.msm("no_probe", key, sc)
    # (the re-run's heavy buckets are not counted here: a uniform vector's top window puts n / 64 .. n / 19 entries into each of its few
    # buckets, and the third's bucket holds 21 846 at 16-bit windows -- both between the bounds that decide)
    moved.pop("heavy", None)
    assert moved == {attempt: 1, fell: 1}, (env.name, moved)
    assert res == env.want(sc), env.name


# ---- case 6: the hidden tails, one child process per curve -----------------------------------------------------------------------------
N_TAIL = (1 << 18) + 1


@pytest.fixture(scope="module")
def tails(env, tmp_path_factory):
    """tests/tail_forms_child.py <inputs> <results> <curve id> under AMSM_DEBUG=1: two batches of two uniform vectors of 2^18 + 1 pairs, over
    a plain key and over the 20-bit key -> (results, the tail forms the library named per batch)"""
    d = tmp_path_factory.mktemp("skew_tails_" + env.name)
    inputs, results = str(d / "inputs.npz"), str(d / "results.npz")
    np.savez(inputs, seed=np.uint64(env.seed))
    run = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tests", "tail_forms_child.py"), inputs, results,
                          str(env.C.curve_id)], cwd=ROOT, env=dict(os.environ, AMSM_DEBUG="1"), capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr[-3000:])
    forms, case = {}, None
    for ln in run.stderr.splitlines():
        if ln.startswith("== "):
            case = ln[3:]
            forms[case] = []
        elif case and ln.startswith("[amsm] tail "):
            forms[case].append(ln.split()[2])
            assert ln.split()[-1] == "success" or "no error" in ln, ln
    return dict(np.load(results)), forms


@pytest.mark.parametrize("batch,inner", [("plain", "one_lane"), ("table20", "red2")])
def test_hidden_tails(env, tails, batch, inner):
    """the first MSM of each batch has another queued behind it, so its tail is hidden: 16 + T sets of 2^15 buckets (a plain key, 16-bit
    windows) take the one-lane reduction and fold, the 2^19 buckets of the 20-bit key the row / column form on single lanes"""
    res, forms = tails
    if batch + "_skipped" in res:
        pytest.skip("no device memory for the 20-bit key of 2^20 generators beside the other modules' keys")
    assert forms[batch][0] == inner and len(forms[batch]) == 2, (env.name, forms)
    mult = mults(env.seed, N_TAIL)
    for j in range(2):
        assert got(env.C, res[batch + "_xy"][j], res[batch + "_inf"][j]) == expect(env.C, mult, ints(res[batch + "_scalars"][j])), (env.name, j)
