"""The curve table of the per-curve suites (tests/test_<curve>_cpu.py, tests/test_<curve>_gpu.py): one `Row` per curve beyond Pallas and
BLS12-381 -- Vesta (2), BN254 G1 (4), Grumpkin (6), BLS12-377 G1 (8) -- with what the shared cases need and cannot derive from the
`Curve` objects of tests/helpers.py, the cases each row runs (their bodies, written once: tests/curve_cases_cpu.py, tests/curve_cases_gpu.py), and the helpers those
cases share, each taking the curve or its row.

Large MSMs need no big oracle: a generated key has G_i = k_i G with k_i = rng_scalar(seed, i) (pyref.rng_scalar, restated below with
numpy; where r < 2^254 a k_i may exceed r, which changes nothing: k_i G is taken over the integers), so
sum s_i G_i = (sum s_i k_i mod r) G, one scalar multiplication in Python.  The adversarial points at the head of an explicit key go
through the oracle's multiplication, one per point."""
import dataclasses
import functools
import json
import os
import re

import numpy as np

from oracle import pyref as o
from oracle import pyref_ser as ser
from tests import helpers as h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "accumulation_amd", "csrc")
# csrc/msm_select.h: an MSM over a 20-bit key is cut into ranges of RANGE_PAIRS = 2^20; a last range takes the bucket-per-lane row
# (and so joins the shared bucket set) only above a quarter of that, P2(18) -- a shorter one runs over the key's 17-bit twin, which
# it would have to build.  The smallest pair count above 2^20 that shares one bucket set without a twin:
N_SHARED = (1 << 20) + (1 << 18) + 1

# The cases every row runs, and the ones every row but Vesta runs (Vesta's suite is the oldest form: it has no shared bucket set, no
# polynomial, sampling or points-check case, and no adversarial-points fixture of its own)
_GPU_ALL = {"test_multiplier_stream_restatement", "test_bases_generate_vs_oracle", "test_msm_adversarial_keys",
            "test_edge_scalars_through_every_accumulation_form", "test_unit_scalars_summed_apart", "test_vector_kernels",
            "test_key_fold_vs_oracle", "test_cpp_driver_bytes_equal_the_mirror", "test_two_shards_on_one_gpu_equal_the_single_key"}
_GPU_LATER = {"test_msm_over_a_shared_bucket_set", "test_polynomial_kernels", "test_key_fold_over_the_negated_doubling_pair",
              "test_bases_sample_equals_the_host_backend", "test_points_check_equals_the_host_backend"}
_CPU_ALL = {"test_saturated_tables", "test_unsaturated_table", "test_generated_multiplication_header_is_current", "test_python_tables",
            "test_fr_helpers", "test_host_lincomb", "test_glv_pairing_and_split", "test_wire_format", "test_poseidon",
            "test_host_msm_adversarial", "test_host_bases_generate_matches_the_oracle_stream", "test_scheme_transcripts",
            "test_profile_as_dump_equals_the_mirror"}
_CPU_LATER = {"test_pack_names_stay_in_the_field_headers", "test_id_is_accepted_where_its_neighbours_are_refused",
              "test_host_bases_sample_against_the_python_sampler", "test_host_points_check"}


@dataclasses.dataclass(frozen=True, eq=False, repr=False)
class Row:
    id: str                 # the test ids' name, and the <id> of csrc/kern_<id>.hip
    curve: o.Curve
    ffi: str                # the id's name in accumulation_amd.ffi and include/amsm.h
    seed: int
    fixture: str            # the adversarial-points file under tests/golden/ (None: the curve has none)
    packs: tuple            # the field packs of csrc/fp.h and csrc/fpu.h: (Fq, FqU, Fr)
    unsat: tuple            # FqU's shape: (limbs, bits per limb)
    wire: tuple             # bytes of a compressed and of an uncompressed point
    gpu_cases: frozenset
    cpu_cases: frozenset
    refused_ids: tuple = ()  # the ids around this one that are no curve
    ipa_fold_of: int = 0    # the curve whose IPA fold thresholds this one takes
    cofactor: int = 1
    off_subgroup: int = 0   # points of the points-check case that are on the curve and outside the subgroup
    other_sponges: tuple = (o.PALLAS.p,)  # moduli whose Poseidon round constants must differ from this Fq's
    twins: tuple = ()       # the packs of fp.h over the same moduli as (Fq, Fr)
    dev_field: bool = True  # fp.h names DevField<Fq> (the curves after the first 9 x 29-bit one)
    fr_dots: bool = True    # fp_mul_gfx950.h has fe_dot2 / fe_dot3 generated for this Fr (Vesta's come from the template)
    header_extra: object = None  # (the generated header) -> None: what only this curve asserts of fp_mul_gfx950.h
    b_cases: object = None  # () -> (points, statuses) joined to the points-check case
    check_case: object = None  # (n) -> the curve's own points-check case, where the shared one does not describe it
    # -- the shapes in which the copies of the suite differed --
    over_r: tuple = (1, 1)  # the least count of multipliers k_i >= r among the 256 (64 on Vesta) of the GPU test and the 64 of the host test
    stream_n: int = 256
    generate_n: int = 256
    adv_log2n: tuple = (8, 12, 16)
    own_long_key: bool = False  # the 20-bit form generates its 2^20 key inside the test (no module key)
    vec_n: int = 1 << 12
    vec_edge: bool = True   # the vector kernels also multiply the field's edge values
    vec_top_bit: bool = True  # 300 uniform scalars reach the field's top bit
    fold: tuple = (1 << 8, 8)  # the fold's size, and the stride of the outputs compared
    fold_negated_doubling: bool = True  # x = r - 2 among the fold's scalars
    samples: tuple = ((b"PC-DL-2020", 1 << 10, 0), (b"PC-DL-2020", 1 << 10, (1 << 32) + 5))  # (domain, n, first)
    host_samples: tuple = ((0, 48), ((1 << 32) + 5, 16))  # (first, n)
    host_adv_n: int = 1 << 10
    cancel_pair: tuple = (0, 2)  # indices of a P / -P pair in adversarial()
    check_n: int = 1 << 10  # points of the GPU points-check case
    ladders: tuple = ()     # AMSM_SUBGROUP_LADDER settings of the GPU points-check case, a fresh context each (none: the module's context)
    aliases: tuple = ()     # (shared case, the name it keeps in this curve's modules)

    def __repr__(self):
        return "Row(%s)" % self.id

    @property
    def R(self):
        return self.curve.r

    @property
    def P(self):
        return self.curve.p


# ---- the multiplier stream of generated keys -------------------------------------------------------------------------------------------
def rng_scalar_limbs(seed, n):
    """(n, 4) uint64: the limbs of pyref.rng_scalar(seed, i), i < n (the multiplier stream of generated keys, the same on every curve)"""
    M = (1 << 64) - 1
    j = np.arange(4 * n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64((seed * 0xD1342543DE82EF95 + 0x632BE59BD9B4E019) & M) + j * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    z = z.reshape(n, 4)
    z[:, 3] &= np.uint64((1 << 62) - 1)
    return z


def ints(a):
    b = np.ascontiguousarray(a, dtype="<u8").reshape(-1, 4).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def mults(seed, n):
    return ints(rng_scalar_limbs(seed, n))


def expect(c, mult, scalars, mont=False):
    """sum s_i (m_i G): the affine oracle point (scalars in Montgomery form when mont)"""
    s = sum(a * b for a, b in zip(scalars, mult)) % c.r
    return o.mul(c, s * pow(1 << 256, -1, c.r) % c.r if mont else s, o.generator(c))


def got(c, xy, inf):
    return h.np_to_point(c, xy, inf)


# ---- the adversarial-points fixtures ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture(row):
    return json.load(open(os.path.join(ROOT, "tests", "golden", row.fixture))) if row.fixture else None


def _fixture_points(row, kind=None):
    out = []
    if row.fixture:
        for k, pts in fixture(row)["curves"][row.curve.name].items():
            if kind is None or k == kind:
                out += [(int(x, 16), int(y, 16)) for x, y in pts]
    return out


def negated_doubling_pair(row):
    """(l, r): l + (r_order - 2) r ends in the doubling of the negated r, whose internal y has a zero top limb"""
    pair = fixture(row)["negated_doubling_pair"]
    return tuple((int(pair[key][0], 16), int(pair[key][1], 16)) for key in ("l", "r"))


def adversarial_head(row):
    """the fixture's points, each as (P, P, -P, P) under one scalar -- equal digits double, double the negated point and cancel in
    one bucket --, then the negated-doubling pair as (l, r, r); -> (points, scalars, their sum by the oracle).  Empty where the curve
    has no fixture"""
    C, R = row.curve, row.R
    pts, sc, acc = [], [], None
    if not row.fixture:
        return pts, sc, acc
    edge = [R - 1, R - 2, (1 << 17) - 1, 15, (1 << 200) - 1, (1 << 16) - 1, 3, (1 << 128) + 1]
    k = 0
    for kind in fixture(row)["curves"][C.name].values():
        for x, y in kind:
            pt, s = (int(x, 16), int(y, 16)), edge[k % len(edge)]
            k += 1
            pts += [pt, pt, o.neg(C, pt), pt]
            sc += [s] * 4
            acc = o.add(C, acc, o.mul(C, 2 * s % R, pt))
    l, r = negated_doubling_pair(row)
    pts += [l, r, r]
    sc += [1, R - 2, R - 2]
    acc = o.add(C, acc, o.add(C, l, o.mul(C, 2 * (R - 2) % R, r)))
    return pts, sc, acc


def adversarial_key(ctx, row, head_pts, n, seed):
    """explicit points: the adversarial head, then a generated key's points with identities, duplicates and P / -P pairs:
    (xy, inf, multipliers of the entries behind the head)"""
    from accumulation_amd import CommitterKey, ffi
    C = row.curve
    hn = len(head_pts)
    assert hn < n
    hxy, hinf = h.points_to_np(C, head_pts)
    g = CommitterKey.generate(ctx, seed, n - hn, ffi.AMSM_BASES_NO_PRECOMPUTE)
    xy, inf = g.read()
    g.free()
    xy, inf, mult = xy.copy(), inf.copy(), mults(seed, n - hn)
    for i in range(0, n - hn, 89):
        xy[i], inf[i], mult[i] = 0, 1, 0
    for i in range(7, n - hn, 41):
        xy[i], inf[i], mult[i] = xy[i - 5], inf[i - 5], mult[i - 5]
    for i in range(13, n - hn, 37):
        q = got(C, xy[i - 1], inf[i - 1])
        q = None if q is None else o.neg(C, q)
        qxy, qinf = h.points_to_np(C, [q])
        xy[i], inf[i], mult[i] = qxy[0], qinf[0], (-mult[i - 1]) % C.r
    return np.concatenate([hxy, xy]), np.concatenate([hinf, inf]), mult


def adversarial(row, seed, n):
    """n points: the fixture's, each also doubled up, negated and in the negated-doubling shape (P, P, -P, P), then stream points with
    identities, duplicates and P / -P pairs; scalars with 0, 1, r - 1 and equal digits on the duplicates among them"""
    C, R = row.curve, row.R
    fix = _fixture_points(row)
    pts = []
    for pt in fix:
        pts += [pt, pt, o.neg(C, pt), pt]
    if fix:
        l, r = negated_doubling_pair(row)
        pts += [l, r, r]
    head = len(pts)
    assert head < n
    pts += o.rng_points(C, seed, n - head)
    for i in range(head, n, 97):
        pts[i] = None
    for i in range(head + 5, n, 61):
        pts[i] = pts[i - 3]
    for i in range(head + 11, n, 53):
        pts[i] = o.neg(C, pts[i - 1])
    sc = [o.rng_fr(C, seed + 1, i) % R for i in range(n)]
    for k in range(len(fix)):  # one scalar per fixture point's four entries: same bucket in every window, doubled, negated, cancelled
        s = [R - 1, R - 2, (1 << 17) - 1, 15, (1 << 200) - 1, sc[4 * k]][k % 6]
        sc[4 * k: 4 * k + 4] = [s, s, s, s]
    if fix:
        sc[head - 2], sc[head - 1] = R - 2, R - 2
    sc[head + 1], sc[head + 2], sc[head + 3] = 0, 1, R - 1
    return pts, sc


# ---- edge scalars through every accumulation form ------------------------------------------------------------------------------------
def edge_scalars(c):
    """the scalars a digit recoding can get wrong, all below r: the ends of the field, its middle, single bits and runs of ones at
    window boundaries, and for every window width w the library uses (msm_select.h: 8, 13, 15, 16, 17, 20) the window patterns
    around the signed digits' carry.  r lies between 2^k and 2^(k+1), so a scalar below r has k free bits (254 on Vesta, 253 on BN254
    and Grumpkin, 252 on BLS12-377): the patterns fill those."""
    R = c.r
    k = R.bit_length() - 1
    vals = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, 1 << k]
    for e in (16, 17, 20, 40, 128, 200, k):
        vals += [(1 << e) - 1, 1 << e]
    # 2^k - 1 (above) has EVERY window of every width all ones: each signed digit is -1 or 0 with a carry into the next, up to the top
    # window.  Beside it, per width: every window 2^w - 2 (with the carry all ones: every digit non-zero, negative and carrying),
    # 2^(w-1) (the sign boundary itself) and 2^(w-1) - 1 (the largest digit that does not carry)
    for w in (8, 13, 15, 16, 17, 20):
        for d in ((1 << w) - 2, 1 << (w - 1), (1 << (w - 1)) - 1):
            vals.append(sum(d << (w * j) for j in range(k // w + 1)) & ((1 << k) - 1))
    assert all(0 <= v < R for v in vals) and (1 << k) - 1 in vals and (1 << k) < R < (1 << (k + 1))
    return vals


# One case per accumulation form, at the smallest size the selection table (csrc/msm_select.h: kPipeline, key_window, tail_plan;
# pinned without a GPU by tests/test_pipeline_select_cpu.py) gives that form -- (key flags, generators, pairs, the counter of
# Context.pipeline_stats() that must move (None: the chunked pipeline, which has none), AMSM_BPL).  generators = 0: the 20-bit key
# (the module's long key; on Vesta a key of 2^20 generators made inside the test):
#   direct sum          any precomputed key of up to 2^15 generators carries the table of 4-bit signed digits
#   13-bit windows      a precomputed key of 2^15 generators without that table, chunked (key_window 2p15)
#   bucket-split        precomputed, 2^16 pairs: the lower edge of (2^16 - 1, 2^17]; 16-bit windows
#   one record per set  a plain key, 2^10 pairs, a blocking call: 8-bit windows, 32 sets of 128 buckets, the fused tail whose first quad
#                       folds serially (test_tail_plan_of_the_gpu_shapes: gpu_a_plain_2p10)
#   bucket-per-lane     plain keys from 2^17 + 1 pairs (15-bit windows) and from 2^18 + 1 (16-bit); over a precomputed key only with
#                       the 20-bit table, 2^20 generators, from 2^18 + 1 pairs (a precomputed key of 2^17 generators is bucket-split)
#   chunked             the same 2^17 + 1 pairs over a plain key in a context without bucket-per-lane: 8-bit windows at the size where
#                       the switch decides
# The chunked pipeline has no counter, so for its three cases (13-bit windows, one record per set, bucket-per-lane off) the device
# says only that no OTHER form ran: that these sizes mean these window widths and this tail form is pinned by
# tests/test_pipeline_select_cpu.py (key_window 2p15 / 2p9 .. 2p19, gpu_a_plain_2p10, "switch bpl=0") -- a change to the selection
# table shows there, and these sizes move with it.
#
# msel::choose is the same for every curve; what depends on r is bpl_geom's part_max (api_pipeline.inc), the entries the fullest
# 1024-bucket partition expects, which the top window decides.  The narrowest top window is BLS12-377's: raw top digits reach
# r >> 240 = 0x12ab (+ 1 for the carry).  At these shapes, against the stage's CAP = 40960 - 3620 = 37340 entries (kern_fr.hip):
#   plain, 15-bit windows, 2^17 + 1 pairs: top window 14 bits wide at bit 242, raw <= 1195, top_shift 1: reach 4780 buckets,
#                                          (2^17 + 1) * 1024 / 4780 = 28 080 (+ 5 sigma = 838): fits
#   plain, 16-bit windows, 2^18 + 1 pairs: raw <= 4780, top_shift 1: reach 9560, (2^18 + 1) * 1024 / 9560 = 28 080: fits
#   20-bit table, 2^18 + 1 pairs:          top_shift 5: reach 152 960; 12 * 512 + 1755 = 7899: fits (2^20 pairs: 31 596 + 889: fits)
# so every row stays on the pipeline the other curves take -- no row moves because of r's top window.  (A PLAIN key of 2^20 pairs
# would expect 2^20 * 1024 / 9560 = 112 316 entries and runs chunked, as on BN254: DESIGN.md 4.1.)
FORMS = {
    "direct_sum": (1, 1 << 12, 1 << 12, "direct_sum", None),
    "chunked_13_bit_table": (1 | 4, 1 << 15, 1 << 12, None, None),
    "bucket_split": (1, 1 << 16, 1 << 16, "bucket_split", None),
    "fused_tail_one_record": (2, 1 << 10, 1 << 10, None, None),
    "bucket_per_lane_plain_15_bit": (2, (1 << 17) + 1, (1 << 17) + 1, "bucket_per_lane", None),
    "bucket_per_lane_plain_16_bit": (2, (1 << 18) + 1, (1 << 18) + 1, "bucket_per_lane", None),
    "bucket_per_lane_20_bit_table": (1, 0, (1 << 18) + 1, "bucket_per_lane", None),
    "chunked_bpl_off": (2, (1 << 17) + 1, (1 << 17) + 1, None, "0"),
}


# ---- point validation ------------------------------------------------------------------------------------------------------------------
def raw_points(c, pts):
    """(x, y) integers -> the ABI's Montgomery words, whether or not the point is on the curve"""
    return np.array([o.int_to_limbs(x * c.R % c.p, c.limbs) + o.int_to_limbs(y * c.R % c.p, c.limbs) for x, y in pts], dtype=np.uint64)


def points_check_case(row, n=None):
    """(xy, infinity bytes, expected statuses, index of the first bad point) over n points (None: the fewest): the fixture's points and
    copies of the generator, eight of them overwritten with non-canonical words, points off the curve and the identity's forms, then
    the row's b-cases where it has some"""
    if row.check_case:
        return row.check_case(n)
    C, P = row.curve, row.P
    pts = _fixture_points(row)
    extra = row.b_cases() if row.b_cases else ([], [])
    k = len(pts)
    n = k + 10 + len(extra[0]) if n is None else n
    xy, _ = h.points_to_np(C, pts + [o.generator(C)] * (n - k))
    want = np.zeros(n, dtype=np.uint8)
    raw = lambda v: np.array(o.int_to_limbs(v, 4), dtype=np.uint64)  # noqa: E731
    xy[k, :4], want[k] = raw(P), 1                          # x = p
    xy[k + 1, 4:], want[k + 1] = raw(P + 1), 1              # y = p + 1
    xy[k + 2, :4], want[k + 2] = raw((1 << 256) - 1), 1     # every bit set
    xy[k + 3, 4:], want[k + 3] = raw(P - 1), 2              # canonical words, off the curve
    xy[k + 4, :4], want[k + 4] = xy[k + 4, 4:], 2           # (y, y)
    xy[k + 5] = 0                                           # (0, 0): the identity
    xy[k + 6, 4:], want[k + 6] = 0, 2                       # (x, 0)
    inf = np.zeros(n, dtype=np.uint8)
    xy[k + 7, :4], inf[k + 7] = raw(P), 1                   # flagged infinite: the words are ignored
    if extra[0]:
        xy[k + 8:k + 8 + len(extra[0])], want[k + 8:k + 8 + len(extra[0])] = raw_points(C, extra[0]), extra[1]
    xy[n - 1, 4:], want[n - 1] = raw(P), 1                  # the last point: y = p
    return xy, inf, want, k


# ---- the field tables ------------------------------------------------------------------------------------------------------------------
def _tables(src, name, limbs, bits):
    blk = src[src.index("struct " + name + " {"):]
    blk = blk[:blk.index("};")]

    def tab(t):
        mm = re.search(r"AMSM_TABLE\(" + t + r", \d+, ([^)]*)\)", blk, re.S)
        vals = [int(x.strip().rstrip("u"), 16) for x in mm.group(1).replace("\n", " ").split(",")]
        assert len(vals) == limbs and all(v < (1 << bits) for v in vals)
        return sum(v << (bits * i) for i, v in enumerate(vals))
    return blk, tab


# ---- Grumpkin's own: the signed b of the curve table (y^2 = x^3 - 17) -------------------------------------------------------------------
def old_cast_point():
    """a point of y^2 = x^3 + (2^64 - 17) over q: what `(u64)(-17)` made of b before curve_b_mont took a signed value"""
    P = h.GRUMPKIN.p
    x = 1
    while True:
        y = ser._sqrt((x * x * x + (1 << 64) - 17) % P, P)
        if y:
            return x, y
        x += 1


def grumpkin_b_cases():
    """(points as (x, y) integers, expected statuses): G, -G, (1, y + 1), a point of the curve the old cast of b described"""
    C = h.GRUMPKIN
    g = o.generator(C)
    wrong = old_cast_point()
    assert not o.is_on_curve(C, wrong) and (wrong[1] ** 2 - wrong[0] ** 3 - ((1 << 64) - 17)) % C.p == 0
    return [g, o.neg(C, g), (1, C.gy + 1), wrong], [0, 0, 2, 2]


def _grumpkin_header(out):
    # the products forward to the schedules of the same moduli; the sums of products are generated for p_BN under the new name,
    # and nothing is added for the field that is no curve's scalar field
    assert "return fe_cast<GrumpkinFq>(fe_mul<Bn254Fr>(" in out and "return fe_cast<GrumpkinFr>(fe_mul<Bn254Fq>(" in out
    assert "fe_dot2<Bn254Fq>" not in out and "fe_dot3<Bn254Fq>" not in out and "fe_dot2<GrumpkinFq>" not in out
    dot = out[out.index("fe_dot3<GrumpkinFr>"):]
    dot = dot[:dot.index("return r;")]
    assert all(f"0x{(h.GRUMPKIN.r >> (32 * j)) & 0xFFFFFFFF:08x}u" in dot for j in range(8))  # every limb of p_BN in its reduction


# (the cycle itself: BN254 coordinates as Grumpkin scalars and back)
def cycle_closes(ctx_a, A, ctx_b, B, seed):
    """Commit on curve A: four MSMs of 2^6 pairs.  The result points' x | y words -- ABI Montgomery form over A's base field, as
    the library returns them -- go UNCHANGED as `mont=True` scalars into one MSM on curve B, whose scalar field is that field;
    the oracle sums over the canonical integers."""
    from accumulation_amd import CommitterKey, VariableBaseMSM, ffi
    assert A.p == B.r and A.limbs == 4
    n, m = 1 << 6, 4
    ck_a = CommitterKey.generate(ctx_a, seed, n, ffi.AMSM_BASES_NO_PRECOMPUTE)
    pts_a = o.rng_points(A, seed, n)
    words, coords = [], []
    for t in range(m):
        sc = [o.rng_fr(A, seed + 1 + t, i) for i in range(n)]
        xy, inf = VariableBaseMSM.multi_scalar_mul(ck_a, h.scalars_to_np(sc))
        pt = h.np_to_point(A, xy, inf)
        assert pt is not None and pt == o.msm_pippenger(A, pts_a, sc)
        words.append(np.asarray(xy, dtype=np.uint64).reshape(2, 4))
        coords += [pt[0], pt[1]]
    ck_a.free()
    scalars = np.ascontiguousarray(np.concatenate(words))  # (2 m, 4): x_0, y_0, x_1, y_1, ...
    assert h.fr_from_mont_np(B, scalars) == coords
    ck_b = CommitterKey.generate(ctx_b, seed + 100, 2 * m, ffi.AMSM_BASES_NO_PRECOMPUTE)
    out, oinf = VariableBaseMSM.multi_scalar_mul(ck_b, scalars, mont=True)
    ck_b.free()
    want = None
    for c, g in zip(coords, o.rng_points(B, seed + 100, 2 * m)):
        want = o.add(B, want, o.mul(B, c, g))
    assert want is not None and h.np_to_point(B, out, oinf) == want


# ---- BLS12-377's own: a 253-bit r (the scalar stream's reduced fallback) and an even cofactor (small-order points) -----------------------
FALLBACK_INDICES = (2008, 14921, 38735, 45849, 61982)  # seed 1, below 2^16: the scalars whose 64 candidates are all >= r


@functools.lru_cache(maxsize=None)
def scalar_stream(seed, n):
    """the rule of csrc/rng.h restated for a modulus of 253 bits or fewer: pyref.rng_fr's value -- the first of 64 candidates below r,
    else candidate 63 with bit 254 cleared -- reduced mod r; -> (the canonical values, the indices where the literal rule gives >= r)"""
    C = h.BLS12_377
    lit = [o.rng_fr(C, seed, i) for i in range(n)]
    return tuple(v % C.r for v in lit), tuple(i for i, v in enumerate(lit) if v >= C.r)


def outside_subgroup_point():
    """the first x = 1, 2, ... with a point on BLS12-377's curve that [r] does not kill"""
    C = h.BLS12_377
    x = 1
    while True:
        y = ser._sqrt((x * x * x + C.b) % C.p, C.p)
        if y is not None and y != 0 and o.mul(C, C.r, (x, y)) is not None:
            return x, y
        x += 1


@functools.lru_cache(maxsize=None)
def cofactor_group_points():
    """[r]Q for the first curve points Q with x = 1, 2, ... outside the subgroup: points of the cofactor's torsion"""
    C = h.BLS12_377
    out, x = [], 1
    while len(out) < 3:
        y = ser._sqrt((x * x * x + C.b) % C.p, C.p)
        if y is not None and y != 0:
            q = o.mul(C, C.r, (x, y))
            if q is not None:
                assert o.is_on_curve(C, q) and o.mul(C, h.BLS12_377_H, q) is None
                out.append(q)
        x += 1
    return tuple(out)


def bls12_377_points_check_case(n=None):
    """(xy, infinity bytes, expected statuses, index of the first bad point): the fixture's points (0), (p - 1, 0), (0, 1), (2, 3) and
    three [r]Q (3 each: on the curve, outside the subgroup), a non-canonical coordinate (1), an off-curve point (2), the identity's
    forms, then the generator up to n points, the last one with y = p (1)"""
    C, P = h.BLS12_377, h.BLS12_377.p
    fix = _fixture_points(BLS12_377)
    bad = [(P - 1, 0), (0, 1), (2, 3)] + list(cofactor_group_points()) + [outside_subgroup_point()]
    k = len(fix)
    total = n if n is not None else k + len(bad) + 10
    pts = fix + bad + [o.generator(C)] * (total - k - len(bad))
    xy = raw_points(C, pts)
    want = np.zeros(total, dtype=np.uint8)
    want[k:k + len(bad)] = 3
    raw = lambda v: np.array(o.int_to_limbs(v, 6), dtype=np.uint64)  # noqa: E731
    j = k + len(bad)
    xy[j, :6], want[j] = raw(P), 1                        # x = p
    xy[j + 1, 6:], want[j + 1] = raw((1 << 384) - 1), 1   # every bit of y set
    xy[j + 2, 6:], want[j + 2] = raw(P - 1), 2            # canonical words, off the curve
    xy[j + 3, :6], want[j + 3] = xy[j + 3, 6:], 2         # (y, y)
    xy[j + 4] = 0                                         # (0, 0): the identity
    inf = np.zeros(total, dtype=np.uint8)
    xy[j + 5, :6], inf[j + 5] = raw(P), 1                 # flagged infinite: the words are ignored
    xy[total - 1, 6:], want[total - 1] = raw(P), 1        # the last point: y = p
    assert list(want[k:k + 9]) == [3, 3, 3, 3, 3, 3, 3, 1, 1] and not want[:k].any() and (want == 2).sum() == 2
    return xy, inf, want, k


def _bls12_377_header(out):
    C = h.BLS12_377
    assert "fe_dot2<Bls12377Fq>" not in out and "fe_dot3<Bls12377Fq>" not in out  # no curve's scalar field
    for name, m, words in (("fe_mul<Bls12377Fq>", C.p, 12), ("fe_dot3<Bls12377Fr>", C.r, 8)):
        body = out[out.index("> " + name):]
        body = body[:body.index("return r;")]
        assert all(f"0x{(m >> (32 * j)) & 0xFFFFFFFF:08x}u" in body for j in range(1, words))  # every limb above p_0 = 1 in its reduction


# ---- the table -------------------------------------------------------------------------------------------------------------------------
VESTA = Row(
    "vesta", h.VESTA, "AMSM_VESTA", 0x5EED2002, None, ("VestaFq", "VestaFqU", "VestaFr"), (9, 29), (33, 65),
    gpu_cases=frozenset(_GPU_ALL | {"test_pipelines_forced_once", "test_msm_2p22_exact"}),
    cpu_cases=frozenset(_CPU_ALL | {"test_host_vec_random_is_uniform_below_r"}),
    aliases=(("test_msm_adversarial_keys", "test_msm_explicit_adversarial_keys"),),
    dev_field=False, fr_dots=False, over_r=(0, 0), stream_n=64, generate_n=2048, adv_log2n=(8, 10, 12, 14, 16), own_long_key=True, vec_n=5000,
    vec_edge=False, vec_top_bit=False, fold=(1024, 16), fold_negated_doubling=False, cancel_pair=(10, 11))
BN254 = Row(
    "bn254", h.BN254, "AMSM_BN254_G1", 0x5EED4004, "bn254_adversarial_points.json", ("Bn254Fq", "Bn254FqU", "Bn254Fr"), (9, 29), (32, 64),
    gpu_cases=frozenset(_GPU_ALL | _GPU_LATER),
    cpu_cases=frozenset(_CPU_ALL | _CPU_LATER | {"test_host_vec_random_is_uniform_below_r", "test_adversarial_fixture_is_what_it_claims",
                                                 "test_generator_encoding_flag_bits_and_rejections"}),
    refused_ids=(3, 5), dev_field=False,
    aliases=(("test_id_is_accepted_where_its_neighbours_are_refused", "test_id_4_is_accepted_where_3_and_5_are_refused"),))
GRUMPKIN = Row(
    "grumpkin", h.GRUMPKIN, "AMSM_GRUMPKIN", 0x5EED6006, "grumpkin_adversarial_points.json", ("GrumpkinFq", "GrumpkinFqU", "GrumpkinFr"),
    (9, 29), (32, 64),
    gpu_cases=frozenset(_GPU_ALL | _GPU_LATER | {"test_the_cycle_closes"}),
    cpu_cases=frozenset(_CPU_ALL | _CPU_LATER | {"test_host_vec_random_is_uniform_below_r", "test_adversarial_fixture_is_what_it_claims",
                                                 "test_generator_encoding_flag_bits_and_rejections"}),
    aliases=(("test_id_is_accepted_where_its_neighbours_are_refused", "test_id_6_is_accepted_where_3_5_and_7_are_refused"),),
    refused_ids=(3, 5, 7), other_sponges=(h.BN254.p, o.PALLAS.p), twins=("Bn254Fr", "Bn254Fq"), header_extra=_grumpkin_header,
    b_cases=grumpkin_b_cases,
    samples=((b"PC-DL-2020", 1 << 10, 0), (b"PC-DL-2020", 1 << 6, (1 << 32) + 5), (b"grumpkin-odd-domain-7", 1 << 6, 0)))
BLS12_377 = Row(
    "bls12_377", h.BLS12_377, "AMSM_BLS12_377_G1", 0x5EED8008, "bls12_377_adversarial_points.json",
    ("Bls12377Fq", "Bls12377FqU", "Bls12377Fr"), (14, 28), (48, 96),
    gpu_cases=frozenset(_GPU_ALL | _GPU_LATER | {"test_scalar_stream_is_canonical", "test_group_law_on_the_small_order_points"}),
    cpu_cases=frozenset(_CPU_ALL | _CPU_LATER),
    aliases=(("test_id_is_accepted_where_its_neighbours_are_refused", "test_id_8_is_accepted_where_3_5_and_7_are_refused"),),
    refused_ids=(3, 5, 7, 9), ipa_fold_of=1, cofactor=h.BLS12_377_H, off_subgroup=7, other_sponges=(o.BLS12_381_G1.p,),
    header_extra=_bls12_377_header, check_case=bls12_377_points_check_case, over_r=(129, 33), fold=(1 << 9, 16),
    samples=((b"PC-DL-2020", 1 << 8, 0), (b"PC-DL-2020", 1 << 6, (1 << 32) + 5), (b"bls12-377-odd-domain7", 1 << 6, 0)),
    host_samples=((0, 24), ((1 << 32) + 5, 8)), host_adv_n=1 << 9, check_n=512, ladders=("1", "2"))
ROWS = (VESTA, BN254, GRUMPKIN, BLS12_377)


def take(cases, names, aliases=()):
    """What a per-curve module takes from a module of shared cases (tests/curve_cases_cpu.py, tests/curve_cases_gpu.py), as a dict for
    its globals(): the fixtures and hook that module names in SHARED, and the cases in `names` -- under the name the curve's own suite
    always had where `aliases` gives one.  The module sets ROW first: the fixtures read it."""
    aliases = dict(aliases)
    out = {n: getattr(cases, n) for n in cases.SHARED}
    out.update({aliases.get(n, n): getattr(cases, n) for n in names})
    return out
