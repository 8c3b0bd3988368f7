"""Host-side mirror of `ASForTrivialPC` (reference: src/trivial_pc_as/mod.rs): index :310-330, prove :332-468,
verify :470-609, decide :611-632, over `ark_poly_commit::trivial_pc::TrivialPC` (ext), whose commitment is the
Pedersen commitment of the coefficient vector and whose opening "proof" is the polynomial itself.

SURVEY.md section 8(a) row a10 (BASELINE config 1): every commitment the scheme issues is an MSM of at most d+1 <=
2^10 pairs through the same ABI as the large ones (`amsm_pedersen_commit_device`); the O(d) polynomial work per
claim -- the quotient (p(X) - v) / (X - z), evaluations at the challenge point, the linear combination of the
witness polynomials -- is sequential host arithmetic in the reference.  Here it is host arithmetic (Python integers) while
the widest polynomial of a call has fewer than TRIVIAL_PC_DEVICE_MIN coefficients (config 1 is below it); from there on
it runs on the device as in include/amsm_trivial_pc_as.hpp: one upload per witness polynomial, amsm_poly_div_linear_batch,
the quotients committed from their device vectors, amsm_poly_evaluate_batch, amsm_vec_combine, one download of the combined
polynomial.  This mirror's polynomials stay lists of integers, so it pays a conversion on each side of the device calls: it
is the correctness mirror, speed is the C++ driver's business.  The sponge is pluggable like in the other mirrors (the SHA-256 stand-in, or sponge.PoseidonSponge: the reference's
sponge with ark-sponge's parameters restated as recalled); what is absorbed and squeezed, and in which order, follows the reference's
`absorb!` lists and is compared with their restatement outside the product in tests/test_transcripts_vs_oracle.py.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .engine import CommitterKey, Context, PedersenCommitment, VariableBaseMSM
from .hp_as import ASForHadamardProducts, MalformedAccumulator, MalformedInput, _pt_eq, combine_vectors
from .scalar_field import Fr
from .sponge import CryptographicSponge, Sha256Sponge

LINEAR_COMBINATION_CHALLENGE_SIZE = 126  # :31
CHALLENGE_POINT_SIZE = 184               # :32
_lincomb = ASForHadamardProducts._lincomb
# polynomials of at least this many coefficients take the device path (include/amsm.hpp: TRIVIAL_PC_DEVICE_MIN, the same number)
TRIVIAL_PC_DEVICE_MIN = 1 << 11


def _on_device(width: int) -> bool:
    """AMSM_TRIVIAL_PC_DEVICE=0: never; =1: always; unset, empty or anything else: the threshold (the same rule as
    include/amsm_trivial_pc_as.hpp: TrivialPC::on_device)"""
    e = os.environ.get("AMSM_TRIVIAL_PC_DEVICE")
    return e == "1" if e in ("0", "1") else width >= TRIVIAL_PC_DEVICE_MIN


def _ints_of(fr: Fr, limbs: np.ndarray) -> List[int]:
    """(n, 4) Montgomery limbs -> canonical integers"""
    b = np.ascontiguousarray(limbs, dtype="<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") * fr._rinv % fr.r for i in range(0, len(b), 32)]


@dataclass
class LabeledPolynomial:  # ark_poly_commit::LabeledPolynomial over DensePolynomial (ext)
    coeffs: List[int]                      # little-endian coefficients, trailing zeros allowed
    degree_bound: Optional[int] = None
    hiding_bound: Optional[int] = None

    def degree(self) -> int:
        d = len(self.coeffs) - 1
        while d > 0 and self.coeffs[d] == 0:
            d -= 1
        return max(d, 0)

    def evaluate(self, fr: Fr, x: int) -> int:
        acc = 0
        for c in reversed(self.coeffs):
            acc = (acc * x + c) % fr.r
        return acc


@dataclass
class LabeledCommitment:  # LabeledCommitment<trivial_pc::Commitment<G>> (ext)
    elem: tuple                            # (xy Montgomery limbs, is_inf)
    degree_bound: Optional[int] = None


@dataclass
class InputInstance:  # data_structures.rs:11-21
    commitment: LabeledCommitment
    point: int
    eval: int

    @staticmethod
    def zero(ctx: Context) -> "InputInstance":  # data_structures.rs:24-35
        return InputInstance(LabeledCommitment((np.zeros((2 * ctx.fq_limbs,), dtype=np.uint64), True)), 0, 0)


@dataclass
class SingleProof:  # data_structures.rs (Proof<G> = Vec<SingleProof<G>>)
    witness_commitment: LabeledCommitment
    witness_eval: int
    eval: int


@dataclass
class Input:
    instance: InputInstance
    witness: LabeledPolynomial


@dataclass
class Accumulator:
    instance: InputInstance
    witness: LabeledPolynomial


class TrivialPC:
    """ark_poly_commit::trivial_pc::TrivialPC (ext): setup / trim / commit / check."""

    @staticmethod
    def setup(ctx: Context, max_degree: int, seed: int = 0x7121A1, domain: Optional[bytes] = None) -> CommitterKey:
        """`domain`: a transparent key over that domain (PedersenCommitment.setup) instead of the seeded synthetic one"""
        return PedersenCommitment.setup(ctx, max_degree + 1, seed, domain=domain)

    @staticmethod
    def trim(pp: CommitterKey, supported_degree: int) -> Tuple[CommitterKey, CommitterKey]:
        """-> (ck, vk); both are the committer key truncated to supported_degree + 1 generators."""
        ctx = pp.ctx
        xy, inf = pp.read(0, supported_degree + 1)
        ck = CommitterKey.load(ctx, xy, inf, hiding_generator=pp.hiding_generator)
        return ck, ck

    @staticmethod
    def supported_degree(ck: CommitterKey) -> int:
        return len(ck) - 1

    @staticmethod
    def commit(ck: CommitterKey, poly: LabeledPolynomial) -> LabeledCommitment:
        """Pedersen commitment of the coefficient vector (no hiding: :145-158 rejects hiding bounds)."""
        ctx = ck.ctx
        fr = Fr(ctx.curve)
        n = min(len(poly.coeffs), len(ck))
        if n == 0:
            return LabeledCommitment((np.zeros((2 * ctx.fq_limbs,), dtype=np.uint64), True))
        vec = ctx.upload(fr.to_limbs_many([c % fr.r for c in poly.coeffs[:n]]))
        out = PedersenCommitment.commit(ck, vec, None)
        vec.free()
        return LabeledCommitment(out)

    @staticmethod
    def commit_many(ck: CommitterKey, polys) -> list:
        """several commitments under one key in ONE library call (amsm_msm_multi_device: small keys sum them in a single launch);
        the same points as len(polys) calls of commit()"""
        ctx = ck.ctx
        fr = Fr(ctx.curve)
        out = [LabeledCommitment((np.zeros((2 * ctx.fq_limbs,), dtype=np.uint64), True)) for _ in polys]
        jobs, which = [], []
        for k, poly in enumerate(polys):
            n = min(len(poly.coeffs), len(ck))
            if n == 0:
                continue
            jobs.append((0, ctx.upload(fr.to_limbs_many([c % fr.r for c in poly.coeffs[:n]]))))
            which.append(k)
        if jobs:
            pts, infs = VariableBaseMSM.multi_scalar_mul_multi(ck, jobs, mont=True)
            for j, k in enumerate(which):
                out[k] = LabeledCommitment((pts[j].copy(), bool(infs[j])))
            for _, v in jobs:
                v.free()
        return out

    @classmethod
    def check(cls, vk: CommitterKey, commitment: LabeledCommitment, point: int, value: int,
              polynomial: LabeledPolynomial) -> bool:
        """check_individual_opening_challenges with one commitment and opening challenge 1: the proof IS the
        polynomial: recommit and re-evaluate."""
        fr = Fr(vk.ctx.curve)
        if polynomial.degree() > cls.supported_degree(vk):
            return False
        if not hasattr(vk, "sharded") and _on_device(len(polynomial.coeffs)):  # one upload serves the commitment and the evaluation
            ctx = vk.ctx
            vec = ctx.upload(fr.to_limbs_many(polynomial.coeffs))
            try:
                # (trailing zeros beyond the key, or no coefficients at all: commit() knows what to do with them)
                fits = 0 < vec.n <= len(vk)
                cm = PedersenCommitment.commit(vk, vec, None) if fits else cls.commit(vk, polynomial).elem
                ev = fr.from_limbs(ctx.poly_evaluate([vec], fr.to_limbs(point))[0])
            finally:
                vec.free()
            return _pt_eq(cm, commitment.elem) and ev == value % fr.r
        return _pt_eq(cls.commit(vk, polynomial).elem, commitment.elem) and polynomial.evaluate(fr, point) == value % fr.r


def _poly_div_linear(fr: Fr, coeffs: Sequence[int], v: int, z: int) -> List[int]:
    """(p(X) - v) / (X - z) by synthetic division (the remainder p(z) - v is dropped, as `Div` does)."""
    n = len(coeffs)
    if n <= 1:
        return [0]
    q = [0] * (n - 1)
    carry = 0
    for i in range(n - 1, 0, -1):
        carry = (coeffs[i] + carry * z) % fr.r
        q[i - 1] = carry
    return q


class ASForTrivialPC:
    sponge_cls = Sha256Sponge

    @classmethod
    def index(cls, pp: CommitterKey, predicate_index: int):
        """:310-330 -> (prover key, verifier key = supported degree, decider key)"""
        ck, vk = TrivialPC.trim(pp, predicate_index)
        return ck, predicate_index, vk

    # ---- structure checks (:101-178) -----------------------------------------------------------------
    @staticmethod
    def _check_instance(inst: InputInstance, is_acc: bool) -> InputInstance:
        if inst.commitment.degree_bound is not None:
            raise (MalformedAccumulator if is_acc else MalformedInput)("Degree bounds on instances are unsupported.")
        return inst

    @staticmethod
    def _check_witness(w: LabeledPolynomial, pk: CommitterKey, is_acc: bool) -> LabeledPolynomial:
        err = MalformedAccumulator if is_acc else MalformedInput
        if w.degree_bound is not None:
            raise err("Degree bounds on witnesses are unsupported.")
        if w.hiding_bound is not None:
            raise err("Hiding bounds on witnesses are unsupported.")
        if w.degree() > TrivialPC.supported_degree(pk):
            raise err(f"A witness of degree {w.degree()} is unsupported for this prover key")
        return w

    # ---- sponge plumbing --------------------------------------------------------------------------------
    @staticmethod
    def _absorb_instance(sp: CryptographicSponge, fr: Fr, inst: InputInstance) -> None:  # data_structures.rs:38-55
        sp.absorb_point(inst.commitment.elem)
        sp.absorb_bytes((inst.point % fr.r).to_bytes(32, "little"))
        sp.absorb_bytes((inst.eval % fr.r).to_bytes(32, "little"))

    @classmethod
    def _challenge_point(cls, fr: Fr, sponge: CryptographicSponge, supported_degree: int, instances, wit_comms) -> int:
        sp = sponge.fork(b"")
        sp.absorb_u64(supported_degree)
        for inst, wc in zip(instances, wit_comms):
            cls._absorb_instance(sp, fr, inst)
            sp.absorb_point(wc.elem)
        return sp.squeeze_field_elements(1, CHALLENGE_POINT_SIZE)[0]

    @staticmethod
    def _lc_challenges(fr: Fr, sponge: CryptographicSponge, challenge_point: int, proof: Sequence[SingleProof]) -> List[int]:
        sp = sponge
        sp.absorb_bytes((challenge_point % fr.r).to_bytes(32, "little")[: (CHALLENGE_POINT_SIZE + 7) // 8])
        for p in proof:
            sp.absorb_bytes((p.eval % fr.r).to_bytes(32, "little"))
            sp.absorb_bytes((p.witness_eval % fr.r).to_bytes(32, "little"))
        return sp.squeeze_field_elements(2 * len(proof), LINEAR_COMBINATION_CHALLENGE_SIZE)

    # ---- prove (:332-468) ---------------------------------------------------------------------------------
    @classmethod
    def prove(cls, pk: CommitterKey, inputs: Sequence[Input], old_accumulators: Sequence[Accumulator], rng=None,
              sponge: Optional[CryptographicSponge] = None):
        ctx = pk.ctx
        fr = Fr(ctx.curve)
        sponge = sponge if sponge is not None else cls.sponge_cls()
        inputs = list(inputs)
        accs = list(old_accumulators)
        if not inputs and not accs:  # default input (:349-364)
            inputs = [Input(InputInstance.zero(ctx), LabeledPolynomial([0]))]
        instances = [cls._check_instance(i.instance, False) for i in inputs] + \
                    [cls._check_instance(a.instance, True) for a in accs]
        witnesses = [cls._check_witness(i.witness, pk, False) for i in inputs] + \
                    [cls._check_witness(a.witness, pk, True) for a in accs]
        if not hasattr(pk, "sharded") and _on_device(max(len(w.coeffs) for w in witnesses)):  # (a dist.ShardedCommitterKey -- a Python-only key type with no C++ twin -- keeps the host path)
            return cls._prove_device(pk, fr, sponge, instances, witnesses)
        # steps 1c-1d: witness polynomials w = (p - v) / (X - z) and their commitments (:181-222)
        wit_polys = [LabeledPolynomial(_poly_div_linear(fr, w.coeffs, inst.eval, inst.point))
                     for inst, w in zip(instances, witnesses)]
        wit_comms = TrivialPC.commit_many(pk, wit_polys)  # (the reference commits one by one, :198)
        # step 2: challenge point
        z = cls._challenge_point(fr, sponge, TrivialPC.supported_degree(pk), instances, wit_comms)
        # steps 3-4: evaluations at the challenge point, linear-combination challenges
        proof = [SingleProof(wc, wp.evaluate(fr, z), w.evaluate(fr, z)) for w, wp, wc in zip(witnesses, wit_polys, wit_comms)]
        ch = cls._lc_challenges(fr, sponge, z, proof)
        # step 5-7: combined polynomial / evaluation / commitment
        polys = witnesses + wit_polys
        width = max(len(p.coeffs) for p in polys)
        combined = [0] * width
        for c, p in zip(ch, polys):
            for i, cf in enumerate(p.coeffs):
                combined[i] = (combined[i] + c * cf) % fr.r
        combined_poly = LabeledPolynomial(combined)
        combined_eval = combined_poly.evaluate(fr, z)
        comms = [i.commitment.elem for i in instances] + [wc.elem for wc in wit_comms]
        combined_comm = _lincomb(ctx, comms, ch, fr)
        acc = Accumulator(InputInstance(LabeledCommitment(combined_comm), z, combined_eval), combined_poly)
        return acc, proof

    @classmethod
    def _prove_device(cls, pk: CommitterKey, fr: Fr, sponge, instances, witnesses):
        """The same steps with the polynomials on the device (the header of this file says when).  A constant witness has the
        quotient [0], as _poly_div_linear gives it."""
        ctx = pk.ctx
        K = len(instances)
        live = []  # every device vector of this call: released whatever happens in between

        def keep(v):
            live.append(v)
            return v

        try:
            wit_vecs = [keep(ctx.upload(fr.to_limbs_many(w.coeffs))) for w in witnesses]
            points = np.stack([fr.to_limbs(inst.point) for inst in instances])
            quots, _ = ctx.poly_div_linear(wit_vecs, points, remainders=False)  # steps 1c-1d (:181-222)
            live.extend(quots)
            for k in range(K):
                if quots[k].n == 0:
                    quots[k] = keep(ctx.upload(np.zeros((1, 4), dtype=np.uint64)))
            pts, infs = VariableBaseMSM.multi_scalar_mul_multi(pk, [(0, q.view(0, min(q.n, len(pk)))) for q in quots], mont=True)
            wit_comms = [LabeledCommitment((pts[k].copy(), bool(infs[k]))) for k in range(K)]
            z = cls._challenge_point(fr, sponge, TrivialPC.supported_degree(pk), instances, wit_comms)  # step 2
            polys = wit_vecs + quots
            evals = ctx.poly_evaluate(polys, fr.to_limbs(z))  # steps 3-4
            proof = [SingleProof(wit_comms[k], fr.from_limbs(evals[K + k]), fr.from_limbs(evals[k])) for k in range(K)]
            ch = cls._lc_challenges(fr, sponge, z, proof)
            combined = keep(combine_vectors(ctx, polys, np.stack([fr.to_limbs(c) for c in ch])))  # steps 5-7
            combined_eval = fr.from_limbs(ctx.poly_evaluate([combined], fr.to_limbs(z))[0])
            combined_poly = LabeledPolynomial(_ints_of(fr, combined.download()))
        finally:
            for v in live:
                v.free()
        comms = [i.commitment.elem for i in instances] + [wc.elem for wc in wit_comms]
        combined_comm = _lincomb(ctx, comms, ch, fr)
        return Accumulator(InputInstance(LabeledCommitment(combined_comm), z, combined_eval), combined_poly), proof

    # ---- verify (:470-609) --------------------------------------------------------------------------------
    @classmethod
    def verify(cls, ctx: Context, vk: int, input_instances: Sequence[InputInstance],
               old_accumulator_instances: Sequence[InputInstance], new_acc: InputInstance, proof: Sequence[SingleProof],
               sponge: Optional[CryptographicSponge] = None) -> bool:
        fr = Fr(ctx.curve)
        sponge = sponge if sponge is not None else cls.sponge_cls()
        try:
            instances = [cls._check_instance(i, False) for i in input_instances] + \
                        [cls._check_instance(a, True) for a in old_accumulator_instances]
            if not instances:
                instances = [InputInstance.zero(ctx)]
            cls._check_instance(new_acc, True)
        except (MalformedInput, MalformedAccumulator):
            return False
        if len(proof) != len(instances):
            return False
        # step 4: eval - v == w(z') * (z' - z) for every claim
        for inst, p in zip(instances, proof):
            if (p.eval - inst.eval) % fr.r != p.witness_eval * (new_acc.point - inst.point) % fr.r:
                return False
        # step 3: the challenge point
        z = cls._challenge_point(fr, sponge, vk, instances, [p.witness_commitment for p in proof])
        if z != new_acc.point % fr.r:
            return False
        # steps 5-7
        ch = cls._lc_challenges(fr, sponge, z, proof)
        evals = [p.eval for p in proof] + [p.witness_eval for p in proof]
        if sum(c * e for c, e in zip(ch, evals)) % fr.r != new_acc.eval % fr.r:
            return False
        comms = [i.commitment.elem for i in instances] + [p.witness_commitment.elem for p in proof]
        return _pt_eq(_lincomb(ctx, comms, ch, fr), new_acc.commitment.elem)

    # ---- decide (:611-632) --------------------------------------------------------------------------------
    @classmethod
    def decide(cls, dk: CommitterKey, accumulator: Accumulator, sponge=None) -> bool:
        return TrivialPC.check(dk, accumulator.instance.commitment, accumulator.instance.point, accumulator.instance.eval,
                               accumulator.witness)
