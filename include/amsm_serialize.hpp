// amsm_serialize.hpp -- wire formats of the accumulation-scheme data structures: the ark-serialize 0.2
// `CanonicalSerialize` / `CanonicalDeserialize` encoding (ext) of every instance / witness / proof type the reference derives
// it for, over the C++ mirrors of include/amsm_*.hpp.  SURVEY.md section 8(f) rank 4.
//
//   reference type (file:line under /root/reference)                      mirror
//   hp_as::{InputInstance :13, InputWitness :53, InputWitnessRandomness :76, Proof :94, ProductPolynomialCommitment :107,
//           ProofHidingCommitments :132}  (src/hp_as/data_structures.rs)  amsm::hp_as::*
//   r1cs_nark::{FirstRoundMessageRandomness :54, FirstRoundMessage :100, SecondRoundMessageRandomness :151,
//           SecondRoundMessage :170, Proof :198}  (src/r1cs_nark_as/r1cs_nark/data_structures.rs)  amsm::r1cs_nark::*
//   r1cs_nark_as::{InputInstance :105, AccumulatorInstance :155, AccumulatorWitness :217, AccumulatorWitnessRandomness :230,
//           Proof :249, ProofRandomness :312}  (src/r1cs_nark_as/data_structures.rs)  amsm::r1cs_nark_as::*
//   ipa_pc_as::{InputInstance :55, Randomness :76}  (src/ipa_pc_as/data_structures.rs)  amsm::ipa_pc_as::*
//   trivial_pc_as::{InputInstance :13, SingleProof :63}  (src/trivial_pc_as/data_structures.rs)  amsm::trivial_pc_as::*
//   InstanceWitnessPair{instance, witness} (src/data_structures.rs:42-56: Input / Accumulator)  the mirrors' {instance, witness}
//
// Encoding (restated from the published ark-serialize / ark-ff / ark-ec 0.2; PARITY UNPINNED -- the reference holds no
// vectors and cannot be built here): a derived impl writes the fields in declaration order; field element = canonical
// integer, 32 bytes little-endian; point = compressed SW form (amsm.h: amsm_points_serialize); Vec<T> = u64 LE length + the
// elements; Option<T> = one byte 0 / 1 + the value; usize = u64 LE; String = Vec<u8>.  Types of ark-poly-commit (ext, git
// branch) are written field by field in the order of their struct definitions: LabeledCommitment{label: String, commitment,
// degree_bound: Option<usize>}, ipa_pc::Commitment{comm, shifted_comm: Option<G>}, ipa_pc::Proof{l_vec, r_vec,
// final_comm_key, c, hiding_comm: Option<G>, rand: Option<F>}, trivial_pc::Commitment{elem}, DensePolynomial{coeffs}; the
// accumulation schemes label every polynomial `PolynomialLabel::new()` = the empty string.
//
// `serialized_size(x)` is what examples/scaling-as.rs:123-131 prints for an accumulator, its instance and its witness.
// Device-resident vectors (FrVector) are downloaded / uploaded here; everything else is host data.
#pragma once
#include <cstdint>
#include <cstring>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include "amsm.hpp"
#include "amsm_hp_as.hpp"
#include "amsm_ipa_pc_as.hpp"
#include "amsm_r1cs_nark.hpp"
#include "amsm_r1cs_nark_as.hpp"
#include "amsm_trivial_pc_as.hpp"

namespace amsm {
namespace ser {

struct Writer {
  int curve;
  bool compressed = true;  // `serialize` (true) or `serialize_uncompressed`
  bool counting = false;   // `serialized_size`: only the length is tracked (device vectors are not downloaded)
  size_t count = 0;
  std::vector<uint8_t> buf;
  explicit Writer(int c, bool comp = true, bool count_only = false) : curve(c), compressed(comp), counting(count_only) {}
  size_t size() const { return counting ? count : buf.size(); }
  void u8(uint8_t v) {
    if (counting) count += 1;
    else buf.push_back(v);
  }
  void u64(uint64_t v) {
    if (counting) {
      count += 8;
      return;
    }
    for (int i = 0; i < 8; i++) buf.push_back((uint8_t)(v >> (8 * i)));
  }
  void bytes(const void* p, size_t n) {
    if (counting) {
      count += n;
      return;
    }
    const uint8_t* b = static_cast<const uint8_t*>(p);
    buf.insert(buf.end(), b, b + n);
  }
  uint8_t* grow(size_t n) {  // n bytes to be filled by the caller
    if (counting) {
      count += n;
      buf.resize(n);  // scratch
      return buf.data();
    }
    buf.resize(buf.size() + n);
    return buf.data() + buf.size() - n;
  }
};

struct Reader {
  int curve;
  bool compressed;
  const uint8_t* p;
  size_t n, pos = 0;
  Reader(int c, const std::vector<uint8_t>& b, bool comp = true) : curve(c), compressed(comp), p(b.data()), n(b.size()) {}
  const uint8_t* take(size_t k) {
    if (k > n - pos) throw Error(AMSM_E_INVALID_ARG, "deserialize: unexpected end of input");
    const uint8_t* q = p + pos;
    pos += k;
    return q;
  }
  uint8_t u8() { return *take(1); }
  uint64_t u64() {
    const uint8_t* q = take(8);
    uint64_t v = 0;
    for (int i = 0; i < 8; i++) v |= (uint64_t)q[i] << (8 * i);
    return v;
  }
  size_t len() {  // a Vec length: bounded by what is left so that a corrupt prefix cannot drive an allocation
    uint64_t v = u64();
    if (v > n - pos) throw Error(AMSM_E_INVALID_ARG, "deserialize: length prefix exceeds the input");
    return (size_t)v;
  }
  bool done() const { return pos == n; }
};

// ---- primitives --------------------------------------------------------------------------------------------------------
inline void put_fr(Writer& w, const Fr& mont) {  // F (Montgomery in memory) -> canonical LE
  check(amsm_fr_serialize(w.curve, mont.data(), 1, w.grow(32)), "amsm_fr_serialize");
}
inline Fr get_fr(Reader& r) {
  Fr out;
  check(amsm_fr_deserialize(r.curve, r.take(32), 1, out.data()), "amsm_fr_deserialize");
  return out;
}
// some mirrors keep O(#inputs) scalars as canonical integers (r1cs_nark_as::InputInstance::r1cs_input)
inline void put_fr_canonical(Writer& w, const Fr& canon) { w.bytes(canon.data(), 32); }
inline Fr get_fr_canonical(Reader& r) {
  Fr out, m;
  memcpy(out.data(), r.take(32), 32);
  check(amsm_fr_to_mont(r.curve, out.data(), 1, m.data()), "amsm_fr_to_mont");  // value check below
  Fr back;
  check(amsm_fr_from_mont(r.curve, m.data(), 1, back.data()), "amsm_fr_from_mont");
  if (back != out) throw Error(AMSM_E_INVALID_ARG, "deserialize: non-canonical field element");
  return out;
}
inline void put_point(Writer& w, const Affine& p) {
  const size_t sz = amsm_point_serialized_size(w.curve, w.compressed ? 1 : 0);
  uint8_t inf = p.infinity ? 1 : 0;
  std::vector<uint64_t> zero;
  const uint64_t* xy = p.xy.data();
  if (p.xy.empty()) {  // a default-constructed identity
    zero.assign(2 * (size_t)curve_info(w.curve).fq_limbs, 0);
    xy = zero.data();
    inf = 1;
  }
  check(amsm_points_serialize(w.curve, xy, &inf, 1, w.compressed ? 1 : 0, w.grow(sz)), "amsm_points_serialize");
}
inline Affine get_point(Reader& r) {
  const size_t sz = amsm_point_serialized_size(r.curve, r.compressed ? 1 : 0);
  Affine p;
  p.xy.assign(2 * (size_t)curve_info(r.curve).fq_limbs, 0);
  uint8_t inf = 0;
  check(amsm_points_deserialize(r.curve, r.take(sz), 1, r.compressed ? 1 : 0, p.xy.data(), &inf), "amsm_points_deserialize");
  p.infinity = inf != 0;
  return p;
}
inline void put_usize(Writer& w, size_t v) { w.u64((uint64_t)v); }
inline size_t get_usize(Reader& r) { return (size_t)r.u64(); }
inline void put_string(Writer& w, const std::string& s) {
  w.u64(s.size());
  w.bytes(s.data(), s.size());
}
inline std::string get_string(Reader& r) {
  size_t k = r.len();
  const uint8_t* q = r.take(k);
  return std::string(reinterpret_cast<const char*>(q), k);
}
template <class T, class F>
inline void put_option(Writer& w, const std::optional<T>& o, F&& put) {
  w.u8(o ? 1 : 0);
  if (o) put(w, *o);
}
template <class T, class F>
inline std::optional<T> get_option(Reader& r, F&& get) {
  uint8_t tag = r.u8();
  if (tag > 1) throw Error(AMSM_E_INVALID_ARG, "deserialize: Option tag");
  if (!tag) return std::nullopt;
  return get(r);
}
inline void put_points(Writer& w, const std::vector<Affine>& v) {
  w.u64(v.size());
  for (const Affine& p : v) put_point(w, p);
}
inline std::vector<Affine> get_points(Reader& r) {
  size_t k = r.len();
  std::vector<Affine> v;
  v.reserve(k);
  for (size_t i = 0; i < k; i++) v.push_back(get_point(r));
  return v;
}
inline void put_frs(Writer& w, const std::vector<Fr>& v) {  // Vec<F>, Montgomery in memory
  w.u64(v.size());
  if (w.counting) {
    w.count += 32 * v.size();
    return;
  }
  if (!v.empty()) check(amsm_fr_serialize(w.curve, v[0].data(), v.size(), w.grow(32 * v.size())), "amsm_fr_serialize");
}
inline std::vector<Fr> get_frs(Reader& r) {
  size_t k = r.len();
  if (k > (r.n - r.pos) / 32) throw Error(AMSM_E_INVALID_ARG, "deserialize: length prefix exceeds the input");
  std::vector<Fr> v(k);
  if (k) check(amsm_fr_deserialize(r.curve, r.take(32 * k), k, v[0].data()), "amsm_fr_deserialize");
  return v;
}
inline void put_frs_canonical(Writer& w, const std::vector<Fr>& v) {
  w.u64(v.size());
  for (const Fr& x : v) put_fr_canonical(w, x);
}
inline std::vector<Fr> get_frs_canonical(Reader& r) {
  size_t k = r.len();
  std::vector<Fr> v;
  v.reserve(k);
  for (size_t i = 0; i < k; i++) v.push_back(get_fr_canonical(r));
  return v;
}
// Vec<F> resident in HBM
inline void put_fr_vector(Writer& w, const FrVector& v) {
  if (w.counting) w.count += 8 + 32 * v.len();
  else put_frs(w, v.to_host());
}
inline std::shared_ptr<FrVector> get_fr_vector(Reader& r, Context& ctx) {
  return std::make_shared<FrVector>(ctx, get_frs(r));
}

// ---- hp_as (src/hp_as/data_structures.rs) ---------------------------------------------------------------------------------
inline void put(Writer& w, const hp_as::InputInstance& x) {  // :13-23
  put_point(w, x.comm_1);
  put_point(w, x.comm_2);
  put_point(w, x.comm_3);
}
inline void get(Reader& r, Context&, hp_as::InputInstance& x) {
  x.comm_1 = get_point(r);
  x.comm_2 = get_point(r);
  x.comm_3 = get_point(r);
}
inline void put(Writer& w, const hp_as::InputWitnessRandomness& x) {  // :76-88
  put_fr(w, x.rand_1);
  put_fr(w, x.rand_2);
  put_fr(w, x.rand_3);
}
inline hp_as::InputWitnessRandomness get_hp_rand(Reader& r) {
  hp_as::InputWitnessRandomness x;
  x.rand_1 = get_fr(r);
  x.rand_2 = get_fr(r);
  x.rand_3 = get_fr(r);
  return x;
}
inline void put(Writer& w, const hp_as::InputWitness& x) {  // :53-63
  put_fr_vector(w, *x.a_vec);
  put_fr_vector(w, *x.b_vec);
  put_option(w, x.randomness, [](Writer& ww, const hp_as::InputWitnessRandomness& v) { put(ww, v); });
}
inline void get(Reader& r, Context& ctx, hp_as::InputWitness& x) {
  x.a_vec = get_fr_vector(r, ctx);
  x.b_vec = get_fr_vector(r, ctx);
  x.randomness = get_option<hp_as::InputWitnessRandomness>(r, get_hp_rand);
}
inline void put(Writer& w, const hp_as::Proof& x) {  // :94-114, :132-144
  put_points(w, x.product_poly_comm.low);
  put_points(w, x.product_poly_comm.high);
  put_option(w, x.hiding_comms, [](Writer& ww, const hp_as::ProofHidingCommitments& h) {
    put_point(ww, h.comm_1);
    put_point(ww, h.comm_2);
    put_point(ww, h.comm_3);
  });
}
inline void get(Reader& r, Context&, hp_as::Proof& x) {
  x.product_poly_comm.low = get_points(r);
  x.product_poly_comm.high = get_points(r);
  x.hiding_comms = get_option<hp_as::ProofHidingCommitments>(r, [](Reader& rr) {
    hp_as::ProofHidingCommitments h;
    h.comm_1 = get_point(rr);
    h.comm_2 = get_point(rr);
    h.comm_3 = get_point(rr);
    return h;
  });
}
inline void put(Writer& w, const hp_as::Accumulator& x) {  // InstanceWitnessPair, src/data_structures.rs:42-56
  put(w, x.instance);
  put(w, x.witness);
}
inline void get(Reader& r, Context& ctx, hp_as::Accumulator& x) {
  get(r, ctx, x.instance);
  get(r, ctx, x.witness);
}

// ---- r1cs_nark (src/r1cs_nark_as/r1cs_nark/data_structures.rs) ---------------------------------------------------------------
inline void put(Writer& w, const r1cs_nark::FirstRoundMessage& x) {  // :100-113, :54-70
  put_point(w, x.comm_a);
  put_point(w, x.comm_b);
  put_point(w, x.comm_c);
  put_option(w, x.randomness, [](Writer& ww, const r1cs_nark::FirstRoundMessageRandomness& m) {
    put_point(ww, m.comm_r_a);
    put_point(ww, m.comm_r_b);
    put_point(ww, m.comm_r_c);
    put_point(ww, m.comm_1);
    put_point(ww, m.comm_2);
  });
}
inline void get(Reader& r, Context&, r1cs_nark::FirstRoundMessage& x) {
  x.comm_a = get_point(r);
  x.comm_b = get_point(r);
  x.comm_c = get_point(r);
  x.randomness = get_option<r1cs_nark::FirstRoundMessageRandomness>(r, [](Reader& rr) {
    r1cs_nark::FirstRoundMessageRandomness m;
    m.comm_r_a = get_point(rr);
    m.comm_r_b = get_point(rr);
    m.comm_r_c = get_point(rr);
    m.comm_1 = get_point(rr);
    m.comm_2 = get_point(rr);
    return m;
  });
}
inline void put(Writer& w, const r1cs_nark::SecondRoundMessage& x) {  // :170-177, :151-167
  put_fr_vector(w, *x.blinded_witness);
  put_option(w, x.randomness, [](Writer& ww, const r1cs_nark::SecondRoundMessageRandomness& s) {
    put_fr(ww, s.sigma_a);
    put_fr(ww, s.sigma_b);
    put_fr(ww, s.sigma_c);
    put_fr(ww, s.sigma_o);
  });
}
inline void get(Reader& r, Context& ctx, r1cs_nark::SecondRoundMessage& x) {
  x.blinded_witness = get_fr_vector(r, ctx);
  x.randomness = get_option<r1cs_nark::SecondRoundMessageRandomness>(r, [](Reader& rr) {
    r1cs_nark::SecondRoundMessageRandomness s;
    s.sigma_a = get_fr(rr);
    s.sigma_b = get_fr(rr);
    s.sigma_c = get_fr(rr);
    s.sigma_o = get_fr(rr);
    return s;
  });
}
inline void put(Writer& w, const r1cs_nark::Proof& x) {  // :198-205
  put(w, x.first_msg);
  put(w, x.second_msg);
}
inline void get(Reader& r, Context& ctx, r1cs_nark::Proof& x) {
  get(r, ctx, x.first_msg);
  get(r, ctx, x.second_msg);
}

// ---- r1cs_nark_as (src/r1cs_nark_as/data_structures.rs) -------------------------------------------------------------------
inline void put(Writer& w, const r1cs_nark_as::InputInstance& x) {  // :105-112 (r1cs_input: canonical in the mirror)
  put_frs_canonical(w, x.r1cs_input);
  put(w, x.first_round_message);
}
inline void get(Reader& r, Context& ctx, r1cs_nark_as::InputInstance& x) {
  x.r1cs_input = get_frs_canonical(r);
  get(r, ctx, x.first_round_message);
}
inline void put(Writer& w, const r1cs_nark_as::Input& x) {  // InstanceWitnessPair<InputInstance, SecondRoundMessage>
  put(w, x.instance);
  put(w, x.witness);
}
inline void get(Reader& r, Context& ctx, r1cs_nark_as::Input& x) {
  get(r, ctx, x.instance);
  get(r, ctx, x.witness);
}
inline void put(Writer& w, const r1cs_nark_as::AccumulatorInstance& x) {  // :155-171
  put_frs_canonical(w, x.r1cs_input);
  put_point(w, x.comm_a);
  put_point(w, x.comm_b);
  put_point(w, x.comm_c);
  put(w, x.hp_instance);
}
inline void get(Reader& r, Context& ctx, r1cs_nark_as::AccumulatorInstance& x) {
  x.r1cs_input = get_frs_canonical(r);
  x.comm_a = get_point(r);
  x.comm_b = get_point(r);
  x.comm_c = get_point(r);
  get(r, ctx, x.hp_instance);
}
inline void put(Writer& w, const r1cs_nark_as::AccumulatorWitness& x) {  // :217-227, :230-243
  put_fr_vector(w, *x.r1cs_blinded_witness);
  put(w, x.hp_witness);
  put_option(w, x.randomness, [](Writer& ww, const r1cs_nark_as::AccumulatorWitnessRandomness& s) {
    put_fr(ww, s.sigma_a);
    put_fr(ww, s.sigma_b);
    put_fr(ww, s.sigma_c);
  });
}
inline void get(Reader& r, Context& ctx, r1cs_nark_as::AccumulatorWitness& x) {
  x.r1cs_blinded_witness = get_fr_vector(r, ctx);
  get(r, ctx, x.hp_witness);
  x.randomness = get_option<r1cs_nark_as::AccumulatorWitnessRandomness>(r, [](Reader& rr) {
    r1cs_nark_as::AccumulatorWitnessRandomness s;
    s.sigma_a = get_fr(rr);
    s.sigma_b = get_fr(rr);
    s.sigma_c = get_fr(rr);
    return s;
  });
}
inline void put(Writer& w, const r1cs_nark_as::Accumulator& x) {
  put(w, x.instance);
  put(w, x.witness);
}
inline void get(Reader& r, Context& ctx, r1cs_nark_as::Accumulator& x) {
  get(r, ctx, x.instance);
  get(r, ctx, x.witness);
}
inline void put(Writer& w, const r1cs_nark_as::Proof& x) {  // :249-256, :312-325
  put(w, x.hp_proof);
  put_option(w, x.randomness, [](Writer& ww, const r1cs_nark_as::ProofRandomness& p) {
    put_frs_canonical(ww, p.r1cs_r_input);
    put_point(ww, p.comm_r_a);
    put_point(ww, p.comm_r_b);
    put_point(ww, p.comm_r_c);
  });
}
inline void get(Reader& r, Context& ctx, r1cs_nark_as::Proof& x) {
  get(r, ctx, x.hp_proof);
  x.randomness = get_option<r1cs_nark_as::ProofRandomness>(r, [](Reader& rr) {
    r1cs_nark_as::ProofRandomness p;
    p.r1cs_r_input = get_frs_canonical(rr);
    p.comm_r_a = get_point(rr);
    p.comm_r_b = get_point(rr);
    p.comm_r_c = get_point(rr);
    return p;
  });
}

// ---- ipa_pc / ipa_pc_as (ark-poly-commit ext; src/ipa_pc_as/data_structures.rs) --------------------------------------------
inline void put_labeled(Writer& w, const ipa_pc::Commitment& c) {  // LabeledCommitment<ipa_pc::Commitment<G>>
  put_string(w, std::string());                                    // PolynomialLabel::new()
  put_point(w, c.comm);
  put_option(w, c.shifted_comm, [](Writer& ww, const Affine& p) { put_point(ww, p); });
  w.u8(0);  // degree_bound: None (explicit degree bounds are refused, src/ipa_pc_as/mod.rs:112-128)
}
inline void get_labeled(Reader& r, ipa_pc::Commitment& c) {
  (void)get_string(r);
  c.comm = get_point(r);
  c.shifted_comm = get_option<Affine>(r, [](Reader& rr) { return get_point(rr); });
  (void)get_option<size_t>(r, [](Reader& rr) { return get_usize(rr); });
}
inline void put(Writer& w, const ipa_pc::Proof& x) {
  put_points(w, x.l_vec);
  put_points(w, x.r_vec);
  put_point(w, x.final_comm_key);
  put_fr(w, x.c);
  put_option(w, x.hiding_comm, [](Writer& ww, const Affine& p) { put_point(ww, p); });
  put_option(w, x.rand, [](Writer& ww, const Fr& f) { put_fr(ww, f); });
}
inline void get(Reader& r, Context&, ipa_pc::Proof& x) {
  x.l_vec = get_points(r);
  x.r_vec = get_points(r);
  x.final_comm_key = get_point(r);
  x.c = get_fr(r);
  x.hiding_comm = get_option<Affine>(r, [](Reader& rr) { return get_point(rr); });
  x.rand = get_option<Fr>(r, [](Reader& rr) { return get_fr(rr); });
}
inline void put(Writer& w, const ipa_pc_as::InputInstance& x) {  // :55-68
  put_labeled(w, x.ipa_commitment);
  put_fr(w, x.point);
  put_fr(w, x.evaluation);
  put(w, x.ipa_proof);
}
inline void get(Reader& r, Context& ctx, ipa_pc_as::InputInstance& x) {
  get_labeled(r, x.ipa_commitment);
  x.point = get_fr(r);
  x.evaluation = get_fr(r);
  get(r, ctx, x.ipa_proof);
}
inline void put(Writer& w, const ipa_pc_as::Randomness& x) {  // :76-86
  put_frs(w, x.random_linear_polynomial);  // DensePolynomial{coeffs}
  put_point(w, x.random_linear_polynomial_commitment);
  put_fr(w, x.commitment_randomness);
}
inline void get(Reader& r, Context&, ipa_pc_as::Randomness& x) {
  x.random_linear_polynomial = get_frs(r);
  x.random_linear_polynomial_commitment = get_point(r);
  x.commitment_randomness = get_fr(r);
}
inline void put(Writer& w, const ipa_pc_as::Proof& x) {  // Option<Randomness>
  put_option(w, x, [](Writer& ww, const ipa_pc_as::Randomness& v) { put(ww, v); });
}
inline void get(Reader& r, Context& ctx, ipa_pc_as::Proof& x) {
  x = get_option<ipa_pc_as::Randomness>(r, [&](Reader& rr) {
    ipa_pc_as::Randomness v;
    get(rr, ctx, v);
    return v;
  });
}

// ---- trivial_pc_as (src/trivial_pc_as/data_structures.rs) -------------------------------------------------------------------
inline void put(Writer& w, const trivial_pc_as::LabeledCommitment& c) {  // LabeledCommitment<trivial_pc::Commitment<G>>
  put_string(w, std::string());
  put_point(w, c.elem);
  put_option(w, c.degree_bound, [](Writer& ww, const size_t& d) { put_usize(ww, d); });
}
inline void get(Reader& r, Context&, trivial_pc_as::LabeledCommitment& c) {
  (void)get_string(r);
  c.elem = get_point(r);
  c.degree_bound = get_option<size_t>(r, [](Reader& rr) { return get_usize(rr); });
}
inline void put(Writer& w, const trivial_pc_as::InputInstance& x) {  // :13-23
  put(w, x.commitment);
  put_fr(w, x.point);
  put_fr(w, x.eval);
}
inline void get(Reader& r, Context& ctx, trivial_pc_as::InputInstance& x) {
  get(r, ctx, x.commitment);
  x.point = get_fr(r);
  x.eval = get_fr(r);
}
inline void put(Writer& w, const trivial_pc_as::SingleProof& x) {  // :63-73
  put(w, x.witness_commitment);
  put_fr(w, x.witness_eval);
  put_fr(w, x.eval);
}
inline void get(Reader& r, Context& ctx, trivial_pc_as::SingleProof& x) {
  get(r, ctx, x.witness_commitment);
  x.witness_eval = get_fr(r);
  x.eval = get_fr(r);
}
inline void put(Writer& w, const trivial_pc_as::Proof& x) {  // Vec<SingleProof>
  w.u64(x.size());
  for (const auto& p : x) put(w, p);
}
inline void get(Reader& r, Context& ctx, trivial_pc_as::Proof& x) {
  size_t k = r.len();
  x.clear();
  for (size_t i = 0; i < k; i++) {
    trivial_pc_as::SingleProof p;
    get(r, ctx, p);
    x.push_back(std::move(p));
  }
}
// the witness of a trivial_pc_as input is the LabeledPolynomial itself (ext): label, DensePolynomial{coeffs}, degree_bound,
// hiding_bound
inline void put(Writer& w, const trivial_pc_as::LabeledPolynomial& x) {
  put_string(w, std::string());
  put_frs(w, x.coeffs);
  put_option(w, x.degree_bound, [](Writer& ww, const size_t& d) { put_usize(ww, d); });
  put_option(w, x.hiding_bound, [](Writer& ww, const size_t& d) { put_usize(ww, d); });
}
inline void get(Reader& r, Context&, trivial_pc_as::LabeledPolynomial& x) {
  (void)get_string(r);
  x.coeffs = get_frs(r);
  x.degree_bound = get_option<size_t>(r, [](Reader& rr) { return get_usize(rr); });
  x.hiding_bound = get_option<size_t>(r, [](Reader& rr) { return get_usize(rr); });
}
inline void put(Writer& w, const trivial_pc_as::Input& x) {
  put(w, x.instance);
  put(w, x.witness);
}
inline void get(Reader& r, Context& ctx, trivial_pc_as::Input& x) {
  get(r, ctx, x.instance);
  get(r, ctx, x.witness);
}

// ---- entry points ---------------------------------------------------------------------------------------------------------
// `x.serialize(&mut bytes)`
template <class T>
inline std::vector<uint8_t> serialize(Context& ctx, const T& x, bool compressed = true) {
  Writer w(amsm_ctx_curve(ctx.get()), compressed);
  put(w, x);
  return std::move(w.buf);
}
// `T::deserialize(&bytes[..])`; throws amsm::Error(AMSM_E_INVALID_ARG) on malformed input or trailing bytes
template <class T>
inline T deserialize(Context& ctx, const std::vector<uint8_t>& bytes, bool compressed = true) {
  Reader r(amsm_ctx_curve(ctx.get()), bytes, compressed);
  T x;
  get(r, ctx, x);
  if (!r.done()) throw Error(AMSM_E_INVALID_ARG, "deserialize: trailing bytes");
  return x;
}
// `x.serialized_size()` (examples/scaling-as.rs:123-131)
template <class T>
inline size_t serialized_size(Context& ctx, const T& x) {
  Writer w(amsm_ctx_curve(ctx.get()), true, /*count_only=*/true);
  put(w, x);
  return w.size();
}

}  // namespace ser
}  // namespace amsm
