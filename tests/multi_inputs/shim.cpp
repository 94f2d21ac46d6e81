// TEST HARNESS ONLY (never linked into libblsw.so): the N+1-pair product (one signature over K (pk_j, msg_j) pairs) with its keys, its messages and its
// signature allocated as Witness or Input, composed from the oracle's building blocks (oracle/ is not changed). mask bits: 1 keys, 4 messages, 8 signature.
//   messages  UInt8::new_input_vec per pair: 47-byte chunks as inputs, each decomposed by fto_bits_le (as tests/msg_input/shim.cpp), or u8witness_vec
//   keys      pv_new_input<FpT> (ProjectiveVar::new_variable_omit_prime_order_check: x, y, z inputs, no witnesses) or g1_new_witness
//   signature pv_new_input<Fp2T> or g2_new_witness
// then bls_verify_multi_gadget of oracle/circuit.h unchanged. Allocation order = column order: one, the messages' chunks pair by pair, the keys pair by
// pair, the signature, then the witnesses.
#include <cstring>
#include "../../oracle/circuit.h"

using namespace orc;

namespace {

const size_t CHUNK = 47;
enum { KEYS = 1, MSG = 4, SIG = 8 };

struct Scope {  // a private constraint system for one synthesis
    CS cs;
    CS* prev;
    explicit Scope(bool record, uint32_t n_inst) {
        cs.record = record;
        cs.n_inst = n_inst;
        prev = cur_cs();
        cur_cs() = &cs;
    }
    ~Scope() { cur_cs() = prev; }
};

size_t chunks(size_t msg_len) { return (msg_len + CHUNK - 1) / CHUNK; }
uint32_t n_inst_of(size_t K, size_t msg_len, int mask) {
    return 1 + (uint32_t)((mask & MSG) ? K * chunks(msg_len) : 0) + (uint32_t)((mask & KEYS) ? 3 * K : 0) + ((mask & SIG) ? 6 : 0);
}

std::vector<U8> u8input_vec(const uint8_t* msg, size_t len) {
    std::vector<Bool> bits;
    for (size_t j = 0; j < chunks(len); j++) {
        const size_t n = std::min(CHUNK, len - j * CHUNK);
        std::vector<uint8_t> be(n);
        for (size_t i = 0; i < n; i++) be[n - 1 - i] = msg[j * CHUNK + i];
        std::vector<Bool> b = fto_bits_le(finput(fp_from_be_bytes_mod_order(be.data(), n)));
        bits.insert(bits.end(), b.begin(), b.begin() + 8 * CHUNK);
    }
    std::vector<U8> r(len);
    for (size_t i = 0; i < len; i++)
        for (int k = 0; k < 8; k++) r[i].b[k] = bits[8 * i + k];
    return r;
}

// allocation order of the product (bls_verify_multi_circuit): msgs, params Constant, pks, sig
Bool circuit(const std::vector<G1Aff>& pks, const uint8_t* msgs, size_t len, const G2Aff& sig, int mask) {
    CSREF.mark("msg");
    std::vector<std::vector<U8>> msg_vars;
    for (size_t j = 0; j < pks.size(); j++) msg_vars.push_back((mask & MSG) ? u8input_vec(msgs + j * len, len) : u8witness_vec(msgs + j * len, len));
    G1Var g1 = pv_constant<FpT>(g1_generator());
    CSREF.mark("pk_alloc");
    std::vector<G1Var> pk_vars;
    for (auto& pk : pks) pk_vars.push_back((mask & KEYS) ? pv_new_input<FpT>(pk) : g1_new_witness(pk));
    CSREF.mark("sig_alloc");
    G2Var sig_var = (mask & SIG) ? pv_new_input<Fp2T>(sig) : g2_new_witness(sig);
    return bls_verify_multi_gadget(g1, pk_vars, msg_vars, sig_var);
}

G1Aff aff1(const uint64_t* in) {
    G1Aff a;
    memcpy(a.x.l, in, 48);
    memcpy(a.y.l, in + 6, 48);
    a.inf = fp_is_zero(a.x) && fp_is_zero(a.y);
    return a;
}
std::vector<G1Aff> affs(const uint64_t* in, size_t K) {
    std::vector<G1Aff> v;
    for (size_t k = 0; k < K; k++) v.push_back(aff1(in + 12 * k));
    return v;
}
G2Aff aff2(const uint64_t* in) {
    G2Aff a;
    memcpy(a.x.c0.l, in, 48);
    memcpy(a.x.c1.l, in + 6, 48);
    memcpy(a.y.c0.l, in + 12, 48);
    memcpy(a.y.c1.l, in + 18, 48);
    a.inf = fp2_is_zero(a.x) && fp2_is_zero(a.y);
    return a;
}
// a dummy instance for the shape-only calls (the matrices and the marks do not depend on values): generator keys, zero messages, sig = H(0...0)
G2Aff dummy_sig(size_t len) {
    std::vector<uint8_t> m(len + 1, 0);
    Scope s(false, 1);
    G2Var h = hash_to_g2_with_cons(u8const_vec(m.data(), len));
    return h.value_affine();
}

}  // namespace

extern "C" {

// witness_assignment (out_witness, capacity in elements; may be null), instance_assignment [n_inst][6] (element 0 = one; may be null), the gadget's
// Boolean and the constraint count. msgs [K][len]. Returns n_witness; *n_inst_out = n_instance_vars.
uint64_t mush_witness(const uint64_t* pks_xy, size_t K, const uint8_t* msgs, size_t len, const uint64_t* sig_xy, int mask, uint64_t* out_witness, uint64_t cap,
                      uint64_t* out_instance, uint64_t* n_inst_out, uint64_t* n_constraints, int* result) {
    Scope s(false, n_inst_of(K, len, mask));
    Bool r = circuit(affs(pks_xy, K), msgs, len, aff2(sig_xy), mask);
    if (result) *result = r.val;
    if (n_constraints) *n_constraints = s.cs.ncons;
    if (n_inst_out) *n_inst_out = s.cs.n_inst;
    const uint64_t n = s.cs.wit.size();
    if (out_witness) memcpy(out_witness, s.cs.wit.data(), std::min(n, cap) * 48);
    if (out_instance) {
        const Fp one = fp_one();
        memcpy(out_instance, one.l, 48);
        if (!s.cs.inst.empty()) memcpy(out_instance + 6, s.cs.inst.data(), s.cs.inst.size() * 48);
    }
    return n;
}
// segment marks of the shape in synthesis order (the hash marks repeat per pair): names '\n'-separated, starts[k] = witness index of mark k.
// Returns the number of marks.
uint64_t mush_layout(size_t K, size_t len, int mask, uint64_t* starts, uint64_t cap, char* names_buf, size_t names_cap, uint64_t* n_wit, uint64_t* n_cons,
                     uint64_t* n_inst) {
    std::vector<uint8_t> msg(K * len + 1, 0);
    G2Aff h = dummy_sig(len);
    Scope s(false, n_inst_of(K, len, mask));
    circuit(std::vector<G1Aff>(K, g1_generator()), msg.data(), len, h, mask);
    std::string names;
    uint64_t k = 0;
    for (auto& m : s.cs.marks) {
        if (k < cap) starts[k] = m.second;
        names += m.first;
        names += '\n';
        k++;
    }
    if (names_buf && names_cap) {
        const size_t c = std::min(names.size(), names_cap - 1);
        memcpy(names_buf, names.data(), c);
        names_buf[c] = 0;
    }
    *n_wit = s.cs.wit.size();
    *n_cons = s.cs.ncons;
    *n_inst = s.cs.n_inst;
    return k;
}
// CSR of A, B, C (two-phase: null arrays -> counts in nnz[3]). Returns the number of constraints.
uint64_t mush_matrices(size_t K, size_t len, int mask, uint64_t* nnz, uint64_t* n_witness, uint64_t* n_inst, uint64_t** row_ptr, uint32_t** col, uint64_t** val) {
    std::vector<uint8_t> msg(K * len + 1, 0);
    G2Aff h = dummy_sig(len);
    Scope s(true, n_inst_of(K, len, mask));
    circuit(std::vector<G1Aff>(K, g1_generator()), msg.data(), len, h, mask);
    const std::vector<LC>* M[3] = {&s.cs.A, &s.cs.B, &s.cs.C};
    for (int m = 0; m < 3; m++) {
        uint64_t k = 0;
        for (size_t i = 0; i < M[m]->size(); i++) {
            const LCv& row = *(*M[m])[i];
            if (row_ptr) row_ptr[m][i] = k;
            if (col)
                for (size_t t = 0; t < row.size(); t++) {
                    col[m][k + t] = row[t].v;
                    memcpy(val[m] + (k + t) * 6, row[t].c.l, 48);
                }
            k += row.size();
        }
        if (row_ptr) row_ptr[m][M[m]->size()] = k;
        nnz[m] = k;
    }
    *n_witness = s.cs.wit.size();
    *n_inst = s.cs.n_inst;
    return s.cs.ncons;
}
// Records the system of this instance and evaluates it on z = [instance | witness] (Montgomery limbs; either may be null: the shim's own
// assignment). Returns the first unsatisfied constraint, -1 when z satisfies the system, -2 on a length mismatch.
int64_t mush_check(const uint64_t* pks_xy, size_t K, const uint8_t* msgs, size_t len, const uint64_t* sig_xy, int mask, const uint64_t* instance,
                   const uint64_t* witness, uint64_t n_witness) {
    Scope s(true, n_inst_of(K, len, mask));
    circuit(affs(pks_xy, K), msgs, len, aff2(sig_xy), mask);
    std::vector<Fp> w = s.cs.wit, inst = s.cs.inst;
    if (witness) {
        if (n_witness != w.size()) return -2;
        memcpy(w.data(), witness, n_witness * 48);
    }
    if (instance && !inst.empty()) memcpy(inst.data(), instance + 6, inst.size() * 48);  // element 0 is the constant one
    for (size_t i = 0; i < s.cs.A.size(); i++) {
        const Fp a = lc_eval(*s.cs.A[i], w, &inst), b = lc_eval(*s.cs.B[i], w, &inst), c = lc_eval(*s.cs.C[i], w, &inst);
        if (!fp_eq(fp_mul(a, b), c)) return (int64_t)i;
    }
    return -1;
}
}
