// TEST HARNESS ONLY (never linked into libblsw.so): the aggregate_verify circuit of constraints.rs:378-441 with each of its four arguments allocated
// as Witness or Input, composed from the oracle's building blocks (oracle/ is not changed). mask bits: 1 keys, 2 bitmap, 4 message, 8 signature.
//   keys      pv_new_input<FpT> (ProjectiveVar::new_variable_omit_prime_order_check: x, y, z inputs, no witnesses) or g1_new_witness
//   bitmap    CSREF.new_input + the booleanity constraint (1 - b) * b = 0 (AllocatedBool::new_variable with Input), or balloc
//   message   UInt8::new_input_vec: 47-byte chunks as inputs, each decomposed by fto_bits_le (as tests/msg_input/shim.cpp), or u8witness_vec
//   signature pv_new_input<Fp2T> or g2_new_witness
// then mapped_aggregate and bls_verify_gadget of oracle/circuit.h unchanged. Allocation order = column order: one, keys, bitmap, message, signature,
// then the witnesses.
#include <cstring>
#include "../../oracle/circuit.h"

using namespace orc;

namespace {

const size_t CHUNK = 47;
enum { KEYS = 1, BITMAP = 2, MSG = 4, SIG = 8 };

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
    return 1 + (uint32_t)((mask & KEYS) ? 3 * K : 0) + (uint32_t)((mask & BITMAP) ? K : 0) + (uint32_t)((mask & MSG) ? chunks(msg_len) : 0) + ((mask & SIG) ? 6 : 0);
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
// AllocatedBool::new_variable(.., Input): an instance variable with the booleanity constraint of every allocated boolean
Bool binput(bool v) {
    Var x = CSREF.new_input(fp_of_bool(v));
    CSREF.enforce(lc_sub(lc_const(fp_one()), lc_var(x)), lc_var(x), lc_zero());
    return {1, v, x};
}

Bool circuit(const std::vector<G1Aff>& pks, const uint8_t* bitmap, const uint8_t* msg, size_t len, const G2Aff& sig, int mask, uint32_t* count_value) {
    CSREF.mark("agg.keys");
    std::vector<G1Var> keys;
    for (auto& pk : pks) keys.push_back((mask & KEYS) ? pv_new_input<FpT>(pk) : g1_new_witness(pk));
    CSREF.mark("agg.bitmap");
    std::vector<Bool> bits;
    for (size_t k = 0; k < pks.size(); k++) bits.push_back((mask & BITMAP) ? binput(bitmap[k] != 0) : balloc(bitmap[k] != 0));
    CSREF.mark("msg");
    std::vector<U8> msg_var = (mask & MSG) ? u8input_vec(msg, len) : u8witness_vec(msg, len);
    G1Var g1 = pv_constant<FpT>(g1_generator());
    CSREF.mark("sig_alloc");
    G2Var sig_var = (mask & SIG) ? pv_new_input<Fp2T>(sig) : g2_new_witness(sig);
    U32 count;
    G1Var agg = mapped_aggregate(keys, bits, &count);
    if (count_value) *count_value = count.value();
    return bls_verify_gadget(g1, agg, msg_var, sig_var);
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
// a dummy instance for the shape-only calls (the matrices and the marks do not depend on values): generator keys, all selected, sig = H(0...0)
G2Aff dummy_sig(size_t len) {
    std::vector<uint8_t> m(len + 1, 0);
    Scope s(false, 1);
    G2Var h = hash_to_g2_with_cons(u8const_vec(m.data(), len));
    return h.value_affine();
}

}  // namespace

extern "C" {

// witness_assignment (out_witness, capacity in elements; may be null), instance_assignment [n_inst][6] (element 0 = one; may be null), the gadget's
// Boolean, the count and the constraint count. Returns n_witness; *n_inst_out = n_instance_vars.
uint64_t agsh_witness(const uint64_t* pks_xy, const uint8_t* bitmap, size_t K, const uint8_t* msg, size_t len, const uint64_t* sig_xy, int mask,
                      uint64_t* out_witness, uint64_t cap, uint64_t* out_instance, uint64_t* n_inst_out, uint64_t* n_constraints, int* result, uint32_t* count) {
    Scope s(false, n_inst_of(K, len, mask));
    Bool r = circuit(affs(pks_xy, K), bitmap, msg, len, aff2(sig_xy), mask, count);
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
// segment marks of the shape: names '\n'-separated, starts[k] = witness index of mark k. Returns the number of marks.
uint64_t agsh_layout(size_t K, size_t len, int mask, uint64_t* starts, uint64_t cap, char* names_buf, size_t names_cap, uint64_t* n_wit, uint64_t* n_cons,
                     uint64_t* n_inst) {
    std::vector<uint8_t> msg(len + 1, 0), bm(K, 1);
    G2Aff h = dummy_sig(len);
    Scope s(false, n_inst_of(K, len, mask));
    circuit(std::vector<G1Aff>(K, g1_generator()), bm.data(), msg.data(), len, h, mask, nullptr);
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
uint64_t agsh_matrices(size_t K, size_t len, int mask, uint64_t* nnz, uint64_t* n_witness, uint64_t* n_inst, uint64_t** row_ptr, uint32_t** col, uint64_t** val) {
    std::vector<uint8_t> msg(len + 1, 0), bm(K, 1);
    G2Aff h = dummy_sig(len);
    Scope s(true, n_inst_of(K, len, mask));
    circuit(std::vector<G1Aff>(K, g1_generator()), bm.data(), msg.data(), len, h, mask, nullptr);
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
int64_t agsh_check(const uint64_t* pks_xy, const uint8_t* bitmap, size_t K, const uint8_t* msg, size_t len, const uint64_t* sig_xy, int mask,
                   const uint64_t* instance, const uint64_t* witness, uint64_t n_witness) {
    Scope s(true, n_inst_of(K, len, mask));
    circuit(affs(pks_xy, K), bitmap, msg, len, aff2(sig_xy), mask, nullptr);
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
