// TEST HARNESS ONLY (never linked into libblsw.so): the SHA-256 gadget layer of csrc/sha.hpp as ONE table of operations, each a function of an
// operand block. The host harness (tests/hostsim: hostsim_sha_op) and the device harness (tests/devsha/devsha.hip, one kernel per entry) compile
// this same table; tests/sha_ref.py states what every entry must return and which bits must leave through the sink.
//   in   [DEVSHA_IN_MAX] u32: the operands. A mask-carrying word is a triple (v, cm, nm) as in sha.hpp's W32.
//   msg  the item's message ([msg_len] bytes; only the entries marked `msg`)
//   out  [DEVSHA_OUT_MAX] u32: the entry's own count of result words is written, the rest is left alone
//   s    the bit sink the entry's witness bits leave through. An entry marked `flushes` ends its stream itself (expand_message_w does), the
//        harness flushes behind every other entry.
#pragma once
#include "sha.hpp"

#define DEVSHA_IN_MAX 72
#define DEVSHA_OUT_MAX 64

// X(name, operand words, result words, msg, flushes)
#define DEVSHA_OPS(X)                \
    X(w_xor, 6, 3, 0, 0)             \
    X(w_and, 6, 3, 0, 0)             \
    X(w_not, 3, 3, 0, 0)             \
    X(w_rotr, 4, 3, 0, 0)            \
    X(w_shr, 4, 3, 0, 0)             \
    X(w_addmany2, 6, 3, 0, 0)        \
    X(w_addmany3, 9, 3, 0, 0)        \
    X(w_addmany4, 12, 3, 0, 0)       \
    X(w_addmany5, 15, 3, 0, 0)       \
    X(pext32, 2, 1, 0, 0)            \
    X(popc32, 1, 1, 0, 0)            \
    X(sigma_var, 2, 4, 0, 0)         \
    X(sha_sched_word, 12, 3, 0, 0)   \
    X(sha_round_var, 10, 16, 0, 0)   \
    X(sha_block_w, 72, 24, 0, 0)     \
    X(sha_block_generic, 72, 24, 0, 0) \
    X(b0_block, 2, 32, 1, 0)         \
    X(expand_message_w, 0, 64, 1, 1) \
    X(expand_message_values, 0, 64, 1, 0) \
    X(hash_to_field_elem, 16, 12, 0, 0)

namespace devsha {
using namespace blsw;

enum {
#define DEVSHA_X_ENUM(name, n_in, n_out, msg, fl) OP_##name,
    DEVSHA_OPS(DEVSHA_X_ENUM)
#undef DEVSHA_X_ENUM
        OP_COUNT
};
#define DEVSHA_X_COL(col, dflt)                                  \
    BLSW_HD int op_##col(int op) {                               \
        switch (op) {                                            \
            DEVSHA_OPS(DEVSHA_X_CASE)                            \
            default:                                             \
                return dflt;                                     \
        }                                                        \
    }
#define DEVSHA_X_CASE(name, n_in, n_out, msg, fl) \
    case OP_##name:                               \
        return n_in;
DEVSHA_X_COL(n_in, -1)
#undef DEVSHA_X_CASE
#define DEVSHA_X_CASE(name, n_in, n_out, msg, fl) \
    case OP_##name:                               \
        return n_out;
DEVSHA_X_COL(n_out, -1)
#undef DEVSHA_X_CASE
#define DEVSHA_X_CASE(name, n_in, n_out, msg, fl) \
    case OP_##name:                               \
        return msg;
DEVSHA_X_COL(msg, 0)
#undef DEVSHA_X_CASE
#define DEVSHA_X_CASE(name, n_in, n_out, msg, fl) \
    case OP_##name:                               \
        return fl;
DEVSHA_X_COL(flushes, 0)
#undef DEVSHA_X_CASE
#undef DEVSHA_X_COL

BLSW_HD W32 ld3(const uint32_t* p) { return {p[0], p[1], p[2]}; }
BLSW_HD void st3(uint32_t* p, const W32& w) {
    p[0] = w.v;
    p[1] = w.cm;
    p[2] = w.nm;
}

template <int OP>
struct ShaOp;
#define DEVSHA_DEF(name)                                                                                                    \
    template <>                                                                                                             \
    struct ShaOp<OP_##name> {                                                                                               \
        static BLSW_HD void run(const uint32_t* in, const uint8_t* msg, uint32_t msg_len, uint32_t* out, BitSink& s);       \
    };                                                                                                                      \
    BLSW_HD void ShaOp<OP_##name>::run(const uint32_t* in, const uint8_t* msg, uint32_t msg_len, uint32_t* out, BitSink& s)

DEVSHA_DEF(w_xor) { st3(out, w_xor(s, ld3(in), ld3(in + 3))); }
DEVSHA_DEF(w_and) { st3(out, w_and(s, ld3(in), ld3(in + 3))); }
DEVSHA_DEF(w_not) { st3(out, w_not(ld3(in))); }
DEVSHA_DEF(w_rotr) { st3(out, w_rotr(ld3(in), (int)in[3])); }  // in[3] = 1 .. 31
DEVSHA_DEF(w_shr) { st3(out, w_shr(ld3(in), (int)in[3])); }    // in[3] = 1 .. 31
template <int K>
BLSW_HD void addmany_k(const uint32_t* in, uint32_t* out, BitSink& s) {
    W32 ops[K];
    for (int i = 0; i < K; i++) ops[i] = ld3(in + 3 * i);
    st3(out, w_addmany(s, ops, K));
}
DEVSHA_DEF(w_addmany2) { addmany_k<2>(in, out, s); }
DEVSHA_DEF(w_addmany3) { addmany_k<3>(in, out, s); }
DEVSHA_DEF(w_addmany4) { addmany_k<4>(in, out, s); }
DEVSHA_DEF(w_addmany5) { addmany_k<5>(in, out, s); }
DEVSHA_DEF(pext32) { out[0] = pext32(in[0], in[1]); }
DEVSHA_DEF(popc32) { out[0] = (uint32_t)popc32(in[0]); }
// in: x, which (0: the schedule's sigma0 = 7, 18, >> 3; 1: sigma1 = 17, 19, >> 10). sigma_var first, then the two w_xor it replaces on the
// same all-variable word: out = sigma_var's value, then the generic triple; the stream holds both sets of bits
DEVSHA_DEF(sigma_var) {
    const int r1 = in[1] ? 17 : 7, r2 = in[1] ? 19 : 18, sh = in[1] ? 10 : 3;
    out[0] = sigma_var(s, in[0], r1, r2, sh);
    const W32 x = {in[0], 0u, 0u};
    st3(out + 1, w_xor(s, w_xor(s, w_rotr(x, r1), w_rotr(x, r2)), w_shr(x, sh)));
}
DEVSHA_DEF(sha_sched_word) { st3(out, sha_sched_word(s, ld3(in), ld3(in + 3), ld3(in + 6), ld3(in + 9))); }
// in: a .. h, w, k. sha_round_var first (out[0..8)), then sha_round_generic on the same all-variable state and word (out[8..16))
DEVSHA_DEF(sha_round_var) {
    uint32_t a = in[0], b = in[1], c = in[2], d = in[3], e = in[4], f = in[5], g = in[6], h = in[7];
    const uint64_t kw = (uint64_t)in[9] + in[8];
    sha_round_var(s, a, b, c, d, e, f, g, h, (uint32_t)kw, (uint32_t)(kw >> 32));
    const uint32_t fin[8] = {a, b, c, d, e, f, g, h};
    W32 st[8];
    for (int i = 0; i < 8; i++) {
        out[i] = fin[i];
        st[i] = {in[i], 0u, 0u};
    }
    sha_round_generic(s, st, W32{in[8], 0u, 0u}, in[9]);
    for (int i = 0; i < 8; i++) out[8 + i] = st[i].v | st[i].cm | st[i].nm;  // all-variable results: the masks must be zero
}
// in: the state (8 triples), the data (16 triples); out: the new state (8 triples)
DEVSHA_DEF(sha_block_w) {
    W32 st[8], data[16];
    for (int i = 0; i < 8; i++) st[i] = ld3(in + 3 * i);
    for (int i = 0; i < 16; i++) data[i] = ld3(in + 24 + 3 * i);
    sha_block_w(s, st, data);
    for (int i = 0; i < 8; i++) st3(out + 3 * i, st[i]);
}
DEVSHA_DEF(sha_block_generic) {
    W32 st[8], data[16];
    for (int i = 0; i < 8; i++) st[i] = ld3(in + 3 * i);
    for (int i = 0; i < 16; i++) data[i] = ld3(in + 24 + 3 * i);
    sha_block_generic(s, st, data);
    for (int i = 0; i < 8; i++) st3(out + 3 * i, st[i]);
}
// in: block index, msg_const. The sixteen data words of one block of the padded msg' as expand_message_w assembles them from b0_byte:
// out[0..16) the values, out[16..32) the constant masks
DEVSHA_DEF(b0_block) {
    const uint32_t total = 64 + msg_len + 3 + BLSW_DST_LEN + 1;
    for (int wi = 0; wi < 16; wi++) {
        uint32_t v = 0, cm = 0;
        for (int b = 0; b < 4; b++) {
            uint32_t bv;
            bool bc;
            b0_byte(msg, msg_len, in[1] != 0, in[0] * 64 + wi * 4 + b, total, bv, bc);
            v |= bv << (8 * (3 - b));
            if (bc) cm |= 0xffu << (8 * (3 - b));
        }
        out[wi] = v;
        out[16 + wi] = cm;
    }
}
DEVSHA_DEF(expand_message_w) { expand_message_w(s, msg, msg_len, false, out); }
DEVSHA_DEF(expand_message_values) { expand_message_values(msg, msg_len, out); }
DEVSHA_DEF(hash_to_field_elem) {
    const Fp r = hash_to_field_elem(in);
    for (int i = 0; i < 12; i++) out[i] = r.l[i];
}
#undef DEVSHA_DEF
}  // namespace devsha
