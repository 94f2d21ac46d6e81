// Host side of the device R1CS evaluator's encoding (blsw_r1cs_device_bytes / blsw_r1cs_create, k_r1cs.hip): validation of a caller's CSR, the
// class of every Montgomery coefficient (POS / NEG / GEN, r1cs_row.hpp) and the cut of the rows into blocks of about equal work. Host only; the
// test harness (tests/hostsim) compiles it with g++ and exports its result.
#pragma once
#include <string.h>
#include <unordered_map>
#include <vector>
#include "../../include/blsw.h"
#include "r1cs_row.hpp"

namespace blsw {
namespace r1cs {

constexpr int WAVES = 4;  // waves (row blocks) per workgroup
// block cut: work units of an entry by class, of a row's reductions and comparison, and per block
constexpr uint64_t W_ONE = 2, W_SMALL = 3, W_GEN = 10, W_ROW = 30, W_BLOCK = 16384;

struct Key {
    uint64_t w[6];
    bool operator==(const Key& o) const { return memcmp(w, o.w, sizeof(w)) == 0; }
};
struct KeyHash {
    size_t operator()(const Key& k) const {
        uint64_t h = 0x9E3779B97F4A7C15ull;
        for (int i = 0; i < 6; i++) h = (h ^ k.w[i]) * 0xBF58476D1CE4E5B9ull;
        return (size_t)(h ^ (h >> 31));
    }
};

// value < p and != 0 (6 little-endian u64 limbs)
inline bool coefficient_ok(const uint64_t* v) {
    static const uint64_t P64[6] = {0xb9feffffffffaaabull, 0x1eabfffeb153ffffull, 0x6730d2a0f6b0f624ull, 0x64774b84f38512bfull, 0x4b1ba7b6434bacd7ull,
                                    0x1a0111ea397fe69aull};
    if ((v[0] | v[1] | v[2] | v[3] | v[4] | v[5]) == 0) return false;
    for (int i = 5; i >= 0; i--)
        if (v[i] != P64[i]) return v[i] < P64[i];
    return false;  // == p
}

struct Encoded {
    std::vector<blsw_u2> ent[3];
    std::vector<Fp> table;
    std::vector<uint64_t> blk;
    uint64_t bytes = 0, off_rp[3] = {}, off_ent[3] = {}, off_table = 0, off_blk = 0;
};

inline uint64_t align256(uint64_t x) { return (x + 255) & ~255ull; }

// validates the CSR (include/blsw.h: blsw_r1cs_create) and encodes it; BLSW_ERR_ARG on the first rule it breaks
inline int encode(const blsw_matrices_info_t* info, const blsw_matrices_t* m, Encoded* out) {
    if (!info || !m || info->n_constraints == 0 || info->n_instance_vars == 0) return BLSW_ERR_ARG;
    const uint64_t n_cons = info->n_constraints, n_z = info->n_instance_vars + info->n_witness;
    if (n_z > 0xFFFFFFFFull) return BLSW_ERR_ARG;  // u32 columns
    std::unordered_map<Key, uint32_t, KeyHash> codes;
    std::vector<uint64_t> row_work(n_cons, W_ROW);
    for (int mi = 0; mi < 3; mi++) {
        const uint64_t* rp = m->row_ptr[mi];
        const uint32_t* col = m->col[mi];
        const uint64_t* val = m->val[mi];
        const uint64_t nnz = info->nnz[mi];
        if (!rp || (nnz && (!col || !val)) || rp[0] != 0 || rp[n_cons] != nnz) return BLSW_ERR_ARG;
        std::vector<blsw_u2>& ent = out->ent[mi];
        ent.resize(nnz);
        for (uint64_t r = 0; r < n_cons; r++) {
            if (rp[r + 1] < rp[r] || rp[r + 1] > nnz) return BLSW_ERR_ARG;
            for (uint64_t k = rp[r]; k < rp[r + 1]; k++) {
                if (col[k] >= n_z || (k > rp[r] && col[k] <= col[k - 1])) return BLSW_ERR_ARG;
                const uint64_t* v = val + k * 6;
                if (!coefficient_ok(v)) return BLSW_ERR_ARG;
                Key key;
                memcpy(key.w, v, sizeof(key.w));
                auto it = codes.find(key);
                uint32_t code;
                if (it != codes.end()) {
                    code = it->second;
                } else {  // canonical value c = v R^-1: +-c small, or a table entry
                    Fp mont, one = fp_zero();
                    memcpy(mont.l, v, sizeof(mont.l));
                    one.l[0] = 1;
                    const Fp c = fp_mul(mont, one), nc = fp_neg(c);
                    auto small = [](const Fp& x) {
                        uint32_t hi = 0;
                        for (int j = 1; j < 12; j++) hi |= x.l[j];
                        return hi == 0 && x.l[0] <= PAYLOAD;
                    };
                    if (small(c)) {
                        code = CLS_POS << PAYLOAD_BITS | c.l[0];
                    } else if (small(nc)) {
                        code = CLS_NEG << PAYLOAD_BITS | nc.l[0];
                    } else {
                        if (out->table.size() > PAYLOAD) return BLSW_ERR_ARG;
                        code = CLS_GEN << PAYLOAD_BITS | (uint32_t)out->table.size();
                        out->table.push_back(mont);
                    }
                    codes.emplace(key, code);
                }
                ent[k] = blsw_u2{col[k], code};
                const uint32_t cls = code >> PAYLOAD_BITS, pv = code & PAYLOAD;
                row_work[r] += cls == CLS_GEN ? W_GEN : (pv == 1 ? W_ONE : W_SMALL);
            }
        }
    }
    // blocks of about W_BLOCK work units (a row longer than that is a block of its own)
    out->blk.assign(1, 0);
    uint64_t acc = 0;
    for (uint64_t r = 0; r < n_cons; r++) {
        if (acc && acc + row_work[r] > W_BLOCK) {
            out->blk.push_back(r);
            acc = 0;
        }
        acc += row_work[r];
    }
    out->blk.push_back(n_cons);
    if (out->blk.size() - 1 > 0xFFFFFFFFull / WAVES) return BLSW_ERR_ARG;
    uint64_t off = 0;
    for (int mi = 0; mi < 3; mi++) {
        out->off_rp[mi] = off;
        off = align256(off + (n_cons + 1) * 8);
    }
    for (int mi = 0; mi < 3; mi++) {
        out->off_ent[mi] = off;
        off = align256(off + info->nnz[mi] * 8);
    }
    out->off_table = off;
    off = align256(off + out->table.size() * sizeof(Fp));
    out->off_blk = off;
    out->bytes = align256(off + out->blk.size() * 8);
    return BLSW_OK;
}

// Head rows (blsw_r1cs_head_rows, blsw_r1cs_check_keyset): cover[r] = the smallest head_len for which rows 0..r read nothing but column 0 and
// witnesses below head_len, i.e. columns in [n_instance_vars, n_instance_vars + head_len). Non-decreasing; cut at the first row that reads a public
// input (no head covers it). Of a CSR encode() has accepted.
inline std::vector<uint32_t> head_cover(const blsw_matrices_info_t* info, const blsw_matrices_t* m) {
    std::vector<uint32_t> cover;
    cover.reserve(info->n_constraints);
    const uint32_t n_inst = (uint32_t)info->n_instance_vars;
    uint32_t need = 0;
    for (uint64_t r = 0; r < info->n_constraints; r++) {
        for (int mi = 0; mi < 3; mi++)
            for (uint64_t k = m->row_ptr[mi][r]; k < m->row_ptr[mi][r + 1]; k++) {
                const uint32_t c = m->col[mi][k];
                if (c == 0) continue;
                if (c < n_inst) return cover;
                if (c - n_inst + 1 > need) need = c - n_inst + 1;
            }
        cover.push_back(need);
    }
    return cover;
}
// the number of leading rows a head of head_len witnesses covers
inline uint64_t head_rows(const std::vector<uint32_t>& cover, uint64_t head_len) {
    uint64_t lo = 0, hi = cover.size();
    while (lo < hi) {
        const uint64_t mid = (lo + hi) / 2;
        if (cover[mid] <= head_len)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}


// Pair families (blsw_r1cs_pair_families, blsw_r1cs_check_compact_multi): K consecutive blocks of R rows in which block j reads nothing but column 0
// and witnesses of pair j, and equals block 0 with every witness column moved by j strides of its run and the same coefficient codes (encode() gives
// equal coefficients equal codes). owner(column) says whose a column is: pair >= 0 a pair-local witness of that pair (stride: its run's), PAIR_CONST
// column 0, PAIR_SHARED anything else (a public input, a witness of the instance). Nothing is assumed of the matrices: a candidate — the rows of
// pair 0 up to the first row of pair 1 — becomes a family only when every entry of all K blocks has been compared. Of an encoding encode() made.
struct PairFamily {
    uint64_t first, rows;  // the template block [first, first + rows); block j follows at first + j * rows
};
struct ColOwner {
    int32_t pair;
    uint32_t stride;
};
constexpr int32_t PAIR_CONST = -1, PAIR_SHARED = -2;
template <class Owner>
inline std::vector<PairFamily> pair_families(uint64_t n_cons, const uint64_t* const rp[3], const blsw_u2* const ent[3], uint32_t K, Owner owner) {
    std::vector<int32_t> own(n_cons);
    for (uint64_t r = 0; r < n_cons; r++) {
        int32_t o = PAIR_CONST;
        for (int mi = 0; mi < 3 && o != PAIR_SHARED; mi++)
            for (uint64_t k = rp[mi][r]; k < rp[mi][r + 1]; k++) {
                const int32_t p = owner(ent[mi][k].x).pair;
                if (p == PAIR_CONST) continue;
                if (p == PAIR_SHARED || (o >= 0 && o != p)) {
                    o = PAIR_SHARED;
                    break;
                }
                o = p;
            }
        own[r] = o;
    }
    auto block_equal = [&](uint64_t r0, uint64_t rj, uint32_t j) {  // row rj == row r0 translated to pair j
        for (int mi = 0; mi < 3; mi++) {
            const uint64_t a0 = rp[mi][r0], a1 = rp[mi][r0 + 1], b0 = rp[mi][rj];
            if (rp[mi][rj + 1] - b0 != a1 - a0) return false;
            for (uint64_t k = 0; k < a1 - a0; k++) {
                const blsw_u2 a = ent[mi][a0 + k], b = ent[mi][b0 + k];
                const ColOwner o = owner(a.x);
                const uint64_t want = o.pair == PAIR_CONST ? a.x : (uint64_t)a.x + (uint64_t)j * o.stride;
                if (a.y != b.y || b.x != want) return false;
            }
        }
        return true;
    };
    std::vector<PairFamily> fam;
    uint64_t r = 0;
    while (r < n_cons) {
        if (own[r] != 0) {
            r++;
            continue;
        }
        uint64_t e = r;
        while (e < n_cons && (own[e] == 0 || own[e] == PAIR_CONST)) e++;
        const uint64_t R = e - r;
        bool ok = K > 1 && e < n_cons && own[e] == 1 && R <= (n_cons - r) / K;
        for (uint32_t j = 1; j < K && ok; j++)
            for (uint64_t t = 0; t < R && ok; t++) ok = block_equal(r + t, r + (uint64_t)j * R + t, j);
        if (ok) {
            fam.push_back(PairFamily{r, R});
            r += (uint64_t)K * R;
        } else {
            r = e;
        }
    }
    return fam;
}

}  // namespace r1cs
}  // namespace blsw
