// Device R1CS evaluator (blsw_r1cs_*; include/blsw.h): <A_j, z> * <B_j, z> == <C_j, z> for n instances at a time, over the CSR matrices that
// blsw_matrices_fill* emit, and the A z, B z, C z rows themselves.
//
// Encoding (host, blsw_r1cs_create): every entry is a u32 column and a u32 code, 8 bytes; the code's top two bits are its class:
//   POS v / NEG v   coefficient +-v with 0 < v < 2^30 (the +-1 / +-2 of the boolean and SHA rows, the small constants of the curve rows)
//   GEN idx         index into a table of the distinct Montgomery coefficients (powers of two from 2^30 up and the general constants)
// Rows are cut into blocks of about equal work (entries weighted by class, plus the row's reductions); a wave walks one block.
//
// Kernel mapping: grid (row blocks / 4, groups of 64 instances), four waves per workgroup, lane = instance. All lanes walk the SAME
// entries, so column, code and row pointers are wave-uniform and the class branch does not diverge; each lane gathers its own z[col].
// A row's terms go into a 14-limb accumulator without reduction (+-v z is a 1 x 12-limb multiply, a table coefficient one Montgomery
// product); the row ends with one Montgomery reduction per matrix (REDC of the 448-bit sum: X 2^-384 mod p) and the comparison
//     REDC(A) * REDC(B) * K  ==  REDC(C)      (products in Montgomery form; K = R^2 for Montgomery input, R^3 for canonical input)
// For Montgomery input (z = v R) REDC gives the canonical row value, for canonical input v R^-1; either way the two sides differ by
// the same power of R. An empty A or B row skips the products.
//
// Two sources of z, one kernel template: expanded witness vectors (Args: [n][stride][6]), or a step's compact wire form (CompactArgs: the engine's
// bit words and staged rows as they travel, blsw_compact_layout_t). The compact source evaluates compact_locate (kcommon.hpp) per entry: the column is
// wave-uniform, so region and row are scalar arithmetic and the three-way branch does not diverge; a bit column is one u32 per lane, a tile row one
// contiguous 3 KB read per wave — the instance-interleaved gather the expanded form cannot give.
// A shared-keys step (ABI 15) carries no key rows: its z is [instance | the key set's table | the compact rows] (KeysetCompactArgs, ABI 16). A head column
// is one address for all 64 lanes — wave-uniform like the column itself, so the fourth branch does not diverge either. The leading rows that read
// nothing but the head (head_cover, r1cs_encode.hpp) are a function of the committee alone: blsw_r1cs_check_keyset evaluates them once per set
// (the plain kernel, one instance whose witness vector is the table) and the step's check may then start at the first row behind them.
// A step of the N+1-pair product (blsw_compact_layout_multi_t: bit words and pair tiles by pair lane i K + j, instance tiles, instance rows) has
// few instances — n K <= 65535 — so one instance per lane leaves most of a wave idle and walks all K copies of the per-pair rows. Two sources: the
// general one (MultiCompactArgs, the k_r1cs template, compact_place_multi / compact_address_multi per entry) for the evaluation and for the rows of
// the check outside the pair families; and k_r1cs_pairs, lane = PAIR lane, over the one template block of each family (pair_families,
// r1cs_encode.hpp: K consecutive blocks that are translated copies of the first, verified entry by entry) — whole tile rows whatever n is, the
// template's entries read once, a failing template row t of pair j reported as t + j R by atomicMin.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include <mutex>
#include <vector>
#include "../../include/blsw.h"
#include "kcommon.hpp"
#include "r1cs_encode.hpp"  // the host's validation, coefficient classes and block cut; r1cs_row.hpp: the accumulator, row_term, redc14

using namespace blsw;
using namespace blsw::r1cs;

namespace {

struct Enc {
    const uint64_t* rp[3];   // row pointers [n_constraints + 1]
    const blsw_u2* ent[3];   // {column, code} [nnz]
    const Fp* table;         // distinct Montgomery coefficients of class GEN
    const uint64_t* blk;     // first row of every block [n_blocks + 1]
};

struct Args {
    Enc e;
    const uint64_t* inst;  // [n][inst_stride][6] or NULL (n_inst == 1)
    const uint64_t* wit;   // [n][wit_stride][6]
    uint64_t inst_stride, wit_stride, n;
    uint32_t n_inst, blk_first, n_blk;
    uint64_t row_lo, row_hi;  // rows evaluated (check: the whole matrix)
    Fp one;                   // the constant one in the input's form (inst == NULL)
    Fp k;                     // check: R^(3 - form); evaluate: R^2
    uint64_t* bad;            // check: [n] first unsatisfied row (u64 max = none)
    uint64_t* out[3];         // evaluate: [n][row_hi - row_lo][6]
};

// z from a compact step: lane i of the buffer is instance i; always Montgomery form (a.one = R mod p serves column 0 and the set bits)
struct CompactArgs : Args {
    blsw_compact_layout_t c;
    const char* compact;
};

// z from a compact step of a shared-keys engine: witness k < head_len is element k of the step's key set, the same for every instance; the rest is
// the compact buffer at k - head_len
struct KeysetCompactArgs : CompactArgs {
    const uint64_t* head;  // [head_len][6] Montgomery (blsw_keyset_table)
    uint32_t head_len;
};

// z from a compact step of the N+1-pair product (blsw_compact_layout_multi_t), one INSTANCE per lane: the general source — every row of the
// evaluation, and the rows of the check that belong to no pair family
struct MultiCompactArgs : Args {
    blsw_compact_layout_multi_t c;
    const char* compact;
};
// ... one PAIR per lane: the template block of a pair family (r1cs_encode.hpp: pair_families). The template's columns are column 0 and witnesses of
// pair 0, i.e. a (region, row) of the bit words or the pair tiles; lane p reads the same (region, row) in its own column
struct PairArgs : MultiCompactArgs {
    uint64_t fam_rows;  // R: template row t of pair j is matrix row t + j * R
};

__device__ __forceinline__ Fp load_fp(const uint64_t* src) {
    const uint4* q = reinterpret_cast<const uint4*>(src);
    const uint4 a = q[0], b = q[1], c = q[2];
    return Fp{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w}};
}
// z[col] of instance i (col is wave-uniform: so is the branch)
__device__ __forceinline__ Fp load_z(const Args& a, uint64_t i, uint32_t col) {
    if (col >= a.n_inst) return load_fp(a.wit + (i * a.wit_stride + (col - a.n_inst)) * 6);
    if (a.inst) return load_fp(a.inst + (i * a.inst_stride + col) * 6);
    return a.one;
}

// witness k of instance i of a compact buffer
__device__ __forceinline__ Fp load_compact(const CompactArgs& a, uint64_t i, uint32_t k) {
    uint64_t off;
    uint32_t bit;
    const uint64_t lane = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(i >> 6)) << 6) | (i & 63);  // the tile is wave-uniform: scalar address terms
    if (compact_locate(a.c, k, lane, &off, &bit) != BLSW_COMPACT_BIT) return load_fp(reinterpret_cast<const uint64_t*>(a.compact + off));
    const uint32_t m = 0u - ((*reinterpret_cast<const uint32_t*>(a.compact + off) >> bit) & 1u);
    Fp r;
#pragma unroll
    for (int j = 0; j < 12; j++) r.l[j] = a.one.l[j] & m;
    return r;
}
__device__ __forceinline__ Fp load_z(const CompactArgs& a, uint64_t i, uint32_t col) {
    if (col >= a.n_inst) return load_compact(a, i, col - a.n_inst);
    if (a.inst) return load_fp(a.inst + (i * a.inst_stride + col) * 6);
    return a.one;
}
__device__ __forceinline__ Fp load_z(const KeysetCompactArgs& a, uint64_t i, uint32_t col) {
    if (col >= a.n_inst) {
        const uint32_t k = col - a.n_inst;
        if (k < a.head_len) return load_fp(a.head + (uint64_t)k * 6);  // one address for the wave
        return load_compact(a, i, k - a.head_len);
    }
    if (a.inst) return load_fp(a.inst + (i * a.inst_stride + col) * 6);
    return a.one;
}

// (region, row, bit) of a multi step for `lane` (a pair lane for BIT / TILE, an instance otherwise)
__device__ __forceinline__ Fp load_multi(const MultiCompactArgs& a, uint32_t region, uint32_t row, uint32_t bit, uint64_t lane) {
    const uint64_t off = compact_address_multi(a.c, region, row, lane);
    if (region != BLSW_COMPACT_BIT) return load_fp(reinterpret_cast<const uint64_t*>(a.compact + off));
    const uint32_t m = 0u - ((*reinterpret_cast<const uint32_t*>(a.compact + off) >> bit) & 1u);
    Fp r;
#pragma unroll
    for (int j = 0; j < 12; j++) r.l[j] = a.one.l[j] & m;
    return r;
}
__device__ __forceinline__ Fp load_z(const MultiCompactArgs& a, uint64_t i, uint32_t col) {
    if (col >= a.n_inst) {
        uint32_t j, row, bit;
        const uint32_t region = compact_place_multi(a.c, col - a.n_inst, &j, &row, &bit);  // wave-uniform
        if (region == BLSW_COMPACT_NONE) return fp_zero();                                  // (no struct compact_layout_multi_ok accepts gets here)
        return load_multi(a, region, row, bit, region <= BLSW_COMPACT_TILE ? i * a.c.n_pairs + j : i);
    }
    if (a.inst) return load_fp(a.inst + (i * a.inst_stride + col) * 6);
    return a.one;
}
// lane = pair lane p of instance i = p / K (computed once per lane, at kernel entry); a column of the template that is no pair-local witness cannot
// occur (pair_families) and reads as zero
struct PairLane {
    uint64_t p, i;
};
__device__ __forceinline__ Fp load_z(const PairArgs& a, const PairLane& l, uint32_t col) {
    if (col >= a.n_inst) {
        uint32_t j, row, bit;
        const uint32_t region = compact_place_multi(a.c, col - a.n_inst, &j, &row, &bit);
        if (region > BLSW_COMPACT_TILE) return fp_zero();
        return load_multi(a, region, row, bit, l.p);
    }
    if (a.inst) return load_fp(a.inst + (l.i * a.inst_stride + col) * 6);
    return a.one;
}

// REDC(<M_row, z>) of one matrix row
template <class A, class Lane>
__device__ __forceinline__ Fp row_dot(const A& a, int m, uint64_t k0, uint64_t k1, const Lane& i) {
    Acc x;
#pragma unroll
    for (int j = 0; j < 14; j++) x.l[j] = 0;
    const blsw_u2* ent = a.e.ent[m];
#pragma unroll 1
    for (uint64_t k = k0; k < k1; k++) {
        const blsw_u2 e = ent[k];
        row_term(x, load_z(a, i, e.x), e.y, a.e.table);
    }
    return redc14(x);
}

template <bool EVAL, class A>
__global__ __launch_bounds__(64 * WAVES) void k_r1cs(A a) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t b = blockIdx.x * WAVES + wave;
    const uint64_t i = (uint64_t)blockIdx.y * 64 + (threadIdx.x & 63);
    if (b >= a.n_blk || i >= a.n) return;
    const uint32_t blk = a.blk_first + b;
    uint64_t r0 = a.e.blk[blk], r1 = a.e.blk[blk + 1];
    r0 = r0 > a.row_lo ? r0 : a.row_lo;
    r1 = r1 < a.row_hi ? r1 : a.row_hi;
    uint64_t bad = ~0ull;
#pragma unroll 1
    for (uint64_t row = r0; row < r1; row++) {
        const uint64_t a0 = a.e.rp[0][row], a1 = a.e.rp[0][row + 1], b0 = a.e.rp[1][row], b1 = a.e.rp[1][row + 1];
        const uint64_t c0 = a.e.rp[2][row], c1 = a.e.rp[2][row + 1];
        const Fp fa = a0 < a1 ? row_dot(a, 0, a0, a1, i) : fp_zero();
        const Fp fb = b0 < b1 ? row_dot(a, 1, b0, b1, i) : fp_zero();
        const Fp fc = c0 < c1 ? row_dot(a, 2, c0, c1, i) : fp_zero();
        if (EVAL) {  // REDC(X) K = the row value in the input's form
            const uint64_t o = (i * (a.row_hi - a.row_lo) + (row - a.row_lo)) * 6;
            const Fp v[3] = {fp_mul(fa, a.k), fp_mul(fb, a.k), fp_mul(fc, a.k)};
#pragma unroll
            for (int m = 0; m < 3; m++) {
                uint4* dst = reinterpret_cast<uint4*>(a.out[m] + o);
                dst[0] = make_uint4(v[m].l[0], v[m].l[1], v[m].l[2], v[m].l[3]);
                dst[1] = make_uint4(v[m].l[4], v[m].l[5], v[m].l[6], v[m].l[7]);
                dst[2] = make_uint4(v[m].l[8], v[m].l[9], v[m].l[10], v[m].l[11]);
            }
        } else {
            const Fp lhs = (a0 < a1 && b0 < b1) ? fp_mul(fp_mul(fa, fb), a.k) : fp_zero();
            if (!fp_eq(lhs, fc) && bad == ~0ull) bad = row;
        }
    }
    if (!EVAL && bad != ~0ull) atomicMin(reinterpret_cast<unsigned long long*>(a.bad + i), (unsigned long long)bad);
}

// The template block of a pair family, one pair per lane: grid (row blocks of the template / 4, pair tiles n K / 64). Column and code stay wave-uniform;
// a staged row is one contiguous 3 KB read per wave whatever n is, and the template's entries are read once, not once per pair. Template row t fails
// for pair j of instance i: matrix row t + j R, by atomicMin into bad[i] — with the other pairs and the general path's rows, the matrix's first row.
__global__ __launch_bounds__(64 * WAVES) void k_r1cs_pairs(PairArgs a) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t b = blockIdx.x * WAVES + wave;
    const uint64_t p = (uint64_t)blockIdx.y * 64 + (threadIdx.x & 63);  // n K is a multiple of 64: every lane is a pair
    if (b >= a.n_blk) return;
    const PairLane lane = {p, (uint64_t)((uint32_t)p / a.c.n_pairs)};  // n K <= 65535
    const uint32_t blk = a.blk_first + b;
    uint64_t r0 = a.e.blk[blk], r1 = a.e.blk[blk + 1];
    r0 = r0 > a.row_lo ? r0 : a.row_lo;
    r1 = r1 < a.row_hi ? r1 : a.row_hi;
    uint64_t bad = ~0ull;
#pragma unroll 1
    for (uint64_t row = r0; row < r1; row++) {
        const uint64_t a0 = a.e.rp[0][row], a1 = a.e.rp[0][row + 1], b0 = a.e.rp[1][row], b1 = a.e.rp[1][row + 1];
        const uint64_t c0 = a.e.rp[2][row], c1 = a.e.rp[2][row + 1];
        const Fp fa = a0 < a1 ? row_dot(a, 0, a0, a1, lane) : fp_zero();
        const Fp fb = b0 < b1 ? row_dot(a, 1, b0, b1, lane) : fp_zero();
        const Fp fc = c0 < c1 ? row_dot(a, 2, c0, c1, lane) : fp_zero();
        const Fp lhs = (a0 < a1 && b0 < b1) ? fp_mul(fp_mul(fa, fb), a.k) : fp_zero();
        if (!fp_eq(lhs, fc) && bad == ~0ull) bad = row;
    }
    if (bad != ~0ull) {
        const uint64_t i = lane.i, j = p - i * a.c.n_pairs;
        atomicMin(reinterpret_cast<unsigned long long*>(a.bad + i), (unsigned long long)(bad + j * a.fam_rows));
    }
}

// first index k of z with z_k >= p: grid (chunks, instances of this slice); a thread's indices ascend, so its first hit is its minimum
__global__ __launch_bounds__(256) void k_r1cs_unreduced(const uint64_t* __restrict__ inst, uint64_t inst_stride, const uint64_t* __restrict__ wit,
                                                        uint64_t wit_stride, uint32_t n_inst, uint64_t n_z, unsigned long long* __restrict__ out) {
    constexpr uint32_t P[12] = BLSW_P_LIMBS;
    const uint64_t i = blockIdx.y;
#pragma unroll 1
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n_z; k += (uint64_t)gridDim.x * 256) {
        const uint64_t* src = k >= n_inst ? wit + (i * wit_stride + (k - n_inst)) * 6 : (inst ? inst + (i * inst_stride + k) * 6 : nullptr);
        if (!src) continue;  // the constant one
        const Fp z = load_fp(src);
        uint32_t borrow = 0;
#pragma unroll
        for (int j = 0; j < 12; j++) subb32(z.l[j], P[j], borrow);
        if (!borrow) {
            atomicMin(out + i, (unsigned long long)k);
            break;
        }
    }
}

// the same over the staged rows of a compact step (a bit cannot be unreduced): grid (chunks, 64-instance tiles), lane = instance, a wave takes one
// staged row at a time — 3 KB contiguous below split_row. j counts the witnesses outside the SHA segment; the moved segment makes a thread's
// indices non-monotonic, so every hit goes to the atomic. base = the index of z of the buffer's witness 0 (n_inst, plus the head of a shared-keys step).
__global__ __launch_bounds__(256) void k_r1cs_unreduced_compact(blsw_compact_layout_t c, const char* __restrict__ compact, uint32_t base, unsigned long long* __restrict__ out) {
    constexpr uint32_t P[12] = BLSW_P_LIMBS;
    const uint64_t i = (uint64_t)blockIdx.y * 64 + (threadIdx.x & 63);
#pragma unroll 1
    for (uint32_t j = blockIdx.x * 4 + (threadIdx.x >> 6); j < c.staging_rows; j += gridDim.x * 4) {
        const uint32_t k = j < c.off_expand ? j : j + c.sha_bits;
        uint64_t off;
        uint32_t bit;
        compact_locate(c, k, i, &off, &bit);
        const Fp z = load_fp(reinterpret_cast<const uint64_t*>(compact + off));
        uint32_t borrow = 0;
#pragma unroll
        for (int l = 0; l < 12; l++) subb32(z.l[l], P[l], borrow);
        if (!borrow) atomicMin(out + i, (unsigned long long)base + k);
    }
}

// ... of the N+1-pair product, one region per launch. part 0: the pair tiles, grid (chunks, n K / 64), lane = pair lane, a wave takes a staged row at
// a time; part 1: the instance tiles, grid (chunks, ceil(n / 64)), lane = instance; part 2: the instance rows, grid (chunks, n), a thread per element.
// Every hit goes to the atomic, at base + the element's witness index (the inverse of compact_place_multi, run by run).
__global__ __launch_bounds__(256) void k_r1cs_unreduced_multi(blsw_compact_layout_multi_t c, const char* __restrict__ compact, uint32_t base, uint32_t part,
                                                              unsigned long long* __restrict__ out) {
    constexpr uint32_t P[12] = BLSW_P_LIMBS;
    const bool rows_major = part == 2;
    const uint64_t lane = rows_major ? blockIdx.y : (uint64_t)blockIdx.y * 64 + (threadIdx.x & 63);
    const uint32_t rows = part == 0 ? c.rows_p : part == 1 ? c.rows_i : c.pair_rows;
    if (lane >= (part == 0 ? c.n * c.n_pairs : c.n)) return;
    const uint64_t i = part == 0 ? lane / c.n_pairs : lane;
    const uint32_t j = part == 0 ? (uint32_t)(lane - i * c.n_pairs) : 0u;
    const uint32_t e0 = rows_major ? blockIdx.x * 256 + threadIdx.x : blockIdx.x * 4 + (threadIdx.x >> 6), step = rows_major ? gridDim.x * 256 : gridDim.x * 4;
#pragma unroll 1
    for (uint32_t e = e0; e < rows; e += step) {
        uint32_t k = c.off_miller + e;
        if (part == 0) {
            for (int r = 0; r < 6; r++)
                if (e >= c.pair_run_row[r] && e - c.pair_run_row[r] < c.pair_run_len[r]) k = c.pair_run_off[r] + j * c.pair_run_stride[r] + (e - c.pair_run_row[r]);
        } else if (part == 1) {
            for (int r = 0; r < 2; r++)
                if (e >= c.inst_run_row[r] && e - c.inst_run_row[r] < c.inst_run_len[r]) k = c.inst_run_off[r] + (e - c.inst_run_row[r]);
        }
        const Fp z = load_fp(reinterpret_cast<const uint64_t*>(compact + compact_address_multi(c, part == 0 ? BLSW_COMPACT_TILE : part == 1 ? BLSW_COMPACT_INST : BLSW_COMPACT_PAIR, e, lane)));
        uint32_t borrow = 0;
#pragma unroll
        for (int l = 0; l < 12; l++) subb32(z.l[l], P[l], borrow);
        if (!borrow) atomicMin(out + i, (unsigned long long)base + k);
    }
}

// ------------------------------------------------------------------------------------------------------------------------- host side
int hip_ok(hipError_t e, const char* what) {
    if (e != hipSuccess) {
        fprintf(stderr, "[blsw] r1cs %s: %s\n", what, hipGetErrorString(e));
        return BLSW_ERR_HIP;
    }
    return BLSW_OK;
}

}  // namespace

struct blsw_r1cs {
    int device;
    uint64_t n_cons, n_inst, n_wit;
    Enc enc;
    std::vector<uint64_t> blk;  // host copy of the block starts (a row range -> blocks)
    std::vector<uint32_t> head;  // head_cover (r1cs_encode.hpp): the head rows of any head_len without the CSR
    uint64_t nnz[3];
    // pair_families of every multi layout a call has named (blsw_r1cs_handle_pair_families): computed once from the encoding on the device, keyed by
    // what the detector reads — K, the runs and the strides, not the step size (family_key). The only state of the handle a check changes: behind
    // families_lock, and an entry never moves once it is made (the calls keep a pointer to its vector).
    struct Families {
        blsw_compact_layout_multi_t key;
        std::vector<PairFamily> fam;
    };
    std::vector<std::unique_ptr<Families>> families;
    std::mutex families_lock;
};

int blsw_r1cs_device_bytes(const blsw_matrices_info_t* info, const blsw_matrices_t* m, uint64_t* bytes) {
    if (!bytes) return BLSW_ERR_ARG;
    Encoded e;
    const int rc = encode(info, m, &e);
    if (rc) return rc;
    *bytes = e.bytes;
    return BLSW_OK;
}

int blsw_r1cs_head_rows(const blsw_matrices_info_t* info, const blsw_matrices_t* m, uint64_t head_len, uint64_t* rows) {
    if (!rows) return BLSW_ERR_ARG;
    Encoded e;
    const int rc = encode(info, m, &e);
    if (rc) return rc;
    if (head_len > info->n_witness) return BLSW_ERR_ARG;
    *rows = head_rows(head_cover(info, m), head_len);
    return BLSW_OK;
}

int blsw_r1cs_create(blsw_r1cs_t** out, const blsw_matrices_info_t* info, const blsw_matrices_t* m, int32_t device, void* d_buffer, uint64_t buffer_bytes,
                     void* stream) {
    if (!out || !d_buffer || (reinterpret_cast<uintptr_t>(d_buffer) & 255)) return BLSW_ERR_ARG;
    *out = nullptr;
    Encoded e;
    int rc = encode(info, m, &e);
    if (rc) return rc;
    if (buffer_bytes < e.bytes) return BLSW_ERR_WORKSPACE;
    int prev = -1, dev = device;
    if (hip_ok(hipGetDevice(&prev), "hipGetDevice")) return BLSW_ERR_NO_DEVICE;
    if (dev < 0) dev = prev;
    if (dev != prev && hip_ok(hipSetDevice(dev), "hipSetDevice")) return BLSW_ERR_NO_DEVICE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* base = reinterpret_cast<char*>(d_buffer);
    auto put = [&](uint64_t off, const void* src, uint64_t bytes) {
        return bytes ? hip_ok(hipMemcpyAsync(base + off, src, bytes, hipMemcpyHostToDevice, st), "hipMemcpyAsync") : BLSW_OK;
    };
    for (int mi = 0; mi < 3 && !rc; mi++) rc = put(e.off_rp[mi], m->row_ptr[mi], (info->n_constraints + 1) * 8);
    for (int mi = 0; mi < 3 && !rc; mi++) rc = put(e.off_ent[mi], e.ent[mi].data(), e.ent[mi].size() * sizeof(blsw_u2));
    if (!rc) rc = put(e.off_table, e.table.data(), e.table.size() * sizeof(Fp));
    if (!rc) rc = put(e.off_blk, e.blk.data(), e.blk.size() * 8);
    if (!rc) rc = hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize");  // the host vectors go out of scope
    if (dev != prev) hipSetDevice(prev);
    if (rc) return rc;
    blsw_r1cs* r = new blsw_r1cs;
    r->device = dev;
    r->n_cons = info->n_constraints;
    r->n_inst = info->n_instance_vars;
    r->n_wit = info->n_witness;
    for (int mi = 0; mi < 3; mi++) r->nnz[mi] = info->nnz[mi];
    for (int mi = 0; mi < 3; mi++) {
        r->enc.rp[mi] = reinterpret_cast<const uint64_t*>(base + e.off_rp[mi]);
        r->enc.ent[mi] = reinterpret_cast<const blsw_u2*>(base + e.off_ent[mi]);
    }
    r->enc.table = reinterpret_cast<const Fp*>(base + e.off_table);
    r->enc.blk = reinterpret_cast<const uint64_t*>(base + e.off_blk);
    r->blk = std::move(e.blk);
    r->head = head_cover(info, m);
    *out = r;
    return BLSW_OK;
}

int blsw_r1cs_destroy(blsw_r1cs_t* r) {
    delete r;
    return BLSW_OK;
}

namespace {

// the argument rules shared by check and evaluate (host only)
int io_args(const blsw_r1cs* r, const uint64_t* d_instance, uint64_t instance_stride, const uint64_t* d_witness, uint64_t witness_stride, uint64_t n, uint32_t form) {
    if (!r || !d_witness || n == 0 || form > 1 || witness_stride < r->n_wit) return BLSW_ERR_ARG;
    if (r->n_inst > 1 && (!d_instance || instance_stride < r->n_inst)) return BLSW_ERR_ARG;
    if (d_instance && instance_stride < r->n_inst) return BLSW_ERR_ARG;
    return BLSW_OK;
}

Args make_args(const blsw_r1cs* r, const uint64_t* d_instance, uint64_t instance_stride, const uint64_t* d_witness, uint64_t witness_stride, uint64_t n, uint32_t form) {
    Args a;
    memset(&a, 0, sizeof(a));
    a.e = r->enc;
    a.inst = d_instance;
    a.wit = d_witness;
    a.inst_stride = instance_stride;
    a.wit_stride = witness_stride;
    a.n = n;
    a.n_inst = (uint32_t)r->n_inst;
    a.one = form ? fp_zero() : fp_one();
    if (form) a.one.l[0] = 1;
    return a;
}

Fp fp_const(const uint32_t (&l)[12]) {
    Fp r;
    memcpy(r.l, l, sizeof(r.l));
    return r;
}

// grid.y <= 65535 groups of 64 instances per launch
int launch(Args a, bool eval, hipStream_t st) {
    const uint64_t n = a.n;
    const Args base = a;
    for (uint64_t first = 0; first < n; first += 65535ull * 64) {
        a = base;
        const uint64_t cnt = n - first < 65535ull * 64 ? n - first : 65535ull * 64;
        a.n = cnt;
        a.wit = base.wit + first * base.wit_stride * 6;
        if (base.inst) a.inst = base.inst + first * base.inst_stride * 6;
        if (base.bad) a.bad = base.bad + first;
        for (int m = 0; m < 3; m++)
            if (base.out[m]) a.out[m] = base.out[m] + first * (base.row_hi - base.row_lo) * 6;
        dim3 grid((a.n_blk + WAVES - 1) / WAVES, (unsigned)((cnt + 63) / 64));
        if (eval)
            hipLaunchKernelGGL((k_r1cs<true, Args>), grid, dim3(64 * WAVES), 0, st, a);
        else
            hipLaunchKernelGGL((k_r1cs<false, Args>), grid, dim3(64 * WAVES), 0, st, a);
    }
    return hip_ok(hipGetLastError(), "launch");
}

// a compact step is at most 65535 tiles (compact_layout_ok): one launch
int launch(const CompactArgs& a, bool eval, hipStream_t st) {
    dim3 grid((a.n_blk + WAVES - 1) / WAVES, (unsigned)(a.n / 64));
    if (eval)
        hipLaunchKernelGGL((k_r1cs<true, CompactArgs>), grid, dim3(64 * WAVES), 0, st, a);
    else
        hipLaunchKernelGGL((k_r1cs<false, CompactArgs>), grid, dim3(64 * WAVES), 0, st, a);
    return hip_ok(hipGetLastError(), "launch");
}

int launch(const KeysetCompactArgs& a, bool eval, hipStream_t st) {
    dim3 grid((a.n_blk + WAVES - 1) / WAVES, (unsigned)(a.n / 64));
    if (eval)
        hipLaunchKernelGGL((k_r1cs<true, KeysetCompactArgs>), grid, dim3(64 * WAVES), 0, st, a);
    else
        hipLaunchKernelGGL((k_r1cs<false, KeysetCompactArgs>), grid, dim3(64 * WAVES), 0, st, a);
    return hip_ok(hipGetLastError(), "launch");
}

struct Guard {
    int prev = -1;
    bool switched = false;
    explicit Guard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~Guard() {
        if (switched) hipSetDevice(prev);
    }
};

}  // namespace

namespace {

// rows [row_lo, row_hi) and the blocks that hold them (the first and the last block are clamped to the range by the kernel)
template <class A>
void set_rows(const blsw_r1cs* r, A& a, uint64_t row_lo, uint64_t row_hi) {
    a.row_lo = row_lo;
    a.row_hi = row_hi;
    const auto& blk = r->blk;
    const uint64_t b0 = (uint64_t)(std::upper_bound(blk.begin(), blk.end(), row_lo) - blk.begin()) - 1;
    const uint64_t b1 = (uint64_t)(std::lower_bound(blk.begin(), blk.end(), row_hi) - blk.begin());
    a.blk_first = (uint32_t)b0;
    a.n_blk = (uint32_t)(b1 - b0);
}
// rows [row_lo, row_hi) (reported as they are numbered in the matrix), first unsatisfied row per instance
template <class A>
int run_check(const blsw_r1cs* r, A& a, uint32_t form, uint64_t row_lo, uint64_t row_hi, int64_t* d_first_unsatisfied, hipStream_t st) {
    static constexpr uint32_t R2[12] = BLSW_R2_LIMBS, R3[12] = BLSW_R3_LIMBS;
    a.k = fp_const(form ? R3 : R2);
    a.bad = reinterpret_cast<uint64_t*>(d_first_unsatisfied);
    if (hip_ok(hipMemsetAsync(d_first_unsatisfied, 0xFF, a.n * 8, st), "hipMemsetAsync")) return BLSW_ERR_HIP;  // all ones = -1 = satisfied
    if (row_lo >= row_hi) return BLSW_OK;  // no row to check (a set without head rows)
    set_rows(r, a, row_lo, row_hi);
    return launch(a, false, st);
}
// rows [row_begin, row_begin + row_count) of A z, B z, C z
template <class A>
int run_evaluate(const blsw_r1cs* r, A& a, uint64_t row_begin, uint64_t row_count, uint64_t* d_az, uint64_t* d_bz, uint64_t* d_cz, hipStream_t st) {
    static constexpr uint32_t R2[12] = BLSW_R2_LIMBS;
    a.k = fp_const(R2);
    set_rows(r, a, row_begin, row_begin + row_count);
    a.out[0] = d_az;
    a.out[1] = d_bz;
    a.out[2] = d_cz;
    return launch(a, true, st);
}
bool row_window_ok(const blsw_r1cs* r, uint64_t row_begin, uint64_t row_count) {
    return row_count != 0 && row_begin < r->n_cons && row_count <= r->n_cons - row_begin;
}
// the argument rules of the compact calls (host only), and their arguments
int compact_args(const blsw_r1cs* r, const blsw_compact_layout_t* c, const void* d_compact, const uint64_t* d_instance, uint64_t instance_stride, uint64_t head_len = 0) {
    if (!r || !c || !d_compact || (reinterpret_cast<uintptr_t>(d_compact) & 15) || !compact_layout_ok(*c) || c->n_witness + head_len != r->n_wit) return BLSW_ERR_ARG;
    if (r->n_inst > 1 && (!d_instance || instance_stride < r->n_inst)) return BLSW_ERR_ARG;
    if (d_instance && instance_stride < r->n_inst) return BLSW_ERR_ARG;
    return BLSW_OK;
}
CompactArgs make_compact_args(const blsw_r1cs* r, const blsw_compact_layout_t* c, const void* d_compact, const uint64_t* d_instance, uint64_t instance_stride) {
    CompactArgs a;
    static_cast<Args&>(a) = make_args(r, d_instance, instance_stride, nullptr, 0, c->n, 0);
    a.c = *c;
    a.compact = reinterpret_cast<const char*>(d_compact);
    return a;
}
// the rules of the calls that take a key set (host only): a set on the handle's device whose table is no longer than the witness vector
bool keyset_ok(const blsw_r1cs* r, const blsw_keyset* ks) { return r && ks && ks->device == r->device && (uint64_t)ks->n_keys * SEG_PK_ALLOC <= r->n_wit; }
// ... of the two compact calls: the set's table is the head of z beside the buffer's Montgomery elements
int keyset_compact_args(const blsw_r1cs* r, const blsw_compact_layout_t* c, const void* d_compact, const blsw_keyset* ks, uint32_t head_rows_mode, const uint64_t* d_instance,
                        uint64_t instance_stride) {
    if (!keyset_ok(r, ks) || ks->form != 0 || head_rows_mode > BLSW_R1CS_HEAD_SKIP) return BLSW_ERR_ARG;
    return compact_args(r, c, d_compact, d_instance, instance_stride, (uint64_t)ks->n_keys * SEG_PK_ALLOC);
}
KeysetCompactArgs make_keyset_compact_args(const blsw_r1cs* r, const blsw_compact_layout_t* c, const void* d_compact, const blsw_keyset* ks, const uint64_t* d_instance,
                                           uint64_t instance_stride) {
    KeysetCompactArgs a;
    static_cast<CompactArgs&>(a) = make_compact_args(r, c, d_compact, d_instance, instance_stride);
    a.head = reinterpret_cast<const uint64_t*>(ks->table);
    a.head_len = ks->n_keys * SEG_PK_ALLOC;
    return a;
}
// the unreduced elements of a compact step: the instance vectors (plain: the pass over the first n_inst indices of z; atomicMin: any order with the
// rows) and the staged rows, reported from index `base` of z on
int unreduced_compact(const blsw_r1cs* r, const blsw_compact_layout_t* layout, const char* compact, const uint64_t* d_instance, uint64_t instance_stride, uint32_t base,
                      int64_t* d_first_unreduced, hipStream_t st) {
    const uint64_t n = layout->n;
    if (hip_ok(hipMemsetAsync(d_first_unreduced, 0xFF, n * 8, st), "hipMemsetAsync")) return BLSW_ERR_HIP;
    unsigned long long* unr = reinterpret_cast<unsigned long long*>(d_first_unreduced);
    if (d_instance) {
        for (uint64_t first = 0; first < n; first += 65535) {
            const uint64_t cnt = n - first < 65535 ? n - first : 65535;
            hipLaunchKernelGGL(k_r1cs_unreduced, dim3(1, (unsigned)cnt), dim3(256), 0, st, d_instance + first * instance_stride * 6, instance_stride, nullptr, 0,
                               (uint32_t)r->n_inst, r->n_inst, unr + first);
        }
    }
    const uint32_t chunks = (layout->staging_rows + 3) / 4;
    if (chunks) hipLaunchKernelGGL(k_r1cs_unreduced_compact, dim3(chunks < 256 ? chunks : 256, (unsigned)(n / 64)), dim3(256), 0, st, *layout, compact, base, unr);
    return hip_ok(hipGetLastError(), "launch");
}

}  // namespace

int blsw_r1cs_check(blsw_r1cs_t* r, const uint64_t* d_instance, uint64_t instance_stride, const uint64_t* d_witness, uint64_t witness_stride, uint64_t n,
                    uint32_t form, int64_t* d_first_unsatisfied, int64_t* d_first_unreduced, void* stream) {
    if (io_args(r, d_instance, instance_stride, d_witness, witness_stride, n, form) || !d_first_unsatisfied) return BLSW_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    Guard guard(r->device);
    Args a = make_args(r, d_instance, instance_stride, d_witness, witness_stride, n, form);
    int rc = run_check(r, a, form, 0, r->n_cons, d_first_unsatisfied, st);
    if (rc || !d_first_unreduced) return rc;
    if (hip_ok(hipMemsetAsync(d_first_unreduced, 0xFF, n * 8, st), "hipMemsetAsync")) return BLSW_ERR_HIP;
    const uint64_t n_z = r->n_inst + r->n_wit, chunks = (n_z + 255) / 256;
    for (uint64_t first = 0; first < n; first += 65535) {
        const uint64_t cnt = n - first < 65535 ? n - first : 65535;
        dim3 grid((unsigned)(chunks < 64 ? chunks : 64), (unsigned)cnt);
        hipLaunchKernelGGL(k_r1cs_unreduced, grid, dim3(256), 0, st, d_instance ? d_instance + first * instance_stride * 6 : nullptr, instance_stride,
                           d_witness + first * witness_stride * 6, witness_stride, (uint32_t)r->n_inst, n_z,
                           reinterpret_cast<unsigned long long*>(d_first_unreduced + first));
    }
    return hip_ok(hipGetLastError(), "launch");
}

int blsw_r1cs_evaluate(blsw_r1cs_t* r, const uint64_t* d_instance, uint64_t instance_stride, const uint64_t* d_witness, uint64_t witness_stride, uint64_t n,
                       uint32_t form, uint64_t row_begin, uint64_t row_count, uint64_t* d_az, uint64_t* d_bz, uint64_t* d_cz, void* stream) {
    if (io_args(r, d_instance, instance_stride, d_witness, witness_stride, n, form) || !d_az || !d_bz || !d_cz) return BLSW_ERR_ARG;
    if (!row_window_ok(r, row_begin, row_count)) return BLSW_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    Guard guard(r->device);
    Args a = make_args(r, d_instance, instance_stride, d_witness, witness_stride, n, form);
    return run_evaluate(r, a, row_begin, row_count, d_az, d_bz, d_cz, st);
}

int blsw_r1cs_check_compact(blsw_r1cs_t* r, const blsw_compact_layout_t* layout, const void* d_compact, const uint64_t* d_instance, uint64_t instance_stride,
                            int64_t* d_first_unsatisfied, int64_t* d_first_unreduced, void* stream) {
    if (compact_args(r, layout, d_compact, d_instance, instance_stride) || !d_first_unsatisfied) return BLSW_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    Guard guard(r->device);
    CompactArgs a = make_compact_args(r, layout, d_compact, d_instance, instance_stride);
    int rc = run_check(r, a, 0, 0, r->n_cons, d_first_unsatisfied, st);
    if (rc || !d_first_unreduced) return rc;
    return unreduced_compact(r, layout, a.compact, d_instance, instance_stride, (uint32_t)r->n_inst, d_first_unreduced, st);
}

int blsw_r1cs_evaluate_compact(blsw_r1cs_t* r, const blsw_compact_layout_t* layout, const void* d_compact, const uint64_t* d_instance, uint64_t instance_stride,
                               uint64_t row_begin, uint64_t row_count, uint64_t* d_az, uint64_t* d_bz, uint64_t* d_cz, void* stream) {
    if (compact_args(r, layout, d_compact, d_instance, instance_stride) || !d_az || !d_bz || !d_cz || !row_window_ok(r, row_begin, row_count)) return BLSW_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    Guard guard(r->device);
    CompactArgs a = make_compact_args(r, layout, d_compact, d_instance, instance_stride);
    return run_evaluate(r, a, row_begin, row_count, d_az, d_bz, d_cz, st);
}

int blsw_r1cs_handle_head_rows(const blsw_r1cs_t* r, uint64_t head_len, uint64_t* rows) {
    if (!r || !rows || head_len > r->n_wit) return BLSW_ERR_ARG;
    *rows = head_rows(r->head, head_len);
    return BLSW_OK;
}

// ABI 16: the committee once, and a shared-keys step from its compact buffer plus the receiver's key set
int blsw_r1cs_check_keyset(blsw_r1cs_t* r, const blsw_keyset_t* ks, int64_t* d_first_unsatisfied, int64_t* d_first_unreduced, void* stream) {
    if (!keyset_ok(r, ks) || !d_first_unsatisfied) return BLSW_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    Guard guard(r->device);
    // one instance whose witness vector is the table: the head rows read nothing else (and column 0, the constant one in the table's form)
    const uint64_t head_len = (uint64_t)ks->n_keys * SEG_PK_ALLOC;
    const uint64_t* table = reinterpret_cast<const uint64_t*>(ks->table);
    Args a = make_args(r, nullptr, 0, table, head_len, 1, ks->form);
    int rc = run_check(r, a, ks->form, 0, head_rows(r->head, head_len), d_first_unsatisfied, st);
    if (rc || !d_first_unreduced) return rc;
    if (hip_ok(hipMemsetAsync(d_first_unreduced, 0xFF, 8, st), "hipMemsetAsync")) return BLSW_ERR_HIP;
    const uint64_t n_z = r->n_inst + head_len, chunks = (n_z + 255) / 256;
    hipLaunchKernelGGL(k_r1cs_unreduced, dim3((unsigned)(chunks < 64 ? chunks : 64), 1), dim3(256), 0, st, nullptr, 0, table, head_len, (uint32_t)r->n_inst, n_z,
                       reinterpret_cast<unsigned long long*>(d_first_unreduced));
    return hip_ok(hipGetLastError(), "launch");
}

int blsw_r1cs_check_compact_keyset(blsw_r1cs_t* r, const blsw_compact_layout_t* rows_layout, const void* d_compact, const blsw_keyset_t* ks, uint32_t head_rows_mode,
                                   const uint64_t* d_instance, uint64_t instance_stride, int64_t* d_first_unsatisfied, int64_t* d_first_unreduced, void* stream) {
    if (keyset_compact_args(r, rows_layout, d_compact, ks, head_rows_mode, d_instance, instance_stride) || !d_first_unsatisfied) return BLSW_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    Guard guard(r->device);
    KeysetCompactArgs a = make_keyset_compact_args(r, rows_layout, d_compact, ks, d_instance, instance_stride);
    const uint64_t row_lo = head_rows_mode == BLSW_R1CS_HEAD_SKIP ? head_rows(r->head, a.head_len) : 0;
    int rc = run_check(r, a, 0, row_lo, r->n_cons, d_first_unsatisfied, st);
    if (rc || !d_first_unreduced) return rc;
    return unreduced_compact(r, rows_layout, a.compact, d_instance, instance_stride, (uint32_t)r->n_inst + a.head_len, d_first_unreduced, st);
}

int blsw_r1cs_evaluate_compact_keyset(blsw_r1cs_t* r, const blsw_compact_layout_t* rows_layout, const void* d_compact, const blsw_keyset_t* ks, const uint64_t* d_instance,
                                      uint64_t instance_stride, uint64_t row_begin, uint64_t row_count, uint64_t* d_az, uint64_t* d_bz, uint64_t* d_cz, void* stream) {
    if (keyset_compact_args(r, rows_layout, d_compact, ks, 0, d_instance, instance_stride) || !d_az || !d_bz || !d_cz || !row_window_ok(r, row_begin, row_count))
        return BLSW_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    Guard guard(r->device);
    KeysetCompactArgs a = make_keyset_compact_args(r, rows_layout, d_compact, ks, d_instance, instance_stride);
    return run_evaluate(r, a, row_begin, row_count, d_az, d_bz, d_cz, st);
}

// ---- the N+1-pair product's compact form (blsw_compact_layout_multi_t): the general source, and one pair per lane over the pair families
namespace {

int multi_args(const blsw_r1cs* r, const blsw_compact_layout_multi_t* c, const void* d_compact, const uint64_t* d_instance, uint64_t instance_stride) {
    if (!r || !c || !d_compact || (reinterpret_cast<uintptr_t>(d_compact) & 15) || !compact_layout_multi_ok(*c) || c->n_witness != r->n_wit) return BLSW_ERR_ARG;
    if (r->n_inst > 1 && (!d_instance || instance_stride < r->n_inst)) return BLSW_ERR_ARG;
    if (d_instance && instance_stride < r->n_inst) return BLSW_ERR_ARG;
    return BLSW_OK;
}
MultiCompactArgs make_multi_args(const blsw_r1cs* r, const blsw_compact_layout_multi_t* c, const void* d_compact, const uint64_t* d_instance, uint64_t instance_stride) {
    MultiCompactArgs a;
    static_cast<Args&>(a) = make_args(r, d_instance, instance_stride, nullptr, 0, c->n, 0);
    a.c = *c;
    a.compact = reinterpret_cast<const char*>(d_compact);
    return a;
}
// n <= 65535 instances: one launch; the lanes past n of the last group of 64 idle (n = 4 and 32 are legal step sizes)
int launch(const MultiCompactArgs& a, bool eval, hipStream_t st) {
    dim3 grid((a.n_blk + WAVES - 1) / WAVES, (unsigned)((a.n + 63) / 64));
    if (eval)
        hipLaunchKernelGGL((k_r1cs<true, MultiCompactArgs>), grid, dim3(64 * WAVES), 0, st, a);
    else
        hipLaunchKernelGGL((k_r1cs<false, MultiCompactArgs>), grid, dim3(64 * WAVES), 0, st, a);
    return hip_ok(hipGetLastError(), "launch");
}
// whose a column is under a multi layout (r1cs_encode.hpp: pair_families)
struct MultiOwner {
    const blsw_compact_layout_multi_t& c;
    uint32_t n_inst;
    ColOwner operator()(uint32_t col) const {
        if (col == 0) return {PAIR_CONST, 0};
        if (col < n_inst) return {PAIR_SHARED, 0};
        uint32_t j, row, bit;
        const uint32_t region = compact_place_multi(c, col - n_inst, &j, &row, &bit);
        if (region == BLSW_COMPACT_BIT) return {(int32_t)j, c.stride_hash};
        if (region != BLSW_COMPACT_TILE) return {PAIR_SHARED, 0};
        for (int r = 0; r < 6; r++)
            if (row >= c.pair_run_row[r] && row - c.pair_run_row[r] < c.pair_run_len[r]) return {(int32_t)j, c.pair_run_stride[r]};
        return {PAIR_SHARED, 0};
    }
};
// the families of the handle's matrices under *c: kept per layout; the first call reads row pointers and entries back from the device
// the layout without what depends on the step size: the families are a function of the rest (pair_families reads K, the runs and the strides)
blsw_compact_layout_multi_t family_key(const blsw_compact_layout_multi_t& c) {
    blsw_compact_layout_multi_t k = c;
    k.n = k.off_staging = k.off_inst = k.off_pair = k.total = 0;
    k.inst_tile_w = 0;
    return k;
}
int handle_families(blsw_r1cs* r, const blsw_compact_layout_multi_t* c, const std::vector<PairFamily>** out) {
    const blsw_compact_layout_multi_t key = family_key(*c);
    std::lock_guard<std::mutex> lock(r->families_lock);
    for (const auto& f : r->families)
        if (memcmp(&f->key, &key, sizeof(key)) == 0) {
            *out = &f->fam;
            return BLSW_OK;
        }
    std::vector<uint64_t> rp[3];
    std::vector<blsw_u2> ent[3];
    const uint64_t* rpp[3];
    const blsw_u2* entp[3];
    for (int mi = 0; mi < 3; mi++) {
        rp[mi].resize(r->n_cons + 1);
        ent[mi].resize(r->nnz[mi]);
        if (hip_ok(hipMemcpy(rp[mi].data(), r->enc.rp[mi], (r->n_cons + 1) * 8, hipMemcpyDeviceToHost), "hipMemcpy")) return BLSW_ERR_HIP;
        if (r->nnz[mi] && hip_ok(hipMemcpy(ent[mi].data(), r->enc.ent[mi], r->nnz[mi] * sizeof(blsw_u2), hipMemcpyDeviceToHost), "hipMemcpy")) return BLSW_ERR_HIP;
        rpp[mi] = rp[mi].data();
        entp[mi] = ent[mi].data();
    }
    r->families.emplace_back(new blsw_r1cs::Families{key, pair_families(r->n_cons, rpp, entp, c->n_pairs, MultiOwner{*c, (uint32_t)r->n_inst})});
    *out = &r->families.back()->fam;
    return BLSW_OK;
}
int families_out(const std::vector<PairFamily>& fam, uint64_t capacity, uint64_t* first_row, uint64_t* rows_per_pair, uint64_t* count) {
    if (capacity && (!first_row || !rows_per_pair)) return BLSW_ERR_ARG;
    for (uint64_t f = 0; f < fam.size() && f < capacity; f++) first_row[f] = fam[f].first, rows_per_pair[f] = fam[f].rows;
    *count = fam.size();
    return BLSW_OK;
}

}  // namespace

int blsw_r1cs_pair_families(const blsw_matrices_info_t* info, const blsw_matrices_t* m, const blsw_compact_layout_multi_t* layout, uint64_t capacity, uint64_t* first_row,
                            uint64_t* rows_per_pair, uint64_t* count) {
    if (!count || !layout || !compact_layout_multi_ok(*layout)) return BLSW_ERR_ARG;
    Encoded e;
    const int rc = encode(info, m, &e);
    if (rc) return rc;
    if (layout->n_witness != info->n_witness) return BLSW_ERR_ARG;
    const uint64_t* rp[3] = {m->row_ptr[0], m->row_ptr[1], m->row_ptr[2]};
    const blsw_u2* ent[3] = {e.ent[0].data(), e.ent[1].data(), e.ent[2].data()};
    return families_out(pair_families(info->n_constraints, rp, ent, layout->n_pairs, MultiOwner{*layout, (uint32_t)info->n_instance_vars}), capacity, first_row, rows_per_pair, count);
}

int blsw_r1cs_handle_pair_families(blsw_r1cs_t* r, const blsw_compact_layout_multi_t* layout, uint64_t capacity, uint64_t* first_row, uint64_t* rows_per_pair, uint64_t* count) {
    if (!r || !count || !layout || !compact_layout_multi_ok(*layout) || layout->n_witness != r->n_wit) return BLSW_ERR_ARG;
    Guard guard(r->device);
    const std::vector<PairFamily>* fam = nullptr;
    if (int rc = handle_families(r, layout, &fam)) return rc;
    return families_out(*fam, capacity, first_row, rows_per_pair, count);
}

int blsw_r1cs_check_compact_multi_ex(blsw_r1cs_t* r, const blsw_compact_layout_multi_t* layout, const void* d_compact, const uint64_t* d_instance, uint64_t instance_stride,
                                     uint32_t use_families, int64_t* d_first_unsatisfied, int64_t* d_first_unreduced, void* stream) {
    if (multi_args(r, layout, d_compact, d_instance, instance_stride) || !d_first_unsatisfied || use_families > 1) return BLSW_ERR_ARG;
    static constexpr uint32_t R2[12] = BLSW_R2_LIMBS;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    Guard guard(r->device);
    static const std::vector<PairFamily> none;
    const std::vector<PairFamily>* fam = &none;
    if (use_families)
        if (int rc = handle_families(r, layout, &fam)) return rc;
    const uint64_t n = layout->n, K = layout->n_pairs;
    MultiCompactArgs a = make_multi_args(r, layout, d_compact, d_instance, instance_stride);
    a.k = fp_const(R2);
    a.bad = reinterpret_cast<uint64_t*>(d_first_unsatisfied);
    if (hip_ok(hipMemsetAsync(d_first_unsatisfied, 0xFF, n * 8, st), "hipMemsetAsync")) return BLSW_ERR_HIP;  // all ones = -1 = satisfied
    // the rows in front of, between and behind the families: one instance per lane; a family: its template block, one pair per lane. Every launch
    // lowers bad[i] by atomicMin, so their order does not matter. At most 2 * families + 1 launches.
    uint64_t cursor = 0;
    auto general = [&](uint64_t lo, uint64_t hi) {
        if (lo >= hi) return (int)BLSW_OK;
        set_rows(r, a, lo, hi);
        return launch(a, false, st);
    };
    for (const PairFamily& f : *fam) {
        if (int rc = general(cursor, f.first)) return rc;
        PairArgs pa;
        static_cast<MultiCompactArgs&>(pa) = a;
        pa.fam_rows = f.rows;
        set_rows(r, pa, f.first, f.first + f.rows);
        hipLaunchKernelGGL(k_r1cs_pairs, dim3((pa.n_blk + WAVES - 1) / WAVES, (unsigned)(n * K / 64)), dim3(64 * WAVES), 0, st, pa);
        if (hip_ok(hipGetLastError(), "launch")) return BLSW_ERR_HIP;
        cursor = f.first + K * f.rows;
    }
    if (int rc = general(cursor, r->n_cons)) return rc;
    if (!d_first_unreduced) return BLSW_OK;
    // the instance vectors (the plain pass over the first n_inst indices of z), then the staged elements of the three row regions
    if (hip_ok(hipMemsetAsync(d_first_unreduced, 0xFF, n * 8, st), "hipMemsetAsync")) return BLSW_ERR_HIP;
    unsigned long long* unr = reinterpret_cast<unsigned long long*>(d_first_unreduced);
    if (d_instance)
        hipLaunchKernelGGL(k_r1cs_unreduced, dim3(1, (unsigned)n), dim3(256), 0, st, d_instance, instance_stride, nullptr, 0, (uint32_t)r->n_inst, r->n_inst, unr);
    auto chunks = [](uint32_t rows, uint32_t per) { return std::min<uint32_t>((rows + per - 1) / per, 256); };
    const uint32_t base = (uint32_t)r->n_inst;
    if (layout->rows_p) hipLaunchKernelGGL(k_r1cs_unreduced_multi, dim3(chunks(layout->rows_p, 4), (unsigned)(n * K / 64)), dim3(256), 0, st, *layout, a.compact, base, 0u, unr);
    if (layout->rows_i) hipLaunchKernelGGL(k_r1cs_unreduced_multi, dim3(chunks(layout->rows_i, 4), (unsigned)((n + 63) / 64)), dim3(256), 0, st, *layout, a.compact, base, 1u, unr);
    if (layout->pair_rows) hipLaunchKernelGGL(k_r1cs_unreduced_multi, dim3(chunks(layout->pair_rows, 256), (unsigned)n), dim3(256), 0, st, *layout, a.compact, base, 2u, unr);
    return hip_ok(hipGetLastError(), "launch");
}

int blsw_r1cs_check_compact_multi(blsw_r1cs_t* r, const blsw_compact_layout_multi_t* layout, const void* d_compact, const uint64_t* d_instance, uint64_t instance_stride,
                                  int64_t* d_first_unsatisfied, int64_t* d_first_unreduced, void* stream) {
    return blsw_r1cs_check_compact_multi_ex(r, layout, d_compact, d_instance, instance_stride, 1, d_first_unsatisfied, d_first_unreduced, stream);
}

int blsw_r1cs_evaluate_compact_multi(blsw_r1cs_t* r, const blsw_compact_layout_multi_t* layout, const void* d_compact, const uint64_t* d_instance, uint64_t instance_stride,
                                     uint64_t row_begin, uint64_t row_count, uint64_t* d_az, uint64_t* d_bz, uint64_t* d_cz, void* stream) {
    if (multi_args(r, layout, d_compact, d_instance, instance_stride) || !d_az || !d_bz || !d_cz || !row_window_ok(r, row_begin, row_count)) return BLSW_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    Guard guard(r->device);
    MultiCompactArgs a = make_multi_args(r, layout, d_compact, d_instance, instance_stride);
    return run_evaluate(r, a, row_begin, row_count, d_az, d_bz, d_cz, st);
}
