// Shared by every translation unit of libblsw.so: the group / workspace / step descriptors, the witness cursor of the one-instance-per-lane
// kernels, and the declarations of the kernels (each family is compiled as its own translation unit, in parallel: build.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
// The compilations of the one-instance-per-lane chain units (build.py: CHAIN_UNITS, which says which unit has which and why). Before chains.hpp:
// fp.hpp's BLSW_FN reads BLSW_INLINE_CHAINS (the programs inlined into the kernel, so that the kernel's register budget governs all of them).
//   k_map      grouped engine: the unit's register policy, -DBLSW_CHAIN_W2 (inlined, two waves per SIMD), -DBLSW_CHAIN_OUTLINE (the programs out of
//              line: 410-420 registers per kernel, which leaves room for a few waves of the streaming kernels on the same SIMD — what the grouped
//              engine wants beside its HBM-bound expansion / placement) or -DBLSW_CHAIN_FULL (inlined, the whole register file)
//   k_map_inl  (-DBLSW_KVARIANT_INL) inlined, the whole 512-register file, 0.1-0.7 KB of stack instead of 1.2-3.9 KB out of line (no argument /
//              callee-saved traffic through scratch): 1.2-3.5x shorter under HBM load (k_map 32.8 -> 9.2 ms, k_g1 22 -> 8.5 ms in
//              blsw_verify_multi_batch) — what the direct-mode entries want (few waves, latency-bound)
//   k_map_q    (-DBLSW_KVARIANT_QUAD) inlined, and every chain on the four lanes of a quad with the independent Fp products of an Fp2 operation
//              on different lanes (fp.hpp: quads, gadgets.hpp): the latency compilation, for small launch groups that start a pipeline
// A unit that is no chain unit defines none of these: its programs are out of line.
#define BLSW_ATTR_W2 __attribute__((amdgpu_waves_per_eu(2, 2)))  // register budget of a kernel: two waves per SIMD
#if defined(BLSW_KVARIANT_QUAD)
#define BLSW_QUAD 1
#define BLSW_INLINE_CHAINS 1
#define BLSW_CHAIN_ATTR
#define BLSW_K(name) name##_q
#define BLSW_LPI 4u  // lanes per item (instance, pair, chunk) of this compilation's kernels
#elif defined(BLSW_KVARIANT_INL)
#define BLSW_INLINE_CHAINS 1
#define BLSW_CHAIN_ATTR
#define BLSW_K(name) name##_inl
#define BLSW_LPI 1u
#else
#if defined(BLSW_CHAIN_W2) || defined(BLSW_CHAIN_FULL)
#define BLSW_INLINE_CHAINS 1
#endif
#ifdef BLSW_CHAIN_W2
#define BLSW_CHAIN_ATTR BLSW_ATTR_W2
#else
#define BLSW_CHAIN_ATTR
#endif
#define BLSW_K(name) name
#define BLSW_LPI 1u
#endif
#include "chains.hpp"
#include "cofactor_vf.hpp"
#include "prepare_vf.hpp"
#include "layout.h"

namespace blsw {

// index of this thread's item, and whether it is the lane of its item that writes the item's outputs (values are identical on the lanes of a quad)
__device__ __forceinline__ uint64_t item_index() { return ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / BLSW_LPI; }
__device__ __forceinline__ bool item_leader() { return BLSW_LPI == 1u || (threadIdx.x & (BLSW_LPI - 1u)) == 0u; }
inline unsigned item_grid(uint64_t items, unsigned lpi) { return (unsigned)((items * lpi + 63) / 64); }

// ---------------------------------------------------------------- workspace
// All per-instance scratch is stored element-major: element e of instance I lives at index e*N + I, so that the
// 64 lanes of a wave touch one contiguous 3 KiB window per element (48 B per lane).
struct Workspace {
    uint32_t* bits;  // [N/64][sha_words/16][64][16] u32: SHA witness bitstream in 64-instance tiles; a wave appends 4 KiB rows
                     // (one 64-byte run of 16 words per instance) to its own tile; sha_words is a multiple of 16
    Fp* u;           // [4][N]   hash_to_field output u0.c0,u0.c1,u1.c0,u1.c1
    Fp* q;           // [12][N]  Q0 (x.c0,x.c1,y.c0,y.c1,z.c0,z.c1), Q1
    Fp* h;           // [6][N]   H(m) projective
    Fp* pkaff;       // [2][N]   prepare_g1(pk)
    Fp* coeff_h;     // [272][N]      line coefficients of prepare_g2(H(m))
    Fp* coeff_sig;   // [272][n_sig]  line coefficients of prepare_g2(sig)
    uint64_t n_sig;  // = N for the single-key circuit; = instances (not pairs) for the N+1-pair product
    Fp* keyproj;     // [3][N * n_keys] allocated keys of the aggregate_verify circuit (projective); nullptr for the other circuits and when the
                     // keys are public inputs (L.pk_mode: nothing allocates them, k_agg_sum_in reads the step's affine keys)
    Fp* staging;     // [N/64][rows_p][64] field witnesses (engine mode), or nullptr (direct mode): each wave of 64
                     // lanes owns one contiguous tile and appends 3 KiB rows to it (sequential HBM writes per wave)
    Fp* staging_inst;  // [n_sig/64][rows_i][64] the per-signature rows of the N+1-pair product staged the same way (sig allocation,
                       // prepare_g2(sig)); = staging (one lane is one instance) for the single-key and aggregate circuits
    uint32_t rows_p, rows_i;  // rows per tile of the two areas (= split_row when they are one)
    uint64_t staging_rows;
    Fp* pair;            // [n_sig][pair_rows]: rows >= split_row of the staging coordinates (Miller loop, final exponentiation,
    uint32_t split_row;  // is_one), instance-major: the six-lane pairing kernel appends each instance's segment sequentially
    uint32_t pair_rows;  // (split_row = staging_rows, pair_rows = 0 when the single-lane pairing kernel is in use)
    uint64_t sha_words;
    Fp* cofv;            // [BLSW_COFV_ELEMS][N] scratch of the values-first cofactor chain (cofactor_vf.hpp), or nullptr (N > BLSW_LATENCY_MAX_LANES)
    Fp* prepv_h;         // [BLSW_PREPV_ELEMS][N] / [BLSW_PREPV_ELEMS][n_sig] scratch of the values-first prepare chains (prepare_vf.hpp), or nullptr
    Fp* prepv_sig;
    uint64_t total_bytes;
};
// launch groups of at most this many lanes may take the latency kernels (quads, values-first cofactor chain): their scratch is carved for them
#define BLSW_LATENCY_MAX_LANES 8192
inline uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }
BLSW_HD uint64_t bits_tile_words(uint64_t sha_words) { return sha_words * 64; }  // u32 per 64-instance tile
// kernel variants, fixed per engine at creation (blsw_engine_options_t)
struct Modes {
    bool pairing_team;  // pairing segment: six lanes per instance (default) or the single-lane chain (kept for A/B runs)
    bool g2_team;       // G2 allocation on the six-lane machinery: its segment is staged instance-major like the pairing rows,
                        // so it moves to the end of the staging coordinates
};
constexpr Modes DEFAULT_MODES = {true, false};
inline blsw_layout_t staging_layout(const blsw_layout_t& L, const Modes& m) {
    blsw_layout_t S = L;
    uint32_t* f = &S.off_msg;
    const uint32_t* g = &L.off_msg;
    for (int k = 0; k < 15; k++) f[k] = g[k] > L.off_expand ? g[k] - L.sha_bits : g[k];
    if (L.off_prep_g1 > L.off_expand) S.off_prep_g1 = L.off_prep_g1 - L.sha_bits;  // off_params_alloc lies in front of the expansion
    if (m.g2_team) {
        const uint32_t lo = L.off_sig_alloc, len = L.off_pk_not_zero - L.off_sig_alloc;
        for (int k = 0; k < 15; k++)
            if (f[k] > lo) f[k] -= len;
        if (S.off_prep_g1 > lo) S.off_prep_g1 -= len;
        S.off_sig_alloc = L.n_witness - L.sha_bits - len;  // last rows of the staging coordinates
    }
    return S;
}
// Staging coordinates of the N+1-pair product in the grouped engine (K = L.n_pairs > 1): a PAIR lane stages the rows of its (pk, msg)
// pair — msg bits, key allocation, pk != 0, map0, map1, add, cofactor, prepare(H), prepare(pk) — in that order in its column of the
// pair tiles; an INSTANCE lane stages sig allocation and prepare(sig) in the instance tiles; Miller loop, final exponentiation and
// is_one are instance-major rows from `split` on. Strides are 0: a pair's copy is found by its lane, not by an offset.
struct MultiStaging {
    blsw_layout_t LS;
    uint32_t rows_p, rows_i, split, pair_rows;
};
inline MultiStaging staging_layout_multi(const blsw_layout_t& L) {
    MultiStaging m;
    m.LS = L;
    blsw_layout_t& S = m.LS;
    uint32_t o = 0;
    S.off_msg = o;
    o += L.stride_msg;
    S.off_pk_alloc = o;
    o += L.stride_pk_alloc;
    S.off_pk_not_zero = o;
    o += L.stride_pk_not_zero;
    S.off_map0 = o;
    S.off_map1 = o + (L.off_map1 - L.off_map0);
    S.off_add = o + (L.off_add - L.off_map0);
    S.off_cofactor = o + (L.off_cofactor - L.off_map0);
    o += L.stride_hash - L.sha_bits;
    S.off_prep_h = o;
    o += L.stride_prep_h;
    S.off_prep_pk = o;
    o += L.stride_prep_pk;
    m.rows_p = o;
    S.off_sig_alloc = 0;
    S.off_prep_sig = L.off_pk_not_zero - L.off_sig_alloc;  // after the sig allocation segment
    m.rows_i = S.off_prep_sig + (L.off_miller - L.off_prep_sig);
    m.split = m.rows_p > m.rows_i ? m.rows_p : m.rows_i;
    S.off_miller = m.split;
    S.off_final_exp = m.split + (L.off_final_exp - L.off_miller);
    S.off_is_one = m.split + (L.off_is_one - L.off_miller);
    m.pair_rows = L.n_witness - L.off_miller;
    S.off_expand = 0xffffffffu;  // never staged
    S.stride_msg = S.stride_pk_alloc = S.stride_pk_not_zero = S.stride_hash = S.stride_prep_h = S.stride_prep_pk = 0;
    return m;
}
// N lanes of per-(pk, msg) work, n_sig lanes of per-signature work (n_sig = N except for the N+1-pair product)
// latency = false leaves out the buffers of the latency kernels, which the value-only hash never touches: a size that is linear in N
inline Workspace carve(void* base, uint64_t N, const blsw_layout_t& L, bool with_staging, const Modes& m, uint64_t n_sig = 0, bool latency = true) {
    Workspace w;
    if (n_sig == 0) n_sig = N;
    w.sha_words = align_up((L.sha_bits + 31) / 32 + 1, BLSW_BITS_CHUNK_WORDS);
    uint64_t off = 0;
    auto take = [&](uint64_t bytes) {
        uint64_t o = off;
        off = align_up(off + bytes, 256);
        return reinterpret_cast<char*>(base) + o;
    };
    w.bits = reinterpret_cast<uint32_t*>(take(bits_tile_words(w.sha_words) * (align_up(N, 64) / 64) * 4));
    w.u = reinterpret_cast<Fp*>(take(4 * N * sizeof(Fp)));
    w.q = reinterpret_cast<Fp*>(take(12 * N * sizeof(Fp)));
    w.h = reinterpret_cast<Fp*>(take(6 * N * sizeof(Fp)));
    w.pkaff = reinterpret_cast<Fp*>(take(2 * N * sizeof(Fp)));
    w.coeff_h = reinterpret_cast<Fp*>(take(272ull * N * sizeof(Fp)));
    w.coeff_sig = reinterpret_cast<Fp*>(take(272ull * n_sig * sizeof(Fp)));
    w.n_sig = n_sig;
    w.keyproj = L.n_keys && !L.pk_mode ? reinterpret_cast<Fp*>(take(3ull * N * L.n_keys * sizeof(Fp))) : nullptr;
    const bool small = latency && N <= BLSW_LATENCY_MAX_LANES;  // (not a test of a carved pointer: with base == nullptr the carve only measures)
    w.cofv = small ? reinterpret_cast<Fp*>(take((uint64_t)BLSW_COFV_ELEMS * N * sizeof(Fp))) : nullptr;
    w.prepv_h = small ? reinterpret_cast<Fp*>(take((uint64_t)BLSW_PREPV_ELEMS * N * sizeof(Fp))) : nullptr;
    w.prepv_sig = small ? reinterpret_cast<Fp*>(take((uint64_t)BLSW_PREPV_ELEMS * n_sig * sizeof(Fp))) : nullptr;
    w.staging_rows = L.n_witness - L.sha_bits;
    if (L.n_pairs > 1 && with_staging) {  // N+1-pair product in the grouped engine: pair tiles, instance tiles, instance-major rows
        const MultiStaging ms = staging_layout_multi(L);
        w.rows_p = ms.rows_p;
        w.rows_i = ms.rows_i;
        w.split_row = ms.split;
        w.pair_rows = ms.pair_rows;
        w.staging = reinterpret_cast<Fp*>(take((uint64_t)w.rows_p * align_up(N, 64) * sizeof(Fp)));
        w.staging_inst = reinterpret_cast<Fp*>(take((uint64_t)w.rows_i * align_up(n_sig, 64) * sizeof(Fp)));
        w.pair = reinterpret_cast<Fp*>(take((uint64_t)w.pair_rows * n_sig * sizeof(Fp)));
        w.total_bytes = off;
        return w;
    }
    w.split_row = m.pairing_team ? staging_layout(L, m).off_miller : (uint32_t)w.staging_rows;
    w.pair_rows = (uint32_t)w.staging_rows - w.split_row;
    w.rows_p = w.rows_i = w.split_row;
    w.staging = with_staging ? reinterpret_cast<Fp*>(take((uint64_t)w.split_row * align_up(N, 64) * sizeof(Fp))) : nullptr;
    w.staging_inst = w.staging;
    w.pair = with_staging && w.pair_rows ? reinterpret_cast<Fp*>(take((uint64_t)w.pair_rows * N * sizeof(Fp))) : nullptr;
    w.total_bytes = off;
    return w;
}

// one submitted batch ("step"): where its inputs are and where its witness tensor / results go
struct StepDesc {
    const uint64_t* pk;
    const uint64_t* sig;
    const uint8_t* msg;
    uint64_t* out;        // [n][out_stride] field elements, or nullptr (results only)
    uint64_t out_stride;  // in field elements
    int32_t* result;
    // aggregate_verify only
    const uint64_t* keys;   // [n][n_keys][12]
    const uint8_t* bitmap;  // [n][n_keys]
    uint32_t* count;        // [n]
    // host side only: the step leaves the engine in its compact wire form (blsw_engine_submit_compact) instead of as witness vectors
    void* compact;
    // blsw_engine_submit_bytes: [n][2] decode statuses of (pk, sig); result[i] = gadget Boolean AND both statuses BLSW_ST_OK
    // (tests/tests.rs:244-263: a point that does not decode is replaced by the default and the case must verify false)
    const int32_t* status;
    // blsw_engine_submit_io: [n][n_instance_vars][6] instance_assignment of every instance (element 0 = one), or nullptr
    uint64_t* inst;
    // blsw_engine_submit_aggregate_keyset (an engine with options.shared_keys): the step's key set — its table of allocation witnesses
    // [n_keys * SEG_PK_ALLOC] elements in the engine's output form (host side: the source of the head broadcast) and its allocated projective keys
    // [3][n_keys] (x, y, z rows, Montgomery), what k_agg_sum_ks reads in place of ws.keyproj
    const uint64_t* ks_table;
    const Fp* ks_proj;
};
__device__ __forceinline__ int32_t step_result(const StepDesc& d, uint32_t i, bool res) {
    if (d.status && (d.status[2 * i] | d.status[2 * i + 1])) return 0;
    return res ? 1 : 0;
}
// Compact wire form of a step of n instances (n a multiple of 64): the step's slices of the group workspace, back to back —
// [n/64][sha_words/16][64][16] u32 bit words | [n/64][split_row][64] Fp tile-major rows | [n][pair_rows] Fp instance-major rows
// N+1-pair product (K pairs per instance, n K a multiple of 64 and n a divisor or a multiple of 64): bit words and pair tiles of the step's
// n K pair lanes | the instance tiles' rows of the step's n lanes, packed [rows_i][tile_w] with tile_w = min(n, 64) per tile | instance-major rows
struct CompactForm {
    uint64_t bits_bytes, staging_bytes, inst_bytes, pair_bytes, off_staging, off_inst, off_pair, total;
    uint32_t inst_tile_w;  // lanes per instance tile in the compact buffer (64, or n when a step is a part of one tile)
};
inline CompactForm compact_form(uint64_t n, const Workspace& w, uint32_t K = 1) {
    CompactForm c;
    c.bits_bytes = bits_tile_words(w.sha_words) * (n * K / 64) * 4;
    c.staging_bytes = (uint64_t)w.rows_p * n * K * sizeof(Fp);
    c.inst_bytes = K > 1 ? (uint64_t)w.rows_i * n * sizeof(Fp) : 0;
    c.inst_tile_w = n % 64 == 0 ? 64u : (uint32_t)n;
    c.pair_bytes = (uint64_t)w.pair_rows * n * sizeof(Fp);
    c.off_staging = align_up(c.bits_bytes, 256);
    c.off_inst = align_up(c.off_staging + c.staging_bytes, 256);
    c.off_pair = align_up(c.off_inst + c.inst_bytes, 256);
    c.total = align_up(c.off_pair + c.pair_bytes, 256);
    return c;
}
// can steps of n instances of K pairs leave in compact form (whole pair tiles; instance lanes = whole tiles or an aligned part of one)?
inline bool compact_shape_ok(uint64_t n, uint32_t K) { return K <= 1 ? n % 64 == 0 : ((n * K) % 64 == 0 && (n % 64 == 0 || 64 % n == 0)); }
// The segment the g2_team mode stages last: moved_len witnesses that belong at index lo of the vector are staged from row `at` on (len 0: none)
struct MovedSegment {
    uint32_t lo, len, at;
};
inline MovedSegment moved_segment(const blsw_layout_t& L, const Modes& m) {
    return {L.off_sig_alloc, m.g2_team ? L.off_pk_not_zero - L.off_sig_alloc : 0u, staging_layout(L, m).off_sig_alloc};
}
// blsw_compact_layout_t (include/blsw.h) of the steps of n instances of a single-key or aggregate engine: the carve's and compact_form's numbers
inline blsw_compact_layout_t compact_layout(uint64_t n, const blsw_layout_t& L, const Modes& m) {
    const Workspace w = carve(nullptr, n, L, true, m, n);
    const CompactForm cf = compact_form(n, w);
    const MovedSegment mv = moved_segment(L, m);
    blsw_compact_layout_t c;
    c.n = n;
    c.off_staging = cf.off_staging;
    c.off_pair = cf.off_pair;
    c.total = cf.total;
    c.n_witness = L.n_witness;
    c.off_expand = L.off_expand;
    c.sha_bits = L.sha_bits;
    c.sha_words = (uint32_t)w.sha_words;
    c.split_row = w.split_row;
    c.staging_rows = (uint32_t)w.staging_rows;
    c.pair_rows = w.pair_rows;
    c.moved_lo = mv.lo;
    c.moved_len = mv.len;
    c.moved_at = mv.at;
    return c;
}
// every access blsw_compact_locate / the compact checker derive from c stays inside [0, c.total) — checked before a caller's struct is used
inline bool compact_layout_ok(const blsw_compact_layout_t& c) {
    if (c.n == 0 || c.n % 64 || c.n > 65535ull * 64 || c.sha_bits > c.n_witness || c.off_expand > c.n_witness - c.sha_bits) return false;
    if (c.staging_rows != c.n_witness - c.sha_bits || c.split_row > c.staging_rows || c.pair_rows != c.staging_rows - c.split_row) return false;
    if (c.sha_words % BLSW_BITS_CHUNK_WORDS || (uint64_t)c.sha_words * 32 < c.sha_bits) return false;
    if (c.moved_len && (c.moved_at > c.staging_rows || c.moved_len != c.staging_rows - c.moved_at || c.moved_lo > c.off_expand || c.moved_len > c.off_expand - c.moved_lo))
        return false;
    if ((c.off_staging | c.off_pair) & 15) return false;
    const uint64_t bits = bits_tile_words(c.sha_words) * (c.n / 64) * 4, tiles = (uint64_t)c.split_row * c.n * sizeof(Fp), rows = (uint64_t)c.pair_rows * c.n * sizeof(Fp);
    return c.off_staging >= bits && c.off_pair >= c.off_staging && c.off_pair - c.off_staging >= tiles && c.total >= c.off_pair && c.total - c.off_pair >= rows;
}
// Where witness k of instance `lane` lives in a compact buffer: the inverse of k_place_field's row -> index rule (the SHA segment is cut out of the
// staged rows; a moved segment is staged last) followed by the addressing of the three regions. Returns BLSW_COMPACT_*; *byte_offset is the u32
// word of the bit (*bit = its position) or the element. k is wave-uniform in the checker, so region and row are scalar; only the lane term is not.
BLSW_HD uint32_t compact_locate(const blsw_compact_layout_t& c, uint32_t k, uint64_t lane, uint64_t* byte_offset, uint32_t* bit) {
    const uint64_t tile = lane >> 6, l = lane & 63;
    *bit = 0;
    if (k >= c.off_expand && k - c.off_expand < c.sha_bits) {
        const uint32_t b = k - c.off_expand, w = b >> 5;
        *bit = b & 31;
        *byte_offset = (tile * bits_tile_words(c.sha_words) + (uint64_t)(w / BLSW_BITS_CHUNK_WORDS) * (64 * BLSW_BITS_CHUNK_WORDS) + l * BLSW_BITS_CHUNK_WORDS +
                        w % BLSW_BITS_CHUNK_WORDS) * 4;
        return BLSW_COMPACT_BIT;
    }
    uint32_t row;
    if (c.moved_len && k >= c.moved_lo && k - c.moved_lo < c.moved_len) {
        row = c.moved_at + (k - c.moved_lo);
    } else {
        row = k < c.off_expand ? k : k - c.sha_bits;
        if (c.moved_len && row >= c.moved_lo) row -= c.moved_len;
    }
    if (row < c.split_row) {
        *byte_offset = c.off_staging + ((tile * c.split_row + row) * 64 + l) * sizeof(Fp);
        return BLSW_COMPACT_TILE;
    }
    *byte_offset = c.off_pair + (lane * c.pair_rows + (row - c.split_row)) * sizeof(Fp);
    return BLSW_COMPACT_PAIR;
}
// blsw_compact_layout_multi_t (include/blsw.h) of the steps of n instances of an N+1-pair engine: what compact_form(n, w, K) and launch_place_multi know
inline blsw_compact_layout_multi_t compact_layout_multi(uint64_t n, const blsw_layout_t& L) {
    const uint32_t K = L.n_pairs;
    const Workspace w = carve(nullptr, n * K, L, true, DEFAULT_MODES, n);
    const CompactForm cf = compact_form(n, w, K);
    const blsw_layout_t S = staging_layout_multi(L).LS;
    blsw_compact_layout_multi_t c;
    memset(&c, 0, sizeof(c));
    c.n = n;
    c.off_staging = cf.off_staging;
    c.off_inst = cf.off_inst;
    c.off_pair = cf.off_pair;
    c.total = cf.total;
    c.n_pairs = K;
    c.n_witness = L.n_witness;
    c.sha_bits = L.sha_bits;
    c.sha_words = (uint32_t)w.sha_words;
    c.off_expand = L.off_expand;
    c.stride_hash = L.stride_hash;
    c.rows_p = w.rows_p;
    c.rows_i = w.rows_i;
    c.pair_rows = w.pair_rows;
    c.inst_tile_w = cf.inst_tile_w;
    c.off_miller = L.off_miller;
    const uint32_t src[7] = {S.off_msg, S.off_pk_alloc, S.off_pk_not_zero, S.off_map0, S.off_prep_h, S.off_prep_pk, w.rows_p};  // launch_place_multi's runs
    const uint32_t dst[6] = {L.off_msg, L.off_pk_alloc, L.off_pk_not_zero, L.off_map0, L.off_prep_h, L.off_prep_pk};
    const uint32_t str[6] = {L.stride_msg, L.stride_pk_alloc, L.stride_pk_not_zero, L.stride_hash, L.stride_prep_h, L.stride_prep_pk};
    for (int r = 0; r < 6; r++) c.pair_run_row[r] = src[r], c.pair_run_off[r] = dst[r], c.pair_run_stride[r] = str[r], c.pair_run_len[r] = src[r + 1] - src[r];
    c.inst_run_row[0] = S.off_sig_alloc;
    c.inst_run_row[1] = S.off_prep_sig;
    c.inst_run_off[0] = L.off_sig_alloc;
    c.inst_run_off[1] = L.off_prep_sig;
    c.inst_run_len[0] = S.off_prep_sig - S.off_sig_alloc;
    c.inst_run_len[1] = w.rows_i - S.off_prep_sig;
    return c;
}
#define BLSW_COMPACT_NONE 0xffffffffu  // compact_place_multi: no region holds the witness (never for a struct compact_layout_multi_ok accepts)
// Where witness k of an N+1-pair instance lives, the part that does not depend on the instance: the region, the pair j whose lane holds it (BIT,
// TILE; 0 otherwise) and the row — the u32 word of the lane's bit stream (BIT, *bit = the position in it) or the staged row of the region. The
// inverse of k_place_runs / k_place_rows and of the expansion's off_expand + j * stride_hash + b rule. k is wave-uniform in the checker: all of
// this is scalar arithmetic.
BLSW_HD uint32_t compact_place_multi(const blsw_compact_layout_multi_t& c, uint32_t k, uint32_t* j, uint32_t* row, uint32_t* bit) {
    *j = 0;
    *row = 0;
    *bit = 0;
    if (k >= c.off_miller) {
        *row = k - c.off_miller;
        return *row < c.pair_rows ? (uint32_t)BLSW_COMPACT_PAIR : BLSW_COMPACT_NONE;
    }
    if (k >= c.off_expand && c.stride_hash) {
        const uint32_t d = k - c.off_expand, jj = d / c.stride_hash, b = d - jj * c.stride_hash;
        if (jj < c.n_pairs) {  // pair jj's hash_to_g2: its SHA bits, then run 3 (compact_layout_multi_ok: pair_run_len[3] = stride_hash - sha_bits) — most of z
            *j = jj;
            if (b < c.sha_bits) {
                *row = b >> 5;
                *bit = b & 31;
                return BLSW_COMPACT_BIT;
            }
            *row = c.pair_run_row[3] + (b - c.sha_bits);
            return BLSW_COMPACT_TILE;
        }
    }
    for (int r = 0; r < 6; r++) {
        if (r == 3 || !c.pair_run_len[r] || !c.pair_run_stride[r] || k < c.pair_run_off[r]) continue;
        const uint32_t d = k - c.pair_run_off[r], jj = d / c.pair_run_stride[r], t = d - jj * c.pair_run_stride[r];
        if (jj < c.n_pairs && t < c.pair_run_len[r]) {
            *j = jj;
            *row = c.pair_run_row[r] + t;
            return BLSW_COMPACT_TILE;
        }
    }
    for (int r = 0; r < 2; r++)
        if (k >= c.inst_run_off[r] && k - c.inst_run_off[r] < c.inst_run_len[r]) {
            *row = c.inst_run_row[r] + (k - c.inst_run_off[r]);
            return BLSW_COMPACT_INST;
        }
    return BLSW_COMPACT_NONE;
}
// ... and the part that does: the byte offset of (region, row) for a lane — the PAIR LANE i K + j for BIT and TILE, the instance for INST and PAIR
BLSW_HD uint64_t compact_address_multi(const blsw_compact_layout_multi_t& c, uint32_t region, uint32_t row, uint64_t lane) {
    const uint64_t tile = lane >> 6, l = lane & 63;
    if (region == BLSW_COMPACT_BIT)
        return (tile * bits_tile_words(c.sha_words) + (uint64_t)(row / BLSW_BITS_CHUNK_WORDS) * (64 * BLSW_BITS_CHUNK_WORDS) + l * BLSW_BITS_CHUNK_WORDS +
                row % BLSW_BITS_CHUNK_WORDS) * 4;
    if (region == BLSW_COMPACT_TILE) return c.off_staging + ((tile * c.rows_p + row) * 64 + l) * sizeof(Fp);
    if (region == BLSW_COMPACT_INST) return c.off_inst + (((lane / c.inst_tile_w) * c.rows_i + row) * c.inst_tile_w + lane % c.inst_tile_w) * sizeof(Fp);
    return c.off_pair + (lane * c.pair_rows + row) * sizeof(Fp);
}
// witness k of instance i: the two together (blsw_compact_locate_multi; the general path of the device checker)
BLSW_HD uint32_t compact_locate_multi(const blsw_compact_layout_multi_t& c, uint32_t k, uint64_t i, uint64_t* byte_offset, uint32_t* bit) {
    uint32_t j, row;
    const uint32_t region = compact_place_multi(c, k, &j, &row, bit);
    *byte_offset = 0;
    if (region == BLSW_COMPACT_NONE) return region;
    *byte_offset = compact_address_multi(c, region, row, region <= BLSW_COMPACT_TILE ? i * c.n_pairs + j : i);
    return region;
}
// The struct is exactly what compact_layout_multi gives for some shape: then the runs tile [0, n_witness) (every k has one place) and every address
// compact_address_multi derives for k < n_witness, instance < n lies inside its region, the regions inside [0, total). Checked on the host before
// the locator or a kernel reads through a caller's struct.
inline bool compact_layout_multi_ok(const blsw_compact_layout_multi_t& c) {
    const uint32_t K = c.n_pairs;
    // n is the caller's u64: bounded on its own before any product is formed (n K <= 65535 is the engine's rule)
    if (c.n == 0 || K < 2 || K > 4096 || c.n > 65535 / K || !compact_shape_ok(c.n, K) || c.reserved) return false;
    if (c.inst_tile_w != (c.n % 64 == 0 ? 64u : (uint32_t)c.n)) return false;
    if (c.sha_bits > c.stride_hash || c.sha_words != align_up((c.sha_bits + 31) / 32 + 1, BLSW_BITS_CHUNK_WORDS)) return false;
    if (c.off_miller > c.n_witness || c.pair_rows != c.n_witness - c.off_miller) return false;
    // staged rows: the runs one after the other from row 0, a pair's copy of a run one stride after the previous pair's
    uint32_t row = 0;
    for (int r = 0; r < 6; r++) {
        if (c.pair_run_row[r] != row || c.pair_run_len[r] > c.rows_p - row) return false;
        if (r == 3 ? (c.pair_run_stride[r] != c.stride_hash || c.pair_run_len[r] != c.stride_hash - c.sha_bits || c.pair_run_off[r] - c.sha_bits != c.off_expand)
                   : (c.pair_run_len[r] != c.pair_run_stride[r]))
            return false;
        row += c.pair_run_len[r];
    }
    if (row != c.rows_p) return false;
    row = 0;
    for (int r = 0; r < 2; r++) {
        if (c.inst_run_row[r] != row || c.inst_run_len[r] > c.rows_i - row) return false;
        row += c.inst_run_len[r];
    }
    if (row != c.rows_i) return false;
    // the witness vector: the nine blocks (K copies of a run; the hash block with its bits; the instance runs; the instance rows), sorted, tile it
    uint64_t lo[9], len[9];
    for (int r = 0; r < 6; r++) lo[r] = r == 3 ? c.off_expand : c.pair_run_off[r], len[r] = (uint64_t)K * c.pair_run_stride[r];
    for (int r = 0; r < 2; r++) lo[6 + r] = c.inst_run_off[r], len[6 + r] = c.inst_run_len[r];
    lo[8] = c.off_miller;
    len[8] = c.pair_rows;
    uint64_t at = 0;
    for (int done = 0; done < 9; done++) {  // the empty blocks first, then the one that starts where the last one ended
        int pick = -1;
        for (int b = 0; b < 9 && pick < 0; b++)
            if (len[b] == 0 && lo[b] != ~0ull) pick = b;
        for (int b = 0; b < 9 && pick < 0; b++)
            if (len[b] && lo[b] == at) pick = b;
        if (pick < 0) return false;
        at += len[pick];
        lo[pick] = ~0ull;
        len[pick] = 1;
    }
    if (at != c.n_witness) return false;
    // the buffer: compact_form's offsets
    const uint64_t bits = bits_tile_words(c.sha_words) * (c.n * K / 64) * 4;
    if (c.off_staging != align_up(bits, 256)) return false;
    if (c.off_inst != align_up(c.off_staging + (uint64_t)c.rows_p * c.n * K * sizeof(Fp), 256)) return false;
    if (c.off_pair != align_up(c.off_inst + (uint64_t)c.rows_i * c.n * sizeof(Fp), 256)) return false;
    return c.total == align_up(c.off_pair + (uint64_t)c.pair_rows * c.n * sizeof(Fp), 256);
}
// a group of `steps` batches of n instances each, processed by one set of launches (N = steps * n * K lanes per chain;
// K = (pk, msg) pairs per instance: 1 except for the N+1-pair product)
struct Group {
    uint64_t N;
    uint32_t n;   // instances per step
    uint32_t K;   // pairs per instance
    uint32_t msg_len;
    uint32_t msg_wit_len;  // message bytes k_sha allocates as witness booleans: msg_len, or 0 when the message is a public input (k_msg_input)
    const StepDesc* desc;  // device array [steps]
    blsw_layout_t L;       // offsets in the witness vector
    blsw_layout_t LS;      // offsets in the staging rows (the vector with the SHA segment cut out)
    Workspace ws;
    int chain_prio;        // chain waves raise s_setprio
    int canonical;         // instance_assignment elements as canonical integers (options.output_form 1) instead of Montgomery limbs
};
// workspace / staging / tensor accesses: global address space stated (see Emitter::put)
__device__ __forceinline__ Fp ld_fp(const Fp* p) {
    const blsw_global_u32x4* s = (const blsw_global_u32x4*)p;
    blsw_u32x4 a = s[0], b = s[1], c = s[2];
    Fp r;
    r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
    r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
    r.l[8] = c.x; r.l[9] = c.y; r.l[10] = c.z; r.l[11] = c.w;
    return r;
}
__device__ __forceinline__ void st_fp(Fp* p, const Fp& v) {
    blsw_global_u32x4* d = (blsw_global_u32x4*)p;
    d[0] = blsw_u32x4{v.l[0], v.l[1], v.l[2], v.l[3]};
    d[1] = blsw_u32x4{v.l[4], v.l[5], v.l[6], v.l[7]};
    d[2] = blsw_u32x4{v.l[8], v.l[9], v.l[10], v.l[11]};
}
__device__ __forceinline__ Fp2 ld_fp2(const Fp* p, uint64_t n) { return {ld_fp(p), ld_fp(p + n)}; }

// lane -> (step, instance-in-step, pair). Inputs of per-pair work are indexed by f (flat [n][K]), outputs by (i, j).
struct LaneId {
    uint64_t I;
    uint32_t s, i, j, f;
};
__device__ __forceinline__ LaneId lane_id(const Group& g, uint64_t I) {
    LaneId r;
    r.I = I;
    const uint32_t nk = g.n * g.K;
    r.s = (uint32_t)(I / nk);
    r.f = (uint32_t)(I - (uint64_t)r.s * nk);
    r.i = g.K == 1 ? r.f : r.f / g.K;
    r.j = g.K == 1 ? 0u : r.f - r.i * g.K;
    return r;
}
// element k of instance (step s, i)'s instance_assignment := v (blsw_engine_submit_io); the witness kernels write the inputs they allocate
__device__ __forceinline__ void put_instance(const Group& g, const LaneId& id, uint32_t k, const Fp& v) {
    uint64_t* base = g.desc[id.s].inst;
    if (!base) return;
    st_fp(reinterpret_cast<Fp*>(base) + ((uint64_t)id.i * g.L.n_instance_vars + k), g.canonical ? fp_to_canonical(v) : v);
}

// witness cursor for a segment: staging row (engine mode), the instance's dense vector (direct mode), or value-only
// per_pair: the segment belongs to a (pk, msg) pair (the lane is a pair lane) — else to the instance / signature
__device__ __forceinline__ Emitter emitter(const Group& g, const LaneId& id, uint32_t off_full, uint32_t off_staging, bool per_pair) {
    Emitter e;
    if (g.ws.staging) {
        if (!per_pair && off_staging >= g.ws.split_row) {  // instance-major rows of the pairing segments
            e.base = reinterpret_cast<uint32_t*>(g.ws.pair + id.I * g.ws.pair_rows);
            e.pos = off_staging - g.ws.split_row;
            e.stride = 12;
            return e;
        }
        Fp* tiles = per_pair ? g.ws.staging : g.ws.staging_inst;
        const uint32_t rows = per_pair ? g.ws.rows_p : g.ws.rows_i;
        e.base = reinterpret_cast<uint32_t*>(tiles + (id.I >> 6) * (uint64_t)rows * 64 + (id.I & 63));
        e.pos = off_staging;
        e.stride = 64 * 12;
        return e;
    }
    const StepDesc& d = g.desc[id.s];
    e.base = d.out ? reinterpret_cast<uint32_t*>(d.out + (uint64_t)id.i * d.out_stride * 6) : nullptr;
    e.pos = off_full;
    e.stride = 12;
    return e;
}
#define EMIT(g, id, field) emitter(g, id, (g).L.field, (g).LS.field, false)
// segment that exists once per pair: in the vector pair j's copy starts j * stride further; in the staging a pair is a lane of its own
// (LS.stride = 0) unless the staging IS the vector (direct mode: LS = L)
#define EMITJ(g, id, field, stride) emitter(g, id, (g).L.field + (id).j * (g).L.stride, (g).LS.field + (id).j * (g).LS.stride, true)

__device__ __forceinline__ Proj<OpsFp2> ld_proj2(const Fp* p, uint64_t n) {
    Proj<OpsFp2> r;
    r.x = ld_fp2(p, n);
    r.y = ld_fp2(p + 2 * n, n);
    r.z = ld_fp2(p + 4 * n, n);
    return r;
}

// line coefficients, element-major: coefficient idx of instance I at p[idx * N]
struct CoeffStrided {
    Fp* p;
    uint64_t n;
    __device__ __forceinline__ void st(uint32_t idx, const Fp& v) const {
        if (item_leader()) st_fp(p + (uint64_t)idx * n, v);
    }
    __device__ __forceinline__ Fp ld(uint32_t idx) const { return ld_fp(p + (uint64_t)idx * n); }
};

// bitstream -> Fp elements: element e of the expand segment = bit ? R mod p : 0. The segment is a stream of 16-byte pieces
// (piece p = element p / 3, column p % 3) that starts at an arbitrary multiple of 16 bytes (instance vectors are 33 956 496
// bytes apart). blockIdx.y = flat (instance, pair) index of the step. Three store geometries (blsw_engine_options_t::
// expand_variant; measured alone in tools/expand_lab.hip -> profiles/r02_expand_lab.txt, and in the pipeline by bench.py):
//   0  384-thread workgroups, 8 pieces per thread 6 KiB apart, pieces counted from the first 256-byte boundary
//   1  256-thread workgroups, ONE piece per thread, every workgroup writes one 4 KiB-aligned 4 KiB chunk of the address space
//   2  768-thread workgroups, 8 pieces per thread 12 KiB apart: every iteration writes three 4 KiB-aligned chunks; column and
//      bit position of a thread are loop invariants (768 = 3 * 256 pieces = 256 elements = 8 bit words per iteration)
//   3  as 2 with 4 pieces per thread;  4  as 2 with 16;  5  384 threads x 16 pieces, 4 KiB-aligned start
struct ExpandArgs {
    const uint32_t* bits;
    uint64_t sha_words, first;
    uint32_t sha_bits, off_expand;
    uint64_t* d_witness;
    uint64_t stride;
    uint32_t K, stride_hash;  // K = 1 for the single-key circuit
    int prio;                 // raise the wave priority (s_setprio 3): wins VALU issue arbitration against the chain waves
    int canonical;            // elements as canonical integers (true = 1) instead of Montgomery form (true = R mod p)
};
#define BLSW_EXPAND_RESIDENT_WGS 512u  // expand_variant 13 (k_stream.hip): two 384-thread workgroups per compute unit

#define BLSW_TEAMS_PER_WAVE 10
#ifndef BLSW_PLACE_ITERS
#define BLSW_PLACE_ITERS 8
#endif
#define BLSW_DIGEST_ITERS 16
#define BLSW_DIGEST_MAX_BLOCKS 4096  // workgroups per instance of k_digest (a single-key vector has 2 073 chunks)
#define BLSW_DIGEST_KEY 0x9E3779B1u  // odd (golden ratio): key_q = (q + 1) * KEY mod 2^32 is a bijection of q
#define BLSW_DIGEST_A 0x85EBCA6Bu

// ---------------------------------------------------------------- kernels (defined in k_*.hip, launched by engine.hip)
// A chain kernel's compilations (build.py: CHAIN_UNITS): grouped engine (name), direct mode (name_inl), latency (name_q)
#define BLSW_CHAIN_I(name, params) __global__ void name params; __global__ void name##_inl params;
#define BLSW_CHAIN_Q(name, params) __global__ void name params; __global__ void name##_q params;
#define BLSW_CHAIN_IQ(name, params) BLSW_CHAIN_I(name, params) __global__ void name##_q params;
BLSW_CHAIN_I(k_sha, (Group g, int want_bits, int write_u))
BLSW_CHAIN_I(k_g1, (Group g))
BLSW_CHAIN_I(k_agg_keys, (Group g, Fp* keyproj))
BLSW_CHAIN_I(k_agg_sum, (Group g, const Fp* keyproj))
BLSW_CHAIN_I(k_agg_sum_in, (Group g))
BLSW_CHAIN_I(k_agg_sum_ks, (Group g))
BLSW_CHAIN_I(k_cofactor, (Group g))
BLSW_CHAIN_I(k_cofactor_chunk, (Group g))
BLSW_CHAIN_I(k_cofactor_join, (Group g))
BLSW_CHAIN_IQ(k_g2_alloc, (Group g))
BLSW_CHAIN_IQ(k_map, (Group g))
BLSW_CHAIN_IQ(k_prepare, (Group g, int which))
// values-first prepare chains (prepare_vf.hpp; k_prepare.hip): the serial value phase per point, then one lane per step
BLSW_CHAIN_Q(k_prepv_chain, (Group g, int which))
__global__ void k_prepv_step_w(Group g, int which);
// values-first cofactor chain (cofactor_vf.hpp; k_cofv.hip): serial value phases (one lane or one quad per item), parallel witness phases, join
BLSW_CHAIN_Q(k_cofv_chain, (Group g, int s))
BLSW_CHAIN_Q(k_cofv_bwd, (Group g, int s))
BLSW_CHAIN_Q(k_cofv_acc, (Group g, int s))
BLSW_CHAIN_Q(k_cofv_az, (Group g))
__global__ void k_cofv_aff(Group g, uint32_t lo, uint32_t cnt);
__global__ void k_cofv_dbl_w(Group g);
__global__ void k_cofv_add_w(Group g);
__global__ void k_cofv_join(Group g);
__global__ void k_sha_values(Group g);
__global__ void k_sha_values_dst(Group g, DstArg a, const uint8_t* d_msg, Fp* d_u);
__global__ void k_msg_input(Group g);
__global__ void k_agg_instance(Group g, uint32_t n_elems, uint32_t s0);
__global__ void k_map_values(Group g);
__global__ void k_cofactor_values(Group g);
__global__ void k_place_field(const Fp* __restrict__ staging, const Fp* __restrict__ pair, uint64_t first, uint32_t off_expand, uint32_t sha_bits,
                              uint32_t staging_rows, uint32_t split_row, uint64_t* __restrict__ d_witness, uint64_t stride, uint32_t n_inst, uint32_t moved_lo,
                              uint32_t moved_len, uint32_t moved_at);
__global__ void k_canonical_rows(uint64_t* __restrict__ d_witness, uint64_t stride, uint32_t off_expand, uint32_t sha_bits, uint32_t rows, uint32_t K, uint32_t stride_hash);
__global__ void k_digest(const uint64_t* __restrict__ w, uint64_t stride, uint64_t n_words, uint64_t* __restrict__ digest);
__global__ void k_pairing(Group g);
__global__ void k_pairing_team(Group g);
__global__ void k_pairing_team_pv(Group g);
__global__ void k_g2_alloc_team(Group g);
__global__ void k_pairing_team_multi(Group gs, uint32_t K, uint64_t n_h);
__global__ void k_decode(const uint8_t* __restrict__ pk48, const uint8_t* __restrict__ sig96, uint64_t n, uint64_t* pk_xy, uint64_t* sig_xy, int32_t* status);
__global__ void k_h_to_affine(uint64_t n, Workspace ws, uint64_t* d_out);
__global__ void k_decode_points(uint32_t group, const uint8_t* __restrict__ in, uint64_t m, Fp* xy, int32_t* st);
__global__ void k_sum_points(uint32_t group, const Fp* __restrict__ xy, const int32_t* __restrict__ pst, uint32_t k, uint64_t n, uint8_t* out, int32_t* status);
__global__ void k_sign(uint64_t n, Workspace ws, const uint8_t* __restrict__ sk32, uint8_t* sig96, uint64_t* sig_xy, uint8_t* pk48, uint64_t* pk_xy, int32_t* status);
__global__ void k_pop_pk(uint64_t n, const uint8_t* __restrict__ sk32, uint8_t* pk48);
__global__ void k_bench_mad(uint32_t iters, uint32_t* out);
__global__ void k_bench_fill(uint4* __restrict__ dst, uint64_t n16);
__global__ void k_bench_fpmul(uint32_t iters, uint32_t* out);
__global__ void k_bench_fpmul32(uint32_t iters, uint32_t* out);
__global__ void k_bench_fpinv(uint32_t iters, uint32_t* out);
__global__ void k_bench_fp2mulw(uint32_t iters, uint32_t* out);
// pair-parallel Miller product (k_miller_par.hip, miller_par.hpp): value stores of n instances, element-major Fp12 rows
struct MillerParArgs {
    Fp* cprod;   // [12][n * 68 * C] chunk products
    Fp* q;       // [12][n * 68 * C] prefixes over the chunks of a step
    Fp* t;       // [12][n * 68]     product of all pairs of a step
    Fp* f1;      // [12][n * 68]     the running value after ell(sig) of a step
    Fp* ffinal;  // [12][n]          conj(f) after the loop
    uint32_t K, B, C;  // pairs, pairs per chunk, chunks
    uint64_t n_h;      // n * K: lanes of the per-pair launches (where the pairs' line coefficients / prepared keys live)
    uint32_t spine_lane;  // 1: the single-lane spine kernel (k_miller_m2; the statement shared with the host harness) instead of the team kernel
};
#define BLSW_MILLER_CHUNK_DEFAULT 12  // pairs per lane of the engine's pair-parallel Miller product
// The value stores of n instances of K pairs at `base`, each 256-byte aligned; *bytes (miller_par_bytes) is the size the same rows are given
inline MillerParArgs carve_miller_par(char* base, uint64_t n, uint32_t K, uint64_t* bytes = nullptr) {
    MillerParArgs a = {};
    a.K = K;
    a.B = BLSW_MILLER_CHUNK_DEFAULT;
    a.C = (K + a.B - 1) / a.B;
    a.n_h = n * K;
    Fp** const store[5] = {&a.cprod, &a.q, &a.t, &a.f1, &a.ffinal};
    const uint64_t rows[5] = {n * 68 * a.C, n * 68 * a.C, n * 68, n * 68, n};
    uint64_t off = 0, need = 0;
    for (int i = 0; i < 5; i++) {
        *store[i] = reinterpret_cast<Fp*>(base + off);
        off += align_up(rows[i] * 12 * sizeof(Fp), 256);
        need += rows[i] * 12 * sizeof(Fp) + 256;
    }
    if (bytes) *bytes = need;
    return a;
}
inline uint64_t miller_par_bytes(uint64_t n, uint32_t K) {
    uint64_t bytes = 0;
    carve_miller_par(nullptr, n, K, &bytes);
    return bytes;
}
void launch_miller_par(const Group& gs, const MillerParArgs& a, hipStream_t st, hipStream_t side, hipEvent_t ev_spine, hipEvent_t ev_side);
// Placement of the N+1-pair product's staged rows (k_stream.hip): up to six runs of consecutive staging rows of a lane, each going to
// dst_off + j * dst_stride of the lane's instance vector (j = pair index of the lane; 0 for instance lanes)
struct PlaceRuns {
    uint32_t n_runs;
    uint32_t src_row[7];  // first staging row of run r; src_row[n_runs] = rows of the tile
    uint32_t dst_off[6], dst_stride[6];
};
__global__ void k_place_runs(const Fp* __restrict__ tiles, uint64_t first, uint32_t rows, PlaceRuns runs, uint64_t* __restrict__ d_witness, uint64_t stride, uint32_t n_y,
                             uint32_t K, uint32_t tile_w);
__global__ void k_place_rows(const Fp* __restrict__ rows, uint32_t n_rows, uint32_t dst_off, uint64_t* __restrict__ d_witness, uint64_t stride);
// The chain kernels a launch group or a direct call starts, in the compilations it picked (chain_kernels). The quad-capable ones — G2 allocation,
// map, prepare and the serial phases of the values-first chains (prepare_vf.hpp, cofactor_vf.hpp) — run `lpi` lanes per item, the others one.
struct ChainKernels {
    void (*sha)(Group, int, int);
    void (*g1)(Group);
    void (*agg_keys)(Group, Fp*);
    void (*agg_sum)(Group, const Fp*);
    void (*agg_sum_in)(Group);  // the keys are public inputs (L.pk_mode): no allocated keys to read
    void (*agg_sum_ks)(Group);  // the keys are the step's shared key set (StepDesc::ks_proj)
    void (*cofactor)(Group);
    void (*cofactor_chunk)(Group);  // the cofactor segment with its three chunks on three lanes, and the join (cofactor_par.hpp)
    void (*cofactor_join)(Group);
    void (*g2_alloc)(Group);
    void (*map)(Group);
    void (*prepare)(Group, int);
    void (*prepv_chain)(Group, int);
    void (*cofv_chain)(Group, int);
    void (*cofv_bwd)(Group, int);
    void (*cofv_acc)(Group, int);
    void (*cofv_az)(Group);
    unsigned lpi;
};
// inlined: the direct-mode compilation (*_inl) instead of the grouped engine's; quad: the latency compilation (*_q, four lanes per item) of the
// quad-capable kernels. The values-first phases have no direct-mode compilation: without quad they are the grouped one whatever `inlined` says.
inline ChainKernels chain_kernels(bool inlined, bool quad) {
#define BLSW_PICK_I(name) (inlined ? name##_inl : name)
#define BLSW_PICK_Q(name) (quad ? name##_q : name)
#define BLSW_PICK_IQ(name) (quad ? name##_q : BLSW_PICK_I(name))
    return {BLSW_PICK_I(k_sha), BLSW_PICK_I(k_g1), BLSW_PICK_I(k_agg_keys), BLSW_PICK_I(k_agg_sum), BLSW_PICK_I(k_agg_sum_in), BLSW_PICK_I(k_agg_sum_ks), BLSW_PICK_I(k_cofactor),
            BLSW_PICK_I(k_cofactor_chunk), BLSW_PICK_I(k_cofactor_join), BLSW_PICK_IQ(k_g2_alloc), BLSW_PICK_IQ(k_map), BLSW_PICK_IQ(k_prepare), BLSW_PICK_Q(k_prepv_chain),
            BLSW_PICK_Q(k_cofv_chain), BLSW_PICK_Q(k_cofv_bwd), BLSW_PICK_Q(k_cofv_acc), BLSW_PICK_Q(k_cofv_az), quad ? 4u : 1u};
#undef BLSW_PICK_I
#undef BLSW_PICK_Q
#undef BLSW_PICK_IQ
}
// clear_cofactor2 of N lanes on `st`: values first, chunked (three lanes per (pk, msg) pair + the join) or as one chain per lane.
// Values first with side streams (CofactorSide): `st` carries the forward doubling chain in its segments and the last segment's tail. Beside it, as soon
// as a segment's doublings are done (ev_seg): its inversion / affine points on pts, in segment order (ev_pts), and its part of its chunk's addition chain
// on acc[0] (chunks 0 and 2) or acc[1] (chunk 1); the join waits for the chunks (ev_acc). The witness phases (one lane per doubling / addition, and the
// chunks' 1 / Z1 sweeps: nothing but the segment's placement waits for them) are left to launch_cofactor_witness on `side`, after ev_join.
// side == nullptr: everything on `st`.
struct CofactorSide {
    hipStream_t side, pts, acc[2];
    hipEvent_t ev_seg[BLSW_COFV_NSEG], ev_pts[BLSW_COFV_NSEG], ev_acc[3], ev_join;
};
#define BLSW_COFV_EVENTS (2 * BLSW_COFV_NSEG + 4)
// a CofactorSide of four streams and an array of BLSW_COFV_EVENTS events: ev_seg, ev_pts, ev_acc, ev_join in that order
inline CofactorSide cofactor_side(hipStream_t side, hipStream_t pts, hipStream_t acc0, hipStream_t acc1, const hipEvent_t ev[BLSW_COFV_EVENTS]) {
    CofactorSide cs;
    cs.side = side;
    cs.pts = pts;
    cs.acc[0] = acc0;
    cs.acc[1] = acc1;
    for (int i = 0; i < BLSW_COFV_NSEG; i++) cs.ev_seg[i] = ev[i], cs.ev_pts[i] = ev[BLSW_COFV_NSEG + i];
    for (int i = 0; i < 3; i++) cs.ev_acc[i] = ev[2 * BLSW_COFV_NSEG + i];
    cs.ev_join = ev[2 * BLSW_COFV_NSEG + 3];
    return cs;
}
inline uint64_t cofv_total_adds() {
    constexpr CofvPlan plan = cofv_plan();
    return (uint64_t)plan.n_adds[0] + plan.n_adds[1] + plan.n_adds[2];
}
// phases 1b and 2a of segment s: 1 / Z of its points, then the points in affine form
inline void launch_cofv_points(const ChainKernels& ck, const Group& g, int s, hipStream_t q) {
    constexpr CofvSeg seg = cofv_seg();
    hipLaunchKernelGGL(ck.cofv_bwd, dim3(item_grid(g.N, ck.lpi)), dim3(64), 0, q, g, s);
    const uint32_t lo = s == 0 ? 0 : seg.bnd[s] + 1u;
    const uint32_t hi = seg.bnd[s + 1] < BLSW_H_EFF_NBITS ? seg.bnd[s + 1] : BLSW_H_EFF_NBITS - 1;  // the last point of the chain is not an operand
    hipLaunchKernelGGL(k_cofv_aff, dim3(item_grid((uint64_t)(hi - lo + 1) * g.N, 1)), dim3(64), 0, q, g, lo, hi - lo + 1);
}
inline void launch_cofv_witness_phases(const ChainKernels& ck, const Group& g, hipStream_t q) {
    hipLaunchKernelGGL(k_cofv_dbl_w, dim3(item_grid((uint64_t)BLSW_H_EFF_NBITS * g.N, 1)), dim3(64), 0, q, g);
    hipLaunchKernelGGL(ck.cofv_az, dim3(item_grid(3 * g.N, ck.lpi)), dim3(64), 0, q, g);
    hipLaunchKernelGGL(k_cofv_add_w, dim3(item_grid(cofv_total_adds() * g.N, 1)), dim3(64), 0, q, g);
}
// vf: clear_cofactor2 values first (cofactor_vf.hpp), if the workspace has its scratch (small groups)
inline void launch_cofactor(const ChainKernels& ck, bool vf, bool chunked, const Group& g, hipStream_t st, const CofactorSide* side = nullptr) {
    const unsigned g1 = item_grid(g.N, 1), g3 = item_grid(3 * g.N, 1), gq = item_grid(g.N, ck.lpi);
    if (vf && g.ws.cofv) {
        constexpr CofvSeg seg = cofv_seg();
        constexpr int last = BLSW_COFV_NSEG - 1;
        if (!side) {
            for (int s = 0; s <= last; s++) {
                hipLaunchKernelGGL(ck.cofv_chain, dim3(gq), dim3(64), 0, st, g, s);
                launch_cofv_points(ck, g, s, st);
                hipLaunchKernelGGL(ck.cofv_acc, dim3(gq), dim3(64), 0, st, g, s);
            }
            hipLaunchKernelGGL(k_cofv_join, dim3(g1), dim3(64), 0, st, g);
            launch_cofv_witness_phases(ck, g, st);
            return;
        }
        for (int s = 0; s <= last; s++) {
            hipLaunchKernelGGL(ck.cofv_chain, dim3(gq), dim3(64), 0, st, g, s);
            hipEventRecord(side->ev_seg[s], st);
        }
        for (int s = 0; s < last; s++) {
            hipStreamWaitEvent(side->pts, side->ev_seg[s], 0);
            launch_cofv_points(ck, g, s, side->pts);
            hipEventRecord(side->ev_pts[s], side->pts);
            hipStream_t q = side->acc[seg.chunk[s] == 1 ? 1 : 0];
            hipStreamWaitEvent(q, side->ev_pts[s], 0);
            hipLaunchKernelGGL(ck.cofv_acc, dim3(gq), dim3(64), 0, q, g, s);
            if (seg.last(s) || s == last - 1) hipEventRecord(side->ev_acc[seg.chunk[s]], q);
        }
        launch_cofv_points(ck, g, last, st);
        hipStreamWaitEvent(st, side->ev_acc[2], 0);  // the chunk's additions before the last segment's
        hipLaunchKernelGGL(ck.cofv_acc, dim3(gq), dim3(64), 0, st, g, last);
        hipStreamWaitEvent(st, side->ev_acc[0], 0);
        hipStreamWaitEvent(st, side->ev_acc[1], 0);
        hipLaunchKernelGGL(k_cofv_join, dim3(g1), dim3(64), 0, st, g);
        hipEventRecord(side->ev_join, st);
    } else if (chunked) {
        hipLaunchKernelGGL(ck.cofactor_chunk, dim3(g3), dim3(64), 0, st, g);
        hipLaunchKernelGGL(ck.cofactor_join, dim3(g1), dim3(64), 0, st, g);
    } else {
        hipLaunchKernelGGL(ck.cofactor, dim3(g1), dim3(64), 0, st, g);
    }
}
// the deferred witness phases of a values-first cofactor chain (launch_cofactor with side streams), enqueued on the side stream
inline void launch_cofactor_witness(const ChainKernels& ck, const Group& g, const CofactorSide& side) {
    hipStreamWaitEvent(side.side, side.ev_join, 0);
    launch_cofv_witness_phases(ck, g, side.side);
}
inline void launch_map(const ChainKernels& ck, const Group& g, hipStream_t st) { hipLaunchKernelGGL(ck.map, dim3(item_grid(2 * g.N, ck.lpi)), dim3(64), 0, st, g); }
// vf: prepare_g2 values first (prepare_vf.hpp), if the workspace has its scratch (small groups)
inline void launch_prepare(const ChainKernels& ck, bool vf, const Group& g, int which, hipStream_t st) {
    if (vf && g.ws.prepv_h) {
        hipLaunchKernelGGL(ck.prepv_chain, dim3(item_grid(g.N, ck.lpi)), dim3(64), 0, st, g, which);
        hipLaunchKernelGGL(k_prepv_step_w, dim3(item_grid((uint64_t)BLSW_PREPV_STEPS * g.N, 1)), dim3(64), 0, st, g, which);
    } else
        hipLaunchKernelGGL(ck.prepare, dim3(item_grid(g.N, ck.lpi)), dim3(64), 0, st, g, which);
}
inline void launch_g2_alloc(const ChainKernels& ck, const Group& g, hipStream_t st) { hipLaunchKernelGGL(ck.g2_alloc, dim3(item_grid(g.N, ck.lpi)), dim3(64), 0, st, g); }
// host-side launch helpers that live next to their (templated) kernels
// shared key sets (k_keyset.hip): the allocation chain of K keys into a dense table + their projective points [3][K]; the table copied into the
// heads of n instance vectors (order: 0 instance fastest, 1 chunk fastest — blsw_keyset_broadcast_rate measures both, the engine launches 0)
void launch_keyset_alloc(const uint64_t* pks_xy, uint32_t n_keys, Fp* table, Fp* proj, hipStream_t st);
void launch_keys_broadcast(const uint64_t* table, uint64_t n_elements, uint64_t* d_witness, uint64_t stride, uint64_t n, uint32_t order, hipStream_t st);
void launch_expand(uint32_t variant, uint32_t store, unsigned lds, hipStream_t st, ExpandArgs a, unsigned n_y);
void launch_pairing(const Group& g, const Modes& m, hipStream_t st);
#define BLSW_VLINE_ROWS (6u * 68u)  // vpairing.hpp: per G2 point, 68 steps x (c0, c1 x_P, c2 y_P), two Fp each
// blsw_verify_batch: projective lines of (sig, H(m)) then the six-lane value-only pairing check (k_team.hip, vpairing.hpp)
void launch_verify_values(uint64_t n, const Workspace& ws, const uint64_t* pk_xy, const uint64_t* sig_xy, Fp* lines_sig, Fp* lines_h, const int32_t* status, int32_t* result,
                          hipStream_t st);
// blsw_verify_groups_batch: scale, group sums, one line chain per instance and per group, chunked fold, one final exponentiation per group
// (k_vgroups.hip, vgroups.hpp). `chunk` <= 31 pairs per team.
void launch_verify_groups(uint64_t n, uint32_t group, uint32_t chunk, const Workspace& ws, const uint64_t* pk_xy, const uint64_t* sig_xy, const int32_t* status, const uint64_t* scalars,
                          Fp* p_scaled, Fp* s_scaled, Fp* sum_xy, int32_t* gflag, Fp* lines_h, Fp* lines_g, Fp* partials, int32_t* result, hipStream_t st);
// blsw_verify_groups_shared_batch: the same over a message table (k_vgroups.hip, vshared.hpp). msg_index [n] names each instance's row of the table
// that ws hashed (n_msgs rows); an index beyond it becomes DEC_BAD_COUNT in status[i][0]. Instances of a group with equal adjacent indices form a
// run: one key sum (rsum [3][n], rflag [n], by compact slot), one line chain and one pair of the fold. slot_leader, slot_len [n], runs [n_groups];
// runs_out (nullable) receives the groups' run counts.
void launch_verify_groups_shared(uint64_t n, uint32_t group, uint32_t chunk, const Workspace& ws, uint64_t n_msgs, const uint32_t* msg_index, const uint64_t* pk_xy,
                                 const uint64_t* sig_xy, int32_t* status, const uint64_t* scalars, Fp* p_scaled, Fp* s_scaled, Fp* sum_xy, int32_t* gflag, Fp* lines_h, Fp* lines_g,
                                 Fp* partials, uint32_t* slot_leader, uint32_t* slot_len, uint32_t* runs, Fp* rsum, int32_t* rflag, uint32_t* runs_out, int32_t* result,
                                 hipStream_t st);
// blsw_verify_pairs_batch: decode of n * n_pairs keys and n signatures, the instances' statuses, one line chain per used pair and per signature,
// chunked fold, one final exponentiation per instance (k_vpairs.hip, vpairs.hpp). `chunk` <= 31 pairs per team; ws holds the hash of the n * n_pairs messages.
void launch_verify_pairs(uint64_t n, uint32_t n_pairs, uint32_t chunk, const Workspace& ws, const uint8_t* pks48, const uint8_t* sig96, const uint32_t* counts, Fp* key_xy,
                         uint64_t* sig_xy, int32_t* key_status, int32_t* status, Fp* lines_h, Fp* lines_s, Fp* partials, int32_t* result, hipStream_t st);
// blsw_committee_verify_batch (k_committee.hip, committee.hpp): the committee's keys into `table` [2][n_keys] and key_status together with the n
// signatures; then per instance the sum of the keys its bitmap row selects -> pk_xy [n][12], status[i][0], count / agg48 (nullable)
void launch_committee_decode(const uint8_t* pks48, uint32_t n_keys, const uint8_t* sig96, uint64_t n, Fp* table, int32_t* key_status, uint64_t* sig_xy, int32_t* status,
                             hipStream_t st);
void launch_committee_sum(const uint8_t* bitmap, uint32_t n_keys, uint64_t n, const Fp* table, const int32_t* key_status, uint64_t* pk_xy, int32_t* status, uint32_t* count,
                          uint8_t* agg48, hipStream_t st);
// blsw_registry_* (k_registry.hip, registry.hpp): keys [first, first + count) decoded into the handle's 128-byte records and its status array; then
// per set the sum of the records its index list names, checked against `size` -> pk_xy [n][12], status[i][0], agg48 (nullable)
void launch_registry_append(const uint8_t* pks48, uint32_t first, uint32_t count, void* records, int32_t* key_status, hipStream_t st);
void launch_registry_sum(const void* records, uint32_t size, const uint32_t* indices, uint64_t n_indices, const uint64_t* offsets, uint64_t n, uint64_t* pk_xy, int32_t* status,
                         uint8_t* agg48, hipStream_t st);
// blsw_combine_points_batch / blsw_recover_points_batch (k_combine.hip, vcombine.hpp): n lists of k (point, scalar) terms, m = n k
struct CombineArgs {
    uint32_t group, k;
    uint64_t n;
    const uint32_t* counts;  // [n], nullable: every list uses all k
    const Fp* xy;            // [m][2 | 4] decoded points (k_decode_points)
    const int32_t* pst;      // [m] their decode statuses
    const uint8_t* scalars;  // [m][32] little-endian
    const int32_t* lag;      // [n] the lists' statuses from launch_lagrange (recover), or nullptr
    Fp* scaled;              // G1: [3][m] Jacobian; G2: [16 * 6][m], slot 0 the scaled point, slots 1..15 the ladder's table
    int32_t* term_status;    // [m][2], nullable
    uint8_t* out;            // [n][48 | 96]
    int32_t* status;         // [n]
};
// decode of `in`, the lists' statuses, scale, sum
void launch_combine(const CombineArgs& a, const uint8_t* in, hipStream_t st);
// coeff [n][k][32] little-endian Lagrange coefficients at 0 of the ids, status [n]
void launch_lagrange(const uint8_t* ids, const uint32_t* counts, uint32_t k, uint64_t n, uint8_t* coeff, int32_t* status, hipStream_t st);
// blsw_msm_points_batch (k_msm.hip, vmsm.hpp): the same n lists of k terms by the bucket method, c = window bits, W windows, B = 2^c buckets,
// S segments per window; point rows are element-major (row * lanes + lane)
struct MsmArgs {
    uint32_t group, k, c;
    uint64_t n;
    const uint32_t* counts;  // [n], nullable
    const Fp* xy;            // [m][2 | 4] decoded points (k_decode_points)
    const int32_t* pst;      // [m] their decode statuses
    const uint8_t* scalars;  // [m][32] little-endian
    uint32_t* hist;          // [n][W][B] counts, then their exclusive prefix per (list, window)
    uint32_t* cursor;        // [n][W][B] the scatter's cursor: a bucket's end once the scatter has run
    uint32_t* sorted;        // [W][m] term indices in bucket order, list i's at [w][i k ..)
    Fp* buckets;             // [3 | 6][n W B] Jacobian bucket sums
    Fp* segments;            // [3 | 6][n W S]
    Fp* windows;             // [3 | 6][n W]
    uint8_t* out;            // [n][48 | 96]
    int32_t* status;         // [n]
    // the registry form (blsw_registry_msm_batch; group 1, k unused): list i = indices[offsets[i] .. offsets[i + 1]), sorted is [W][n_indices] and
    // holds positions relative to the list's first
    const uint64_t* offsets;  // [n + 1]
    const uint32_t* indices;  // [n_indices]
    uint64_t n_indices;
    const void* records;      // the registry's 128-byte records
    uint32_t size;            // the registry's size as of the call
    uint32_t* claims;         // [n_indices] OK lists that hold the position
    uint32_t* owner;          // [n_indices] the list that holds it, where there is one
    int32_t* serial;          // [n] 1: the list shares a position and is summed by its own lane
};
// decode of `in`, the lists' statuses, histogram, scan, scatter, bucket sums, window reduction, final sum
void launch_msm(const MsmArgs& a, const uint8_t* in, hipStream_t st);
// the same over registry records: the lists' statuses and claims, then the stages from the histogram on
void launch_msm_registry(const MsmArgs& a, hipStream_t st);

}  // namespace blsw

// blsw_keyset_t (include/blsw.h, ABI 15): engine.hip creates it; the compact checker of a shared-keys step (k_r1cs.hip) reads its table as the head of z
struct blsw_keyset {
    uint32_t n_keys = 0, form = 0;
    int device = -1;
    blsw::Fp* table = nullptr;  // [n_keys * SEG_PK_ALLOC] in `form`
    blsw::Fp* proj = nullptr;   // [3][n_keys] Montgomery
};
