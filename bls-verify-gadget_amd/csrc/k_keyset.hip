// libblsw.so, one translation unit per kernel family (see kcommon.hpp, build.py).
// Shared key sets (blsw_keyset_t): the allocation chain of a set's keys, once, and the broadcast of its table into the heads of a step's vectors.
// One compilation: the chain inlined with the whole register file, as a direct-mode unit (K = 512 keys are eight waves, once per set: latency-bound).
#define BLSW_KVARIANT_INL
#include "kcommon.hpp"

namespace blsw {

// lane k allocates key k: chain_g1_alloc_only — the chain k_agg_keys runs per (instance, key) — with its cursor on the key's SEG_PK_ALLOC elements of the
// dense table (element stride 12 u32, as a direct-mode vector), and the allocated point to proj [3][K]
__global__ __launch_bounds__(64) void k_keyset_alloc(const uint64_t* __restrict__ pks_xy, uint32_t n_keys, Fp* table, Fp* proj) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_keys) return;
    const Fp* p = reinterpret_cast<const Fp*>(pks_xy + (uint64_t)k * 12);
    Emitter e;
    e.base = reinterpret_cast<uint32_t*>(table + (uint64_t)k * SEG_PK_ALLOC);
    e.pos = 0;
    e.stride = 12;
    const Proj<OpsFp> r = chain_g1_alloc_only(e, ld_fp(p), ld_fp(p + 1));
    st_fp(proj + k, r.x);
    st_fp(proj + n_keys + k, r.y);
    st_fp(proj + 2 * (uint64_t)n_keys + k, r.z);
}
void launch_keyset_alloc(const uint64_t* pks_xy, uint32_t n_keys, Fp* table, Fp* proj, hipStream_t st) {
    hipLaunchKernelGGL(k_keyset_alloc, dim3((n_keys + 63) / 64), dim3(64), 0, st, pks_xy, n_keys, table, proj);
}

// The table (n_pieces 16-byte pieces, 256-byte aligned) -> pieces [0, n_pieces) of each of n_inst vectors `stride` elements apart (a vector starts at a
// multiple of 16 bytes). A workgroup copies ONE chunk of 256 x BLSW_BCAST_ITERS pieces (32 KiB: the block k_place_field writes) into ONE vector:
// all its loads first, then its stores back to back; every wave-instruction moves 1 KiB contiguous, no LDS, plain stores. The table is read n_inst
// times and written n_inst times: the reads are meant to hit a cache, so which workgroups run together decides what the kernel costs beside its
// HBM writes. ORDER 0 (k_place_field's XCD-aware order: workgroups go round-robin to the 8 XCDs, each with its own L2): the instances of one chunk run
// back to back on ONE XCD — linear id L -> xcd = L % 8, chunk = xcd + 8 * ((L / 8) / n_inst), instance = (L / 8) % n_inst. ORDER 1: consecutive
// workgroups walk the chunks of one instance (each chunk then comes from the Infinity Cache once per instance and XCD).
#define BLSW_BCAST_ITERS 8
template <int ORDER>
__global__ __launch_bounds__(256) void k_keys_broadcast(const uint4* __restrict__ table, uint32_t n_pieces, uint32_t n_chunks8, uint64_t* __restrict__ d_witness, uint64_t stride,
                                                        uint32_t n_inst) {
    uint32_t chunk, inst;
    if (ORDER == 0) {
        const uint32_t s_in_xcd = blockIdx.x >> 3;
        chunk = (blockIdx.x & 7) + 8 * (s_in_xcd / n_inst);
        inst = s_in_xcd % n_inst;
    } else {
        inst = blockIdx.x / n_chunks8;
        chunk = blockIdx.x - inst * n_chunks8;
    }
    const uint32_t q0 = chunk * (256u * BLSW_BCAST_ITERS);  // < 2^32: n_pieces = n_keys * 5826 with n_keys <= 65535, plus at most 8 chunks
    if (q0 >= n_pieces || inst >= n_inst) return;
    uint4* out = reinterpret_cast<uint4*>(d_witness + (uint64_t)inst * stride * 6);
    const uint32_t q = q0 + threadIdx.x;
    if (q0 + 256u * BLSW_BCAST_ITERS <= n_pieces) {  // whole chunk in range: no bounds checks, no wait between a store and the next load
        uint4 v[BLSW_BCAST_ITERS];
#pragma unroll
        for (int k = 0; k < BLSW_BCAST_ITERS; k++) v[k] = table[q + k * 256];
#pragma unroll
        for (int k = 0; k < BLSW_BCAST_ITERS; k++) out[q + k * 256] = v[k];
        return;
    }
#pragma unroll 1
    for (int k = 0; k < BLSW_BCAST_ITERS; k++)
        if (q + k * 256 < n_pieces) out[q + k * 256] = table[q + k * 256];
}
void launch_keys_broadcast(const uint64_t* table, uint64_t n_elements, uint64_t* d_witness, uint64_t stride, uint64_t n, uint32_t order, hipStream_t st) {
    const uint32_t n_pieces = (uint32_t)(n_elements * 3);
    const uint32_t per = 256u * BLSW_BCAST_ITERS;
    const uint32_t n_chunks8 = 8 * (((n_pieces + per - 1) / per + 7) / 8);
    // one launch per slice of instances whose grid stays below 2^31 workgroups (512 keys: 1 464 workgroups per instance)
    const uint64_t slice = 0x7fffffffull / n_chunks8;
    for (uint64_t first = 0; first < n; first += slice) {
        const uint32_t cnt = (uint32_t)(n - first < slice ? n - first : slice);
        uint64_t* out = d_witness + first * stride * 6;
        if (order == 0)
            hipLaunchKernelGGL(k_keys_broadcast<0>, dim3(n_chunks8 * cnt), dim3(256), 0, st, reinterpret_cast<const uint4*>(table), n_pieces, n_chunks8, out, stride, cnt);
        else
            hipLaunchKernelGGL(k_keys_broadcast<1>, dim3(n_chunks8 * cnt), dim3(256), 0, st, reinterpret_cast<const uint4*>(table), n_pieces, n_chunks8, out, stride, cnt);
    }
}

}  // namespace blsw
