// libblsw.so, one translation unit per kernel family (see kcommon.hpp, build.py).
// A chain unit: its compilations and the register policy of its grouped compilation are its entry in build.py's CHAIN_UNITS.
#include "kcommon.hpp"
#include "agg_input.hpp"
#include "multi_input.hpp"

namespace blsw {

// Lanes [0, N): the public key of a (pk, msg) pair. ParametersVar allocated as witnesses (L.params_mode, single-key circuit: constraints.rs:198-211
// with AllocationMode::Witness): lanes [N, 2 N) run the same chain on the generator of instance I - N — G1Var::new_variable, then g1.negate()
// (linear) and prepare_g1(&g1_neg) = to_affine; no enforce_not_equal on it (constraints.rs:97-99 is about the public key only).
__global__ __launch_bounds__(64) BLSW_CHAIN_ATTR void BLSW_K(k_g1)(Group g) {
    if (g.chain_prio) __builtin_amdgcn_s_setprio(3);  // latency-critical chain: win VALU issue arbitration against the streaming placement waves
    uint64_t I = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool params = g.L.params_mode && I >= g.N;
    if (params) I -= g.N;
    if (I >= g.N) return;
    LaneId id = lane_id(g, I);
    const Fp* p = reinterpret_cast<const Fp*>(g.desc[id.s].pk + (uint64_t)id.f * 12);
    Emitter e_alloc = EMITJ(g, id, off_pk_alloc, stride_pk_alloc), e_nz = EMITJ(g, id, off_pk_not_zero, stride_pk_not_zero),
            e_prep = EMITJ(g, id, off_prep_pk, stride_prep_pk);
    Fp x = ld_fp(p), y = ld_fp(p + 1);
    if (params) {
        e_alloc = EMIT(g, id, off_params_alloc);
        e_prep = EMIT(g, id, off_prep_g1);
        e_nz.base = nullptr;
        x = K_G1_GEN_X();
        y = fp_neg(K_G1_GEN_NEG_Y());
    }
    Proj<OpsFp> pk;
    if (g.L.pk_mode && !params) {
        // PublicKeyVar::new_variable(Input) (constraints.rs:214-232) = new_variable_omit_prime_order_check: x, y, z are public inputs (after the
        // messages', before the signature's; pair j's own three in the N+1-pair product: multi_input.hpp), no witnesses, no in-circuit prime-order
        // check: a pair lane then runs only chain_g1_post
        pk = multi_key_input(g.L, id.j, x, y, [&](uint32_t k, const Fp& v) { put_instance(g, id, k, v); });
    } else {
        pk = chain_g1_alloc_only(e_alloc, x, y);
    }
    if (!params && id.j == 0) put_instance(g, id, 0, fp_one());  // instance_assignment[0], once per instance
    if (params) pk.y = fp_neg(pk.y);
    G1ChainOut o = chain_g1_post(e_nz, e_prep, pk);
    if (params) return;  // its affine form is the constant the pairing kernel uses
    st_fp(g.ws.pkaff + I, o.ax);
    st_fp(g.ws.pkaff + g.N + I, o.ay);
}

// aggregate_verify: lane t = k * N + I allocates key k of instance I (N * n_keys lanes), result to ws.keyproj
__global__ __launch_bounds__(64) BLSW_CHAIN_ATTR void BLSW_K(k_agg_keys)(Group g, Fp* keyproj) {
    if (g.chain_prio) __builtin_amdgcn_s_setprio(3);
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t N = g.N, nk = g.L.n_keys;
    if (t >= N * nk) return;
    uint32_t k = (uint32_t)(t / N);
    LaneId id = lane_id(g, t - (uint64_t)k * N);
    const Fp* p = reinterpret_cast<const Fp*>(g.desc[id.s].keys + ((uint64_t)id.i * nk + k) * 12);
    Proj<OpsFp> r = chain_g1_alloc_only(emitter(g, id, g.L.off_keys + k * SEG_PK_ALLOC, g.LS.off_keys + k * SEG_PK_ALLOC, false), ld_fp(p), ld_fp(p + 1));
    Fp* o = keyproj + t;
    st_fp(o, r.x);
    st_fp(o + N * nk, r.y);
    st_fp(o + 2 * N * nk, r.z);
}
struct KeyProjSrc {
    const Fp* p;  // keyproj + I
    uint64_t N, total;
    __device__ __forceinline__ Proj<OpsFp> ld(uint32_t k) const {
        const Fp* q = p + (uint64_t)k * N;
        return {ld_fp(q), ld_fp(q + total), ld_fp(q + 2 * total)};
    }
};
// aggregate_verify: bitmap booleans (Boolean::new_witness per key, constraints.rs:414-419; none when the bits are public inputs: the bitmap
// segment is then empty, L.off_msg == L.off_bitmap), mapped_aggregate, then pk != 0 and prepare_g1 on the aggregated key
template <class K>
__device__ __forceinline__ void agg_sum_lane(const Group& g, const LaneId& id, uint64_t I, const K& src, const uint8_t* bm) {
    const uint32_t nk = g.L.n_keys, n_bits = g.L.off_msg - g.L.off_bitmap;
    Emitter eb = EMIT(g, id, off_bitmap);
    for (uint32_t k = 0; k < n_bits; k++) eb.put_bool(bm[k] != 0);
    uint32_t count = 0;
    Proj<OpsFp> pk = chain_mapped_aggregate(EMIT(g, id, off_count), EMIT(g, id, off_agg), src, bm, nk, &count);
    G1ChainOut o = chain_g1_post(EMIT(g, id, off_pk_not_zero), EMIT(g, id, off_prep_pk), pk);
    st_fp(g.ws.pkaff + I, o.ax);
    st_fp(g.ws.pkaff + g.N + I, o.ay);
    uint32_t* c = g.desc[id.s].count;
    if (c) c[id.i] = count;
}
__global__ __launch_bounds__(64) BLSW_CHAIN_ATTR void BLSW_K(k_agg_sum)(Group g, const Fp* keyproj) {
    if (g.chain_prio) __builtin_amdgcn_s_setprio(3);
    uint64_t I = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= g.N) return;
    LaneId id = lane_id(g, I);
    const uint32_t nk = g.L.n_keys;
    KeyProjSrc src = {keyproj + I, g.N, g.N * nk};
    agg_sum_lane(g, id, I, src, g.desc[id.s].bitmap + (uint64_t)id.i * nk);
}
// the same with the keys as public inputs (L.pk_mode; agg_input.hpp): the affine keys of the step's inputs are the operands, k_agg_keys has not run
struct LdFpGlobal {
    __device__ __forceinline__ Fp operator()(const Fp* p) const { return ld_fp(p); }
};
__global__ __launch_bounds__(64) BLSW_CHAIN_ATTR void BLSW_K(k_agg_sum_in)(Group g) {
    if (g.chain_prio) __builtin_amdgcn_s_setprio(3);
    uint64_t I = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= g.N) return;
    LaneId id = lane_id(g, I);
    const uint32_t nk = g.L.n_keys;
    KeyInputSrc<LdFpGlobal> src = {reinterpret_cast<const Fp*>(g.desc[id.s].keys + (uint64_t)id.i * nk * 12), LdFpGlobal()};
    agg_sum_lane(g, id, I, src, g.desc[id.s].bitmap + (uint64_t)id.i * nk);
}
// the same with the keys of the step's shared key set (options.shared_keys): K allocated projective points [3][K], the same for every lane of the
// step — the address is wave-uniform wherever a wave lies within one step, and nothing of the keys is written by this engine
struct KeySetSrc {
    const Fp* p;
    uint32_t K;
    __device__ __forceinline__ Proj<OpsFp> ld(uint32_t k) const { return {ld_fp(p + k), ld_fp(p + K + k), ld_fp(p + 2 * (uint64_t)K + k)}; }
};
__global__ __launch_bounds__(64) BLSW_CHAIN_ATTR void BLSW_K(k_agg_sum_ks)(Group g) {
    if (g.chain_prio) __builtin_amdgcn_s_setprio(3);
    uint64_t I = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= g.N) return;
    LaneId id = lane_id(g, I);
    const uint32_t nk = g.L.n_keys;
    KeySetSrc src = {g.desc[id.s].ks_proj, nk};
    agg_sum_lane(g, id, I, src, g.desc[id.s].bitmap + (uint64_t)id.i * nk);
}

}  // namespace blsw
