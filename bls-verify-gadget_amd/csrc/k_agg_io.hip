// libblsw.so, one translation unit per kernel family (see kcommon.hpp, build.py).
// Not a chain unit: one compilation, its programs out of line.
#include "kcommon.hpp"
#include "agg_input.hpp"

namespace blsw {

struct LdFpGlobalIo {
    __device__ __forceinline__ Fp operator()(const Fp* p) const { return ld_fp(p); }
};
// aggregate_verify with public inputs (blsw_engine_submit_aggregate_io): the head of every instance's instance_assignment — the constant one, the
// Input keys' x, y, z and the Input bitmap bits, n_elems = agg_instance_head(L) elements (1 when neither is Input). One lane per ELEMENT:
// blockIdx.y = instance of the step, s0 + blockIdx.z = step, so a wave stores 64 consecutive 48-byte elements (3 KB contiguous); one lane per instance
// would put its lanes n_instance_vars * 48 bytes apart (98 KB at 512 keys). No LDS: a key's (x, y) is read by the three lanes that write its
// x, y, z (cache hits), every output byte is written once. The message's and the signature's elements are written by the kernels that have
// them at hand (k_msg_input, the signature's prepare chain). Steps submitted without an instance tensor are skipped.
__global__ __launch_bounds__(256) void k_agg_instance(Group g, uint32_t n_elems, uint32_t s0) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y, s = s0 + blockIdx.z;
    if (e >= n_elems || i >= g.n) return;
    const StepDesc& d = g.desc[s];
    if (!d.inst) return;
    const uint32_t nk = g.L.n_keys;
    const Fp v = agg_instance_element(g.L, reinterpret_cast<const Fp*>(d.keys + (uint64_t)i * nk * 12), d.bitmap + (uint64_t)i * nk, e, LdFpGlobalIo());
    st_fp(reinterpret_cast<Fp*>(d.inst) + ((uint64_t)i * g.L.n_instance_vars + e), g.canonical ? fp_to_canonical(v) : v);
}

}  // namespace blsw
