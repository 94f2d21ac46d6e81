// libblsw.so, one translation unit per kernel family (see kcommon.hpp, build.py).
// Not a chain unit: one compilation, its programs out of line.
#include "kcommon.hpp"
#include "multi_input.hpp"

namespace blsw {

// UInt8::new_input_vec(msg) (options.msg_mode 1; constraints.rs:341 with AllocationMode::Input): one lane per (instance, pair) — one per instance
// outside the N+1-pair product — writes its message's inputs (instance_assignment[1 + j c .. 1 + (j + 1) c) for pair j: multi_input.hpp; in an
// aggregate_verify circuit they follow the keys' and the bitmap's inputs: agg_inst_msg_base) and its message segment; k_sha then allocates no
// message booleans (Group::msg_wit_len = 0)
__global__ __launch_bounds__(64) void k_msg_input(Group g) {
    const uint64_t I = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= g.N) return;
    const LaneId id = lane_id(g, I);
    const uint8_t* msg = g.desc[id.s].msg + (uint64_t)id.f * g.msg_len;
    const Emitter e = EMITJ(g, id, off_msg, stride_msg);
    if (g.L.n_keys) {
        const uint32_t k0 = agg_inst_msg_base(g.L);
        chain_msg_input(e, msg, g.msg_len, [&](uint32_t t, const Fp& v) { put_instance(g, id, k0 + t, v); });
    } else {
        multi_msg_input(g.L, id.j, e, msg, [&](uint32_t k, const Fp& v) { put_instance(g, id, k, v); });
    }
}

}  // namespace blsw
