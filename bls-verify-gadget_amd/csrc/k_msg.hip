// libblsw.so, one translation unit per kernel family (see kcommon.hpp, build.py).
// Not a chain unit: one compilation, its programs out of line.
#include "kcommon.hpp"
#include "msg_input.hpp"

namespace blsw {

// UInt8::new_input_vec(msg) (options.msg_mode 1; constraints.rs:341 with AllocationMode::Input): one lane per instance writes its message
// inputs (instance_assignment[1 .. c]; in an aggregate_verify circuit they follow the keys' and the bitmap's inputs: agg_inst_msg_base) and the
// message segment; k_sha then allocates no message booleans (Group::msg_wit_len = 0)
__global__ __launch_bounds__(64) void k_msg_input(Group g) {
    const uint64_t I = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= g.N) return;
    const LaneId id = lane_id(g, I);
    const uint8_t* msg = g.desc[id.s].msg + (uint64_t)id.f * g.msg_len;
    const uint32_t k0 = g.L.n_keys ? agg_inst_msg_base(g.L) : 1u;
    chain_msg_input(EMIT(g, id, off_msg), msg, g.msg_len, [&](uint32_t j, const Fp& v) { put_instance(g, id, k0 + j, v); });
}

}  // namespace blsw
