// UInt8::new_input_vec (ark-r1cs-std 0.4.0) — the message as public inputs. ToConstraintField<Fq> for [u8] (ark-ff 0.4) cuts the message into
// chunks of MSG_CHUNK_BYTES = (MODULUS_BIT_SIZE - 1) / 8 = 47 bytes (the last one may be shorter); chunk j, read as a little-endian integer
// (< 2^376 < p), is instance variable 1 + j (AllocatedFp::new_input), and AllocatedFp::to_bits_le on it allocates the chunk's segment of the
// witness vector: 381 booleans LSB first, then the AND witnesses of enforce_in_field_le (SEG_MSG_CHUNK in all). Byte k of the message is
// UInt8::from_bits_le of bits [8 k, 8 k + 8) of the chunks' low 376 bits concatenated: no allocation. Shared by the device kernel (k_msg.hip)
// and the host test harness.
#pragma once
#include "gadgets.hpp"
#include "layout.h"

namespace blsw {

// chunk j of the message as a field element, Montgomery form
BLSW_HD Fp msg_chunk_value(const uint8_t* msg, uint32_t msg_len, uint32_t j) {
    const uint32_t b0 = j * MSG_CHUNK_BYTES;
    const uint32_t nb = msg_len - b0 < MSG_CHUNK_BYTES ? msg_len - b0 : (uint32_t)MSG_CHUNK_BYTES;
    Fp a = fp_zero();
#pragma unroll
    for (uint32_t k = 0; k < MSG_CHUNK_BYTES; k++)
        if (k < nb) a.l[k >> 2] |= (uint32_t)msg[b0 + k] << (8 * (k & 3));
    constexpr uint32_t R2[12] = BLSW_R2_LIMBS;
    return fp_mul(a, fp_from_limbs(R2));  // a * R mod p
}
// the message segment of one instance (msg_input_chunks(msg_len) chunks of SEG_MSG_CHUNK witnesses); put(j, v): instance variable 1 + j := v
template <class PutInput>
BLSW_HD void chain_msg_input(Emitter e, const uint8_t* msg, uint32_t msg_len, const PutInput& put) {
    const uint32_t c = msg_input_chunks(msg_len);
#pragma unroll 1
    for (uint32_t j = 0; j < c; j++) {
        const Fp v = msg_chunk_value(msg, msg_len, j);
        put(j, v);
        fp_to_bits_le_w(e, v);
    }
}

}  // namespace blsw
