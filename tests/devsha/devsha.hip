// TEST HARNESS ONLY (never linked into libblsw.so): the SHA gadget operation table of ops.hpp on the device, one kernel per entry. Compiled once
// per compilation csrc/k_sha.hip gets in build.py's CHAIN_UNITS, through csrc/kcommon.hpp's own switches:
//   -DBLSW_CHAIN_W2       the grouped engine's k_sha: programs inlined, two waves per SIMD; entries devsha_run
//   -DBLSW_KVARIANT_INL   the direct mode's k_sha_inl: programs inlined, the whole register file; entries devsha_run_inl
// A workgroup is one tile of 64 lanes, as in k_sha: the sink's [16][64] word buffer in LDS, a lane's column at lds + threadIdx.x, its first 64-byte
// run at tile * bits_tile_words(sha_words) + lane * 16 words.
#include "kcommon.hpp"
#include "ops.hpp"

using namespace devsha;

template <int OP>
__global__ __launch_bounds__(64) BLSW_CHAIN_ATTR void BLSW_K(k_devsha)(uint64_t n, const uint32_t* in, const uint8_t* msg, uint32_t msg_len, uint32_t* out, uint32_t* bits,
                                                                      uint64_t sha_words, uint32_t* nwords) {
    __shared__ uint32_t sink_lds[BLSW_BITS_CHUNK_WORDS * 64];
    const uint64_t I = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= n) return;
    BitSink s;
    s.init_device(sink_lds + threadIdx.x, reinterpret_cast<uint4*>(bits + (I >> 6) * bits_tile_words(sha_words) + (I & 63) * BLSW_BITS_CHUNK_WORDS));
    ShaOp<OP>::run(in + I * DEVSHA_IN_MAX, msg + I * (uint64_t)msg_len, msg_len, out + I * DEVSHA_OUT_MAX, s);
    if (!op_flushes(OP)) s.flush();
    nwords[I] = s.widx;
}

namespace {
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};
}  // namespace

extern "C" {
// Runs entry `op` on n items. Host arrays: in [n][DEVSHA_IN_MAX] u32; msg [n][msg_len] bytes; out [n][DEVSHA_OUT_MAX] u32 and nwords [n] u32, copied
// to the device first (the caller's sentinel) and back; bits [bits_total] u32, copied likewise, with tile 0 at word bits_origin: guards on both
// sides, and sha_words (a multiple of 16) words per lane inside. Returns 0, a HIP error code, -1 for an unknown entry, -2 for arguments that cannot
// be launched (n 0 or above 2^16, a tile region that does not fit the buffer).
int BLSW_K(devsha_run)(int op, uint64_t n, const uint32_t* in, const uint8_t* msg, uint32_t msg_len, uint32_t* out, uint32_t* bits, uint64_t bits_total, uint64_t bits_origin,
                       uint64_t sha_words, uint32_t* nwords) {
    if (op < 0 || op >= OP_COUNT) return -1;
    const uint64_t tiles = (n + 63) / 64;
    if (n == 0 || n > (1u << 16) || sha_words == 0 || sha_words % BLSW_BITS_CHUNK_WORDS || bits_origin % 4 ||
        bits_origin + tiles * bits_tile_words(sha_words) > bits_total)
        return -2;
    const size_t in_bytes = n * DEVSHA_IN_MAX * 4, msg_bytes = n * (size_t)msg_len + 16, out_bytes = n * DEVSHA_OUT_MAX * 4, bits_bytes = bits_total * 4, nw_bytes = n * 4;
    DevBuf din, dmsg, dout, dbits, dnw;
    hipError_t rc;
#define DEVSHA_TRY(x) \
    if ((rc = (x)) != hipSuccess) return (int)rc
    (void)hipGetLastError();
    DEVSHA_TRY(hipMalloc(&din.p, in_bytes));
    DEVSHA_TRY(hipMalloc(&dmsg.p, msg_bytes));
    DEVSHA_TRY(hipMalloc(&dout.p, out_bytes));
    DEVSHA_TRY(hipMalloc(&dbits.p, bits_bytes));
    DEVSHA_TRY(hipMalloc(&dnw.p, nw_bytes));
    DEVSHA_TRY(hipMemcpy(din.p, in, in_bytes, hipMemcpyHostToDevice));
    DEVSHA_TRY(hipMemset(dmsg.p, 0, msg_bytes));
    if (msg_len) DEVSHA_TRY(hipMemcpy(dmsg.p, msg, n * (size_t)msg_len, hipMemcpyHostToDevice));
    DEVSHA_TRY(hipMemcpy(dout.p, out, out_bytes, hipMemcpyHostToDevice));
    DEVSHA_TRY(hipMemcpy(dbits.p, bits, bits_bytes, hipMemcpyHostToDevice));
    DEVSHA_TRY(hipMemcpy(dnw.p, nwords, nw_bytes, hipMemcpyHostToDevice));
    const unsigned grid = (unsigned)tiles;
    switch (op) {
#define DEVSHA_X_LAUNCH(name, n_in, n_out, m, fl)                                                                                                                    \
    case OP_##name:                                                                                                                                                 \
        BLSW_K(k_devsha)<OP_##name><<<grid, 64>>>(n, (const uint32_t*)din.p, (const uint8_t*)dmsg.p, msg_len, (uint32_t*)dout.p, (uint32_t*)dbits.p + bits_origin, sha_words, \
                                                 (uint32_t*)dnw.p);                                                                                                 \
        break;
        DEVSHA_OPS(DEVSHA_X_LAUNCH)
#undef DEVSHA_X_LAUNCH
    }
    DEVSHA_TRY(hipGetLastError());
    DEVSHA_TRY(hipDeviceSynchronize());
    DEVSHA_TRY(hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost));
    DEVSHA_TRY(hipMemcpy(bits, dbits.p, bits_bytes, hipMemcpyDeviceToHost));
    DEVSHA_TRY(hipMemcpy(nwords, dnw.p, nw_bytes, hipMemcpyDeviceToHost));
#undef DEVSHA_TRY
    return 0;
}
}
