// TEST HARNESS ONLY (never linked into libblsw.so): the operation table of ops.hpp on the device, one kernel per operation. Compiled three times
// into libdevfield.so, as the library compiles its chain units (csrc/kcommon.hpp):
//   plain                    programs out of line (BLSW_FN is noinline), entries devfield_run
//   -DDEVFIELD_VARIANT_INL   BLSW_INLINE_CHAINS, entries devfield_run_inl
//   -DDEVFIELD_VARIANT_QUAD  BLSW_QUAD and BLSW_INLINE_CHAINS, four lanes per item, entries devfield_run_q
// Every lane writes its results to its own slot (the four lanes of a quad must agree); witnesses go to the item's buffer through an Emitter.
#include <hip/hip_runtime.h>
#include <stdint.h>
#if defined(DEVFIELD_VARIANT_QUAD)
#define BLSW_QUAD 1
#define BLSW_INLINE_CHAINS 1
#define DEVFIELD_K(name) name##_q
#define DEVFIELD_LPI 4u  // lanes per item
#elif defined(DEVFIELD_VARIANT_INL)
#define BLSW_INLINE_CHAINS 1
#define DEVFIELD_K(name) name##_inl
#define DEVFIELD_LPI 1u
#else
#define DEVFIELD_K(name) name
#define DEVFIELD_LPI 1u
#endif
#include "ops.hpp"

using namespace devfield;

// a, b: [n][12] elements; out: [n * LPI][12]; wit: [n][wcap]; npos: [n * LPI] the lane's cursor after the operation
template <int OP>
__global__ __launch_bounds__(64) void DEVFIELD_K(k_devfield)(uint64_t n, const Fp* a, const Fp* b, Fp* out, uint32_t* wit, uint32_t wcap, uint32_t* npos) {
    const uint64_t lane = (uint64_t)blockIdx.x * 64 + threadIdx.x, item = lane / DEVFIELD_LPI;
    if (item >= n) return;  // whole quads leave together
    Emitter e = {wit + item * (uint64_t)wcap * 12, 0};
    FieldOp<OP>::run(a + item * 12, b + item * 12, out + lane * DEVFIELD_OUT_MAX, e);
    npos[lane] = e.pos;
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
uint32_t DEVFIELD_K(devfield_lpi)() { return DEVFIELD_LPI; }
// Runs operation `op` on n items. Host arrays: a, b [n][12][6] u64; out [n * LPI][12][6]; wit [n][wcap][6], copied to the device first (the
// caller's sentinel) and back; npos [n * LPI]. Returns 0, a HIP error code (the launch's, then the synchronisation's), -1 for an unknown
// operation, -2 when wcap is below the operation's witness count or n is 0.
int DEVFIELD_K(devfield_run)(int op, uint64_t n, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t* wit, uint32_t wcap, uint32_t* npos) {
    if (op < 0 || op >= OP_COUNT) return -1;
    if (n == 0 || n > (1u << 20) || (int64_t)wcap < op_n_wit(op) || wcap == 0) return -2;
    const size_t in_bytes = n * 12 * sizeof(Fp), out_bytes = n * DEVFIELD_LPI * DEVFIELD_OUT_MAX * sizeof(Fp), wit_bytes = n * (size_t)wcap * sizeof(Fp),
                 pos_bytes = n * DEVFIELD_LPI * sizeof(uint32_t);
    DevBuf da, db, dout, dwit, dpos;
    hipError_t rc;
#define DEVFIELD_TRY(x) \
    if ((rc = (x)) != hipSuccess) return (int)rc
    DEVFIELD_TRY(hipMalloc(&da.p, in_bytes));
    DEVFIELD_TRY(hipMalloc(&db.p, in_bytes));
    DEVFIELD_TRY(hipMalloc(&dout.p, out_bytes));
    DEVFIELD_TRY(hipMalloc(&dwit.p, wit_bytes));
    DEVFIELD_TRY(hipMalloc(&dpos.p, pos_bytes));
    DEVFIELD_TRY(hipMemcpy(da.p, a, in_bytes, hipMemcpyHostToDevice));
    DEVFIELD_TRY(hipMemcpy(db.p, b, in_bytes, hipMemcpyHostToDevice));
    DEVFIELD_TRY(hipMemcpy(dout.p, out, out_bytes, hipMemcpyHostToDevice));
    DEVFIELD_TRY(hipMemcpy(dwit.p, wit, wit_bytes, hipMemcpyHostToDevice));
    DEVFIELD_TRY(hipMemcpy(dpos.p, npos, pos_bytes, hipMemcpyHostToDevice));
    const unsigned grid = (unsigned)((n * DEVFIELD_LPI + 63) / 64);
    switch (op) {
#define DEVFIELD_X_LAUNCH(name, n_out, n_wit)                                                                                                    \
    case OP_##name:                                                                                                                              \
        DEVFIELD_K(k_devfield)<OP_##name><<<grid, 64>>>(n, (const Fp*)da.p, (const Fp*)db.p, (Fp*)dout.p, (uint32_t*)dwit.p, wcap, (uint32_t*)dpos.p); \
        break;
        DEVFIELD_OPS(DEVFIELD_X_LAUNCH)
#undef DEVFIELD_X_LAUNCH
    }
    DEVFIELD_TRY(hipGetLastError());
    DEVFIELD_TRY(hipDeviceSynchronize());
    DEVFIELD_TRY(hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost));
    DEVFIELD_TRY(hipMemcpy(wit, dwit.p, wit_bytes, hipMemcpyDeviceToHost));
    DEVFIELD_TRY(hipMemcpy(npos, dpos.p, pos_bytes, hipMemcpyDeviceToHost));
#undef DEVFIELD_TRY
    return 0;
}
}
