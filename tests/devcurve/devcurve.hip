// TEST HARNESS ONLY (never linked into libblsw.so): the curve operation table of ops.hpp on the device, one kernel per operation. Compiled three
// times into libdevcurve.so, as the library compiles its chain units (csrc/kcommon.hpp, whose variant switches this file sets):
//   plain                    programs out of line (BLSW_FN is noinline), entries devcurve_run
//   -DDEVCURVE_VARIANT_INL   BLSW_KVARIANT_INL: BLSW_INLINE_CHAINS, entries devcurve_run_inl
//   -DDEVCURVE_VARIANT_QUAD  BLSW_KVARIANT_QUAD: BLSW_QUAD and BLSW_INLINE_CHAINS, four lanes per item, entries devcurve_run_q; only the entries the
//                            table marks for it (the others return -3)
// Every lane writes its results to its own slot (the four lanes of a quad must agree); witnesses go to the item's buffer through an Emitter. The
// PARK of v_clear_cofactor and v_g2_mul_gls is the library's ParkRows (csrc/values.hpp) over rows with the item count as their stride.
#include <hip/hip_runtime.h>
#include <stdint.h>
#if defined(DEVCURVE_VARIANT_QUAD)
#define BLSW_KVARIANT_QUAD 1
#define DEVCURVE_K(name) name##_q
#define DEVCURVE_IN_BUILD(quad) ((quad) != 0)
#elif defined(DEVCURVE_VARIANT_INL)
#define BLSW_KVARIANT_INL 1
#define DEVCURVE_K(name) name##_inl
#define DEVCURVE_IN_BUILD(quad) true
#else
#define DEVCURVE_K(name) name
#define DEVCURVE_IN_BUILD(quad) true
#endif
#include "values.hpp"
#include "ops.hpp"

using namespace devcurve;

// a, b: [n][12] elements; out: [n * LPI][12]; wit: [n][wcap]; npos: [n * LPI] the lane's cursor after the operation; park: [16 * 6][n] or null
template <int OP>
__global__ __launch_bounds__(64) void DEVCURVE_K(k_devcurve)(uint64_t n, const Fp* a, const Fp* b, Fp* out, uint32_t* wit, uint32_t wcap, uint32_t* npos, Fp* park) {
    const uint64_t lane = (uint64_t)blockIdx.x * 64 + threadIdx.x, item = lane / BLSW_LPI;
    if (item >= n) return;  // whole quads leave together
    Emitter e = {wit + item * (uint64_t)wcap * 12, 0};
    CurveOp<OP>::run(a + item * 12, b + item * 12, out + lane * DEVCURVE_OUT_MAX, e, ParkRows{park + item, n});
    npos[lane] = e.pos;
}

namespace {
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};
template <int OP, bool IN_BUILD>
struct Launch {
    static bool go(unsigned grid, uint64_t n, const Fp* a, const Fp* b, Fp* out, uint32_t* wit, uint32_t wcap, uint32_t* npos, Fp* park) {
        DEVCURVE_K(k_devcurve)<OP><<<grid, 64>>>(n, a, b, out, wit, wcap, npos, park);
        return true;
    }
};
template <int OP>
struct Launch<OP, false> {  // not in this build: the kernel is never instantiated
    static bool go(unsigned, uint64_t, const Fp*, const Fp*, Fp*, uint32_t*, uint32_t, uint32_t*, Fp*) { return false; }
};
}  // namespace

extern "C" {
uint32_t DEVCURVE_K(devcurve_lpi)() { return BLSW_LPI; }
// Runs operation `op` on n items. Host arrays: a, b [n][12][6] u64; out [n * LPI][12][6]; wit [n][wcap][6], copied to the device first (the
// caller's sentinel) and back; npos [n * LPI]. Returns 0, a HIP error code (the launch's, then the synchronisation's), -1 for an unknown
// operation, -2 when wcap is below the operation's witness count or n is 0 or above 2^16, -3 for an operation this build does not carry.
int DEVCURVE_K(devcurve_run)(int op, uint64_t n, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t* wit, uint32_t wcap, uint32_t* npos) {
    if (op < 0 || op >= OP_COUNT) return -1;
    if (!DEVCURVE_IN_BUILD(op_quad(op))) return -3;
    if (n == 0 || n > (1u << 16) || (int64_t)wcap < op_n_wit(op) || wcap == 0) return -2;
    const size_t in_bytes = n * 12 * sizeof(Fp), out_bytes = n * BLSW_LPI * DEVCURVE_OUT_MAX * sizeof(Fp), wit_bytes = n * (size_t)wcap * sizeof(Fp),
                 pos_bytes = n * BLSW_LPI * sizeof(uint32_t), park_bytes = n * DEVCURVE_PARK_SLOTS * 6 * sizeof(Fp);
    const bool parked = op == OP_v_clear_cofactor || op == OP_v_g2_mul_gls;
    DevBuf da, db, dout, dwit, dpos, dpark;
    hipError_t rc;
#define DEVCURVE_TRY(x) \
    if ((rc = (x)) != hipSuccess) return (int)rc
    DEVCURVE_TRY(hipMalloc(&da.p, in_bytes));
    DEVCURVE_TRY(hipMalloc(&db.p, in_bytes));
    DEVCURVE_TRY(hipMalloc(&dout.p, out_bytes));
    DEVCURVE_TRY(hipMalloc(&dwit.p, wit_bytes));
    DEVCURVE_TRY(hipMalloc(&dpos.p, pos_bytes));
    if (parked) {
        DEVCURVE_TRY(hipMalloc(&dpark.p, park_bytes));
        DEVCURVE_TRY(hipMemset(dpark.p, 0xA5, park_bytes));
    }
    DEVCURVE_TRY(hipMemcpy(da.p, a, in_bytes, hipMemcpyHostToDevice));
    DEVCURVE_TRY(hipMemcpy(db.p, b, in_bytes, hipMemcpyHostToDevice));
    DEVCURVE_TRY(hipMemcpy(dout.p, out, out_bytes, hipMemcpyHostToDevice));
    DEVCURVE_TRY(hipMemcpy(dwit.p, wit, wit_bytes, hipMemcpyHostToDevice));
    DEVCURVE_TRY(hipMemcpy(dpos.p, npos, pos_bytes, hipMemcpyHostToDevice));
    const unsigned grid = (unsigned)((n * BLSW_LPI + 63) / 64);
    bool carried = false;
    switch (op) {
#define DEVCURVE_X_LAUNCH(name, n_out, n_wit, quad)                                                                                                          \
    case OP_##name:                                                                                                                                          \
        carried = Launch<OP_##name, DEVCURVE_IN_BUILD(quad)>::go(grid, n, (const Fp*)da.p, (const Fp*)db.p, (Fp*)dout.p, (uint32_t*)dwit.p, wcap, (uint32_t*)dpos.p, \
                                                                 (Fp*)dpark.p);                                                                              \
        break;
        DEVCURVE_OPS(DEVCURVE_X_LAUNCH)
#undef DEVCURVE_X_LAUNCH
    }
    if (!carried) return -3;
    DEVCURVE_TRY(hipGetLastError());
    DEVCURVE_TRY(hipDeviceSynchronize());
    DEVCURVE_TRY(hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost));
    DEVCURVE_TRY(hipMemcpy(wit, dwit.p, wit_bytes, hipMemcpyDeviceToHost));
    DEVCURVE_TRY(hipMemcpy(npos, dpos.p, pos_bytes, hipMemcpyDeviceToHost));
#undef DEVCURVE_TRY
    return 0;
}
}
