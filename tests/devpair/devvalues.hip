// TEST HARNESS ONLY (never linked into libblsw.so): the shipped VALUE kernels on chosen points. csrc/k_vgroups.hip and csrc/k_team.hip are included
// whole (with k_pairing_lane.hip, whose kernel k_team.hip's launch_pairing names), so the kernels and launch_verify_groups / launch_verify_values are
// the library's text compiled with the library's flags, and are called UNCHANGED. The entry points take host arrays, copy them to the device (the
// outputs with the caller's sentinel) and back; the hash and decode stages are not run: the caller writes pk_xy, sig_xy, ws.h, status and scalars.
#include <cstring>
#include <vector>
#include "k_pairing_lane.hip"
#include "k_team.hip"
#include "k_vgroups.hip"

using namespace blsw;

namespace {
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    hipError_t up(const void* src, size_t n) {
        bytes = n;
        hipError_t rc = hipMalloc(&p, n ? n : 1);
        if (rc == hipSuccess && n) rc = hipMemcpy(p, src, n, hipMemcpyHostToDevice);
        return rc;
    }
    hipError_t down(void* dst) const { return bytes ? hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
};
}  // namespace

extern "C" {
// launch_verify_groups on n instances. Host arrays: pk_xy [n][12], sig_xy [n][24] u64 (affine, Montgomery), h [6][n][6] (ws.h), status [n][2],
// scalars [n]; outputs p_scaled [3][n][6], s_scaled [6][n][6], sum_xy [4][G][6], gflag [G], lines_h [408][n][6], lines_g [408][G][6], partials
// [G cpg][12][6], result [G], G = ceil(n / group), cpg = ceil(min(group, n) / chunk). Returns 0, a HIP error code, -2 for arguments out of range.
int devvalues_groups(uint64_t n, uint32_t group, uint32_t chunk, const uint64_t* pk_xy, const uint64_t* sig_xy, const uint64_t* h, const int32_t* status,
                     const uint64_t* scalars, uint64_t* p_scaled, uint64_t* s_scaled, uint64_t* sum_xy, int32_t* gflag, uint64_t* lines_h, uint64_t* lines_g, uint64_t* partials,
                     int32_t* result) {
    if (n == 0 || n > 4096 || group == 0 || chunk == 0 || chunk > 31) return -2;
    const uint64_t G = vg_groups(n, group);
    const uint32_t cpg = vg_chunks_per_group(n, group, chunk);
    hipError_t rc;
#define DEVVALUES_TRY(x) \
    if ((rc = (x)) != hipSuccess) return (int)rc
    DevBuf dpk, dsig, dh, dst, dsc, dp, ds, dsum, dfl, dlh, dlg, dpar, dres;
    DEVVALUES_TRY(dpk.up(pk_xy, n * 12 * 8));
    DEVVALUES_TRY(dsig.up(sig_xy, n * 24 * 8));
    DEVVALUES_TRY(dh.up(h, 6 * n * sizeof(Fp)));
    DEVVALUES_TRY(dst.up(status, n * 2 * sizeof(int32_t)));
    DEVVALUES_TRY(dsc.up(scalars, n * 8));
    DEVVALUES_TRY(dp.up(p_scaled, 3 * n * sizeof(Fp)));
    DEVVALUES_TRY(ds.up(s_scaled, 6 * n * sizeof(Fp)));
    DEVVALUES_TRY(dsum.up(sum_xy, 4 * G * sizeof(Fp)));
    DEVVALUES_TRY(dfl.up(gflag, G * sizeof(int32_t)));
    DEVVALUES_TRY(dlh.up(lines_h, (size_t)BLSW_VLINE_ROWS * n * sizeof(Fp)));
    DEVVALUES_TRY(dlg.up(lines_g, (size_t)BLSW_VLINE_ROWS * G * sizeof(Fp)));
    DEVVALUES_TRY(dpar.up(partials, G * cpg * 12 * sizeof(Fp)));
    DEVVALUES_TRY(dres.up(result, G * sizeof(int32_t)));
    Workspace ws;
    memset(&ws, 0, sizeof(ws));
    ws.h = (Fp*)dh.p;
    launch_verify_groups(n, group, chunk, ws, (const uint64_t*)dpk.p, (const uint64_t*)dsig.p, (const int32_t*)dst.p, (const uint64_t*)dsc.p, (Fp*)dp.p, (Fp*)ds.p, (Fp*)dsum.p,
                         (int32_t*)dfl.p, (Fp*)dlh.p, (Fp*)dlg.p, (Fp*)dpar.p, (int32_t*)dres.p, nullptr);
    DEVVALUES_TRY(hipGetLastError());
    DEVVALUES_TRY(hipDeviceSynchronize());
    DEVVALUES_TRY(dp.down(p_scaled));
    DEVVALUES_TRY(ds.down(s_scaled));
    DEVVALUES_TRY(dsum.down(sum_xy));
    DEVVALUES_TRY(dfl.down(gflag));
    DEVVALUES_TRY(dlh.down(lines_h));
    DEVVALUES_TRY(dlg.down(lines_g));
    DEVVALUES_TRY(dpar.down(partials));
    DEVVALUES_TRY(dres.down(result));
    return 0;
}
// launch_verify_values on n instances: lines_sig, lines_h [408][n][6], result [n]
int devvalues_values(uint64_t n, const uint64_t* pk_xy, const uint64_t* sig_xy, const uint64_t* h, const int32_t* status, uint64_t* lines_sig, uint64_t* lines_h, int32_t* result) {
    if (n == 0 || n > 4096) return -2;
    hipError_t rc;
    DevBuf dpk, dsig, dh, dst, dls, dlh, dres;
    DEVVALUES_TRY(dpk.up(pk_xy, n * 12 * 8));
    DEVVALUES_TRY(dsig.up(sig_xy, n * 24 * 8));
    DEVVALUES_TRY(dh.up(h, 6 * n * sizeof(Fp)));
    DEVVALUES_TRY(dst.up(status, n * 2 * sizeof(int32_t)));
    DEVVALUES_TRY(dls.up(lines_sig, (size_t)BLSW_VLINE_ROWS * n * sizeof(Fp)));
    DEVVALUES_TRY(dlh.up(lines_h, (size_t)BLSW_VLINE_ROWS * n * sizeof(Fp)));
    DEVVALUES_TRY(dres.up(result, n * sizeof(int32_t)));
    Workspace ws;
    memset(&ws, 0, sizeof(ws));
    ws.h = (Fp*)dh.p;
    launch_verify_values(n, ws, (const uint64_t*)dpk.p, (const uint64_t*)dsig.p, (Fp*)dls.p, (Fp*)dlh.p, (const int32_t*)dst.p, (int32_t*)dres.p, nullptr);
    DEVVALUES_TRY(hipGetLastError());
    DEVVALUES_TRY(hipDeviceSynchronize());
    DEVVALUES_TRY(dls.down(lines_sig));
    DEVVALUES_TRY(dlh.down(lines_h));
    DEVVALUES_TRY(dres.down(result));
#undef DEVVALUES_TRY
    return 0;
}
}
