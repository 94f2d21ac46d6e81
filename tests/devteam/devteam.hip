// TEST HARNESS ONLY (never linked into libblsw.so): the team operation table of ops.hpp on the device, one kernel per entry (two where the library
// runs the op through exec and through exec_hot), shaped like the library's team kernels (csrc/k_team.hip): 64-thread workgroups, ten teams of six
// lanes per wave with lanes 60..63 idle, the teams' slot files in LDS, idle teams of a ragged last wave on slot file 0 with a null cursor, every
// lane in every barrier. Lane j of a team loads coefficient j of its item's operands and writes its own coefficient of the result and its own
// cursor; the result and cursor arrays have a slot for EVERY lane of the grid, and an idle lane leaves its slots alone.
#include "kcommon.hpp"
#include "team_multi.hpp"
#include "ops.hpp"

using namespace devteam;

// the device team of the table: TeamLanesPv (load_pair_sig / load_pair_h / first_f_var) with TeamLanesValues' one() / load_lines and the table's
// operand and result access. The operand block c is read as a coefficient row of one instance (CoeffStrided with n = 1).
struct TeamLanesTable : TeamLanesPv {
    Fp* out;  // this lane's result slot: [2]
    BLSW_TEAM_DEV void set_coeffs(const Fp* c) { coeff_sig = coeff_h = CoeffStrided{const_cast<Fp*>(c), 1}; }
    BLSW_TEAM_DEV Reg one() const { return j == 0 ? fp2_one() : fp2_zero(); }
    BLSW_TEAM_DEV void load_lines(uint32_t k) {
        if (active) team_load_lines_lane(j, slots, coeff_sig, coeff_h, k);
        team_sync();
    }
    BLSW_TEAM_DEV void load_pair_lines(uint32_t k) {
        if (active) team_load_pair_lines_lane(j, slots, coeff_h, k);
        team_sync();
    }
    BLSW_TEAM_DEV Reg ld(const Fp* p) const { return active ? Fp2{ld_fp(p + 2 * j), ld_fp(p + 2 * j + 1)} : fp2_zero(); }
    BLSW_TEAM_DEV void st(const Reg& r) const {
        if (!active) return;
        st_fp(out, r.c0);
        st_fp(out + 1, r.c1);
    }
    BLSW_TEAM_DEV void st_flag(bool v) const { st(Fp2{fp_of_bool(v), fp_zero()}); }
};

// a, b, c: [n][12] elements; out: [lanes][2]; wit: [n][wcap]; npos: [lanes] the lane's cursor after the entry; lanes = 64 * gridDim.x
template <int OP, bool HOT>
__global__ __launch_bounds__(64) void k_devteam(uint64_t n, const Fp* a, const Fp* b, const Fp* c, Fp* out, uint32_t* wit, uint32_t wcap, uint32_t* npos, uint32_t alt) {
    constexpr uint32_t NSLOTS = TeamEntry<OP>::g2 ? TS_P + 12 : TS_NSLOTS;  // k_g2_alloc_team sizes its file by the G2 tables' slots
    __shared__ Fp2 lds[BLSW_TEAMS_PER_WAVE * NSLOTS];
    const uint32_t team = threadIdx.x / 6, j = threadIdx.x % 6;
    const uint64_t I0 = (uint64_t)blockIdx.x * BLSW_TEAMS_PER_WAVE + team;
    const bool active = team < BLSW_TEAMS_PER_WAVE && I0 < n;
    const uint64_t I = active ? I0 : 0;  // idle lanes only take part in the barriers
    const uint64_t lane = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    TeamLanesTable t;
    t.slots = lds + (active ? team : 0) * NSLOTS;
    t.j = j;
    t.active = active;
    t.coeff_sig = t.coeff_h = CoeffStrided{nullptr, 0};
    t.pkx = t.pky = fp_zero();
    t.e = {wit + I * (uint64_t)wcap * 12, 0};
    if (!active) t.e.base = nullptr;
    t.out = out + lane * 2;
    TeamEntry<OP>::template team<HOT>(t, a + I * 12, b + I * 12, c + I * 12, alt);
    if (active) npos[lane] = t.e.pos;
}

namespace {
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};
// the tables' witness counts, copied from constant memory (the host pass of this unit sees the tables as device symbols, not as data)
struct NwCopied {
    uint32_t v[T_COUNT];
    uint32_t operator()(int id) const { return v[id]; }
};
hipError_t copy_counts(NwCopied& nw) {
    hipError_t rc = hipSuccess;
    uint32_t hdr[2];
#define DEVTEAM_COUNT(id, sym)                                                                                         \
    if (rc == hipSuccess && (rc = hipMemcpyFromSymbol(hdr, HIP_SYMBOL(sym), sizeof(hdr))) == hipSuccess) nw.v[id] = hdr[1];
    DEVTEAM_COUNT(T_MUL, TEAM_OP_MUL)
    DEVTEAM_COUNT(T_SQR, TEAM_OP_SQR)
    DEVTEAM_COUNT(T_CYC, TEAM_OP_CYC)
    DEVTEAM_COUNT(T_ELLC, TEAM_OP_ELLC)
    DEVTEAM_COUNT(T_ELLV, TEAM_OP_ELLV)
    DEVTEAM_COUNT(T_ELLGS, TEAM_OP_ELLGS)
    DEVTEAM_COUNT(T_ELLGH, TEAM_OP_ELLGH)
    DEVTEAM_COUNT(T_G2DBL, TEAM_OP_G2DBL)
    DEVTEAM_COUNT(T_G2ADD, TEAM_OP_G2ADD)
    DEVTEAM_COUNT(T_INVCHK, TEAM_OP_INVCHK)
#undef DEVTEAM_COUNT
    return rc;
}
template <int OP>
void launch(bool hot, unsigned grid, uint64_t n, const Fp* a, const Fp* b, const Fp* c, Fp* out, uint32_t* wit, uint32_t wcap, uint32_t* npos, uint32_t alt) {
    if constexpr (TeamEntry<OP>::dual) {
        if (hot) {
            k_devteam<OP, true><<<grid, 64>>>(n, a, b, c, out, wit, wcap, npos, alt);
            return;
        }
    }
    k_devteam<OP, false><<<grid, 64>>>(n, a, b, c, out, wit, wcap, npos, alt);
}
}  // namespace

extern "C" {
uint32_t devteam_teams_per_wave() { return BLSW_TEAMS_PER_WAVE; }
// Runs entry `op` on n items, through exec_hot where hot != 0 (entries that have both kernels). Host arrays: a, b, c [n][12][6] u64; out
// [lanes][2][6] and npos [lanes] with lanes = 64 * ceil(n / 10), copied to the device first (the caller's sentinel) and back, as is wit
// [n][wcap][6]. Returns 0, a HIP error code, -1 for an unknown entry (or hot on an entry with one kernel), -2 when wcap is below the entry's
// witness count or n is out of range.
int devteam_run(int op, int hot, uint64_t n, const uint64_t* a, const uint64_t* b, const uint64_t* c, uint64_t* out, uint64_t* wit, uint32_t wcap, uint32_t* npos) {
    if (op < 0 || op >= OP_COUNT || (hot && !op_dual(op))) return -1;
    hipError_t rc;
#define DEVTEAM_TRY(x) \
    if ((rc = (x)) != hipSuccess) return (int)rc
    NwCopied nw;
    DEVTEAM_TRY(copy_counts(nw));
    if (n == 0 || n > (1u << 16) || wcap == 0 || (int64_t)wcap < op_n_wit(op, nw)) return -2;
    const unsigned grid = (unsigned)((n + BLSW_TEAMS_PER_WAVE - 1) / BLSW_TEAMS_PER_WAVE);
    const size_t lanes = (size_t)grid * 64;
    const size_t in_bytes = n * 12 * sizeof(Fp), out_bytes = lanes * 2 * sizeof(Fp), wit_bytes = n * (size_t)wcap * sizeof(Fp), pos_bytes = lanes * sizeof(uint32_t);
    DevBuf da, db, dc, dout, dwit, dpos;
    DEVTEAM_TRY(hipMalloc(&da.p, in_bytes));
    DEVTEAM_TRY(hipMalloc(&db.p, in_bytes));
    DEVTEAM_TRY(hipMalloc(&dc.p, in_bytes));
    DEVTEAM_TRY(hipMalloc(&dout.p, out_bytes));
    DEVTEAM_TRY(hipMalloc(&dwit.p, wit_bytes));
    DEVTEAM_TRY(hipMalloc(&dpos.p, pos_bytes));
    DEVTEAM_TRY(hipMemcpy(da.p, a, in_bytes, hipMemcpyHostToDevice));
    DEVTEAM_TRY(hipMemcpy(db.p, b, in_bytes, hipMemcpyHostToDevice));
    DEVTEAM_TRY(hipMemcpy(dc.p, c, in_bytes, hipMemcpyHostToDevice));
    DEVTEAM_TRY(hipMemcpy(dout.p, out, out_bytes, hipMemcpyHostToDevice));
    DEVTEAM_TRY(hipMemcpy(dwit.p, wit, wit_bytes, hipMemcpyHostToDevice));
    DEVTEAM_TRY(hipMemcpy(dpos.p, npos, pos_bytes, hipMemcpyHostToDevice));
    switch (op) {
#define DEVTEAM_X_LAUNCH(name, dual, g2, w, tail)                                                                                                            \
    case OP_##name:                                                                                                                                          \
        launch<OP_##name>(hot != 0, grid, n, (const Fp*)da.p, (const Fp*)db.p, (const Fp*)dc.p, (Fp*)dout.p, (uint32_t*)dwit.p, wcap, (uint32_t*)dpos.p, 0u); \
        break;
        DEVTEAM_OPS(DEVTEAM_X_LAUNCH)
#undef DEVTEAM_X_LAUNCH
    }
    DEVTEAM_TRY(hipGetLastError());
    DEVTEAM_TRY(hipDeviceSynchronize());
    DEVTEAM_TRY(hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost));
    DEVTEAM_TRY(hipMemcpy(wit, dwit.p, wit_bytes, hipMemcpyDeviceToHost));
    DEVTEAM_TRY(hipMemcpy(npos, dpos.p, pos_bytes, hipMemcpyDeviceToHost));
#undef DEVTEAM_TRY
    return 0;
}
}
