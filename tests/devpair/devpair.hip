// TEST HARNESS ONLY (never linked into libblsw.so): the table of pairing programs of ops.hpp on the device, shaped like the library's kernels.
//   team form    one kernel per entry on the library's OWN device team of that program (TeamLanes<CoeffStrided> for team_miller as in k_pairing_team,
//                TeamLanesPv, TeamLanesMulti, TeamLanesValues, TeamLanesGroups), bound to element-major operand arrays exactly as k_team.hip binds them to the
//                workspace: coeff_sig [272][n], coeff_h [272][n K], pkaff [2][n K], pair j of item I at flat index I K + j; 64-thread workgroups,
//                ten teams per wave, lanes 60..63 and the idle teams of a ragged last wave on slot file 0 with a null cursor, in every barrier
//   single form  one thread per item, 64-thread workgroups: chain_miller as k_pairing runs it, vline_chain as k_vlines / k_vg_lines run it
//   miller_par   csrc/k_miller_par.hip is included whole, and devpair_par calls launch_miller_par UNCHANGED on a Group in direct mode (no staging:
//                a lane's cursor is its row of the caller's witness array) whose workspace is the operand arrays above, with either spine
// Lane j of a team writes coefficient j of the value and the team's cursor; a single lane writes its item's whole result, element-major
// ([n_out][lanes], CoeffStrided / Fp12Rows as in the library). The result and cursor arrays have a slot for EVERY lane of the grid.
#include <cstring>
#include <vector>
#include "k_miller_par.hip"  // the library's text as part of this unit: its five kernels and launch_miller_par
#include "ops.hpp"

using namespace devpair;

namespace {
struct DevArgs {
    uint64_t n;
    uint32_t K;
    const Fp* coeff_sig;  // [272][n] (miller_values: lines_sig [408][n]; vlines: the operand block [n_in][n])
    const Fp* coeff_h;    // [272][n K] (miller_values: lines_h [408][n])
    const Fp* pkaff;      // [2][n K]
    Fp* out;              // team: [lanes][2]; single: [n_out][lanes]
    uint32_t* wit;        // [n][wcap] elements
    uint32_t wcap;
    uint32_t* npos;       // [lanes]
    const uint32_t* hdr;  // [n][3] miller_groups: count, own, mask of the item; groups_finish: its number of partials (coeff_sig: lines_h [408][9 n], the
                          // instance sets of item I at columns 9 I ..; coeff_h: lines_g [408][n], its own pair; pkaff: partials [3 n][12])
};
// the library's team of each program, and what the table's interface adds to it
template <int OP>
struct DevTeam;
template <>
struct DevTeam<OP_miller> : TeamLanes<CoeffStrided> {};
template <>
struct DevTeam<OP_miller_pv> : TeamLanesPv {};
template <>
struct DevTeam<OP_miller_multi> : TeamLanesMulti {
    BLSW_TEAM_DEV void set_gen_y() {
        if (active && j == 0) team_st(slots, TS_XYC, {K_G1_GEN_NEG_Y(), fp_zero()});
        team_sync();
    }
};
template <>
struct DevTeam<OP_miller_values> : TeamLanesValues {};
template <>
struct DevTeam<OP_miller_groups> : TeamLanesGroups {};
}  // namespace

template <int OP>
__global__ __launch_bounds__(64) void k_devpair_team(DevArgs a) {
    __shared__ Fp2 lds[BLSW_TEAMS_PER_WAVE * TS_NSLOTS];
    const uint32_t team = threadIdx.x / 6, j = threadIdx.x % 6;
    const uint64_t I0 = (uint64_t)blockIdx.x * BLSW_TEAMS_PER_WAVE + team;
    const bool active = team < BLSW_TEAMS_PER_WAVE && I0 < a.n;
    const uint64_t I = active ? I0 : 0, n_h = a.n * a.K;  // idle lanes only take part in the barriers
    const uint64_t lane = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    DevTeam<OP> t;
    t.slots = lds + (active ? team : 0) * TS_NSLOTS;
    t.j = j;
    t.active = active;
    t.coeff_sig = {const_cast<Fp*>(a.coeff_sig) + I, a.n};
    t.coeff_h = {const_cast<Fp*>(a.coeff_h) + I, a.n};
    t.e = {a.wit + I * (uint64_t)a.wcap * 12, 0};
    if (!active) t.e.base = nullptr;
    Fp px = fp_zero(), py = fp_zero();
    uint32_t K = a.K;
    if constexpr (OP == OP_miller_groups) {  // bound as k_vg_fold binds a chunk: `count` instance pairs from lines_h, the own pair from lines_g
        t.coeff_sig = t.coeff_h = {nullptr, 0};
        t.lines_h = a.coeff_sig;
        t.lines_g = a.coeff_h;
        t.partials = nullptr;
        t.n = a.n * DEVPAIR_GROUPS_SETS;
        t.n_groups = a.n;
        t.first = I * DEVPAIR_GROUPS_SETS;
        t.grp = I;
        t.count = a.hdr[3 * I];
        t.mask = a.hdr[3 * I + 2];
        K = t.count + (a.hdr[3 * I + 1] ? 1u : 0u);
    } else if constexpr (OP == OP_miller_multi) {
        t.coeff_h = {nullptr, 0};
        t.coeff_h_all = a.coeff_h;
        t.pkaff = a.pkaff;
        t.n_h = n_h;
        t.flat0 = I * a.K;
    } else if constexpr (OP != OP_miller_values) {
        px = ld_fp(a.pkaff + I);
        py = ld_fp(a.pkaff + a.n + I);
    }
    const Fp2 f = run_team<OP>(t, px, py, K);
    if (active) {
        st_fp(a.out + lane * 2, f.c0);
        st_fp(a.out + lane * 2 + 1, f.c1);
        a.npos[lane] = t.e.pos;
    }
}
// groups_finish, bound as k_vg_finish binds a group: the verdict on all six lanes of the team
__global__ __launch_bounds__(64) void k_devpair_finish(DevArgs a) {
    __shared__ Fp2 lds[BLSW_TEAMS_PER_WAVE * TS_NSLOTS];
    const uint32_t team = threadIdx.x / 6, j = threadIdx.x % 6;
    const uint64_t I0 = (uint64_t)blockIdx.x * BLSW_TEAMS_PER_WAVE + team;
    const bool active = team < BLSW_TEAMS_PER_WAVE && I0 < a.n;
    const uint64_t I = active ? I0 : 0;
    const uint64_t lane = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    TeamLanesGroups t;
    t.slots = lds + (active ? team : 0) * TS_NSLOTS;
    t.j = j;
    t.active = active;
    t.coeff_sig = t.coeff_h = {nullptr, 0};
    t.lines_h = t.lines_g = nullptr;
    t.partials = a.pkaff;
    t.n = t.n_groups = a.n;
    t.first = 0;
    t.grp = I;
    t.count = t.mask = 0;
    const bool one = run_team_finish(t, I * DEVPAIR_FINISH_PARTIALS, a.hdr[3 * I]);
    if (active) {
        st_fp(a.out + lane * 2, devteam::fp_of_bool(one));
        st_fp(a.out + lane * 2 + 1, fp_zero());
        a.npos[lane] = t.e.pos;
    }
}

// single-lane forms: lanes = 64 * gridDim.x
__global__ __launch_bounds__(64) void k_devpair_lane_miller(DevArgs a, uint32_t n_wit) {
    const uint64_t I = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, lanes = (uint64_t)gridDim.x * 64;
    if (I >= a.n) return;
    const Fp pkx = ld_fp(a.pkaff + I), pky = ld_fp(a.pkaff + a.n + I);
    const Fp12 f = chain_miller(Emitter{a.wit + I * (uint64_t)a.wcap * 12, 0}, pkx, pky, CoeffStrided{const_cast<Fp*>(a.coeff_sig) + I, a.n},
                                CoeffStrided{const_cast<Fp*>(a.coeff_h) + I, a.n});
    Fp12Rows{a.out, lanes}.st(I, f);
    a.npos[I] = n_wit;  // chain_miller takes its cursor by value: the stream and the sentinel behind it state the count
}
template <bool THREE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_devpair_lane_vlines(DevArgs a) {
    const uint64_t I = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, lanes = (uint64_t)gridDim.x * 64;
    if (I >= a.n) return;
    const Fp* p = a.coeff_sig + I;  // the operand block, element-major
    const Fp2 qx = {ld_fp(p), ld_fp(p + a.n)}, qy = {ld_fp(p + 2 * a.n), ld_fp(p + 3 * a.n)};
    if constexpr (THREE)
        vline_chain(qx, qy, ld_fp(p + 4 * a.n), ld_fp(p + 5 * a.n), ld_fp(p + 6 * a.n), CoeffStrided{a.out + I, lanes});
    else
        vline_chain(qx, qy, ld_fp(p + 4 * a.n), ld_fp(p + 5 * a.n), CoeffStrided{a.out + I, lanes});
    a.npos[I] = 0;
}

namespace {
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};
struct NwCopied {
    uint32_t v[devteam::T_COUNT];
    uint32_t operator()(int id) const { return v[id]; }
};
// the tables' witness counts, copied from constant memory (the host pass of this unit sees the tables as device symbols, not as data)
hipError_t copy_counts(NwCopied& nw) {
    hipError_t rc = hipSuccess;
    uint32_t hdr[2];
    for (int i = 0; i < devteam::T_COUNT; i++) nw.v[i] = 0;
#define DEVPAIR_COUNT(id, sym)                                                                                         \
    if (rc == hipSuccess && (rc = hipMemcpyFromSymbol(hdr, HIP_SYMBOL(sym), sizeof(hdr))) == hipSuccess) nw.v[id] = hdr[1];
    DEVPAIR_COUNT(devteam::T_MUL, TEAM_OP_MUL)
    DEVPAIR_COUNT(devteam::T_CYC, TEAM_OP_CYC)
    DEVPAIR_COUNT(devteam::T_INVCHK, TEAM_OP_INVCHK)
    DEVPAIR_COUNT(T_SQR, TEAM_OP_SQR)
    DEVPAIR_COUNT(T_ELLC, TEAM_OP_ELLC)
    DEVPAIR_COUNT(T_ELLV, TEAM_OP_ELLV)
#undef DEVPAIR_COUNT
    return rc;
}
// src [rows][cols] elements -> dst [cols][rows]
void transpose(const Fp* src, Fp* dst, size_t rows, size_t cols) {
    for (size_t r = 0; r < rows; r++)
        for (size_t c = 0; c < cols; c++) dst[c * rows + r] = src[r * cols + c];
}
}  // namespace

extern "C" {
uint32_t devpair_teams_per_wave() { return BLSW_TEAMS_PER_WAVE; }
// Runs entry `op` on n items in form 0 (single lane; the entries whose single-lane form the library ships) or 1 (team). Host arrays: in
// [n][n_in][6] u64 operand blocks (ops.hpp; rearranged here into the element-major arrays the kernels bind); wit [n][wcap][6]; npos [lanes]; out:
// team form [lanes][2][6] with lanes = 64 * ceil(n / 10), single form [lanes][n_out][6] with lanes = 64 * ceil(n / 64). out, wit and npos are
// copied to the device first (the caller's sentinel) and back. Returns 0, a HIP error code, -1 for an unknown entry, form or K, -2 when wcap is
// below the entry's witness count or n is out of range.
int devpair_run(int form, int op, uint32_t K, uint64_t n, const uint64_t* in, uint64_t* out, uint64_t* wit, uint32_t wcap, uint32_t* npos) {
    const int forms = op_forms(op);
    if (forms < 0 || form < 0 || form > 1 || !k_ok(op, K) || !(form == 1 ? (forms & 2) : (forms & 4))) return -1;
    hipError_t rc;
#define DEVPAIR_TRY(x) \
    if ((rc = (x)) != hipSuccess) return (int)rc
    NwCopied nw;
    DEVPAIR_TRY(copy_counts(nw));
    const int64_t n_wit = op_n_wit(op, K, nw);
    const size_t n_in = (size_t)op_n_in(op, K), n_out = (size_t)op_n_out(op);
    if (n == 0 || n > 4096 || wcap == 0 || (int64_t)wcap < n_wit) return -2;
    const unsigned per_block = form == 1 ? BLSW_TEAMS_PER_WAVE : 64u;
    const unsigned grid = (unsigned)((n + per_block - 1) / per_block);
    const size_t lanes = (size_t)grid * 64, out_elems = form == 1 ? lanes * 2 : lanes * n_out;
    const Fp* fin = reinterpret_cast<const Fp*>(in);
    // the element-major operand arrays
    std::vector<Fp> cs, ch, pk;
    std::vector<uint32_t> hdr(3, 0);
    const bool witness_op = op == OP_miller || op == OP_miller_pv || op == OP_miller_multi;
    if (witness_op) {
        const size_t n_h = n * K;
        cs.resize(DEVPAIR_COEFFS * n);
        ch.resize(DEVPAIR_COEFFS * n_h);
        pk.resize(2 * n_h);
        for (size_t i = 0; i < n; i++) {
            const Fp* it = fin + i * n_in;
            for (size_t k = 0; k < DEVPAIR_COEFFS; k++) cs[k * n + i] = it[k];
            for (size_t j = 0; j < K; j++) {
                const Fp* pr = it + DEVPAIR_COEFFS + j * DEVPAIR_PAIR;
                const size_t t = i * K + j;
                for (size_t k = 0; k < DEVPAIR_COEFFS; k++) ch[k * n_h + t] = pr[k];
                pk[t] = pr[DEVPAIR_COEFFS];
                pk[n_h + t] = pr[DEVPAIR_COEFFS + 1];
            }
        }
    } else if (op == OP_miller_groups) {
        const size_t cols = n * DEVPAIR_GROUPS_SETS;
        cs.assign(BLSW_VLINE_ROWS * cols, fp_zero());
        ch.assign(BLSW_VLINE_ROWS * n, fp_zero());
        pk.resize(2);
        hdr.resize(3 * n);
        for (size_t i = 0; i < n; i++) {
            const Fp* it = fin + i * n_in;
            const uint32_t count = it[0].l[0], own = it[1].l[0] ? 1u : 0u;
            if (count + own > DEVPAIR_GROUPS_SETS) return -2;
            hdr[3 * i] = count;
            hdr[3 * i + 1] = own;
            hdr[3 * i + 2] = it[2].l[0] & ((1u << (count + own)) - 1u);  // the program never asks for a pair beyond n_pairs
            for (size_t j = 0; j < count; j++)
                for (size_t k = 0; k < BLSW_VLINE_ROWS; k++) cs[k * cols + i * DEVPAIR_GROUPS_SETS + j] = it[DEVPAIR_GROUPS_HDR + j * BLSW_VLINE_ROWS + k];
            for (size_t k = 0; own && k < BLSW_VLINE_ROWS; k++) ch[k * n + i] = it[DEVPAIR_GROUPS_HDR + count * BLSW_VLINE_ROWS + k];
        }
    } else if (op == OP_groups_finish) {
        cs.resize(1);
        ch.resize(1);
        pk.resize(n * DEVPAIR_FINISH_PARTIALS * 12);
        hdr.assign(3 * n, 0);
        for (size_t i = 0; i < n; i++) {
            const Fp* it = fin + i * n_in;
            if (it[0].l[0] < 1 || it[0].l[0] > DEVPAIR_FINISH_PARTIALS) return -2;
            hdr[3 * i] = it[0].l[0];
            for (size_t k = 0; k < DEVPAIR_FINISH_PARTIALS * 12; k++) pk[i * DEVPAIR_FINISH_PARTIALS * 12 + k] = it[1 + k];
        }
    } else if (op == OP_miller_values) {
        cs.resize(BLSW_VLINE_ROWS * n);
        ch.resize(BLSW_VLINE_ROWS * n);
        for (size_t i = 0; i < n; i++)
            for (size_t k = 0; k < BLSW_VLINE_ROWS; k++) {
                cs[k * n + i] = fin[i * n_in + k];
                ch[k * n + i] = fin[i * n_in + BLSW_VLINE_ROWS + k];
            }
        pk.resize(2);
    } else {
        cs.resize(n_in * n);
        transpose(fin, cs.data(), n, n_in);  // [n][n_in] -> [n_in][n]
        ch.resize(1);
        pk.resize(2);
    }
    std::vector<Fp> hout(out_elems);
    if (form == 1)
        memcpy(hout.data(), out, out_elems * sizeof(Fp));
    else
        transpose(reinterpret_cast<const Fp*>(out), hout.data(), lanes, n_out);  // [lanes][n_out] -> [n_out][lanes]
    const size_t wit_bytes = n * (size_t)wcap * sizeof(Fp), pos_bytes = lanes * sizeof(uint32_t);
    DevBuf dcs, dch, dpk, dout, dwit, dpos, dhdr;
    DEVPAIR_TRY(hipMalloc(&dhdr.p, hdr.size() * sizeof(uint32_t)));
    DEVPAIR_TRY(hipMemcpy(dhdr.p, hdr.data(), hdr.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    DEVPAIR_TRY(hipMalloc(&dcs.p, cs.size() * sizeof(Fp)));
    DEVPAIR_TRY(hipMalloc(&dch.p, ch.size() * sizeof(Fp)));
    DEVPAIR_TRY(hipMalloc(&dpk.p, pk.size() * sizeof(Fp)));
    DEVPAIR_TRY(hipMalloc(&dout.p, out_elems * sizeof(Fp)));
    DEVPAIR_TRY(hipMalloc(&dwit.p, wit_bytes));
    DEVPAIR_TRY(hipMalloc(&dpos.p, pos_bytes));
    DEVPAIR_TRY(hipMemcpy(dcs.p, cs.data(), cs.size() * sizeof(Fp), hipMemcpyHostToDevice));
    DEVPAIR_TRY(hipMemcpy(dch.p, ch.data(), ch.size() * sizeof(Fp), hipMemcpyHostToDevice));
    DEVPAIR_TRY(hipMemcpy(dpk.p, pk.data(), pk.size() * sizeof(Fp), hipMemcpyHostToDevice));
    DEVPAIR_TRY(hipMemcpy(dout.p, hout.data(), out_elems * sizeof(Fp), hipMemcpyHostToDevice));
    DEVPAIR_TRY(hipMemcpy(dwit.p, wit, wit_bytes, hipMemcpyHostToDevice));
    DEVPAIR_TRY(hipMemcpy(dpos.p, npos, pos_bytes, hipMemcpyHostToDevice));
    const DevArgs a = {n, K, (const Fp*)dcs.p, (const Fp*)dch.p, (const Fp*)dpk.p, (Fp*)dout.p, (uint32_t*)dwit.p, wcap, (uint32_t*)dpos.p, (const uint32_t*)dhdr.p};
    if (form == 1) {
        switch (op) {
            case OP_miller: k_devpair_team<OP_miller><<<grid, 64>>>(a); break;
            case OP_miller_pv: k_devpair_team<OP_miller_pv><<<grid, 64>>>(a); break;
            case OP_miller_multi: k_devpair_team<OP_miller_multi><<<grid, 64>>>(a); break;
            case OP_miller_groups: k_devpair_team<OP_miller_groups><<<grid, 64>>>(a); break;
            case OP_groups_finish: k_devpair_finish<<<grid, 64>>>(a); break;
            default: k_devpair_team<OP_miller_values><<<grid, 64>>>(a); break;
        }
    } else {
        switch (op) {
            case OP_miller: k_devpair_lane_miller<<<grid, 64>>>(a, (uint32_t)n_wit); break;
            case OP_vlines2: k_devpair_lane_vlines<false><<<grid, 64>>>(a); break;
            default: k_devpair_lane_vlines<true><<<grid, 64>>>(a); break;
        }
    }
    DEVPAIR_TRY(hipGetLastError());
    DEVPAIR_TRY(hipDeviceSynchronize());
    DEVPAIR_TRY(hipMemcpy(hout.data(), dout.p, out_elems * sizeof(Fp), hipMemcpyDeviceToHost));
    DEVPAIR_TRY(hipMemcpy(wit, dwit.p, wit_bytes, hipMemcpyDeviceToHost));
    DEVPAIR_TRY(hipMemcpy(npos, dpos.p, pos_bytes, hipMemcpyDeviceToHost));
#undef DEVPAIR_TRY
    if (form == 1)
        memcpy(out, hout.data(), out_elems * sizeof(Fp));
    else
        transpose(hout.data(), reinterpret_cast<Fp*>(out), n_out, lanes);  // [n_out][lanes] -> [lanes][n_out]
    return 0;
}

// The pair-parallel Miller product through launch_miller_par: n items of K pairs in chunks of B (MillerParArgs.B is a runtime value), spine_lane = 1
// the single-lane spine k_miller_m2, 0 the team spine. Host arrays, copied to the device first (the caller's sentinel) and back: in [n][272 + 274 K][6]
// operand blocks of miller_multi; ffinal [12][n][6]; f1, t [12][n 68][6]; q [12][n 68 C][6]; wit [n][wcap][6]: the Miller segment at cursor 0, the
// final exponentiation of k_final_team at off_final_exp = the Miller segment's length, its is_one tail at off_is_one; result [n]. wcap must hold
// off_is_one + n_is_one. Returns 0, a HIP error code, -1 / -2 as devpair_run.
int devpair_par(uint32_t K, uint32_t B, uint32_t spine_lane, uint64_t n, const uint64_t* in, uint64_t* ffinal, uint64_t* wit, uint32_t wcap, uint32_t off_is_one,
                uint32_t n_is_one, uint64_t* f1, uint64_t* t, uint64_t* q, int32_t* result) {
    if (!k_ok(OP_miller_multi, K) || B < 1 || B > 64) return -1;
    hipError_t rc;
#define DEVPAIR_TRY(x) \
    if ((rc = (x)) != hipSuccess) return (int)rc
    NwCopied nw;
    DEVPAIR_TRY(copy_counts(nw));
    const int64_t n_wit = op_n_wit(OP_miller_multi, K, nw);
    // k_final_team's cursor runs over the final exponentiation from the end of the Miller segment, its second cursor over the is_one tail
    const int64_t n_fe = devteam::op_n_wit(devteam::OP_final_exp_is_one, nw) - (int64_t)DEVTEAM_IS_ONE_WITNESSES;
    if (n == 0 || n > 64 || (int64_t)off_is_one != n_wit + n_fe || n_is_one != DEVTEAM_IS_ONE_WITNESSES || (uint64_t)off_is_one + n_is_one > wcap) return -2;
    const size_t n_in = (size_t)op_n_in(OP_miller_multi, K), n_h = n * K;
    const uint32_t C = miller_chunks(K, B);
    const size_t steps = n * BLSW_MILLER_STEPS, tasks = steps * C;
    const Fp* fin = reinterpret_cast<const Fp*>(in);
    std::vector<Fp> cs(DEVPAIR_COEFFS * n), ch(DEVPAIR_COEFFS * n_h), pk(2 * n_h);
    for (size_t i = 0; i < n; i++) {
        const Fp* it = fin + i * n_in;
        for (size_t k = 0; k < DEVPAIR_COEFFS; k++) cs[k * n + i] = it[k];
        for (size_t j = 0; j < K; j++) {
            const Fp* pr = it + DEVPAIR_COEFFS + j * DEVPAIR_PAIR;
            const size_t x = i * K + j;
            for (size_t k = 0; k < DEVPAIR_COEFFS; k++) ch[k * n_h + x] = pr[k];
            pk[x] = pr[DEVPAIR_COEFFS];
            pk[n_h + x] = pr[DEVPAIR_COEFFS + 1];
        }
    }
    const size_t wit_bytes = n * (size_t)wcap * sizeof(Fp), step_bytes = 12 * steps * sizeof(Fp), task_bytes = 12 * tasks * sizeof(Fp), fin_bytes = 12 * n * sizeof(Fp);
    DevBuf dcs, dch, dpk, dwit, dcp, dq, dt, df1, dff, dres, ddesc;
    DEVPAIR_TRY(hipMalloc(&dcs.p, cs.size() * sizeof(Fp)));
    DEVPAIR_TRY(hipMalloc(&dch.p, ch.size() * sizeof(Fp)));
    DEVPAIR_TRY(hipMalloc(&dpk.p, pk.size() * sizeof(Fp)));
    DEVPAIR_TRY(hipMalloc(&dwit.p, wit_bytes));
    DEVPAIR_TRY(hipMalloc(&dcp.p, task_bytes));
    DEVPAIR_TRY(hipMalloc(&dq.p, task_bytes));
    DEVPAIR_TRY(hipMalloc(&dt.p, step_bytes));
    DEVPAIR_TRY(hipMalloc(&df1.p, step_bytes));
    DEVPAIR_TRY(hipMalloc(&dff.p, fin_bytes));
    DEVPAIR_TRY(hipMalloc(&dres.p, n * sizeof(int32_t)));
    DEVPAIR_TRY(hipMalloc(&ddesc.p, sizeof(StepDesc)));
    DEVPAIR_TRY(hipMemcpy(dcs.p, cs.data(), cs.size() * sizeof(Fp), hipMemcpyHostToDevice));
    DEVPAIR_TRY(hipMemcpy(dch.p, ch.data(), ch.size() * sizeof(Fp), hipMemcpyHostToDevice));
    DEVPAIR_TRY(hipMemcpy(dpk.p, pk.data(), pk.size() * sizeof(Fp), hipMemcpyHostToDevice));
    DEVPAIR_TRY(hipMemcpy(dwit.p, wit, wit_bytes, hipMemcpyHostToDevice));
    DEVPAIR_TRY(hipMemset(dcp.p, 0xA5, task_bytes));
    DEVPAIR_TRY(hipMemcpy(dq.p, q, task_bytes, hipMemcpyHostToDevice));
    DEVPAIR_TRY(hipMemcpy(dt.p, t, step_bytes, hipMemcpyHostToDevice));
    DEVPAIR_TRY(hipMemcpy(df1.p, f1, step_bytes, hipMemcpyHostToDevice));
    DEVPAIR_TRY(hipMemcpy(dff.p, ffinal, fin_bytes, hipMemcpyHostToDevice));
    DEVPAIR_TRY(hipMemcpy(dres.p, result, n * sizeof(int32_t), hipMemcpyHostToDevice));
    StepDesc desc;
    memset(&desc, 0, sizeof(desc));
    desc.out = reinterpret_cast<uint64_t*>(dwit.p);
    desc.out_stride = wcap;
    desc.result = reinterpret_cast<int32_t*>(dres.p);
    DEVPAIR_TRY(hipMemcpy(ddesc.p, &desc, sizeof(desc), hipMemcpyHostToDevice));
    Group gs;
    memset(&gs, 0, sizeof(gs));
    gs.N = n;  // the per-signature view: one lane (one team) per instance, one step
    gs.n = (uint32_t)n;
    gs.K = 1;
    gs.desc = reinterpret_cast<const StepDesc*>(ddesc.p);
    gs.L.off_miller = 0;
    gs.L.off_final_exp = (uint32_t)n_wit;
    gs.L.off_is_one = off_is_one;
    gs.LS = gs.L;
    gs.ws.coeff_sig = (Fp*)dcs.p;
    gs.ws.n_sig = n;
    gs.ws.coeff_h = (Fp*)dch.p;
    gs.ws.pkaff = (Fp*)dpk.p;
    MillerParArgs a;
    memset(&a, 0, sizeof(a));
    a.cprod = (Fp*)dcp.p;
    a.q = (Fp*)dq.p;
    a.t = (Fp*)dt.p;
    a.f1 = (Fp*)df1.p;
    a.ffinal = (Fp*)dff.p;
    a.K = K;
    a.B = B;
    a.C = C;
    a.n_h = n_h;
    a.spine_lane = spine_lane;
    launch_miller_par(gs, a, nullptr, nullptr, nullptr, nullptr);
    DEVPAIR_TRY(hipGetLastError());
    DEVPAIR_TRY(hipDeviceSynchronize());
    DEVPAIR_TRY(hipMemcpy(wit, dwit.p, wit_bytes, hipMemcpyDeviceToHost));
    DEVPAIR_TRY(hipMemcpy(q, dq.p, task_bytes, hipMemcpyDeviceToHost));
    DEVPAIR_TRY(hipMemcpy(t, dt.p, step_bytes, hipMemcpyDeviceToHost));
    DEVPAIR_TRY(hipMemcpy(f1, df1.p, step_bytes, hipMemcpyDeviceToHost));
    DEVPAIR_TRY(hipMemcpy(ffinal, dff.p, fin_bytes, hipMemcpyDeviceToHost));
    DEVPAIR_TRY(hipMemcpy(result, dres.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
#undef DEVPAIR_TRY
    return 0;
}
}
