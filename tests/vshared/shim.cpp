// TEST HARNESS ONLY (never linked into libblsw.so): compiles vshared.hpp of bls-verify-gadget_amd/csrc for the HOST with g++, on top of the host
// team and the helpers of tests/vgroups/shim.cpp, and runs (a) the run rule — the scan as the wave executes it, tile by tile with the ballot
// computed by a loop over the lanes — and (b) the stages of blsw_verify_groups_shared_batch next to the plain stages on materialised messages, lanes
// and teams one after the other, so that the kernels' logic is checked without a GPU (pytest -m "not gpu").
#include "../vgroups/shim.cpp"
#include "../../bls-verify-gadget_amd/csrc/vshared.hpp"

// k_vs_scan: every group, tiles of `tile` <= 64 lanes. status may be null (the rule alone).
static void scan_host(uint64_t n, uint32_t group, uint32_t tile, const uint32_t* idx, uint64_t n_msgs, uint32_t* slot_leader, uint32_t* slot_len, uint32_t* runs, int32_t* status) {
    const uint64_t G = vg_groups(n, group);
    for (uint64_t g = 0; g < G; g++) {
        const uint64_t first = g * group;
        const uint32_t size = vs_group_size(n, group, g);
        VsCarry c = {0, 0};
        for (uint32_t base = 0; base < size; base += tile) {
            const uint32_t m = size - base < tile ? size - base : tile;
            const bool last = base + m == size;
            uint64_t ballot = 0;
            for (uint32_t lane = 0; lane < m; lane++) ballot |= vs_is_leader(idx, first + base + lane, group) ? 1ull << lane : 0ull;
            for (uint32_t lane = 0; lane < m; lane++) {
                const uint64_t i = first + base + lane;
                if (status && vs_bad_index(idx[i], n_msgs)) status[2 * i] = VS_BAD_INDEX;
                const VsLaneOut o = vs_tile_lane(c, ballot, base, m, last, lane);
                if (o.put_leader) slot_leader[first + o.slot] = (uint32_t)i;
                if (o.put_len) slot_len[first + o.slot] = o.len;
                if (o.put_close) slot_len[first + o.close_slot] = o.close_len;
            }
            c = vs_tile_carry(c, ballot, base);
        }
        runs[g] = c.slots;
    }
}

typedef TeamHostValues::Reg Reg;
static Reg reg_mul(const Reg& a, const Reg& b) {
    TeamHostValues t;
    return t.exec_hot(TEAM_OP_MUL, a, b);
}
static void reg_out(const Reg& f, uint64_t* out) {
    for (uint32_t j = 0; j < 6; j++) {
        memcpy(out + 12 * j, f[j].c0.l, 48);
        memcpy(out + 12 * j + 6, f[j].c1.l, 48);
    }
}

extern "C" {
// The rule over n instances: leader [n] flags, slot_leader / slot_len [n] by slot and runs [G] as the scan stores them (the caller's sentinel stays
// in every slot at or beyond a group's runs), bad [n] flags, and per team T = g * cpg + q the chunk's first slot, its count and whether it walks.
// Returns cpg, -1 for arguments out of range.
int32_t vshared_rule(uint64_t n, uint32_t group, uint32_t chunk, uint32_t tile, const uint32_t* idx, uint64_t n_msgs, uint8_t* leader, uint32_t* slot_leader, uint32_t* slot_len,
                     uint32_t* runs, uint8_t* bad, uint64_t* chunk_first, uint32_t* chunk_count, uint8_t* chunk_walks) {
    if (n == 0 || group == 0 || chunk == 0 || chunk > 31 || tile == 0 || tile > 64) return -1;
    for (uint64_t i = 0; i < n; i++) {
        leader[i] = vs_is_leader(idx, i, group);
        bad[i] = vs_bad_index(idx[i], n_msgs);
    }
    scan_host(n, group, tile, idx, n_msgs, slot_leader, slot_len, runs, nullptr);
    const uint64_t G = vg_groups(n, group);
    const uint32_t cpg = vg_chunks_per_group(n, group, chunk);
    for (uint64_t T = 0; T < G * cpg; T++) {
        const VgChunk c = vs_chunk(group, chunk, T / cpg, (uint32_t)(T % cpg), runs[T / cpg]);
        chunk_first[T] = c.first;
        chunk_count[T] = c.count;
        chunk_walks[T] = vs_chunk_walks(c, (uint32_t)(T % cpg));
    }
    return (int32_t)cpg;
}

// n triples in groups of `group`: pk48s [n][48], sig96s [n][96], the table msgs [n_msgs][msg_len], msg_index [n], scalars [n]. Runs the shared
// stages (scan, scale, sum, merge, lines, fold, finish) and the plain ones on msgs[msg_index[i]] (an instance whose index is beyond the table is
// excluded there too: nothing of it can be materialised). Outputs per group: res_shared, res_plain, runs, f_shared / f_plain [72] the product of
// the partials BEFORE the final exponentiation, same_gt = the two products differ by a factor the final exponentiation sends to one; per instance
// st_shared [n][2], st_plain [n][2]. Returns the number of groups, -1 for arguments out of range.
int64_t vshared_groups(const uint8_t* pk48s, const uint8_t* sig96s, const uint8_t* msgs, uint32_t msg_len, uint32_t n_msgs, const uint32_t* msg_index, const uint64_t* scalars,
                       uint32_t n, uint32_t group, uint32_t chunk, uint32_t tile, int32_t* st_shared, int32_t* st_plain, int32_t* res_shared, int32_t* res_plain, uint32_t* runs,
                       uint64_t* f_shared, uint64_t* f_plain, int32_t* same_gt) {
    if (n == 0 || n_msgs == 0 || group == 0 || chunk == 0 || chunk > 31 || tile == 0 || tile > 64) return -1;
    const uint64_t G = vg_groups(n, group);
    const uint32_t cpg = vg_chunks_per_group(n, group, chunk);
    // decode (k_decode), then the scan's rule in front of [i][0]
    std::vector<Fp> px(n), py(n);
    std::vector<Fp2> sx(n), sy(n);
    for (uint32_t i = 0; i < n; i++) {
        st_plain[2 * i] = st_shared[2 * i] = g1_decode(pk48s + 48 * i, px[i], py[i]);
        st_plain[2 * i + 1] = st_shared[2 * i + 1] = g2_decode(sig96s + 96 * i, sx[i], sy[i]);
    }
    std::vector<uint32_t> slot_leader(n, 0xffffffffu), slot_len(n, 0xffffffffu);
    scan_host(n, group, tile, msg_index, n_msgs, slot_leader.data(), slot_len.data(), runs, st_shared);
    // hash: every table row once (launch_values_hash over n_msgs)
    std::vector<Fp2> hx(n_msgs), hy(n_msgs);
    for (uint32_t r = 0; r < n_msgs; r++) {
        bool inf;
        hash_to_g2_affine(msgs + (size_t)msg_len * r, msg_len, hx[r], hy[r], inf);
        if (inf) return -1;
    }
    // scale, sum (k_vg_scale, k_vg_sum): the same for both forms
    std::vector<Jac1v> P(n);
    std::vector<Jac2> S(n);
    std::vector<bool> in(n);
    for (uint32_t i = 0; i < n; i++) {
        in[i] = vg_included(st_shared[2 * i], st_shared[2 * i + 1], scalars[i]);
        const uint64_t r = in[i] ? scalars[i] : 0;
        P[i] = vg_scale_g1(px[i], py[i], r);
        S[i] = vg_scale_g2(sx[i], sy[i], r);
    }
    std::vector<Fp> lines_g((size_t)BLSW_VLINE_ROWS * G), lines_h((size_t)BLSW_VLINE_ROWS * n), lines_p((size_t)BLSW_VLINE_ROWS * n);
    std::vector<int32_t> gflag(G);
    for (uint64_t g = 0; g < G; g++) {
        const uint64_t first = g * group;
        const uint32_t m = vs_group_size(n, group, g);
        bool ok = true;
        for (uint32_t i = 0; i < m; i++) ok = ok && in[first + i];
        Fp2 x, y;
        const bool some = vg_affine2(vg_sum(m, [&](uint32_t i) { return S[first + i]; }), x, y);
        gflag[g] = (ok ? VG_FLAG_OK : 0) | (some ? VG_FLAG_SUM : 0);
        if (some) vline_chain(x, y, K_G1_GEN_X(), K_G1_GEN_NEG_Y(), RowsHost{lines_g.data() + g, G});
    }
    // merge, lines per slot (k_vs_merge, k_vs_lines); the plain lines per instance (k_vg_lines)
    std::vector<int32_t> rflag(n, -1);
    for (uint32_t t = 0; t < n; t++) {
        if (in[t]) {
            Fp m0, m1, m2;
            vg_line_multipliers(P[t], m0, m1, m2);
            vline_chain(hx[msg_index[t]], hy[msg_index[t]], m0, m1, m2, RowsHost{lines_p.data() + t, n});
        }
        if (t % group >= runs[t / group]) continue;
        const uint32_t lead = slot_leader[t], len = slot_len[t];
        if (lead >= n || len == 0 || len > n - lead) return -2;
        const Jac1v r = vs_merge(len, [&](uint32_t i) { return P[lead + i]; });
        rflag[t] = fp_is_zero(r.z) ? 0 : 1;
        if (!rflag[t]) continue;
        const uint32_t row = msg_index[lead];
        if (row >= n_msgs) return -3;  // a run that is not the identity holds an included instance
        Fp m0, m1, m2;
        vg_line_multipliers(r, m0, m1, m2);
        vline_chain(hx[row], hy[row], m0, m1, m2, RowsHost{lines_h.data() + t, n});
    }
    // fold and finish, shared (k_vs_fold) then plain (k_vg_fold)
    for (int form = 0; form < 2; form++) {
        std::vector<Fp> partials((size_t)G * cpg * 12);
        for (uint64_t T = 0; T < G * cpg; T++) {
            const uint64_t g = T / cpg;
            const uint32_t q = (uint32_t)(T % cpg);
            const VgChunk c = form == 0 ? vs_chunk(group, chunk, g, q, runs[g]) : vg_chunk(n, group, chunk, g, q);
            TeamHostGroups t;
            t.lines_h = form == 0 ? lines_h.data() : lines_p.data();
            t.lines_g = lines_g.data();
            t.parts = nullptr;
            t.n = n;
            t.n_groups = G;
            t.first = c.first;
            t.grp = g;
            t.count = c.count;
            uint32_t mask = 0;
            for (uint32_t p = 0; p < c.count; p++) mask |= (form == 0 ? rflag[c.first + p] == 1 : (bool)in[c.first + p]) ? 1u << p : 0u;
            const bool own = q == 0;
            if (own && (gflag[g] & VG_FLAG_SUM)) mask |= 1u << c.count;
            t.mask = mask;
            const Reg f = (form == 1 || vs_chunk_walks(c, q)) ? team_miller_groups(t, (uint32_t)c.first, c.count + (own ? 1u : 0u)) : t.one();
            for (uint32_t j = 0; j < 6; j++) {
                partials[(T * 6 + j) * 2] = f[j].c0;
                partials[(T * 6 + j) * 2 + 1] = f[j].c1;
            }
        }
        for (uint64_t g = 0; g < G; g++) {
            TeamHostGroups t;
            t.parts = partials.data();
            Reg f = t.load_partial(g * cpg);
            for (uint32_t q = 1; q < cpg; q++) f = reg_mul(f, t.load_partial(g * cpg + q));
            reg_out(f, (form == 0 ? f_shared : f_plain) + 72 * g);
            const bool one = team_groups_finish(t, g * cpg, cpg);
            (form == 0 ? res_shared : res_plain)[g] = (one && (gflag[g] & VG_FLAG_OK)) ? 1 : 0;
        }
    }
    for (uint64_t g = 0; g < G; g++) {  // f_shared / f_plain goes to one: the same element of GT
        Reg a, b;
        for (uint32_t j = 0; j < 6; j++) {
            memcpy(a[j].c0.l, f_shared + 72 * g + 12 * j, 48);
            memcpy(a[j].c1.l, f_shared + 72 * g + 12 * j + 6, 48);
            memcpy(b[j].c0.l, f_plain + 72 * g + 12 * j, 48);
            memcpy(b[j].c1.l, f_plain + 72 * g + 12 * j + 6, 48);
        }
        TeamHostValues t;
        const Reg ratio = reg_mul(a, t.inverse_w(b));
        same_gt[g] = team_final_exp_is_one(t, t.conj(ratio), Emitter{nullptr, 0}) ? 1 : 0;
    }
    return (int64_t)G;
}
}
