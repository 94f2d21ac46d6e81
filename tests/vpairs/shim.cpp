// TEST HARNESS ONLY (never linked into libblsw.so): compiles vpairs.hpp and what it rests on for the HOST with g++ and runs the stages of
// blsw_verify_pairs_batch (k_vpairs.hip), lanes and teams one after the other, on arrays laid out as the device's, so that the kernels' logic is
// checked against the CPU oracle without a GPU (pytest -m "not gpu"). The host team, the element-major rows and the hash lanes are those of
// tests/vgroups, whose translation unit is included whole (its own entry points come along unused).
#include "../vgroups/shim.cpp"

#include "../../bls-verify-gadget_amd/csrc/vpairs.hpp"

extern "C" {
// n instances of K pairs: pks48 [n][K][48], msgs [n][K][msg_len], counts [n] or null, sig96 [n][96]. The decode, hash, status and line stages run
// once; the fold and the finish run once per entry of chunks [n_chunks], result [n_chunks][n]. status [n][2], key_status [n][K].
// written [n][K + 1] (nullable): 1 where the line stage stored a pair's rows (column K: the signature's). Returns 0, -1 for arguments out of range.
int vpairs_instances(const uint8_t* pks48, const uint8_t* msgs, uint32_t msg_len, uint32_t K, const uint32_t* counts, const uint8_t* sig96, uint64_t n,
                     const uint32_t* chunks, uint32_t n_chunks, int32_t* result, int32_t* status, int32_t* key_status, uint8_t* written) {
    if (n == 0 || K == 0 || n_chunks == 0) return -1;
    for (uint32_t c = 0; c < n_chunks; c++)
        if (chunks[c] == 0 || chunks[c] > 31) return -1;
    const uint64_t NK = n * K;
    std::vector<Fp> key_xy(2 * NK), sig_xy(4 * n), lines_h((size_t)BLSW_VLINE_ROWS * NK), lines_s((size_t)BLSW_VLINE_ROWS * n);
    for (uint64_t t = 0; t < NK + n; t++) {  // decode
        if (t < NK) {
            key_status[t] = g1_decode(pks48 + t * 48, key_xy[2 * t], key_xy[2 * t + 1]);
        } else {
            const uint64_t i = t - NK;
            Fp2 x, y;
            status[2 * i + 1] = g2_decode(sig96 + i * 96, x, y);
            sig_xy[4 * i] = x.c0;
            sig_xy[4 * i + 1] = x.c1;
            sig_xy[4 * i + 2] = y.c0;
            sig_xy[4 * i + 3] = y.c1;
        }
    }
    for (uint64_t i = 0; i < n; i++) status[2 * i] = vp_instance_status(counts, i, K, key_status);  // status
    auto folds = [&](uint64_t i) { return status[2 * i] == DEC_OK && status[2 * i + 1] == DEC_OK; };
    if (written) memset(written, 0, n * (K + 1));
    for (uint64_t t = 0; t < NK + n; t++) {  // hash of the used messages, and lines: a pair the fold never reads writes nothing
        if (t < NK) {
            const uint64_t i = t / K;
            if (!folds(i) || (uint32_t)(t - i * K) >= vp_count_eff(counts, i, K)) continue;
            Fp2 hx, hy;
            bool inf;
            hash_to_g2_affine(msgs + (size_t)msg_len * t, msg_len, hx, hy, inf);
            vline_chain(hx, hy, key_xy[2 * t], key_xy[2 * t + 1], RowsHost{lines_h.data() + t, NK});
            if (written) written[i * (K + 1) + (t - i * K)] = 1;
        } else {
            const uint64_t i = t - NK;
            if (!folds(i)) continue;
            vline_chain(Fp2{sig_xy[4 * i], sig_xy[4 * i + 1]}, Fp2{sig_xy[4 * i + 2], sig_xy[4 * i + 3]}, K_G1_GEN_X(), K_G1_GEN_NEG_Y(), RowsHost{lines_s.data() + i, n});
            if (written) written[i * (K + 1) + K] = 1;
        }
    }
    for (uint32_t ci = 0; ci < n_chunks; ci++) {
        const uint32_t chunk = chunks[ci], cpi = vp_chunks_per_instance(K, chunk);
        std::vector<Fp> partials((size_t)n * cpi * 12);
        for (uint64_t T = 0; T < n * cpi; T++) {  // fold
            const uint64_t i = T / cpi;
            const uint32_t q = (uint32_t)(T % cpi);
            const VpChunk c = vp_chunk(chunk, vp_count_eff(counts, i, K), q);
            TeamHostGroups t;
            t.lines_h = lines_h.data();
            t.lines_g = lines_s.data();
            t.parts = nullptr;
            t.n = NK;
            t.n_groups = n;
            t.first = i * K + c.first;
            t.grp = i;
            t.count = c.count;
            t.mask = vp_chunk_mask(c, q, folds(i));
            const TeamHostValues::Reg f = team_miller_groups(t, (uint32_t)t.first, c.count + (q == 0 ? 1u : 0u));
            for (uint32_t j = 0; j < 6; j++) {
                partials[(T * 6 + j) * 2] = f[j].c0;
                partials[(T * 6 + j) * 2 + 1] = f[j].c1;
            }
        }
        for (uint64_t i = 0; i < n; i++) {  // finish
            TeamHostGroups t;
            t.parts = partials.data();
            const bool one = team_groups_finish(t, i * cpi, cpi);
            result[(uint64_t)ci * n + i] = (one && folds(i)) ? 1 : 0;
        }
    }
    return 0;
}
// the rules alone
int32_t vpairs_status(const uint32_t* counts, uint64_t i, uint32_t K, const int32_t* key_status) { return vp_instance_status(counts, i, K, key_status); }
uint32_t vpairs_count_eff(const uint32_t* counts, uint64_t i, uint32_t K) { return vp_count_eff(counts, i, K); }
uint32_t vpairs_chunks_per_instance(uint32_t K, uint32_t chunk) { return vp_chunks_per_instance(K, chunk); }
// chunk q of an instance: out = {first, count, mask with both statuses OK, mask otherwise}
void vpairs_chunk(uint32_t chunk, uint32_t count, uint32_t q, uint32_t* out) {
    const VpChunk c = vp_chunk(chunk, count, q);
    out[0] = c.first;
    out[1] = c.count;
    out[2] = vp_chunk_mask(c, q, true);
    out[3] = vp_chunk_mask(c, q, false);
}
}
