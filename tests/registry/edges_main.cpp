// TEST PROGRAM (stand-alone, built with -fsanitize=address,undefined; run on the CPU only): the host walk of registry.hpp over the bad-offset and
// bad-index cases. Every array is allocated at exactly its stated length — the records at `size`, not at the capacity; the indices at n_indices — so
// that a read of a row at or beyond the size, or of a list entry that bad offsets name, is a heap overflow the sanitizer reports.
//   edges_main      prints one line per case and L, exits 0 iff every status, aggregate and coordinate is as expected
#include <cstdio>
#include <memory>
#include "shim.cpp"

static void unhex(const char* h, uint8_t* out, size_t n) {
    for (size_t i = 0; i < n; i++) {
        unsigned v = 0;
        std::sscanf(h + 2 * i, "%2x", &v);
        out[i] = (uint8_t)v;
    }
}
struct Case {
    const char* name;
    std::vector<uint32_t> indices;
    std::vector<uint64_t> offsets;  // two entries: one set
    uint64_t n_indices;             // what the call is told; the array holds min(n_indices, indices.size()) entries
    int32_t status;
    int agg;  // 0: zeros, 1: the generator's encoding, 2: the infinity encoding, -1: not checked
};

int main() {
    // the registry: g, -g, the identity, the point of order 3 at (0, 2), g — five keys of a capacity of 64
    uint8_t keys[5][48] = {};
    unhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb", keys[0], 48);
    std::memcpy(keys[1], keys[0], 48);
    keys[1][0] ^= 0x20;
    keys[2][0] = 0xC0;
    keys[3][0] = 0x80;
    std::memcpy(keys[4], keys[0], 48);
    const uint32_t size = 5;
    std::vector<RegistryRecord> records(size);  // exactly `size` rows
    std::vector<int32_t> key_status(size);
    registry_append(keys[0], 0, 3, reinterpret_cast<uint8_t*>(records.data()), key_status.data());  // in two parts
    registry_append(keys[3], 3, 2, reinterpret_cast<uint8_t*>(records.data()), key_status.data());
    const int32_t want_keys[5] = {DEC_OK, DEC_OK, DEC_IDENTITY, DEC_NOT_IN_SUBGROUP, DEC_OK};
    int failures = 0;
    for (int k = 0; k < 5; k++)
        if (key_status[k] != want_keys[k] || records[k].status != want_keys[k]) {
            std::printf("key %d: status %d, expected %d\n", k, key_status[k], want_keys[k]);
            failures++;
        }
    uint8_t inf48[48] = {0xC0}, zero48[48] = {};
    const std::vector<Case> cases = {
        {"one good key", {0}, {0, 1}, 1, DEC_OK, 1},
        {"the empty list", {}, {0, 0}, 0, DEC_IDENTITY, 2},
        {"the empty list at the end of the indices", {0}, {1, 1}, 1, DEC_IDENTITY, 2},
        {"a key and its negation", {0, 1}, {0, 2}, 2, DEC_IDENTITY, 2},
        {"an identity key is a summand", {2, 0}, {0, 2}, 2, DEC_OK, 1},
        {"index == size", {0, 5}, {0, 2}, 2, DEC_BAD_INDEX, 0},
        {"index == 0xffffffff", {0xffffffffu, 0}, {0, 2}, 2, DEC_BAD_INDEX, 0},
        {"index >= size, below the capacity", {0, 1, 63}, {0, 3}, 3, DEC_BAD_INDEX, 0},
        {"a bad key, then a bad index: the earlier position wins", {0, 3, 9}, {0, 3}, 3, DEC_NOT_IN_SUBGROUP, 0},
        {"a bad index, then a bad key", {0, 9, 3}, {0, 3}, 3, DEC_BAD_INDEX, 0},
        {"both bad, one per lane and far apart", {9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3}, {0, 35}, 35, DEC_BAD_INDEX, 0},
        {"descending offsets", {0, 0}, {2, 1}, 2, DEC_BAD_INDEX, 0},
        {"an offset beyond n_indices", {0, 0}, {1, 3}, 2, DEC_BAD_INDEX, 0},
        {"both offsets beyond n_indices", {0}, {7, 9}, 1, DEC_BAD_INDEX, 0},
        {"an offset of 2^63", {0}, {0, 1ull << 63}, 1, DEC_BAD_INDEX, 0},
        {"offsets with n_indices == 0 and no index array", {}, {0, 1}, 0, DEC_BAD_INDEX, 0},
    };
    for (const Case& c : cases) {
        // a heap block of exactly the entries the call may read (none: a one-byte block, never dereferenced)
        std::unique_ptr<uint32_t[]> idx(new uint32_t[c.indices.empty() ? 1 : c.indices.size()]);
        for (size_t k = 0; k < c.indices.size(); k++) idx[k] = c.indices[k];
        for (uint32_t L = 1; L <= 64; L *= 2) {
            uint32_t pk_xy[24];
            int32_t status = -1;
            uint8_t agg[48];
            std::memset(agg, 0x5A, 48);
            const int rc = registry_sum(reinterpret_cast<const uint8_t*>(records.data()), size, c.indices.empty() ? nullptr : idx.get(), c.n_indices, c.offsets.data(), 1, L, pk_xy,
                                        &status, agg);
            bool ok = rc == 0 && status == c.status;
            const uint8_t* want = c.agg == 0 ? zero48 : c.agg == 1 ? keys[0] : inf48;
            if (c.agg >= 0) ok = ok && std::memcmp(agg, want, 48) == 0;
            bool zero_xy = true;
            for (uint32_t w : pk_xy) zero_xy = zero_xy && w == 0;
            ok = ok && (zero_xy == (c.status != DEC_OK));
            if (c.status == DEC_OK) ok = ok && std::memcmp(pk_xy, &records[0].x, 48) == 0 && std::memcmp(pk_xy + 12, &records[0].y, 48) == 0;
            std::printf("%-60s L %2u status %d %s\n", c.name, L, status, ok ? "ok" : "FAILED");
            failures += !ok;
        }
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
