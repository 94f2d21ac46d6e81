// TEST HARNESS ONLY (never linked into libblsw.so): the output layer of csrc/k_stream.hip, kernel by kernel. This file includes k_stream.hip as its
// own translation unit, so the kernels and launch_expand are the library's text compiled with the library's flags. Every entry point takes DEVICE
// pointers (the caller's guarded, sentinel-filled buffers), launches on the null stream, synchronises and returns 0, the launch's HIP error, or 1000 + the
// synchronisation's; -2 for arguments a wrapper cannot launch.
//   devstream_expand          fills an ExpandArgs and calls launch_expand: the grid rule under test is the shipped one
//   devstream_place_* / _canonical_rows   the kernels with their arguments one by one; the grid formulas of engine.hip's static launch_place,
//                             launch_place_multi and launch_canonical are RESTATED here (the lines they were taken from are named); the shipped
//                             formulas themselves are held through blsw_engine_expand_compact (tests/test_stream_device_gpu.py)
//   devstream_sink            sha.hpp's device BitSink alone: a 64-lane kernel shaped like k_sha's bit path, every lane runs one script of pushes
#include "k_stream.hip"

using namespace blsw;

// One workgroup is one tile of 64 lanes, as in k_sha: the [16][64] word buffer in LDS, a lane's column at lds + threadIdx.x, its first 64-byte run
// at tile * bits_tile_words + lane * 16 words. Lanes >= n_lanes leave before any push. Entry i of the script is (op, n): op 0 = push(data, n) with
// n = 1 .. 32, op 1 = push32(data); data = the lane's word i ([n_lanes][n_ops], bits above n zero). The stream is flushed once, at the end.
__global__ __launch_bounds__(64) void k_devstream_sink(const uint32_t* __restrict__ script, uint32_t n_ops, const uint32_t* __restrict__ data, uint32_t n_lanes,
                                                       uint32_t* bits_out, uint64_t sha_words) {
    __shared__ uint32_t sink_lds[BLSW_BITS_CHUNK_WORDS * 64];
    const uint64_t I = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= n_lanes) return;
    BitSink s;
    s.init_device(sink_lds + threadIdx.x, reinterpret_cast<uint4*>(bits_out + (I >> 6) * bits_tile_words(sha_words) + (I & 63) * BLSW_BITS_CHUNK_WORDS));
    const uint32_t* d = data + I * n_ops;
    for (uint32_t i = 0; i < n_ops; i++) {
        if (script[2 * i] == 0)
            s.push(d[i], script[2 * i + 1]);
        else
            s.push32(d[i]);
    }
    s.flush();
}

namespace {
// hipGetLastError reports the last error of ANY earlier runtime call of this thread (the caller's too) until someone reads it: every entry point
// reads it away before its launch, so that what finish() returns is this launch's
void begin() { (void)hipGetLastError(); }
int finish() {
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return (int)rc;
    rc = hipDeviceSynchronize();
    return rc == hipSuccess ? 0 : 1000 + (int)rc;
}
// blocks of the XCD-ordered placement kernels: engine.hip:185-186 (launch_place) and engine.hip:205-208 (launch_place_multi's `blocks`)
unsigned place_blocks(uint32_t rows, uint32_t n_y) {
    const unsigned chunks = (rows * 3 + 256 * BLSW_PLACE_ITERS - 1) / (256 * BLSW_PLACE_ITERS);
    return 8 * ((chunks + 7) / 8) * n_y;
}
}  // namespace

extern "C" {
uint32_t devstream_place_iters() { return BLSW_PLACE_ITERS; }
uint32_t devstream_digest_iters() { return BLSW_DIGEST_ITERS; }
uint32_t devstream_resident_wgs() { return BLSW_EXPAND_RESIDENT_WGS; }

int devstream_expand(uint32_t variant, uint32_t store, const uint32_t* bits, uint64_t sha_words, uint64_t first, uint32_t sha_bits, uint32_t off_expand, uint64_t* out,
                     uint64_t stride, uint32_t K, uint32_t stride_hash, int canonical, uint32_t n_y) {
    if (!bits || !out || n_y == 0 || n_y > 65535 || K == 0 || sha_bits == 0) return -2;
    begin();
    ExpandArgs a = {bits, sha_words, first, sha_bits, off_expand, out, stride, K, stride_hash, 0, canonical};
    launch_expand(variant, store, 0, nullptr, a, n_y);
    return finish();
}
int devstream_place_field(const uint64_t* staging, const uint64_t* pair, uint64_t first, uint32_t off_expand, uint32_t sha_bits, uint32_t staging_rows, uint32_t split_row,
                          uint64_t* out, uint64_t stride, uint32_t n_inst, uint32_t moved_lo, uint32_t moved_len, uint32_t moved_at) {
    if (!staging || !pair || !out || n_inst == 0 || staging_rows == 0) return -2;
    begin();
    hipLaunchKernelGGL(k_place_field, dim3(place_blocks(staging_rows, n_inst)), dim3(256), 0, nullptr, reinterpret_cast<const Fp*>(staging), reinterpret_cast<const Fp*>(pair), first,
                       off_expand, sha_bits, staging_rows, split_row, out, stride, n_inst, moved_lo, moved_len, moved_at);
    return finish();
}
// src_row [7], dst_off [6], dst_stride [6]: the fields of PlaceRuns
int devstream_place_runs(const uint64_t* tiles, uint64_t first, uint32_t rows, uint32_t n_runs, const uint32_t* src_row, const uint32_t* dst_off, const uint32_t* dst_stride,
                         uint64_t* out, uint64_t stride, uint32_t n_y, uint32_t K, uint32_t tile_w) {
    if (!tiles || !out || n_runs == 0 || n_runs > 6 || n_y == 0 || K == 0 || tile_w == 0 || rows == 0) return -2;
    begin();
    PlaceRuns pr = {};
    pr.n_runs = n_runs;
    for (int r = 0; r < 7; r++) pr.src_row[r] = src_row[r];
    for (int r = 0; r < 6; r++) pr.dst_off[r] = dst_off[r], pr.dst_stride[r] = dst_stride[r];
    hipLaunchKernelGGL(k_place_runs, dim3(place_blocks(rows, n_y)), dim3(256), 0, nullptr, reinterpret_cast<const Fp*>(tiles), first, rows, pr, out, stride, n_y, K, tile_w);
    return finish();
}
int devstream_place_rows(const uint64_t* rows, uint32_t n_rows, uint32_t dst_off, uint64_t* out, uint64_t stride, uint32_t n) {
    if (!rows || !out || n == 0 || n > 65535 || n_rows == 0) return -2;
    begin();
    const unsigned chunks = (n_rows * 3 + 256 * BLSW_PLACE_ITERS - 1) / (256 * BLSW_PLACE_ITERS);  // engine.hip:218-219
    hipLaunchKernelGGL(k_place_rows, dim3(chunks, n), dim3(256), 0, nullptr, reinterpret_cast<const Fp*>(rows), n_rows, dst_off, out, stride);
    return finish();
}
int devstream_canonical_rows(uint64_t* out, uint64_t stride, uint32_t off_expand, uint32_t sha_bits, uint32_t rows, uint32_t K, uint32_t stride_hash, uint32_t n) {
    if (!out || n == 0 || n > 65535 || rows == 0) return -2;
    begin();
    hipLaunchKernelGGL(k_canonical_rows, dim3((rows + 255) / 256, n), dim3(256), 0, nullptr, out, stride, off_expand, sha_bits, rows, K, stride_hash);  // engine.hip:224
    return finish();
}
// bits_out: [ceil(n_lanes / 64)][sha_words / 16][64][16] u32, sha_words a multiple of 16 that holds the script's stream
int devstream_sink(const uint32_t* script, uint32_t n_ops, const uint32_t* data, uint32_t n_lanes, uint32_t* bits_out, uint64_t sha_words) {
    if (!script || !data || !bits_out || n_lanes == 0 || sha_words == 0 || sha_words % BLSW_BITS_CHUNK_WORDS) return -2;
    begin();
    hipLaunchKernelGGL(k_devstream_sink, dim3((n_lanes + 63) / 64), dim3(64), 0, nullptr, script, n_ops, data, n_lanes, bits_out, sha_words);
    return finish();
}
}
