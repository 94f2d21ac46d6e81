"""ctypes loader for tests/devstream/libdevstream.so (TEST HARNESS ONLY) and the launch-and-compare steps of tests/test_stream_device_gpu.py: every
launch writes into a buffer that carries a position-dependent sentinel, with guards of more than one workgroup's span on both sides, and the WHOLE
buffer is compared with the reference's expected buffer on the device (torch), 16-byte piece by piece."""
import ctypes
import os
import subprocess

import numpy as np

from tests import stream_ref as S

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "devstream")
GUARD = 16384  # pieces (256 KiB) in front of and behind everything a launch may write: the largest workgroup writes 12 288 pieces

_lib = None


def load():
    global _lib
    if _lib is None:
        import torch  # noqa: F401  BEFORE the library: it brings the process's HIP runtime. Loaded after libdevstream.so (which then resolves its own
        # from the ROCm installation first) every launch of this library returned hipErrorNoDevice (100) on an MI355X.

        subprocess.check_call(["make", "-s", "-C", HERE])
        _lib = ctypes.CDLL(os.path.join(HERE, "libdevstream.so"))
        for name in ("devstream_expand", "devstream_place_field", "devstream_place_runs", "devstream_place_rows", "devstream_canonical_rows", "devstream_sink"):
            getattr(_lib, name).restype = ctypes.c_int
    return _lib


def device():
    import torch

    return torch.device("cuda:0")


_SENT = {}


def sentinel(n_pieces):
    """int32 [n_pieces][4] on the device: word i = i * 2654435761 + 0x7F4A7C15 mod 2^32 (no piece of it is a piece of R, of 1 or of 0)"""
    import torch

    have = _SENT.get("t")
    if have is None or have.shape[0] < n_pieces:
        n = max(n_pieces, 1 << 22)
        w = (np.arange(4 * n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(0x7F4A7C15)).astype(np.uint32)
        have = torch.from_numpy(w.view(np.int32).reshape(n, 4)).to(device())
        _SENT["t"] = have
    return have[:n_pieces]


def _dev(a, dtype):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).to(device())


def guarded(n_pieces, align=1):
    """-> (buffer int32 [N][4] holding the sentinel, index of its piece 0: GUARD or more pieces in, on a multiple of `align` pieces in memory)"""
    buf = sentinel(n_pieces + 2 * GUARD + align).clone()
    origin = GUARD + (-(buf.data_ptr() // 16 + GUARD)) % align
    return buf, origin


def first_difference(got, want, written):
    """-> None, or a description of the first piece that differs; written = bool tensor [N] of the pieces the launch owns"""
    import torch

    if torch.equal(got, want):
        return None
    bad = (got != want).any(dim=1).nonzero().flatten()
    q = int(bad[0])
    return "%d pieces differ, the first is piece %d (%s): got %s, expected %s" % (bad.numel(), q, "a written piece" if bool(written[q]) else "a SENTINEL piece: a stray store",
                                                                                [hex(v & 0xFFFFFFFF) for v in got[q].tolist()], [hex(v & 0xFFFFFFFF) for v in want[q].tolist()])


def run_expand(c, bits_dev=None, streams=None):
    """One launch of devstream_expand for a case of stream_ref.expand_cases -> None or the first difference. bits_dev / streams: a bit-word buffer
    that is on the device already (the chained sink case) and the bits it must hold."""
    import torch

    L = load()
    if streams is None:
        streams = S.expand_streams(c)
    if bits_dev is None:
        bits_dev = _dev(S.pack_streams(streams, c["first"], c["sha_words"], np.random.default_rng(c["seed"] ^ 0x55)), np.int32)
    buf, origin = guarded(3 * S.n_instances(c) * c["stride"], S.ORIGIN_ALIGN)
    idx, vals = S.expand_expected(c, streams)
    want = buf.clone()
    idx_dev = torch.from_numpy(idx + origin).to(device())
    want[idx_dev] = _dev(vals, np.int32)
    written = torch.zeros(buf.shape[0], dtype=torch.bool, device=device())
    written[idx_dev] = True
    rc = L.devstream_expand(c["variant"], c["store"], ctypes.c_void_p(bits_dev.data_ptr()), ctypes.c_uint64(c["sha_words"]), ctypes.c_uint64(c["first"]), c["sha_bits"],
                            c["off_expand"], ctypes.c_void_p(buf.data_ptr() + 16 * origin), ctypes.c_uint64(c["stride"]), c["K"], c["stride_hash"], c["canonical"], c["n_y"])
    assert rc == 0, "devstream_expand returned %d for %r" % (rc, c)
    return first_difference(buf, want, written)


def _elements_buffer(n_elements):
    """a guarded buffer for n_elements 48-byte elements -> (buffer, origin piece)"""
    return guarded(3 * n_elements)


def _write_expected(buf, origin, mask, vals):
    """expected buffer and ownership mask from (mask [..], vals [.., 6] u64) laid out from the origin on"""
    import torch

    want = buf.clone()
    m = np.repeat(np.asarray(mask).reshape(-1), 3)
    idx = torch.from_numpy(np.flatnonzero(m) + origin).to(device())
    pieces = np.ascontiguousarray(vals, dtype=np.uint64).reshape(-1, 2).view(np.int32).reshape(-1, 4)
    want[idx] = torch.from_numpy(pieces[m]).to(device())
    written = torch.zeros(buf.shape[0], dtype=torch.bool, device=device())
    written[idx] = True
    return want, written


def run_place_field(c):
    L = load()
    tiles, pair = S.place_field_sources(c)
    d_tiles, d_pair = _dev(np.concatenate([tiles.reshape(-1), np.zeros(6, np.uint64)]), np.int64), _dev(np.concatenate([pair.reshape(-1), np.zeros(6, np.uint64)]), np.int64)
    mask, vals = S.place_field_expected(c)
    buf, origin = _elements_buffer(c["n_inst"] * c["stride"])
    want, written = _write_expected(buf, origin, np.broadcast_to(mask, (c["n_inst"], c["stride"])), vals)
    rc = L.devstream_place_field(ctypes.c_void_p(d_tiles.data_ptr()), ctypes.c_void_p(d_pair.data_ptr()), ctypes.c_uint64(c["first"]), c["off_expand"], c["sha_bits"],
                                 c["staging_rows"], c["split_row"], ctypes.c_void_p(buf.data_ptr() + 16 * origin), ctypes.c_uint64(c["stride"]), c["n_inst"], c["moved_lo"],
                                 c["moved_len"], c["moved_at"])
    assert rc == 0, "devstream_place_field returned %d for %r" % (rc, c)
    return first_difference(buf, want, written)


def run_place_runs(c):
    L = load()
    d_tiles = _dev(S.place_runs_sources(c), np.int64)
    mask, vals = S.place_runs_expected(c)
    buf, origin = _elements_buffer(mask.shape[0] * c["stride"])
    want, written = _write_expected(buf, origin, mask, vals)
    u32 = lambda v: (ctypes.c_uint32 * len(v))(*v)
    rc = L.devstream_place_runs(ctypes.c_void_p(d_tiles.data_ptr()), ctypes.c_uint64(c["first"]), c["rows"], c["n_runs"], u32(c["src_row"]), u32(c["dst_off"]), u32(c["dst_stride"]),
                                ctypes.c_void_p(buf.data_ptr() + 16 * origin), ctypes.c_uint64(c["stride"]), c["n_y"], c["K"], c["tile_w"])
    assert rc == 0, "devstream_place_runs returned %d for %r" % (rc, c)
    return first_difference(buf, want, written)


def run_place_rows(n_rows, n, dst_off, stride):
    L = load()
    rows = S.tag_rows(np.arange(n, dtype=np.uint64).reshape(-1, 1), np.arange(n_rows, dtype=np.uint64).reshape(1, -1), kind=2)
    mask = np.zeros((n, stride), dtype=bool)
    mask[:, dst_off:dst_off + n_rows] = True
    vals = np.zeros((n, stride, 6), dtype=np.uint64)
    vals[:, dst_off:dst_off + n_rows] = rows
    d_rows = _dev(rows, np.int64)
    buf, origin = _elements_buffer(n * stride)
    want, written = _write_expected(buf, origin, mask, vals)
    rc = L.devstream_place_rows(ctypes.c_void_p(d_rows.data_ptr()), n_rows, dst_off, ctypes.c_void_p(buf.data_ptr() + 16 * origin), ctypes.c_uint64(stride), n)
    assert rc == 0, "devstream_place_rows returned %d" % rc
    return first_difference(buf, want, written)


def run_canonical(c):
    """k_canonical_rows works in place: every element of the n vectors (segments and padding too) starts as a tagged element; the field rows must
    come back as x R^-1 mod p, everything else as it was"""
    L = load()
    n, stride = c["n"], c["stride"]
    start = S.tag_rows(np.arange(n, dtype=np.uint64).reshape(-1, 1), np.arange(stride, dtype=np.uint64).reshape(1, -1), kind=3)
    field = np.zeros(stride, dtype=bool)
    field[:c["n_witness"]] = S.canonical_field_mask(c)
    vals = start.copy()
    vals[:, field] = S.to_canonical(start[:, field])
    buf, origin = _elements_buffer(n * stride)
    everything = np.ones((n, stride), dtype=bool)
    buf, _ = _write_expected(buf, origin, everything, start)
    want, written = _write_expected(buf, origin, everything, vals)
    rows = c["n_witness"] - c["K"] * c["sha_bits"]
    rc = L.devstream_canonical_rows(ctypes.c_void_p(buf.data_ptr() + 16 * origin), ctypes.c_uint64(stride), c["off_expand"], c["sha_bits"], rows, c["K"], c["stride_hash"], n)
    assert rc == 0, "devstream_canonical_rows returned %d for %r" % (rc, c)
    return first_difference(buf, want, written)


def run_sink(script, n_lanes, seed):
    """One launch of the device BitSink -> (None or a description of the first difference, the bit-word buffer on the device, sha_words, the lanes'
    words). Compared: every word of every lane's stream at its 64-byte-run address, the sentinel in every run behind a lane's last run and in every
    run of the lanes >= n_lanes. The words of a partial last run beyond the stream are not defined (never read) and not compared."""
    L = load()
    data = S.sink_data(script, n_lanes, seed)
    words = [S.concat_bits(script, data[l, :len(script)].tolist())[0] for l in range(n_lanes)]
    n_words = len(words[0])
    sha_words = S.align_up(n_words, S.CHUNK_WORDS) + S.CHUNK_WORDS  # one run more than the stream needs: the sentinel behind every lane's stream
    tiles = (n_lanes + 63) // 64
    buf, origin = guarded(tiles * sha_words * 64 // 4)
    want = buf.cpu().numpy().view(np.uint32).reshape(-1).copy()  # (the buffers of this kernel are small: compared on the host)
    compared = np.ones(want.size, dtype=bool)
    w = np.arange(n_words, dtype=np.int64)
    tail = np.arange(n_words, S.align_up(n_words, S.CHUNK_WORDS), dtype=np.int64)
    for l in range(n_lanes):
        base = 4 * origin + (l >> 6) * sha_words * 64 + (l & 63) * S.CHUNK_WORDS
        want[base + (w // 16) * 1024 + w % 16] = np.array(words[l], dtype=np.uint32)
        compared[base + (tail // 16) * 1024 + tail % 16] = False
    script_arr = np.array([v for e in script for v in e] + [0, 0], dtype=np.uint32)
    d_script, d_data = _dev(script_arr, np.int32), _dev(data, np.int32)
    rc = L.devstream_sink(ctypes.c_void_p(d_script.data_ptr()), len(script), ctypes.c_void_p(d_data.data_ptr()), n_lanes, ctypes.c_void_p(buf.data_ptr() + 16 * origin),
                          ctypes.c_uint64(sha_words))
    assert rc == 0, "devstream_sink returned %d" % rc
    got = buf.cpu().numpy().view(np.uint32).reshape(-1)
    bad = np.flatnonzero((got != want) & compared)
    msg = None
    if bad.size:
        i = int(bad[0]) - 4 * origin
        msg = "%d words differ, the first at word %d of the buffer (tile %d, run %d, lane %d, word %d): got %#x, expected %#x" % (
            bad.size, i, i // (sha_words * 64), i % (sha_words * 64) // 1024, i % 1024 // 16, i % 16, int(got[bad[0]]), int(want[bad[0]]))
    return msg, buf, origin, sha_words, words


def host_sink(script, data):
    """sha.hpp's host BitSink on a script (hostsim_sink_script) -> (words, nbits)"""
    from tests import hostsim_lib

    H = hostsim_lib.load()
    H.hostsim_sink_script.restype = ctypes.c_int64
    cap = 2 * (sum(n if op == 0 else 32 for op, n in script) // 32) + 16  # (room for a sink that miscounts: a failed comparison, not an overrun)
    out = np.full(cap, 0xA5A5A5A5, dtype=np.uint32)
    script_arr = np.array([v for e in script for v in e] + [0, 0], dtype=np.uint32)
    d = np.ascontiguousarray(list(data) + [0], dtype=np.uint32)
    nbits = ctypes.c_uint64(0)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    n = H.hostsim_sink_script(script_arr.ctypes.data_as(u32p), len(script), d.ctypes.data_as(u32p), out.ctypes.data_as(u32p), ctypes.c_uint64(cap), ctypes.byref(nbits))
    assert n >= 0
    return out[:n].tolist(), nbits.value, out[n:].tolist()
