"""The output layer on the device (csrc/k_stream.hip: the fourteen expansion geometries and three store flavours, the placement kernels, the
canonical form, the digest; sha.hpp's device BitSink) against tests/stream_ref.py, kernel by kernel through tests/devstream (libdevstream.so
includes k_stream.hip as its own translation unit), and the shipped launch rules through the public ABI: a synthetic compact step expanded by
blsw_engine_expand_compact, and blsw_witness_digest on synthetic tensors. Every launch writes into a buffer that carries a position-dependent
sentinel with guards on both sides, and the whole buffer is compared: a store one piece too far is a failed comparison. The case lists and what
they cover are asserted on the host by tests/test_stream_ref.py; nothing is sampled and nothing is skipped here."""
import importlib

import numpy as np
import pytest

from tests import devstream_lib as D
from tests import stream_ref as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = importlib.import_module("bls-verify-gadget_amd")
    p.lib()
    return p


# ---------------------------------------------------------------- the kernels alone, between guards
def test_case_lists_assume_the_librarys_constants():
    """the workgroup spans the case lists and their coverage conditions are built on are the compiled ones"""
    L = D.load()
    assert L.devstream_place_iters() == S.PLACE_ITERS and 256 * L.devstream_digest_iters() == S.DIGEST_CHUNK and L.devstream_resident_wgs() == S.RESIDENT_WGS


@pytest.mark.parametrize("variant,store", S.KERNELS)
def test_expansion_alone_between_guards(variant, store):
    cases = S.expand_cases(variant, store)
    bad = []
    for c in cases:
        msg = D.run_expand(c)
        if msg:
            bad.append((msg, c))
    print("expand_variant %d, expand_store %d: %d launches, %d differ" % (variant, store, len(cases), len(bad)))
    assert not bad, bad[:5]


@pytest.mark.parametrize("rows", S.PLACE_FIELD_ROWS)
def test_place_field_tagged_rows(rows):
    cases = S.place_field_cases(rows)
    bad = [(m, c) for c in cases for m in [D.run_place_field(c)] if m]
    print("k_place_field, %d staged rows: %d launches, %d differ" % (rows, len(cases), len(bad)))
    assert not bad, bad[:5]


def test_place_runs_tagged_rows():
    cases = S.place_runs_cases()
    bad = [(m, c) for c in cases for m in [D.run_place_runs(c)] if m]
    print("k_place_runs: %d launches, %d differ" % (len(cases), len(bad)))
    assert not bad, bad[:5]


def test_place_rows_tagged_rows():
    bad = []
    for n_rows in (1, 2, 682, 683, 684, 1366):
        for n, dst_off in ((1, 0), (3, 11)):
            m = D.run_place_rows(n_rows, n, dst_off, dst_off + n_rows + 4)
            if m:
                bad.append((m, n_rows, n, dst_off))
    assert not bad, bad[:5]


def test_canonical_rows_every_border():
    cases = S.canonical_cases()
    bad = [(m, c) for c in cases for m in [D.run_canonical(c)] if m]
    assert not bad, bad[:5]


@pytest.mark.parametrize("name", list(S.sink_scripts()))
def test_device_bit_sink(name):
    script = S.sink_scripts()[name]
    bad = []
    for n_lanes in (1, 63, 64, 70):
        msg = D.run_sink(script, n_lanes, seed=n_lanes + len(name))[0]
        if msg:
            bad.append((n_lanes, msg))
    assert not bad, bad


@pytest.mark.parametrize("variant", [0, 10, 7])
def test_sink_output_feeds_the_expansion(variant):
    """the chain of the pipeline without the SHA code: the device sink's buffer is the expansion's input, the elements are the script's bits"""
    script = S.sink_scripts()["1025 bits"] + S.sink_scripts()["every n at every fill"][:500]
    n_lanes = 70
    msg, buf, origin, sha_words, words = D.run_sink(script, n_lanes, seed=variant)
    assert msg is None, msg
    nbits = sum(n for _, n in script)
    streams = np.stack([np.unpackbits(np.array(w, dtype=np.uint32).view(np.uint8), bitorder="little")[:nbits] for w in words])
    c = dict(variant=variant, store=0, sha_bits=nbits, sha_words=sha_words, off_expand=3, stride=nbits + 9, n_y=n_lanes, first=0, K=1, stride_hash=0, canonical=0)
    bits_dev = buf.view(-1)[4 * origin:]
    assert bits_dev.data_ptr() % 16 == 0
    msg = D.run_expand(c, bits_dev=bits_dev, streams=streams)
    assert msg is None, msg


# ---------------------------------------------------------------- the shipped launch rules: a synthetic compact step through blsw_engine_expand_compact
POOL = 4093  # distinct values of the canonical-form step (a prime: neighbouring rows and lanes differ)


def _sentinel64(torch, shape, dev):
    n = int(np.prod(shape))
    return (torch.arange(n, dtype=torch.int64, device=dev) * (0x9E3779B97F4A7C15 - (1 << 64)) + 0x1234567).reshape(shape)


@pytest.mark.parametrize("name", list(S.COMPACT_LAYOUTS))
def test_synthetic_compact_step_through_the_public_abi(pkg, name):
    """A compact step of 64 instances built by hand — random bit words with the pad bits set, tagged rows (distinct over the whole step) in the tile
    and pair regions at the addresses the header states — expanded by blsw_engine_expand_compact into a sentinel-filled tensor of stride
    n_witness + 5; the whole tensor against a tensor built with torch from the same buffer. With output_form 1 the rows are drawn from a pool of
    4 093 values whose canonical forms Python computed (3.3 million big-integer products otherwise)."""
    import torch

    dev = torch.device("cuda:0")
    opts = S.COMPACT_LAYOUTS[name]
    canonical = int(opts.get("output_form", 0))
    n = 64
    eng = pkg.WitnessEngine(n, 32, max_steps=2, device=dev, n_buffers=1, **opts)
    c = eng.compact_layout()
    assert c.total == eng.compact_bytes() and c.n_witness == eng.n_witness and c.n == n
    rng = np.random.default_rng(len(name))
    host = np.zeros(c.total, dtype=np.uint8)
    streams = rng.integers(0, 2, size=(n, c.sha_bits), dtype=np.uint8)
    words = S.pack_streams(streams, 0, c.sha_words, rng)
    host[:words.nbytes] = words.view(np.uint8)
    lanes = np.arange(n, dtype=np.uint64)
    rows_t, rows_p = np.arange(c.split_row, dtype=np.uint64), np.arange(c.split_row, c.staging_rows, dtype=np.uint64)
    if canonical:
        prng = __import__("random").Random(7)
        pool = [prng.randrange(S.P) for _ in range(POOL)]
        pool_in = np.stack([S.limbs64(v) for v in pool])
        pool_out = np.stack([S.limbs64(v * S.R_INV % S.P) for v in pool])
        pick = lambda lane, row: pool_in[((row * np.uint64(64) + lane) % np.uint64(POOL)).astype(np.int64)]
        tiles, pair = pick(lanes.reshape(1, 64), rows_t.reshape(-1, 1)), pick(lanes.reshape(-1, 1), rows_p.reshape(1, -1))
    else:
        tiles, pair = S.tag_rows(lanes.reshape(1, 64), rows_t.reshape(-1, 1)), S.tag_rows(lanes.reshape(-1, 1), rows_p.reshape(1, -1))
    host[c.off_staging:c.off_staging + tiles.nbytes] = np.ascontiguousarray(tiles).view(np.uint8).reshape(-1)  # [tile 0][row][64]
    host[c.off_pair:c.off_pair + pair.nbytes] = np.ascontiguousarray(pair).view(np.uint8).reshape(-1)          # [lane][row - split_row]
    compact = torch.from_numpy(host).to(dev)
    stride = c.n_witness + 5
    out = _sentinel64(torch, (n, stride, 6), dev)
    want = out.clone()
    comp64, comp32 = compact.view(torch.int64), compact.view(torch.int32)
    one = torch.from_numpy(S.limbs64(1 if canonical else S.R).view(np.int64)).to(dev)
    six = torch.arange(6, device=dev)
    row_of = S.staged_rows(c.n_witness, c.off_expand, c.sha_bits, c.moved_lo, c.moved_len, c.moved_at)
    is_bit = torch.from_numpy(row_of < 0).to(dev)
    if canonical:
        d_pool_out = torch.from_numpy(pool_out.view(np.int64)).to(dev)
        d_row = torch.from_numpy(np.where(row_of < 0, 0, row_of)).to(dev)
    for lane in range(n):
        region, off, bit = S.compact_locate_all(c, lane)
        d_off, d_bit = torch.from_numpy(off).to(dev), torch.from_numpy(bit.astype(np.int64)).to(dev)
        elem = comp64[(torch.where(is_bit, 0, d_off) // 8)[:, None] + six]
        if canonical:
            elem = d_pool_out[(d_row * 64 + lane) % POOL]
        b = (comp32[torch.where(is_bit, d_off, 0) // 4].to(torch.int64) >> d_bit) & 1
        want[lane, :c.n_witness] = torch.where(is_bit[:, None], b[:, None] * one[None, :], elem)
    eng.expand_compact(compact, out)
    torch.cuda.synchronize()
    if not torch.equal(out, want):
        bad = (out != want).any(dim=2).nonzero()
        lane, k = bad[0].tolist()
        where = "padding column" if k >= c.n_witness else ("SHA bit" if row_of[k] < 0 else "staged row %d" % row_of[k])
        raise AssertionError("%s: %d elements differ, the first at instance %d, witness %d (%s): got %s, expected %s" % (
            name, bad.shape[0], lane, k, where, [hex(v & (2**64 - 1)) for v in out[lane, k].tolist()], [hex(v & (2**64 - 1)) for v in want[lane, k].tolist()]))
    eng.close()


# ---------------------------------------------------------------- blsw_witness_digest on synthetic tensors
def _digest(pkg, torch, host, n_witness):
    t = torch.from_numpy(host.view(np.int64)).to("cuda:0")
    got = pkg.witness_digest(t, n_witness=n_witness)
    torch.cuda.synchronize()
    return got.cpu().numpy().view(np.uint64)


# A vector has 3 n_witness pieces, so 4096, 4097 and 8192 + 3 pieces do not exist: 4095 and 4098 straddle one chunk of 16 x 256 pieces, 12 285 /
# 12 288 / 12 291 three chunks (the exact multiple runs no checked path at all), 8 196 = 8 192 + 4 has a tail of four pieces
@pytest.mark.parametrize("n_witness", [1, 2, 1365, 1366, 2732, 4095, 4096, 4097])
def test_digest_chunk_borders(pkg, n_witness):
    import torch

    n, stride = 3, n_witness + 2
    rng = np.random.default_rng(n_witness)
    host = rng.integers(0, 1 << 63, size=(n, stride, 6), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, stride, 6), dtype=np.uint64)
    want = S.digest_many(host[:, :n_witness].reshape(n, -1))
    assert want[0].tolist() == pkg.witness_digest_reference(host[0, :n_witness])
    got = _digest(pkg, torch, host, n_witness)
    assert np.array_equal(got, want), (got, want)
    host[:, n_witness:] = ~host[:, n_witness:]  # the padding between the vectors is no part of them
    assert np.array_equal(_digest(pkg, torch, host, n_witness), want)
    for fill in (0, 0xFFFFFFFFFFFFFFFF):  # sums that wrap, and the keys alone
        host[:, :n_witness] = fill
        want_fill = S.digest_many(host[:, :n_witness].reshape(n, -1))
        assert np.array_equal(_digest(pkg, torch, host, n_witness), want_fill) and want_fill[0].tolist() == S.digest_int(host[0, :n_witness].reshape(-1).view(np.uint32))


def test_digest_one_bit_flips(pkg):
    import torch

    n_witness = 4097  # 12 291 pieces: three whole chunks and a tail chunk of three pieces
    rng = np.random.default_rng(9)
    host = rng.integers(0, 1 << 63, size=(1, n_witness + 1, 6), dtype=np.uint64)
    base = _digest(pkg, torch, host, n_witness)
    assert np.array_equal(base, S.digest_many(host[:, :n_witness].reshape(1, -1)))
    for piece, word, bit in ((0, 0, 0), (3 * n_witness - 1, 3, 31), (3 * S.DIGEST_CHUNK, 1, 7), (S.DIGEST_CHUNK - 1, 2, 13)):
        h = host.copy()
        h.reshape(-1).view(np.uint32)[4 * piece + word] ^= np.uint32(1 << bit)
        got = _digest(pkg, torch, h, n_witness)
        assert np.array_equal(got, S.digest_many(h[:, :n_witness].reshape(1, -1)))
        assert got[0, 0] != base[0, 0] and got[0, 1] != base[0, 1], "a flipped bit in piece %d changes both words" % piece


def test_digest_workgroups_walk_several_chunks(pkg):
    """one vector just past 4096 x 4096 pieces: 4 097 chunks on the 4 096 workgroups of an instance, so workgroup 0 walks a second chunk — the tail
    chunk of two pieces — and resets its key for it (268 MB)"""
    import torch

    n_witness = (S.DIGEST_MAX_WGS * S.DIGEST_CHUNK + 2) // 3
    assert 3 * n_witness == S.DIGEST_MAX_WGS * S.DIGEST_CHUNK + 2
    rng = np.random.default_rng(11)
    host = rng.integers(0, 1 << 63, size=(1, n_witness, 6), dtype=np.uint64)
    host[0, -1] = 0xFFFFFFFFFFFFFFFF
    want = S.digest_many(host.reshape(1, -1))
    got = _digest(pkg, torch, host, n_witness)
    assert np.array_equal(got, want), (got, want)
    host[0, -1, 5] ^= np.uint64(1 << 40)  # the last piece of the tail chunk
    got2 = _digest(pkg, torch, host, n_witness)
    assert np.array_equal(got2, S.digest_many(host.reshape(1, -1))) and got2[0, 0] != got[0, 0] and got2[0, 1] != got[0, 1]


def test_digest_two_slices_of_instances(pkg):
    import torch

    n = 65536  # 65 535 + 1: two launches
    rng = np.random.default_rng(13)
    host = rng.integers(0, 1 << 63, size=(n, 1, 6), dtype=np.uint64)
    want = S.digest_many(host.reshape(n, -1))
    for i in (0, 1, 65534, 65535):
        assert want[i].tolist() == pkg.witness_digest_reference(host[i])
    got = _digest(pkg, torch, host, 1)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, bad[:10]
