"""Where a witness element lives in a step's compact wire form (blsw_compact_layout / blsw_compact_locate, ABI 14), host side: the locator
is a bijection from the witness indices onto the bits, tile rows and pairing rows of the buffer for every shape a compact step exists for,
the sizes are the engine's, and the argument rules hold. No GPU: the functions are host logic."""
import ctypes
import importlib

import numpy as np
import pytest

BLSW_ERR_ARG = 1
N = 128  # two 64-instance tiles
FP = 48
CHUNK = 16  # u32 words of one lane's run in a [64][16] bit-word chunk

SHAPES = {
    "single_key_32": dict(msg_len=32),
    "single_key_0": dict(msg_len=0),
    "params_witness": dict(msg_len=32, params_mode=1),
    "inputs": dict(msg_len=32, pk_mode=1, sig_mode=1, msg_mode=1),
    "aggregate_2": dict(msg_len=32, n_keys=2, agg_inputs=0),
    "aggregate_2_inputs": dict(msg_len=32, n_keys=2, agg_inputs=15),
    "g2_team": dict(msg_len=32, g2_mode=1),  # the moved segment: the G2 allocation is staged last
}


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bls-verify-gadget_amd")


def product_layout(pkg, msg_len=32, n_keys=0, agg_inputs=0, g2_mode=0, **modes):
    return pkg.layout_aggregate(msg_len, n_keys, agg_inputs) if n_keys else pkg.layout(msg_len, **modes)


def decode(c, lane, region, off, bit):
    """byte offsets of one lane -> the bit index / tile row / pairing row they address, from the CompactForm geometry
    ([n/64][sha_words/16][64][16] u32 | [n/64][split_row][64] Fp | [n][pair_rows] Fp); asserts alignment and that the lane is the one asked for"""
    tile, l = lane >> 6, lane & 63
    idx = np.zeros(off.shape, np.int64)
    m = region == 0
    assert (off[m] % 4 == 0).all()
    u = off[m] // 4 - tile * c.sha_words * 64
    assert ((u >= 0) & (u < c.sha_words * 64)).all() and ((u % (64 * CHUNK)) // CHUNK == l).all()
    idx[m] = ((u // (64 * CHUNK)) * CHUNK + u % CHUNK) * 32 + bit[m]
    assert (bit[~m] == 0).all()
    m = region == 1
    e = off[m] - c.off_staging
    assert (e % FP == 0).all()
    e //= FP
    assert (e % 64 == l).all() and (e // 64 // max(c.split_row, 1) == tile).all()
    idx[m] = e // 64 - tile * c.split_row
    m = region == 2
    e = off[m] - c.off_pair
    assert (e % FP == 0).all()
    e //= FP
    assert (e // max(c.pair_rows, 1) == lane).all()
    idx[m] = e - lane * c.pair_rows
    return idx


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_locator_is_a_bijection_onto_the_buffer(pkg, name):
    shape = dict(SHAPES[name])
    msg_len = shape.pop("msg_len")
    c = pkg.compact_layout(N, msg_len, **shape)
    L = product_layout(pkg, msg_len, **shape)
    assert (c.n, c.n_witness, c.off_expand, c.sha_bits) == (N, L["n_witness"], L["off_expand"], L["sha_bits"])
    assert c.staging_rows == c.n_witness - c.sha_bits == c.split_row + c.pair_rows
    assert (c.moved_len > 0) == (name == "g2_team")
    for lane in (0, 63, 64):
        region, off, bit = pkg.compact_locate_all(c, lane)
        # inside the buffer, a whole word / element
        size = np.where(region == 0, 4, FP)
        assert (off >= 0).all() and (off + size <= c.total).all()
        # the witnesses of the SHA segment are the bits, in order; everything else is a row
        k = np.arange(c.n_witness)
        in_sha = (k >= c.off_expand) & (k < c.off_expand + c.sha_bits)
        assert ((region == 0) == in_sha).all()
        idx = decode(c, lane, region, off, bit)
        assert np.array_equal(idx[region == 0], np.arange(c.sha_bits))
        # pairwise distinct, covering exactly the tile rows below split_row and every pairing row
        assert np.array_equal(np.sort(idx[region == 1]), np.arange(c.split_row))
        assert np.array_equal(np.sort(idx[region == 2]), np.arange(c.pair_rows))
        # rows keep the witness order except for the moved segment, which is staged last
        row = np.where(region == 2, idx + c.split_row, idx)[~in_sha]
        kk = k[~in_sha]
        moved = (kk >= c.moved_lo) & (kk < c.moved_lo + c.moved_len)
        assert (np.diff(row[~moved]) == 1).all() and row[~moved][0] == 0
        if c.moved_len:
            assert np.array_equal(row[moved], c.moved_at + np.arange(c.moved_len)) and c.moved_at + c.moved_len == c.staging_rows
    # a lane's three regions do not overlap each other's: bits < off_staging <= tile rows < off_pair <= pairing rows
    assert c.sha_words * 64 * 4 * (N // 64) <= c.off_staging and c.off_staging + c.split_row * N * FP <= c.off_pair and c.off_pair + c.pair_rows * N * FP <= c.total


def test_sizes_match_the_compact_form(pkg):
    """2 593 280 B per instance for the 32-byte single-key shape; the offsets are CompactForm's (regions back to back, 256-byte aligned)"""
    for n in (64, 128, 1024):
        c = pkg.compact_layout(n, 32)
        assert c.total == 2593280 * n
        bits = c.sha_words * 64 * 4 * (n // 64)
        assert c.sha_words % CHUNK == 0 and c.sha_words * 32 >= c.sha_bits + 32
        assert c.off_staging == -(-bits // 256) * 256
        assert c.off_pair == -(-(c.off_staging + c.split_row * n * FP) // 256) * 256
        assert c.total == -(-(c.off_pair + c.pair_rows * n * FP) // 256) * 256
    lay = pkg.layout(32)
    assert c.split_row == lay["off_miller"] - lay["sha_bits"]  # the pairing segments are the instance-major rows
    one = pkg.compact_layout(1024, 32, pairing_mode=1)  # single-lane pairing kernel: every row is a tile row
    assert one.pair_rows == 0 and one.split_row == one.staging_rows and one.total == c.total


def test_refusals(pkg):
    L = pkg.lib()
    c = pkg.blsw_compact_layout_t()
    opt = pkg.engine_options()
    assert L.blsw_compact_layout(128, 32, ctypes.byref(opt), ctypes.byref(c)) == 0
    assert L.blsw_compact_layout(100, 32, ctypes.byref(opt), ctypes.byref(c)) == BLSW_ERR_ARG
    assert L.blsw_compact_layout(128, 32, ctypes.byref(opt), None) == BLSW_ERR_ARG
    assert L.blsw_compact_layout(128, 32, None, ctypes.byref(c)) == BLSW_ERR_ARG
    assert L.blsw_compact_layout(128, 32, ctypes.byref(pkg.engine_options(n_pairs=2)), ctypes.byref(c)) == BLSW_ERR_ARG
    # what the engine refuses, the layout refuses: n beyond a launch's rows, an unknown mode, modes that do not combine
    assert L.blsw_compact_layout(65536, 32, ctypes.byref(opt), ctypes.byref(c)) == BLSW_ERR_ARG
    for kw in (dict(params_mode=2), dict(n_keys=2, pk_mode=1), dict(agg_inputs=3), dict(g2_mode=1, pairing_mode=1), dict(msg_mode=1, params_mode=1)):
        assert L.blsw_compact_layout(128, 32, ctypes.byref(pkg.engine_options(**kw)), ctypes.byref(c)) == BLSW_ERR_ARG, kw
    with pytest.raises(pkg.BlswError):
        pkg.compact_layout(100, 32)
    # the locator: NULL pointers, indices out of range, a layout that is not one
    c = pkg.compact_layout(128, 32)
    r, o, b = ctypes.c_uint32(7), ctypes.c_uint64(7), ctypes.c_uint32(7)
    args = (ctypes.byref(r), ctypes.byref(o), ctypes.byref(b))
    assert L.blsw_compact_locate(ctypes.byref(c), 0, 0, *args) == 0 and (r.value, o.value, b.value) == (pkg.COMPACT_TILE, c.off_staging, 0)
    assert pkg.compact_locate(c, c.off_expand + 33, 65) == (pkg.COMPACT_BIT, (c.sha_words * 64 + 16 + 1) * 4, 1)
    assert pkg.compact_locate(c, c.n_witness - 1, 127) == (pkg.COMPACT_PAIR, c.off_pair + (128 * c.pair_rows - 1) * FP, 0)
    r.value, o.value, b.value = 7, 7, 7
    assert L.blsw_compact_locate(None, 0, 0, *args) == BLSW_ERR_ARG
    assert L.blsw_compact_locate(ctypes.byref(c), 0, 0, None, args[1], args[2]) == BLSW_ERR_ARG
    assert L.blsw_compact_locate(ctypes.byref(c), c.n_witness, 0, *args) == BLSW_ERR_ARG
    assert L.blsw_compact_locate(ctypes.byref(c), 0, 128, *args) == BLSW_ERR_ARG
    for field, v in (("n", 100), ("split_row", c.split_row + 1), ("sha_words", c.sha_words - 16 * 700), ("off_pair", c.off_pair - 256), ("total", c.total - 256),
                     ("moved_len", 5), ("staging_rows", c.staging_rows + 1)):
        bad = pkg.blsw_compact_layout_t.from_buffer_copy(c)
        setattr(bad, field, v)
        assert L.blsw_compact_locate(ctypes.byref(bad), 0, 0, *args) == BLSW_ERR_ARG, field
    assert (r.value, o.value, b.value) == (7, 7, 7)  # nothing written on refusal
