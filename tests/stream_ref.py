"""A plain reference of the output layer (csrc/k_stream.hip: bit expansion, placement, canonical form, digest; sha.hpp's BitSink), and the cases
tests/test_stream_ref.py validates on the host and tests/test_stream_device_gpu.py runs on the device.

numpy and Python integers. Nothing here is copied from csrc/: R = 2^384 mod p and R^-1 come from pow, and every rule is restated from the text of
include/blsw.h —
  bit words    [tile][word / 16][lane][word % 16] u32: bit b of a lane's stream is bit b & 31 of its word b / 32
  pieces       element off_expand + pair * stride_hash + b of an instance = bit ? R : 0 (canonical form: bit ? 1 : 0)
  staged rows  the witness vector with the SHA segment cut out; a moved segment (moved_len witnesses from moved_lo on) is staged last, from row
               moved_at on; rows below split_row live in 64-lane tiles [tile][row][64], the others instance-major [lane][row - split_row]
  runs         staged rows [src_row[r], src_row[r + 1]) of a lane go to dst_off[r] + pair * dst_stride[r] of its instance
  canonical    every element of a vector outside its K SHA segments is x R^-1 mod p
  digest       the two sums of blsw_witness_digest
The geometry of a workgroup (pieces per workgroup, alignment of its first piece) enters only the CHOICE of cases and the coverage conditions, never
an expected value."""
import random

import numpy as np

from tests.field_edges import P

R = pow(2, 384, P)
R_INV = pow(R, -1, P)
CHUNK_WORDS = 16  # words of one 64-byte run
M32 = 0xFFFFFFFF


def limbs32(v):
    return np.frombuffer(int(v).to_bytes(48, "little"), dtype=np.uint32).copy()


def limbs64(v):
    return np.frombuffer(int(v).to_bytes(48, "little"), dtype=np.uint64).copy()


def to_int(a):
    return int.from_bytes(np.ascontiguousarray(a).tobytes(), "little")


def align_up(x, a):
    return (x + a - 1) // a * a


def carve_sha_words(sha_bits):
    """words of a lane's stream as the workspace carves them: one spare word, whole 64-byte runs"""
    return align_up((sha_bits + 31) // 32 + 1, CHUNK_WORDS)


# ---------------------------------------------------------------- bit words
def word_index(lane, w, sha_words):
    """u32 index of word w of `lane`'s stream in a bit-word buffer"""
    return (lane >> 6) * sha_words * 64 + (w // CHUNK_WORDS) * (64 * CHUNK_WORDS) + (lane & 63) * CHUNK_WORDS + w % CHUNK_WORDS


def pack_streams(streams, first, sha_words, rng):
    """streams [n_y][sha_bits] of 0 / 1 for lanes first .. first + n_y -> the u32 buffer of every tile those lanes touch. Pad bits of these
    lanes (from sha_bits to 32 * sha_words) are ONE; the other lanes of the tiles hold random words."""
    streams = np.asarray(streams, dtype=np.uint8)
    n_y, sha_bits = streams.shape
    tiles = (first + n_y + 63) // 64
    buf = rng.integers(0, 1 << 32, size=(tiles, sha_words // CHUNK_WORDS, 64, CHUNK_WORDS), dtype=np.uint64).astype(np.uint32)
    full = np.ones((n_y, 32 * sha_words), dtype=np.uint8)
    full[:, :sha_bits] = streams
    words = np.packbits(full, axis=1, bitorder="little").view(np.uint32).reshape(n_y, sha_words // CHUNK_WORDS, CHUNK_WORDS)
    for y in range(n_y):
        lane = first + y
        buf[lane >> 6, :, lane & 63, :] = words[y]
    return buf.reshape(-1)


def unpack_stream(buf, lane, sha_words, sha_bits):
    """the inverse, by word_index: bits [sha_bits] of one lane"""
    idx = np.array([word_index(lane, w, sha_words) for w in range((sha_bits + 31) // 32)], dtype=np.int64)
    return np.unpackbits(np.asarray(buf, dtype=np.uint32)[idx].view(np.uint8), bitorder="little")[:sha_bits]


def element_columns(canonical):
    """the three 16-byte pieces of the element a ONE bit expands to, [3][4] u32"""
    return limbs32(1 if canonical else R).reshape(3, 4)


PATTERNS = ("ones", "zeros", "alternating", "first", "last", "random")


def pattern_bits(name, sha_bits, rng):
    b = np.zeros(sha_bits, dtype=np.uint8)
    if name == "ones":
        b[:] = 1
    elif name == "alternating":
        b[::2] = 1
    elif name == "first":
        b[0] = 1
    elif name == "last":
        b[-1] = 1
    elif name == "random":
        b[:] = rng.integers(0, 2, size=sha_bits, dtype=np.uint8)
    return b


# ---------------------------------------------------------------- expansion cases
# expand_variant -> (pieces a workgroup writes behind the head, alignment of its first piece in pieces): restated from the comments of kcommon.hpp
# and k_stream.hip. Used to choose cases and to state what they cover.
GEOMETRY = {0: (384 * 8, 16), 1: (256, 256), 2: (768 * 8, 256), 3: (768 * 4, 256), 4: (768 * 16, 256), 5: (384 * 16, 256), 6: (512, 512), 7: (1024, 1024),
            8: (384 * 8, 16), 9: (384 * 4, 16), 10: (384 * 8, 16), 11: (384 * 16, 16), 12: (384 * 32, 16), 13: (384 * 8, 16)}
SCALAR_WORD_VARIANTS = {8: 8, 9: 4, 10: 8, 11: 16, 12: 32}  # bit words in scalar registers, clamped to the stream's last word: variant -> iterations
KERNELS = [(v, 0) for v in range(14)] + [(0, 1), (0, 2), (0, 3)]  # (expand_variant, expand_store)
RESIDENT_WGS = 512
ORIGIN_ALIGN = 1024  # pieces: the device test puts piece 0 of instance 0's vector on a 16 KiB boundary, the largest alignment of any variant


def elements_per_wg(variant):
    return -(-GEOMETRY[variant][0] // 3)


def expand_sizes(variant):
    E = elements_per_wg(variant)
    return sorted({1, 2, 31, 32, 33, 127, 128, 129, E - 1, E, E + 1, 2 * E - 21, 2 * E + 1, 3 * E + 37})


def expand_residues(variant):
    A = GEOMETRY[variant][1]
    return list(range(16)) if A == 16 else [0, 1, 2, A - 2, A - 1, A // 2 - 3, A // 3]


def _expand_case(variant, store, sha_bits, residue, rng, n_y=None, first=None, K=None):
    A = GEOMETRY[variant][1]
    inv3 = pow(3, -1, A)
    if n_y is None:
        n_y = rng.choice((1, 3, 65) if sha_bits <= elements_per_wg(variant) + 1 else (1, 3))  # (65 lanes cross a tile border at any size)
    first = rng.choice((0, 5, 63, 70)) if first is None else first
    K = rng.choice((1, 3)) if K is None else K
    stride_hash = sha_bits + rng.randrange(1, 40) if K > 1 else 0
    off_expand = residue * inv3 % A + A * rng.randrange(2)  # 3 * off_expand = residue mod A
    stride = off_expand + (K - 1) * stride_hash + sha_bits + rng.randrange(0, 30)
    stride += 1 - stride % 2  # odd: the instances of one launch differ in their first piece's alignment
    return dict(variant=variant, store=store, sha_bits=sha_bits, sha_words=carve_sha_words(sha_bits), off_expand=off_expand, stride=stride, n_y=n_y, first=first, K=K,
                stride_hash=stride_hash, canonical=rng.randrange(2), pattern0=rng.randrange(len(PATTERNS)), seed=rng.randrange(1 << 30))


def segments(c):
    """[(y, lane, first piece of the segment counted from piece 0 of instance 0)] of a case"""
    out = []
    for y in range(c["n_y"]):
        inst, pair = (y, 0) if c["K"] == 1 else divmod(y, c["K"])
        out.append((y, c["first"] + y, 3 * (inst * c["stride"] + c["off_expand"] + pair * c["stride_hash"])))
    return out


def n_instances(c):
    return -(-c["n_y"] // c["K"])


def segment_shape(c, start):
    """What the geometry makes of a segment that starts at piece `start`: P0 pieces in front of the first boundary, the workgroups of the grid, the
    piece count of the last workgroup that has any, whether the grid's spare workgroup is empty."""
    W, A = GEOMETRY[c["variant"]]
    n_pieces = 3 * c["sha_bits"]
    P0 = (A - start % A) % A
    grid_x = -(-n_pieces // W) + 1
    body = max(0, n_pieces - P0)
    last = 0 if body == 0 else (body - 1) % W + 1
    spare_empty = P0 + (grid_x - 1) * W >= n_pieces
    return dict(P0=P0, grid_x=grid_x, last_pieces=last, per_wg=W, spare_empty=spare_empty, head_only=body == 0)


def clamped_waves(c, start):
    """scalar-word variants: the (workgroup, wave, iteration) triples whose SECOND bit word index reaches the stream's last word or lies beyond it"""
    iters = SCALAR_WORD_VARIANTS[c["variant"]]
    sh = segment_shape(c, start)
    w_last = c["sha_words"] - 1
    hits = []
    for bx in range(sh["grid_x"]):
        for wave in range(6):
            e_first = bx * 128 * iters + (sh["P0"] + 64 * wave) // 3
            hits += [(bx, wave, k) for k in range(iters) if (e_first >> 5) + 4 * k + 1 >= w_last]
    return hits


_CASES = {}


def expand_cases(variant, store=0):
    """The launches of one kernel: every size with every start residue, the other parameters drawn so that each value occurs (asserted by
    test_stream_ref.py); then the launches that make a last workgroup of exactly one piece and of all its pieces at this geometry, and for the
    resident grid one launch of more blocks than resident workgroups."""
    if (variant, store) in _CASES:
        return _CASES[(variant, store)]
    rng = random.Random(1000 * variant + store)
    W, A = GEOMETRY[variant]
    cases = [_expand_case(variant, store, s, r, rng) for s in expand_sizes(variant) for r in expand_residues(variant)]
    cases.append(_expand_case(variant, store, 1, 4 % A, rng, n_y=1, K=1))  # one bit behind a head of A - 4 >= 4 pieces: the head's own bound
    for want in (1, W):  # 3 sha_bits - P0 = want (mod W): the two smallest heads that allow it, with K = 1 and one instance
        found = [(body + P0) // 3 for P0 in range(A) for body in (want, want + W) if (body + P0) % 3 == 0][:2]
        cases += [_expand_case(variant, store, s, (A - (3 * s - want) % W % A) % A, rng, n_y=1, K=1) for s in found]
    if variant == 13:
        cases.append(_expand_case(variant, store, 1025, 5, rng, n_y=200, first=5, K=1))  # 3 x 200 blocks walked by 512 workgroups
    _CASES[(variant, store)] = cases
    return cases


def expand_streams(c):
    """bits [n_y][sha_bits] of a case: the patterns in turn over the lanes, starting at the case's own"""
    rng = np.random.default_rng(c["seed"])
    return np.stack([pattern_bits(PATTERNS[(c["pattern0"] + y) % len(PATTERNS)], c["sha_bits"], rng) for y in range(c["n_y"])])


def expand_expected(c, streams):
    """-> (piece indices [n_y * 3 sha_bits] counted from piece 0 of instance 0, pieces [n_y * 3 sha_bits][4] u32) of everything the launch writes"""
    cols = element_columns(c["canonical"])
    n = 3 * c["sha_bits"]
    idx = np.concatenate([start + np.arange(n, dtype=np.int64) for _, _, start in segments(c)])
    vals = (np.asarray(streams, dtype=np.uint32)[:, :, None, None] * cols[None, None]).reshape(-1, 4)
    return idx, vals


# ---------------------------------------------------------------- tagged rows
def tag_rows(lane, row, kind=0):
    """[..., 6] u64 elements, distinct for every (lane, row, kind) and below p (the top limb is 1): broadcasting over lane and row"""
    lane, row = np.broadcast_arrays(np.asarray(lane, dtype=np.uint64), np.asarray(row, dtype=np.uint64))
    out = np.empty(lane.shape + (6,), dtype=np.uint64)
    out[..., 0] = row | (lane << np.uint64(32))
    out[..., 1] = (row * np.uint64(0x9E3779B97F4A7C15)) ^ lane
    out[..., 2] = lane * np.uint64(1000003) + row
    out[..., 3] = np.uint64(kind) + np.uint64(0x5151515100000000)
    out[..., 4] = ~row
    out[..., 5] = 1
    return out


def staged_row(k, off_expand, sha_bits, moved_lo=0, moved_len=0, moved_at=0):
    """witness index -> staged row (None for a witness of the SHA segment): the header's rule, witness by witness"""
    if off_expand <= k < off_expand + sha_bits:
        return None
    if moved_len and moved_lo <= k < moved_lo + moved_len:
        return moved_at + (k - moved_lo)
    row = k if k < off_expand else k - sha_bits
    if moved_len and k >= moved_lo + moved_len:
        row -= moved_len  # the moved segment lies in front of the SHA segment and is not among the rows in front of this one
    return row


def staged_rows(n_witness, off_expand, sha_bits, moved_lo=0, moved_len=0, moved_at=0):
    """staged_row of every witness index, vectorised: int64 [n_witness], -1 inside the SHA segment"""
    k = np.arange(n_witness, dtype=np.int64)
    row = np.where(k < off_expand, k, k - sha_bits)
    if moved_len:
        row = np.where(k >= moved_lo + moved_len, row - moved_len, row)
        row = np.where((k >= moved_lo) & (k < moved_lo + moved_len), moved_at + (k - moved_lo), row)
    return np.where((k >= off_expand) & (k < off_expand + sha_bits), -1, row)


def compact_locate(c, k, lane):
    """blsw_compact_locate restated from the header's description of the three regions; c = any object with blsw_compact_layout_t's fields
    -> (region 0 bit / 1 tile / 2 pair, byte offset, bit)"""
    row = staged_row(k, c.off_expand, c.sha_bits, c.moved_lo, c.moved_len, c.moved_at)
    if row is None:
        b = k - c.off_expand
        return 0, 4 * word_index(lane, b // 32, c.sha_words), b % 32
    if row < c.split_row:
        return 1, c.off_staging + 48 * (((lane >> 6) * c.split_row + row) * 64 + (lane & 63)), 0
    return 2, c.off_pair + 48 * (lane * c.pair_rows + (row - c.split_row)), 0


def compact_locate_all(c, lane):
    """compact_locate of every witness index, vectorised -> (region, byte offset, bit)"""
    k = np.arange(c.n_witness, dtype=np.int64)
    row = staged_rows(c.n_witness, c.off_expand, c.sha_bits, c.moved_lo, c.moved_len, c.moved_at)
    b = np.clip(k - c.off_expand, 0, None)
    w = b // 32
    off_bit = 4 * ((lane >> 6) * c.sha_words * 64 + (w // CHUNK_WORDS) * (64 * CHUNK_WORDS) + (lane & 63) * CHUNK_WORDS + w % CHUNK_WORDS)
    off_tile = c.off_staging + 48 * (((lane >> 6) * c.split_row + row) * 64 + (lane & 63))
    off_pair = c.off_pair + 48 * (lane * c.pair_rows + (row - c.split_row))
    region = np.where(row < 0, 0, np.where(row < c.split_row, 1, 2))
    off = np.where(row < 0, off_bit, np.where(row < c.split_row, off_tile, off_pair))
    return region.astype(np.uint8), off.astype(np.int64), np.where(row < 0, b % 32, 0).astype(np.uint8)


# the engines whose compact steps the device test builds by hand (options of WitnessEngine): n = 64, msg_len = 32
COMPACT_LAYOUTS = {"default": dict(), "g2_team": dict(g2_mode="team"), "aggregate_3": dict(n_keys=3), "canonical": dict(output_form=1)}
PLACE_ITERS = 8  # 256 * 8 pieces per workgroup of the placement kernels: 682.67 rows


def place_field_cases(staging_rows):
    """[dict] for one row count: split_row and off_expand at 0, a middle value and staging_rows; with and without a moved segment (wherever
    moved_lo + moved_len <= off_expand leaves room for one); n_inst 1, 3, 64, 70; first 0 and 5; two lengths of the cut-out segment"""
    rng = random.Random(staging_rows)
    mids = sorted({0, staging_rows // 3, staging_rows})
    cases = []
    for split_row in mids:
        for off_expand in sorted({0, (2 * staging_rows) // 5, staging_rows}):
            for moved in (0, 1):
                if moved and off_expand == 0:
                    continue
                moved_len = min(off_expand, 1 + staging_rows // 7) if moved else 0
                moved_lo = (off_expand - moved_len) // 2 if moved else 0
                for n_inst in (1, 3, 64, 70):
                    if staging_rows > 1000 and n_inst > 3:
                        continue
                    for first in (0, 5):
                        sha_bits = rng.choice((7, 100))
                        cases.append(dict(staging_rows=staging_rows, split_row=split_row, off_expand=off_expand, sha_bits=sha_bits, moved_lo=moved_lo, moved_len=moved_len,
                                          moved_at=staging_rows - moved_len if moved else 0, n_inst=n_inst, first=first, stride=staging_rows + sha_bits + 5))
    return cases


PLACE_FIELD_ROWS = (1, 2, 85, 86, 682, 683, 5462)  # 683 rows are 2 049 pieces (a second workgroup of one piece); 5 462 rows need a ninth workgroup: a second round over the XCDs


def place_field_sources(c):
    """-> (tiles [n_tiles][split_row][64][6], pair rows [n_lanes][pair_rows][6]) of every lane of the tiles the launch touches"""
    n_lanes = align_up(c["first"] + c["n_inst"], 64)
    lanes = np.arange(n_lanes, dtype=np.uint64)
    rows_t = np.arange(c["split_row"], dtype=np.uint64)
    tiles = tag_rows(lanes.reshape(-1, 1, 64), rows_t.reshape(1, -1, 1))
    rows_p = np.arange(c["split_row"], c["staging_rows"], dtype=np.uint64)
    pair = tag_rows(lanes.reshape(-1, 1), rows_p.reshape(1, -1))
    return tiles, pair


def place_field_expected(c):
    """-> (mask [stride] of the elements the launch writes, values [n_inst][stride][6])"""
    n_witness = c["staging_rows"] + c["sha_bits"]
    row = staged_rows(n_witness, c["off_expand"], c["sha_bits"], c["moved_lo"], c["moved_len"], c["moved_at"])
    mask = np.zeros(c["stride"], dtype=bool)
    mask[:n_witness] = row >= 0
    lanes = c["first"] + np.arange(c["n_inst"], dtype=np.uint64)
    vals = np.zeros((c["n_inst"], c["stride"], 6), dtype=np.uint64)
    vals[:, :n_witness] = tag_rows(lanes.reshape(-1, 1), np.where(row >= 0, row, 0).astype(np.uint64).reshape(1, -1))
    return mask, vals


def place_runs_cases():
    """k_place_runs: 1, 2 and 6 runs, K 1 and 3, tiles 64 and 16 lanes wide, row counts on both sides of a workgroup's 2 048 pieces; the runs'
    targets lie in another order than their sources, with gaps, and a pair's copies dst_stride apart"""
    cases = []
    for n_runs in (1, 2, 6):
        for K in (1, 3):
            for tile_w in (64, 16):
                for rows, n_y, first in ((40, 7, 0), (683, 21, 5), (700, 66, 60), (6, 3, 14)):
                    if rows < n_runs:
                        continue
                    rng = random.Random(n_runs * 1000 + K * 100 + tile_w + rows)
                    cuts = sorted(rng.sample(range(1, rows), n_runs - 1))
                    src_row = [0] + cuts + [rows]
                    lens = [src_row[r + 1] - src_row[r] for r in range(n_runs)]
                    order = list(range(n_runs))
                    rng.shuffle(order)
                    dst_off, dst_stride, cursor = [0] * 6, [0] * 6, rng.randrange(4)
                    for r in order:
                        dst_stride[r] = lens[r] + rng.randrange(3)
                        dst_off[r] = cursor
                        cursor += K * dst_stride[r] + rng.randrange(5)
                    cases.append(dict(n_runs=n_runs, K=K, tile_w=tile_w, rows=rows, n_y=n_y, first=first, src_row=src_row + [0] * (7 - len(src_row)), dst_off=dst_off,
                                      dst_stride=dst_stride, stride=cursor + 5))
    return cases


def place_runs_sources(c):
    n_lanes = align_up(c["first"] + c["n_y"], c["tile_w"])
    lanes = np.arange(n_lanes, dtype=np.uint64).reshape(-1, 1, c["tile_w"])
    return tag_rows(lanes, np.arange(c["rows"], dtype=np.uint64).reshape(1, -1, 1), kind=1)


def place_runs_expected(c):
    n_inst = -(-c["n_y"] // c["K"])
    mask = np.zeros((n_inst, c["stride"]), dtype=bool)
    vals = np.zeros((n_inst, c["stride"], 6), dtype=np.uint64)
    for y in range(c["n_y"]):
        inst, j = divmod(y, c["K"])
        for r in range(c["n_runs"]):
            lo, hi = c["src_row"][r], c["src_row"][r + 1]
            d = c["dst_off"][r] + j * c["dst_stride"][r]
            assert not mask[inst, d:d + hi - lo].any()
            mask[inst, d:d + hi - lo] = True
            vals[inst, d:d + hi - lo] = tag_rows(c["first"] + y, np.arange(lo, hi, dtype=np.uint64), kind=1)
    return mask, vals


def canonical_cases():
    """k_canonical_rows: [dict(n_witness, off_expand, sha_bits, K, stride_hash, n, stride)] — K = 1 and K = 3, segments at the front, in the middle and
    at the very end of the vector, a hash tail of one row, row counts on both sides of a workgroup's 256"""
    cases = []
    for K, off_expand, sha_bits, tail, behind, n in ((1, 0, 9, 0, 300, 2), (1, 250, 33, 0, 10, 3), (1, 256, 1, 0, 0, 1), (1, 40, 64, 0, 216, 2), (3, 0, 5, 1, 7, 2),
                                                     (3, 100, 31, 60, 0, 3), (3, 255, 16, 90, 300, 1), (3, 7, 40, 249, 1, 2)):
        stride_hash = sha_bits + tail if K > 1 else 0
        n_witness = off_expand + (K * stride_hash if K > 1 else sha_bits) + behind
        cases.append(dict(K=K, off_expand=off_expand, sha_bits=sha_bits, stride_hash=stride_hash, n_witness=n_witness, n=n, stride=n_witness + 3))
    return cases


def canonical_field_mask(c):
    """[n_witness] True where the element is a field row (outside the K SHA segments)"""
    m = np.ones(c["n_witness"], dtype=bool)
    for j in range(c["K"]):
        lo = c["off_expand"] + j * c["stride_hash"]
        m[lo:lo + c["sha_bits"]] = False
    return m


def to_canonical(elems):
    """[..., 6] u64 stored integers -> x R^-1 mod p, element by element with Python integers"""
    flat = np.ascontiguousarray(elems, dtype=np.uint64).reshape(-1, 6)
    out = np.empty_like(flat)
    for i in range(flat.shape[0]):
        out[i] = limbs64(to_int(flat[i]) * R_INV % P)
    return out.reshape(np.shape(elems))


# ---------------------------------------------------------------- the bit sink
def concat_bits(script, data):
    """[(op, n)], data words -> (words, nbits) of the plain concatenation: op 0 appends the low n bits of its word, op 1 all 32; the last word is
    filled with zeros"""
    acc, nbits = 0, 0
    for (op, n), d in zip(script, data):
        n = n if op == 0 else 32
        assert 1 <= n <= 32 and 0 <= d < (1 << n)
        acc |= int(d) << nbits
        nbits += n
    n_words = (nbits + 31) // 32
    return [(acc >> (32 * i)) & M32 for i in range(n_words)], nbits


def sink_scripts():
    """{name: [(op, n)]}"""
    s = {}
    every = []
    for fill in range(32):
        for n in range(1, 33):
            step = ([(0, fill)] if fill else []) + [(0, n)]
            rest = -(fill + n) % 32
            every += step + ([(0, rest)] if rest else [])  # back to a word border
    s["every n at every fill"] = every
    p32 = []
    for fill in range(32):
        p32 += ([(0, fill)] if fill else []) + [(1, 32)] + ([(0, 32 - fill)] if fill else [])
    s["push32 at every fill"] = p32
    for words in (0, 1, 15, 16, 17, 31, 32, 33):
        s["%d words" % words] = [(1, 32)] * words
    rng = random.Random(0x51)
    for bits in (511, 512, 513, 1023, 1024, 1025, 31, 33):
        script, left = [], bits
        while left:
            n = min(left, rng.randrange(1, 33))
            script.append((0, n))
            left -= n
        s["%d bits" % bits] = script
    return s


def sink_data(script, n_lanes, seed):
    """per-lane data words [n_lanes][max(1, n_ops)] u32, the bits above an entry's n zero"""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 1 << 32, size=(n_lanes, max(1, len(script))), dtype=np.uint64)
    for i, (op, n) in enumerate(script):
        if op == 0:
            d[:, i] &= np.uint64((1 << n) - 1)
    return d.astype(np.uint32)


# ---------------------------------------------------------------- the digest
DIGEST_KEY = 0x9E3779B1
DIGEST_A = 0x85EBCA6B


def digest_int(words32):
    """the definition with Python integers: words32 = the vector's little-endian u32 words -> [d0, d1]"""
    d0 = lo = hi = 0
    for q in range(len(words32) // 4):
        x = [int(v) for v in words32[4 * q:4 * q + 4]]
        key = (q + 1) * DIGEST_KEY & M32
        t = [(x[i] + key + i * DIGEST_A) & M32 for i in range(4)]
        d0 = (d0 + t[0] * t[1] + t[2] * t[3]) & 0xFFFFFFFFFFFFFFFF
        lo = (lo + (x[0] ^ key) + (x[2] ^ (~key & M32))) & M32
        hi = (hi + (x[1] ^ key) + (x[3] ^ (~key & M32))) & M32
    return [d0, lo | hi << 32]


def digest_many(words64):
    """the same for [n][n_witness * 6] u64 -> uint64 [n][2], with numpy's wrapping unsigned arithmetic"""
    x = np.ascontiguousarray(words64, dtype=np.uint64)
    n = x.shape[0]
    x = x.reshape(n, -1).view(np.uint32).reshape(n, -1, 4)
    with np.errstate(over="ignore"):
        key = (np.arange(1, x.shape[1] + 1, dtype=np.uint64) * np.uint64(DIGEST_KEY)).astype(np.uint32)[None, :]
        t = [x[:, :, i] + key + np.uint32(i * DIGEST_A & M32) for i in range(4)]
        d0 = (t[0].astype(np.uint64) * t[1].astype(np.uint64) + t[2].astype(np.uint64) * t[3].astype(np.uint64)).sum(axis=1, dtype=np.uint64)
        lo = ((x[:, :, 0] ^ key) + (x[:, :, 2] ^ ~key)).sum(axis=1, dtype=np.uint32)
        hi = ((x[:, :, 1] ^ key) + (x[:, :, 3] ^ ~key)).sum(axis=1, dtype=np.uint32)
    return np.stack([d0, lo.astype(np.uint64) | (hi.astype(np.uint64) << np.uint64(32))], axis=1)


DIGEST_CHUNK = 16 * 256  # pieces a workgroup of the digest kernel takes at a time (a vector has 3 n_witness pieces)
DIGEST_MAX_WGS = 4096    # workgroups per instance: beyond 4096 chunks a workgroup walks several
