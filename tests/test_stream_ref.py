"""tests/stream_ref.py held to account on the host, and what of the output layer has a host compilation held to it: the reference's own checks
(R R^-1 = 1, the digest definition on a vector computed by hand, the layout restatement against blsw_compact_locate), the coverage conditions of
the case lists tests/test_stream_device_gpu.py runs, the bounds of every launch it makes, and sha.hpp's host BitSink against plain bit
concatenation. No GPU."""
import importlib

import numpy as np
import pytest

from tests import devstream_lib as D
from tests import stream_ref as S
from tests.field_edges import P

COMPACT_LAYOUTS = S.COMPACT_LAYOUTS


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bls-verify-gadget_amd")


def test_constants():
    assert S.R * S.R_INV % P == 1 and S.R == (1 << 384) % P and 0 < S.R < P
    assert S.to_int(S.element_columns(0)) == S.R and S.to_int(S.element_columns(1)) == 1
    assert S.to_int(S.to_canonical(S.limbs64(S.R))) == 1 and S.to_int(S.to_canonical(S.limbs64(0))) == 0
    t = S.tag_rows(np.arange(70).reshape(-1, 1), np.arange(700).reshape(1, -1))
    assert len({r.tobytes() for r in t.reshape(-1, 6)}) == 70 * 700 and all(S.to_int(r) < P for r in t.reshape(-1, 6)[::997])


def test_digest_definition_by_hand(pkg):
    # two pieces (1, 2, 3, 4) and (0xffffffff, 0, 0x80000000, 7): keys 0x9e3779b1 and 0x3c6ef362; every term written out and summed by hand
    words = [1, 2, 3, 4, 0xFFFFFFFF, 0, 0x80000000, 7]
    want = [0x05669F9A3BB3DA55, 0x07221937 | 0xFFFFFFF9 << 32]
    assert S.digest_int(words) == want
    w64 = np.array(words, dtype=np.uint32).view(np.uint64)
    assert S.digest_many(w64.reshape(1, -1)).tolist() == [want]
    assert pkg.witness_digest_reference(w64) == want
    rng = np.random.default_rng(3)
    v = rng.integers(0, 1 << 63, size=(5, 6 * 37), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    many = S.digest_many(v)
    for i in range(5):
        assert many[i].tolist() == S.digest_int(v[i].view(np.uint32)) == pkg.witness_digest_reference(v[i])
    ones = np.full((1, 6 * 1000), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)  # sums that wrap
    assert S.digest_many(ones)[0].tolist() == S.digest_int(ones[0].view(np.uint32))


def test_bit_word_addressing_round_trip():
    rng = np.random.default_rng(1)
    for sha_bits, first, n_y in ((1, 0, 1), (33, 63, 3), (1025, 5, 65), (511, 70, 3)):
        sha_words = S.carve_sha_words(sha_bits)
        assert sha_words % 16 == 0 and 32 * (sha_words - 1) >= sha_bits
        streams = rng.integers(0, 2, size=(n_y, sha_bits), dtype=np.uint8)
        buf = S.pack_streams(streams, first, sha_words, rng)
        assert buf.size == (first + n_y + 63) // 64 * sha_words * 64
        for y in range(n_y):
            assert np.array_equal(S.unpack_stream(buf, first + y, sha_words, sha_bits), streams[y])
            pad = S.unpack_stream(buf, first + y, sha_words, 32 * sha_words)[sha_bits:]
            assert pad.all()
    idx = {S.word_index(lane, w, 32) for lane in range(128) for w in range(32)}
    assert idx == set(range(128 * 32))  # the addressing is a bijection onto the buffer


@pytest.mark.parametrize("variant,store", S.KERNELS)
def test_expansion_cases_cover_the_geometry(variant, store):
    cases = S.expand_cases(variant, store)
    W, A = S.GEOMETRY[variant]
    assert {c["sha_bits"] for c in cases} >= set(S.expand_sizes(variant)) and {c["canonical"] for c in cases} == {0, 1}
    assert {c["n_y"] for c in cases} >= {1, 3, 65} and {c["first"] for c in cases} == {0, 5, 63, 70} and {c["K"] for c in cases} == {1, 3}
    assert all(c["stride"] % 2 == 1 and c["sha_words"] == S.carve_sha_words(c["sha_bits"]) for c in cases)
    assert any(c["K"] == 3 and c["stride_hash"] > c["sha_bits"] and c["n_y"] > 1 for c in cases)
    assert any((c["first"] + c["n_y"] - 1) >> 6 > c["first"] >> 6 for c in cases)  # the lanes of one launch cross a tile border
    residues = {3 * c["off_expand"] % A for c in cases}
    assert residues >= set(S.expand_residues(variant))
    shapes = [(c, S.segment_shape(c, start)) for c in cases for _, _, start in S.segments(c)]
    p0 = {s["P0"] for _, s in shapes}
    assert 0 in p0 and A - 1 in p0 and (A > 16 or p0 == set(range(16)))
    assert any(s["last_pieces"] == 1 for _, s in shapes), "no last workgroup of exactly one piece"
    assert any(s["last_pieces"] == W for _, s in shapes), "no last workgroup that ends exactly at the segment's end"
    assert any(s["spare_empty"] for _, s in shapes) and any(s["head_only"] for _, s in shapes)
    assert any(c["sha_bits"] == 1 and s["P0"] >= 4 for c, s in shapes)  # one bit behind a longer head: the head's own bound
    patterns = {S.PATTERNS[(c["pattern0"] + y) % len(S.PATTERNS)] for c in cases for y in range(c["n_y"])}
    assert patterns == set(S.PATTERNS)
    if variant in S.SCALAR_WORD_VARIANTS:
        hits = [(c, S.clamped_waves(c, start)) for c in cases for _, _, start in S.segments(c)]
        assert any(h for _, h in hits), "no wave whose second bit word is the clamped last word"
        assert any(any(bx < S.segment_shape(c, 0)["grid_x"] - 1 for bx, _, _ in h) for c, h in hits)  # and not only in the spare workgroup
    if variant == 13:
        assert any(S.segment_shape(c, 0)["grid_x"] * c["n_y"] > S.RESIDENT_WGS for c in cases)


@pytest.mark.parametrize("variant,store", S.KERNELS)
def test_expansion_launches_stay_inside_their_buffers(variant, store):
    """no case can leave its allocation whatever the kernel does right: every segment lies inside its instance's stride, every lane has its tile,
    and a workgroup that runs one whole span past either end of the written range is still inside the guards"""
    W, _ = S.GEOMETRY[variant]
    assert D.GUARD >= W + 1024
    for c in S.expand_cases(variant, store):
        assert c["sha_bits"] >= 1 and c["n_y"] <= 65535
        n_inst = S.n_instances(c)
        for y, lane, start in S.segments(c):
            assert 0 <= start and start + 3 * c["sha_bits"] <= 3 * n_inst * c["stride"]
        streams = S.expand_streams(c)
        buf = S.pack_streams(streams, c["first"], c["sha_words"], np.random.default_rng(0))
        assert buf.size >= ((c["first"] + c["n_y"] - 1) >> 6) * c["sha_words"] * 64 + c["sha_words"] * 64
        idx, vals = S.expand_expected(c, streams)
        assert len(np.unique(idx)) == idx.size == vals.shape[0]  # the segments of one launch do not overlap


def test_staged_row_rule_is_a_bijection():
    for off_expand, sha_bits, rows, moved_lo, moved_len in ((0, 5, 9, 0, 0), (4, 3, 10, 0, 0), (10, 7, 10, 0, 0), (6, 4, 12, 1, 3), (6, 4, 12, 0, 6), (12, 2, 12, 9, 3)):
        moved_at = rows - moved_len if moved_len else 0
        n_witness = rows + sha_bits
        vec = S.staged_rows(n_witness, off_expand, sha_bits, moved_lo, moved_len, moved_at)
        one = [S.staged_row(k, off_expand, sha_bits, moved_lo, moved_len, moved_at) for k in range(n_witness)]
        assert [(-1 if r is None else r) for r in one] == vec.tolist()
        assert sorted(r for r in one if r is not None) == list(range(rows)) and one.count(None) == sha_bits


@pytest.mark.parametrize("name", list(COMPACT_LAYOUTS))
def test_layout_restatement_equals_compact_locate(pkg, name):
    c = pkg.compact_layout(64, 32, **{k: v for k, v in COMPACT_LAYOUTS[name].items() if k != "output_form"})
    assert (c.moved_len > 0) == (name == "g2_team")
    for lane in (0, 63):
        region, off, bit = pkg.compact_locate_all(c, lane)
        r2, o2, b2 = S.compact_locate_all(c, lane)
        assert np.array_equal(region, r2) and np.array_equal(off, o2) and np.array_equal(bit, b2)
        for k in (0, c.off_expand - 1, c.off_expand, c.off_expand + c.sha_bits - 1, c.off_expand + c.sha_bits, c.n_witness - 1, c.moved_lo, c.moved_lo + max(c.moved_len, 1) - 1):
            assert S.compact_locate(c, k, lane) == (int(region[k]), int(off[k]), int(bit[k]))


@pytest.mark.parametrize("rows", S.PLACE_FIELD_ROWS)
def test_place_field_cases_are_layouts_the_library_accepts(rows):
    cases = S.place_field_cases(rows)
    assert {c["n_inst"] for c in cases} >= {1, 3} and {c["first"] for c in cases} == {0, 5} and {c["split_row"] for c in cases} >= {0, rows}
    assert {c["off_expand"] for c in cases} >= {0, rows} and any(c["moved_len"] for c in cases)
    for c in cases:  # compact_layout_ok's conditions on the fields this kernel reads
        assert c["split_row"] <= c["staging_rows"] and c["off_expand"] <= c["staging_rows"]
        if c["moved_len"]:
            assert c["moved_at"] == c["staging_rows"] - c["moved_len"] and c["moved_lo"] + c["moved_len"] <= c["off_expand"]
        mask, vals = S.place_field_expected(c)
        assert mask.sum() == c["staging_rows"] and c["stride"] >= c["staging_rows"] + c["sha_bits"]
        got = {v.tobytes() for v in vals[0][mask]}
        assert len(got) == c["staging_rows"]  # every staged row exactly once
    if rows <= 683:
        assert {c["n_inst"] for c in cases} == {1, 3, 64, 70}


def test_place_runs_and_canonical_cases():
    cases = S.place_runs_cases()
    assert {c["n_runs"] for c in cases} == {1, 2, 6} and {c["K"] for c in cases} == {1, 3} and {c["tile_w"] for c in cases} == {64, 16}
    for c in cases:
        mask, vals = S.place_runs_expected(c)  # (asserts that no two runs overlap)
        assert mask.sum() == c["n_y"] * c["rows"] and S.place_runs_sources(c).shape[0] * c["tile_w"] >= c["first"] + c["n_y"]
    cc = S.canonical_cases()
    assert {c["K"] for c in cc} == {1, 3}
    for c in cc:
        m = S.canonical_field_mask(c)
        assert m.sum() == c["n_witness"] - c["K"] * c["sha_bits"] and (c["K"] == 1 or c["stride_hash"] > c["sha_bits"])
        assert c["off_expand"] + (c["K"] * c["stride_hash"] if c["K"] > 1 else c["sha_bits"]) <= c["n_witness"]


@pytest.mark.parametrize("name", list(S.sink_scripts()))
def test_host_bit_sink_is_plain_concatenation(name):
    script = S.sink_scripts()[name]
    data = S.sink_data(script, 2, seed=len(name))
    for lane in range(2):
        d = data[lane, :len(script)].tolist()
        words, nbits = S.concat_bits(script, d)
        got, got_bits, behind = D.host_sink(script, d)
        assert got_bits == nbits == sum(n if op == 0 else 32 for op, n in script)
        assert got == words and all(v == 0xA5A5A5A5 for v in behind)


def test_sink_scripts_cover_every_fill_and_run_shape():
    scripts = S.sink_scripts()
    seen, seen32 = set(), set()
    for script in scripts.values():
        fill = 0
        for op, n in script:
            (seen if op == 0 else seen32).add((fill, n))
            fill = (fill + n) % 32
    assert seen >= {(f, n) for f in range(32) for n in range(1, 33)} and seen32 >= {(f, 32) for f in range(32)}
    n_words = {(sum(n for _, n in s) + 31) // 32 for s in scripts.values()}
    assert n_words >= {0, 1, 15, 16, 17, 31, 32, 33} and any(w % 16 == 0 and w for w in n_words) and any(w % 16 for w in n_words)
    assert {sum(n for _, n in s) for s in scripts.values()} >= {511, 512, 513, 1023, 1024, 1025}
