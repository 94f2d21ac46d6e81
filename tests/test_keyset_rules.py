"""Shared key sets (options.shared_keys, blsw_keyset_*, ABI 15): the header, the ctypes mirror and every argument rule that is checked on the host
before any HIP call. Runs without a GPU."""
import ctypes
import importlib

import pytest

gen = importlib.import_module("tools.gen_bindings")
H = gen.parse_header()
ERR_ARG = 1
SEG_PK_ALLOC = 1942
NEW = ["blsw_keyset_bytes", "blsw_keyset_create", "blsw_keyset_table", "blsw_keyset_destroy", "blsw_keyset_broadcast_rate", "blsw_engine_submit_aggregate_keyset",
       "blsw_engine_submit_aggregate_keyset_compact", "blsw_engine_expand_compact_keyset"]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bls-verify-gadget_amd")


def options(pkg, **kw):
    o = pkg.blsw_engine_options_t()
    assert pkg.lib().blsw_engine_options_default(ctypes.byref(o)) == 0
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def workspace_bytes(pkg, n, max_steps, n_buffers, **kw):
    b = ctypes.c_uint64(0)
    rc = pkg.lib().blsw_engine_workspace_bytes_ex(n, 32, max_steps, n_buffers, ctypes.byref(options(pkg, **kw)), ctypes.byref(b))
    return rc, b.value


def test_symbols_and_struct(pkg):
    L = pkg.lib()
    assert L.blsw_version() == H["defines"]["BLSW_ABI_VERSION"] >= 15
    params = {name: p for name, _, p in H["functions"]}
    for name in NEW:
        assert name in params and name in pkg.EXPORTED_SYMBOLS
        assert len(getattr(L, name).argtypes) == len(params[name]), name
    assert "blsw_keyset_t" in H["opaque"]
    fields = [f for _, f in H["structs"]["blsw_engine_options_t"]]
    assert fields[-1] == "shared_keys" and fields == [n for n, _ in pkg.blsw_engine_options_t._fields_]
    assert ctypes.sizeof(pkg.blsw_engine_options_t) == 4 * len(fields)
    assert options(pkg).shared_keys == 0 and pkg.engine_options(n_keys=5, shared_keys=1).shared_keys == 1


def test_keyset_bytes(pkg):
    L = pkg.lib()
    b = ctypes.c_uint64(0)
    for K in (1, 5, 512, 65535):
        assert L.blsw_keyset_bytes(K, ctypes.byref(b)) == 0
        assert b.value >= K * SEG_PK_ALLOC * 48 + 3 * K * 48 and b.value % 256 == 0
        assert pkg.keyset_bytes(K) == b.value
    assert L.blsw_keyset_bytes(0, ctypes.byref(b)) == ERR_ARG and L.blsw_keyset_bytes(65536, ctypes.byref(b)) == ERR_ARG
    assert L.blsw_keyset_bytes(5, None) == ERR_ARG


def test_option_refusals(pkg):
    L = pkg.lib()
    e = ctypes.c_void_p()
    ws = ctypes.c_void_p(0x1000)  # never dereferenced: the calls fail before any device work

    def create(n, max_steps, n_buffers, **kw):
        return L.blsw_engine_create_ex(ctypes.byref(e), n, 32, max_steps, n_buffers, ctypes.byref(options(pkg, **kw)), ws, 1 << 50)

    bad = [dict(n_keys=5, shared_keys=2), dict(shared_keys=1), dict(n_keys=5, shared_keys=1, agg_inputs=1), dict(n_keys=5, shared_keys=1, agg_inputs=3),
           dict(n_keys=5, shared_keys=1, agg_inputs=15), dict(n_pairs=4, shared_keys=1), dict(n_keys=5, shared_keys=1, consumer_mode=2)]
    for kw in bad:
        assert create(64, 2, 2, **kw) == ERR_ARG and workspace_bytes(pkg, 64, 2, 2, **kw)[0] == ERR_ARG, kw
    # every mask without the keys, staged and direct engines, consumer mode (staged), both output forms
    for mask in range(0, 16, 2):
        assert workspace_bytes(pkg, 64, 2, 2, n_keys=5, shared_keys=1, agg_inputs=mask)[0] == 0, mask
        assert workspace_bytes(pkg, 64, 1, 1, n_keys=5, shared_keys=1, agg_inputs=mask)[0] == 0, mask
    assert workspace_bytes(pkg, 64, 2, 2, n_keys=5, shared_keys=1, consumer_mode=1, output_form=1)[0] == 0
    assert workspace_bytes(pkg, 64, 1, 1, n_keys=5, shared_keys=1, consumer_mode=1)[0] == ERR_ARG  # as for every direct-mode engine
    assert create(64, 2, 2, n_keys=5, shared_keys=1) != ERR_ARG  # valid: fails later (no device here) or succeeds
    if e.value:
        L.blsw_engine_destroy(e)


def test_workspace_shrinks_by_the_key_rows(pkg):
    n, K, max_steps, n_buffers = 64, 5, 2, 2
    rc0, plain = workspace_bytes(pkg, n, max_steps, n_buffers, n_keys=K)
    rc1, shared = workspace_bytes(pkg, n, max_steps, n_buffers, n_keys=K, shared_keys=1)
    assert rc0 == 0 and rc1 == 0
    assert plain - shared >= n_buffers * max_steps * n * K * SEG_PK_ALLOC * 48
    # direct mode: no staging either way, the projective keys [3][n K] go
    rc0, plain = workspace_bytes(pkg, n, 1, 1, n_keys=K)
    rc1, shared = workspace_bytes(pkg, n, 1, 1, n_keys=K, shared_keys=1)
    assert rc0 == 0 and rc1 == 0 and plain - shared >= 3 * n * K * 48
    # the layout the caller sees does not change
    assert pkg.layout_aggregate(32, K)["n_witness"] == pkg.layout_aggregate(32, K, 1)["n_witness"] + K * SEG_PK_ALLOC


def test_compact_layout_refuses_the_option(pkg):
    L = pkg.lib()
    c = pkg.blsw_compact_layout_t()
    assert L.blsw_compact_layout(64, 32, ctypes.byref(options(pkg, n_keys=5)), ctypes.byref(c)) == 0
    assert L.blsw_compact_layout(64, 32, ctypes.byref(options(pkg, n_keys=5, shared_keys=1)), ctypes.byref(c)) == ERR_ARG
    with pytest.raises(pkg.BlswError):
        pkg.compact_layout(64, 32, n_keys=5, shared_keys=1)


def test_keyset_create_refusals(pkg):
    L = pkg.lib()
    ks = ctypes.c_void_p()
    keys, buf = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000)  # never dereferenced
    need = pkg.keyset_bytes(5)

    def create(out=ctypes.byref(ks), pks=keys, K=5, form=0, d_buffer=buf, nbytes=need):
        return L.blsw_keyset_create(out, pks, K, form, -1, d_buffer, nbytes, None)

    assert create(out=None) == ERR_ARG and create(pks=None) == ERR_ARG and create(K=0) == ERR_ARG and create(K=65536, nbytes=1 << 50) == ERR_ARG
    assert create(d_buffer=None) == ERR_ARG and create(nbytes=need - 1) == ERR_ARG and create(nbytes=0) == ERR_ARG
    assert create(d_buffer=ctypes.c_void_p(0x20000 + 128)) == ERR_ARG and create(d_buffer=ctypes.c_void_p(0x20000 + 16)) == ERR_ARG
    assert create(form=2) == ERR_ARG
    assert ks.value is None
    import torch

    if not torch.cuda.is_available():  # valid arguments: no device to run on (with one, tests/test_keyset_gpu.py creates sets)
        assert create() == 4 and ks.value is None
    p, nel = ctypes.c_void_p(), ctypes.c_uint64(0)
    assert L.blsw_keyset_table(None, ctypes.byref(p), ctypes.byref(nel)) == ERR_ARG and L.blsw_keyset_destroy(None) == ERR_ARG
    r = ctypes.c_double(0)
    assert L.blsw_keyset_broadcast_rate(None, buf, 1 << 20, 4, 0, 1, ctypes.byref(r)) == ERR_ARG


def test_keyset_entry_points_refuse_null_handles(pkg):
    L = pkg.lib()
    p = ctypes.c_void_p(0x10000)
    assert L.blsw_engine_submit_aggregate_keyset(None, p, p, p, p, None, p, 1 << 30, p, p, None) == ERR_ARG
    assert L.blsw_engine_submit_aggregate_keyset_compact(None, p, p, p, p, p, p, p, None) == ERR_ARG
    assert L.blsw_engine_expand_compact_keyset(None, p, p, p, 1 << 30, None) == ERR_ARG
