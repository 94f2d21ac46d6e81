"""ctypes loader for tests/msm/libmsm.so — the stages of blsw_msm_points_batch (csrc/vmsm.hpp) compiled for the host (TEST HARNESS ONLY), with the
scatter's lane order as a parameter — and the bucket-edge lists that the CPU and the GPU tests share. The reference is tests/combine_lib.ref_combine:
Python integers and the affine group law."""
import ctypes
import functools
import os
import random
import subprocess

import numpy as np

from tests import combine_lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
R = L.R
WINDOWS = (1, 2, 3, 5, 7, 8, 13, 16)
_libs = {}


def load(name="libmsm.so"):
    """libmsm.so: the shipped BLSW_MSM_SEGMENT; libmsm_seg4.so: 4 buckets per segment"""
    if name not in _libs:
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "msm"), name])
        lib = ctypes.CDLL(os.path.join(HERE, "msm", name))
        lib.msm_shape.restype = ctypes.c_uint32
        lib.msm_digit_of.restype = ctypes.c_uint32
        _libs[name] = lib
    return _libs[name]


def shape(what, v, name="libmsm.so"):
    """windows(c), segments(c), default_window(k), segment (the compile-time constant)"""
    return load(name).msm_shape(["windows", "segments", "default_window", "segment"].index(what), ctypes.c_uint32(v))


def digit(x, win, c):
    return load().msm_digit_of(L.words(x).ctypes.data_as(L.u32p), ctypes.c_uint32(win), ctypes.c_uint32(c))


def host_msm(group, points, scalars, counts=None, window_bits=0, order=None, name="libmsm.so"):
    """uint8 [n, k, W], [n, k, 32] -> (out uint8 [n, W], status int32 [n]) by the host stages; order: None (forward), "reversed" or an int seed"""
    points, scalars = np.ascontiguousarray(points, dtype=np.uint8), np.ascontiguousarray(scalars, dtype=np.uint8)
    n, k = points.shape[:2]
    assert points.shape == (n, k, L.WIDTH[group]) and scalars.shape == (n, k, 32)
    cn = None if counts is None else np.array([int(c) for c in counts], dtype=np.uint32)
    perm = None
    if order is not None:
        perm = list(range(n * k))
        if order == "reversed":
            perm.reverse()
        else:
            random.Random(order).shuffle(perm)
        perm = np.array(perm, dtype=np.uint64)
    out, st = np.full((n, L.WIDTH[group]), 0xA5, np.uint8), np.full(n, -1, np.int32)
    rc = load(name).msm_points(ctypes.c_uint32(group), points.ctypes.data_as(L.u8p), scalars.ctypes.data_as(L.u8p), None if cn is None else cn.ctypes.data_as(L.u32p),
                               ctypes.c_uint32(k), ctypes.c_uint64(n), ctypes.c_uint32(window_bits), None if perm is None else perm.ctypes.data_as(L.u64p), out.ctypes.data_as(L.u8p),
                               st.ctypes.data_as(L.i32p))
    assert rc == 0
    return out, st


def _pack(rows, group):
    exp = [L.ref_combine(group, pts, scs, count) for _, pts, scs, count in rows]
    W = L.WIDTH[group]
    return ([r[0] for r in rows], L.pack([r[1] for r in rows], W), L.pack([[L.le32(v) for v in r[2]] for r in rows], 32), [r[3] for r in rows],
            np.frombuffer(b"".join(e[1] for e in exp), np.uint8).reshape(len(rows), W).copy(), [e[0] for e in exp])


@functools.lru_cache(maxsize=None)
def edge_vectors(group, c, k=130, segment=32):
    """(names, points [n, k, W], scalars [n, k, 32], counts [n], expected out [n, W], expected status [n]): six lists at the bucket method's edges for
    window width c and `segment` buckets per segment, n = 3 at a time with counts (k, k // 2, 1) — the GPU test's shape; every expected value from
    ref_combine. Scalars: 0, 1, r - 1, 2^c - 1, 2^c, single windows 2^(c j), the first and last bucket of a segment and of a partial last segment."""
    rng = random.Random(0xB0C + 64 * group + c)
    P, N = L.pool(group)
    W = (255 + c - 1) // c
    B = 1 << c
    seg = [v for v in (segment - 1, segment, segment + 1, 2 * segment - 1, 2 * segment, B - segment, B - segment - 1, B - 2, B - 1) if 0 < v < B]
    single = [1 << (c * j) for j in (0, 1, W // 2, W - 2, W - 1) if 0 <= j < W and (1 << (c * j)) < R]
    edge = [0, 1, R - 1, B - 1, B, B + 1] + single + seg + [d << (c * (W // 2)) for d in seg] + [(B - 1) << (c * (W - 2))]
    half = k // 2
    base = [P[j % 6] for j in range(k)]
    s = [rng.randrange(1, R) for _ in range(k)]
    eq = rng.randrange(1, R)
    garbage_pt, garbage_sc = bytes([0xFF]) * L.WIDTH[group], (1 << 256) - 1
    rows = [
        ("edge scalars over the pool", base, [edge[j % len(edge)] for j in range(k)], k),
        # one bucket per window takes everything; P[0] sits at 0, 6, 12, ... in it (the doubling branch) and -P[1] cancels one P[1]
        ("all scalars equal, repeats and a negative", [N[1] if j == 2 else base[j] for j in range(k)], [eq] * k, half),
        ("one term, garbage behind the count", [P[3]] + [garbage_pt] * (k - 1), [(B - 1) | (1 << 254)] + [garbage_sc] * (k - 1), 1),
        # the total is the identity: pairs P, -P under one scalar (identity buckets), then s P + (r - s) P
        ("identity total", [(P if j % 2 == 0 else N)[(j // 2) % 6] for j in range(k - 2)] + [P[0], P[0]], [s[j // 2] for j in range(k - 2)] + [s[0], R - s[0]], k),
        ("a scalar of 2^255 - 1 is refused", base, s[:half - 1] + [(1 << 255) - 1] + s[half:], half),
        ("one term, scalar r - 1", [P[4]] + base[1:], [R - 1] + s[1:], 1),
    ]
    return _pack(rows, group)


@functools.lru_cache(maxsize=None)
def long_list(k, seed, equal=False):
    """one G1 list of k terms over the six pool points, whose discrete logs are known: -> (points [1, k, 48], scalars [1, k, 32], expected 48 bytes
    = [sum s_j a_j mod r] G by ONE Python scalar multiplication)"""
    rng = random.Random(0xC0B1 + 1)  # combine_lib.pool(1)'s stream: the same six logs
    logs = [rng.randrange(1, R) for _ in range(6)]
    P, _ = L.pool(1)
    assert all(L.COMPRESS[1](L.mul(1, a, L.GEN[1])) == p for a, p in zip(logs, P))
    r2 = random.Random(seed)
    which = np.array([r2.randrange(6) for _ in range(k)])
    if equal:
        sc = [r2.randrange(1, R)] * k
    else:
        sc = [r2.randrange(0, R) for _ in range(k)]
    total = sum(s * logs[w] for s, w in zip(sc, which)) % R
    table = np.stack([np.frombuffer(p, np.uint8) for p in P])
    scalars = np.frombuffer(b"".join(L.le32(v) for v in sc), np.uint8).reshape(1, k, 32).copy()
    return table[which].reshape(1, k, 48).copy(), scalars, L.COMPRESS[1](L.mul(1, total, L.GEN[1]))
