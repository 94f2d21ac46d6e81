"""Small synthetic R1CS systems at the arithmetic edges of the device evaluator (blsw_r1cs_*, csrc/k_r1cs.hip), satisfiable by construction, and a
big-integer reference of the same operation. Plain numpy and Python integers: no GPU, no library.

A system is a matrices()-shaped dict (what ConstraintChecker.from_matrices, blsw_r1cs_device_bytes and hostsim_lib.r1cs_check take) with extra keys:
"rows" (per row, per matrix, the entries as (column, canonical coefficient)), "slack" (per row, the column of its slack or None) and "tags" (name ->
row). Every row but the ones with an empty C has one slack witness column of its own in C; an assignment solves it from <A, z> <B, z> = <C, z>, so
adding anything non-zero to a slack breaks exactly that row.

Number forms. A stored integer s stands for the field value s R^-1 in form 0 (Montgomery, R = 2^384) and for s in form 1 (canonical). A matrix holds
the Montgomery integer c R mod p of the canonical coefficient c. The kernel's row value REDC(sum) is (sum of c s) R^-1 mod p over STORED integers
(redc_ref); the reference below works on field values and re-encodes them in the input's form where stored integers are compared."""
import collections
import random

import numpy as np

from tests.oracle_lib import P_MOD as P

R = 1 << 384
R_INV = pow(R, -1, P)
SMALL = (1 << 30) - 1  # the largest payload of the small classes
POS, NEG, GEN = 0, 1, 2

# canonical coefficients at the encoder's class borders -> (class, payload; None: a table index)
BOUNDARY = {
    1: (POS, 1), 2: (POS, 2), SMALL - 1: (POS, SMALL - 1), SMALL: (POS, SMALL), SMALL + 1: (GEN, None), SMALL + 2: (GEN, None),
    P - 1: (NEG, 1), P - 2: (NEG, 2), P - SMALL: (NEG, SMALL), P - SMALL - 1: (GEN, None),
    (P + 1) // 2: (GEN, None), (P - 1) // 2: (GEN, None), R % P: (GEN, None), 1 << 380: (GEN, None),
}
# stored z values at the edges of the kernel's limb arithmetic
EDGE_Z = [0, 1, P - 1, P - 2, R % P, 1 << 380] + [v % P for k in range(1, 12) for v in ((1 << (32 * k)) - 1, 1 << (32 * k))]


def expected_class(c):
    """the class the encoder must give the canonical coefficient c (0 < c < p), stated from the encoding's definition"""
    if c <= SMALL:
        return POS, c
    if P - c <= SMALL:
        return NEG, P - c
    return GEN, None


def coefficients(seed=7):
    """the boundary set, powers of two across the whole range, and random ones"""
    rng = random.Random(seed)
    out = list(BOUNDARY) + [1 << k for k in range(3, 380, 13)] + [rng.randrange(1, P) for _ in range(36)]
    assert len(set(out)) == len(out)
    return out


def decode(s, form):
    return s * R_INV % P if form == 0 else s


def encode(v, form):
    return v * R % P if form == 0 else v


def limbs(ints):
    """non-negative integers below 2^384 -> uint64 [len, 6]"""
    return np.frombuffer(b"".join(int(v).to_bytes(48, "little") for v in ints), dtype=np.uint64).reshape(-1, 6).copy()


def to_int(a):
    return int.from_bytes(np.ascontiguousarray(a, dtype=np.uint64).tobytes(), "little")


# witness columns (relative to the first witness): a pool of edge values that differ per instance, blocks of fixed stored values, then the slacks
N_POOL, N_PM1, N_ONE, N_ZERO = 64, 6000, 128, 128
BIG_ROW = 6000  # entries of the row that is a block of its own (6000 small-class terms: 18 030 work units against blocks of 16 384)


def make_system(n_instance_vars=1, seed=1, n_packing=24):
    rng = random.Random(seed * 1000 + n_instance_vars)
    ni = n_instance_vars
    coeffs = coefficients()
    pool = [ni + k for k in range(N_POOL)]
    pm1 = [ni + N_POOL + k for k in range(N_PM1)]                    # stored p - 1 in every instance
    ones = [pm1[-1] + 1 + k for k in range(N_ONE)]                    # stored 1
    zeros = [ones[-1] + 1 + k for k in range(N_ZERO)]                 # stored 0
    first_slack = zeros[-1] + 1
    free = list(range(ni)) + pool                                     # column 0, the instance columns, the pool

    def entries(k=None, cols=free):
        k = k if k is not None else rng.randint(1, 5)
        return sorted(zip(rng.sample(cols, k), (rng.choice(coeffs) for _ in range(k))))

    def cancel(cols, c):
        a, b = sorted(rng.sample(cols, 2))  # equal stored values: +c z_a - c z_b = 0
        return [(a, c), (b, P - c)]

    generic, special = [], []
    for ci, c in enumerate(coeffs):  # every coefficient in A, in B and in C
        for m in range(3):
            row = [entries(), entries(), entries()]
            row[m][0] = (row[m][0][0], c)
            generic.append((None, row, coeffs[(3 * ci + m) % len(coeffs)]))
    sc = lambda: rng.choice(coeffs)
    special.append(("empty_A", [[], entries(), []], sc()))
    special.append(("empty_B", [entries(), [], []], sc()))
    special.append(("all_empty", [[], [], []], None))
    # a cancelling pair: the accumulator holds a non-zero multiple of p (small classes on equal z, 0 included: neg_raw(0) = p times 2^30 - 1), the row value is 0
    for name, cols, c in (("pm1", pm1, SMALL), ("zero", zeros, SMALL), ("one", ones, 2), ("gen", pm1, (P + 1) // 2), ("gen_zero", zeros, 1 << 380)):
        special.append(("cancel_%s_empty_B" % name, [cancel(cols, c), [], []], sc()))
        special.append(("cancel_%s_empty_C" % name, [cancel(cols, c), entries(), []], None))
        special.append(("cancel_%s_in_B_empty_C" % name, [entries(), cancel(cols, c), []], None))
        special.append(("cancel_%s_in_C" % name, [entries(), entries(), cancel(cols, c)], sc()))
    x = pool[5]
    special.append(("same_column", [[(x, sc())], [(x, sc())], [(x, sc())]], sc()))
    special.append(("column_0", [[(0, sc())], [(0, P - SMALL)], [(0, 1 << 380)]], sc()))
    inst = list(range(ni))
    special.append(("instance_columns", [[(k, sc()) for k in inst], [(inst[-1], sc())], [(k, sc()) for k in inst[-2:]]], sc()))
    # packing-like: 381 table-class powers of two (2^30 .. 2^410 mod p) over every kind of column, in A, B or C in turn
    pack_cols = list(range(ni)) + pool + pm1[:200] + ones + zeros
    for j in range(n_packing):
        row = [entries(), entries(), entries(2)]
        row[j % 3] = sorted(zip(rng.sample(pack_cols, 381), (pow(2, 30 + k, P) for k in range(381))))
        special.append(("packing_%d" % j, row, sc()))
    # accumulator limb 13: 128 maximal small-class terms, (2^30 - 1)(p - 1) from z = p - 1, from -(2^30 - 1) on z = 1, and (2^30 - 1) p from z = 0
    for name, cols, c in (("pos_pm1", pm1, SMALL), ("neg_one", ones, P - SMALL), ("neg_zero", zeros, P - SMALL)):
        for m in range(3):
            row = [entries(), entries(), entries(2)]
            row[m] = [(k, c) for k in sorted(rng.sample(cols, 128))]
            special.append(("limb13_%s_%s" % (name, "ABC"[m]), row, sc()))
    special.append(("big", [[(k, SMALL) for k in pm1[:BIG_ROW]], entries(), []], sc()))
    # order: the special rows spread between the generic ones; the first and the last row are generic (they have a slack)
    rng.shuffle(special)
    step = max(1, (len(generic) - 2) // len(special))
    order = []
    for j, g in enumerate(generic):
        order.append(g)
        if j % step == 0 and special and j < len(generic) - 1:
            order.append(special.pop())
    assert not special and order[0][0] is None and order[-1][0] is None
    sys = system_from_rows(order, ni, first_slack=first_slack)
    assert sys["n_witness"] <= 16384
    sys["blocks"] = {"pool": pool, "pm1": pm1, "ones": ones, "zeros": zeros}
    return sys


def system_from_rows(order, ni, first_slack=None, n_witness=None):
    """order: [(tag or None, [A, B, C] entries, the slack's coefficient or None, the slack's column)] -> the system dict. Without a column the slacks
    are the columns from first_slack on, one after the other, and n_witness ends with the last of them."""
    rows, slack, slack_coeff, tags = [], [], [], {}
    for r, (tag, row, c_slack, *given) in enumerate(order):
        if tag:
            tags[tag] = r
        if c_slack is not None:
            s = given[0] if given else first_slack + sum(x is not None for x in slack)
            row[2] = sorted(row[2] + [(s, c_slack)])
            slack.append(s)
        else:
            slack.append(None)
        slack_coeff.append(c_slack)
        for m in range(3):
            cols = [k for k, _ in row[m]]
            assert cols == sorted(set(cols)) and all(0 < c < P for _, c in row[m])
        rows.append(row)
    if n_witness is None:
        n_witness = first_slack + sum(x is not None for x in slack) - ni
    uses = collections.Counter(k for row in rows for mat in row for k, _ in mat)
    assert all(uses[s] == 1 for s in slack if s is not None)  # a slack is in its row's C and nowhere else
    sys = {"n_constraints": len(rows), "n_instance_vars": ni, "n_witness": n_witness, "rows": rows, "slack": slack, "tags": tags,
           "slack_inv": [pow(c, -1, P) if c else None for c in slack_coeff]}
    for m, name in enumerate("ABC"):
        rp = np.zeros(len(rows) + 1, dtype=np.uint64)
        rp[1:] = np.cumsum([len(row[m]) for row in rows])
        col = np.array([k for row in rows for k, _ in row[m]], dtype=np.uint32)
        val = limbs([c * R % P for row in rows for _, c in row[m]]) if len(col) else np.zeros((0, 6), dtype=np.uint64)
        sys[name] = (rp, col, val)
    return sys


def dot(entries, field):
    s = 0
    for k, c in entries:
        s += c * field[k]
    return s % P


def redc_ref(entries, z):
    """what the kernel's row_dot returns for stored integers z: (sum of c z) R^-1 mod p"""
    return dot(entries, z) * R_INV % P


def assignment(sys, d, form, seed=11):
    """the stored integers z = [instance | witness] of base instance d: column 0 is the one of the form, the instance columns and the pool take the
    edge values in an order that depends on d (plus random values), the blocks are fixed, and every slack solves its row"""
    rng = random.Random(seed * 4096 + d)
    ni, B = sys["n_instance_vars"], sys["blocks"]
    vals = EDGE_Z + [rng.randrange(P) for _ in range(N_POOL + ni - len(EDGE_Z))]
    z = [0] * (ni + sys["n_witness"])
    for j, k in enumerate(list(range(1, ni)) + B["pool"]):
        z[k] = vals[(j + 5 * d) % len(vals)]
    z[0] = encode(1, form)
    for k in B["pm1"]:
        z[k] = P - 1
    for k in B["ones"]:
        z[k] = 1
    solve_slacks(sys, z, form)
    return z


def solve_slacks(sys, z, form):
    """sets every slack of the stored integers z (a list, or a dict of the columns the rows use) to the value that satisfies its row"""
    field = Field(z, form)
    for row, s, inv in zip(sys["rows"], sys["slack"], sys["slack_inv"]):
        if s is not None:
            v = (dot(row[0], field) * dot(row[1], field) - dot([e for e in row[2] if e[0] != s], field)) * inv % P
            z[s] = encode(v, form)


def assignments(sys, n, form, distinct=16):
    """n instances from `distinct` base assignments (instance i = base i % distinct): lists of stored integers, each its own copy"""
    base = [assignment(sys, d, form) for d in range(min(n, distinct))]
    return [list(base[i % len(base)]) for i in range(n)]


class Field:
    """the field values of the stored integers z, decoded when a row asks for them"""

    def __init__(self, z, form):
        self.z, self.form, self.memo = z, form, {}

    def __getitem__(self, k):
        if k not in self.memo:
            self.memo[k] = decode(self.z[k], self.form)
        return self.memo[k]


def row_values(sys, z, form, rows=None):
    """(<A, z>, <B, z>, <C, z>) as field values, one row of the range (default all) after the other"""
    field = Field(z, form)
    for row in sys["rows"] if rows is None else sys["rows"][rows[0]:rows[0] + rows[1]]:
        yield tuple(dot(row[m], field) for m in range(3))


def first_unsatisfied(sys, z, form):
    for r, (a, b, c) in enumerate(row_values(sys, z, form)):
        if a * b % P != c:
            return r
    return -1


def evaluate_ref(sys, z, form, rows=None):
    """the rows of A z, B z, C z as stored integers in the input's form: what blsw_r1cs_evaluate writes"""
    return [tuple(encode(v, form) for v in t) for t in row_values(sys, z, form, rows)]


def bump(sys, z, row, delta):
    """the slack of `row` + delta (mod p) in the stored integers z: that row, and no other, fails"""
    s = sys["slack"][row]
    assert s is not None and delta % P
    z[s] = (z[s] + delta) % P


def witness_array(sys, zs, pad=0, seed=3):
    """uint64 [n, n_witness + pad, 6]: the witness part of every instance, the padding filled with junk"""
    ni, nw = sys["n_instance_vars"], sys["n_witness"]
    out = np.random.default_rng(seed).integers(0, 1 << 63, size=(len(zs), nw + pad, 6), dtype=np.uint64)
    for i, z in enumerate(zs):
        out[i, :nw] = limbs(z[ni:])
    return out


def instance_array(sys, zs, pad=0, seed=4):
    ni = sys["n_instance_vars"]
    out = np.random.default_rng(seed).integers(0, 1 << 63, size=(len(zs), ni + pad, 6), dtype=np.uint64)
    for i, z in enumerate(zs):
        out[i, :ni] = limbs(z[:ni])
    return out
