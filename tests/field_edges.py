"""Edge operands for the field and tower arithmetic of csrc/fp.hpp, gadgets.hpp and tower.hpp, shared by the host tests (test_r1cs_synth.py,
test_field_ref.py) and the device test (test_field_device_gpu.py). Every value is a STORED integer below p: what the 12 limbs of an Fp hold (the
Montgomery form of some field element); limb patterns, carries and the divstep count of fp_inv are properties of the stored integer."""
import random

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 1 << 384
ONE = R % P  # the stored form of 1


def field_edge_values():
    """110 values (a few of them equal: 2^384 is R, 2^392 - 1 is the value with all fourteen 28-bit limbs set), all below p"""
    v = [0, 1, 2, P - 1, P - 2, R, R * R, (P + 1) // 2, (P - 1) // 2, sum(0xFFFFFFF << (28 * k) for k in range(14))]
    for w, kmax in ((28, 14), (30, 13), (32, 13)):  # the limb widths of fp_mul (28), fp_inv (30) and fp_mul32 (32), up to and past their top limb
        for k in range(1, kmax + 1):
            v += [1 << (w * k), (1 << (w * k)) - 1]
    rng = random.Random(0xF1E1D)
    return [x % P for x in v] + [rng.randrange(P) for _ in range(20)]


# ---------------------------------------------------------------- fp_inv's loop, modelled
INV_MAX_BATCHES = 37  # fp_inv's bound on its batches of 30 divsteps


def inv_batches(g):
    """The number of 30-divstep batches fp_inv runs on the stored integer g before its g is 0 (a lane alone in its wave: the host compilation; on
    the device a lane goes on until the slowest lane of its wave is done). The divstep and the zeta rule are fp_inv's, on whole integers: with
    zeta < 0 and g odd, (f, g) <- (g, g - f) and zeta <- -zeta - 2; otherwise g <- g + (g odd) f and zeta <- zeta - 1; then g <- g / 2."""
    f, zeta, n = P, -1, 0
    while g != 0:
        assert n < INV_MAX_BATCHES, "fp_inv's bound on its batches does not hold"
        for _ in range(30):
            if g & 1:
                if zeta < 0:
                    f, g, zeta = g, g - f, -zeta - 2
                else:
                    g, zeta = g + f, zeta - 1
            else:
                zeta -= 1
            g >>= 1
        n += 1
    return n


# Inversion stress values. Search: inv_batches over field_edge_values() and over SEARCH_N values of random.Random(SEARCH_SEED).randrange(P), in that
# order (about a minute of CPU time). It found counts 25..27 only (0 for the value 0): among the random values 25 batches for 20, 26 for
# 447 065, 27 for 2 915; among the edge values 27 for two (2^360 - 1 and one random value) and 26 for every other non-zero one. Nothing above
# 27 of the 37 permitted batches has been seen. Frozen: the first random value with the largest count (index 124 of the search) and the first
# with the smallest (index 35 977); 2^360 - 1 is a second slow value, of another shape.
SEARCH_SEED, SEARCH_N = 0xD1F5, 450000
INV_SLOW = 0x187EC5A13FDA30278603277F72FD407AA7CB6D32BF7AF3EFFA51C99176BF0FF84633F72F4D8B114924AA4AC472812FBD  # 27 batches
INV_FAST = 0x149DA0BD7A35C8A0EACE76FBB0BF185708E7D712BC8B22DABE0B29C679DE15762CF08F54EB8493BE68755146F9BBEC79  # 25 batches
INV_SLOW_EDGE = (1 << 360) - 1  # 27 batches
INV_STRESS = ((INV_SLOW, 27), (INV_FAST, 25), (INV_SLOW_EDGE, 27))  # (value, batches): the host test asserts that the model reproduces them


def fp_reduced_edges():
    """the Fp values the Fp2 operand set is built from: the ends of the range, the half, all-ones limb patterns of the three limb widths, a power
    of two inside a limb of each width, the stored one, the two inversion stress values"""
    return [0, 1, P - 1, P - 2, (P - 1) // 2, ONE, (1 << 32) - 1, (1 << 352) - 1, sum(0xFFFFFFF << (28 * k) for k in range(14)) % P, INV_SLOW_EDGE, 1 << 379,
            INV_SLOW, INV_FAST]


def fp2_operand_set():
    """(x, 0), (0, x), (x, x) and (x, p - x) for the reduced Fp edge list ((x, x) makes a0 - a1 zero in the square, (x, p - x) makes a0 + a1 wrap to
    0), then 0, 1 (stored 1 and the stored one), u, (p-1, p-1), and four seeded random elements each with its negative. Distinct, in a fixed order."""
    s = []
    for x in fp_reduced_edges():
        s += [(x, 0), (0, x), (x, x), (x, (P - x) % P)]
    s += [(0, 0), (1, 0), (ONE, 0), (0, ONE), (0, 1), (P - 1, P - 1)]
    rng = random.Random(0xF2E1D)
    for _ in range(4):
        a = (rng.randrange(P), rng.randrange(P))
        s += [a, ((P - a[0]) % P, (P - a[1]) % P)]
    return list(dict.fromkeys(s))


def fp2_random(n, seed):
    rng = random.Random(seed)
    return [(rng.randrange(P), rng.randrange(P)) for _ in range(n)]


def runs_of_ones(v, nbits=381):
    """[(hi, lo)] bit positions of the maximal runs of ones of v, from the top"""
    out, i = [], nbits - 1
    while i >= 0:
        if (v >> i) & 1:
            hi = i
            while i >= 0 and (v >> i) & 1:
                i -= 1
            out.append((hi, i + 1))
        else:
            i -= 1
    return out


def to_bits_canonical_values():
    """canonical integers for fp_to_bits_le_w: 0, 1, p-1, p-2, (p-1)/2, 2^380, p-1 with one bit cleared at the top, the bottom and each end of every
    run of ones of p-1, and four seeded random values"""
    v = [0, 1, P - 1, P - 2, (P - 1) // 2, 1 << 380]
    bits = {380, 1}  # the top and the lowest set bit of p - 1 (bit 0 of p - 1 is clear)
    for hi, lo in runs_of_ones(P - 1):
        bits |= {hi, lo}
    assert all(((P - 1) >> b) & 1 for b in bits)
    v += [(P - 1) ^ (1 << b) for b in sorted(bits, reverse=True)]
    rng = random.Random(0xB175)
    v += [rng.randrange(P) for _ in range(4)]
    return list(dict.fromkeys(v))


# ---------------------------------------------------------------- how the items sit in a wave
ITEM_COUNTS = (1, 15, 16, 17, 64, 100)  # with one lane per item and with four: a partial last wave, and a wave with a single item
WAVE = 64


def uniform_waves(values):
    """each value 64 times: with one lane per item a wave of its own, with four lanes per item four such waves"""
    return [v for v in values for _ in range(WAVE)]


def interleaved(pattern, n=2 * WAVE):
    """the pattern repeated side by side over n items: every wave, in both lane layouts, holds all of it"""
    return [pattern[i % len(pattern)] for i in range(n)]
