"""Seeded vectors and pure-Python checkers for the kernels' arithmetic units, shared by the host
backend test (tests/test_devarith_cases_host.py: libhostcheck.so, the bounds-checked HOST build of the
headers) and the GPU test (tests/test_gpu_devarith.py: libdevcheck.so, the same headers' DEVICE
branches on gfx950). The edge lists of tests/test_native_host.py and tests/test_lp_host.py live here.

A unit (UNITS) has seeded inputs, a runner over a backend and a checker against Python big integers,
`% L`, digit sums or hashlib. Every input respects its unit's documented preconditions: the host
backend aborts otherwise (PV_BOUNDS_CHECK). Nothing here needs a GPU."""
import ctypes
import hashlib
import random

import numpy as np

P = 2 ** 255 - 19
L = 2 ** 252 + 27742317777372353535851937790883648493
N8L = 8 * L
W = [26 if i % 2 == 0 else 25 for i in range(10)]
D = (-121665 * pow(121666, P - 2, P)) % P
SQRTM1 = pow(2, (P - 1) // 4, P)
PV_GMAX = 0xD000000
LANE_CHUNK = 4160   # at most this many lanes per per-lane launch
WAVE_CHUNK = 700    # at most this many waves per per-wave launch


def to_limbs(x):
    out, off = [], 0
    for w in W:
        out.append((x >> off) & ((1 << w) - 1))
        off += w
    return out


def from_limbs(lim):
    v, off = 0, 0
    for i, w in enumerate(W):
        v += int(lim[i]) << off
        off += w
    return v


def to_limbs_wide(x):
    """Limbs of x < 2^256 with the bits from 2^255 up left in limb 9."""
    lim = to_limbs(x)
    lim[9] = x >> 230
    return lim


def max_mul_input():
    return [3 * (1 << w) + (1 << 18) - 1 for w in W]


def wide_f_operand_pairs():
    """The (f, g) maxima of fe_mul's call sites with an uncarried f (ge_p2_dbl's r.X = S + 4p - r.Y, the
    niels F = 2Z + 2p - c, a sum / difference of reduced values on both sides)."""
    R = [(1 << w) + (1 << 17) - 1 for w in W]
    G3 = [3 * (1 << w) + (1 << 18) - 1 for w in W]
    dbl_rx = [R[i] + (0xFFFFFB4 if i == 0 else (0x7FFFFFC if i % 2 else 0xFFFFFFC)) for i in range(10)]
    niels_f = [2 * R[i] + (0x7FFFFDA if i == 0 else (0x3FFFFFE if i % 2 else 0x7FFFFFE)) for i in range(10)]
    return [(dbl_rx, R), (niels_f, G3), (G3, G3)]


# ---------------------------------------------------------------- edge lists (also used by the host tests)
TOBYTES_EDGES = [0, 1, 18, 19, P - 1, P, P + 1, P + 18, 2 ** 255 - 1]
TOBYTES_UNNORMALISED = [P, 2 * P - 1, 2 * P, 2 * P + 7, 3 * P]
SC_REDUCE_EDGES = [0, 2 ** 512 - 1, L, L - 1, L + 1, 2 ** 256, 2 ** 252, 2 * L, L * 2 ** 259, 2 ** 511]
SC_CANONICAL_EDGES = [L, L - 1, L + 1, 0, 2 ** 256 - 1, 2 ** 253]
SC_RECODE_EDGES = [0, 1, L - 1, 2 ** 252]
SC_RECODE_ANY_EDGES = [2 ** 256 - 1, 2 ** 255, 0x7777777777777777]
SC_MUL_EDGES = [(0, 0), (L - 1, L - 1), (2 ** 256 - 1, 2 ** 256 - 1), (1, L + 5)]
SC_MUL5_EDGES = [(0, 0), (1, L + 5), (2 ** 160 - 1, 2 ** 256 - 1), (2 ** 160 - 1, L - 1), (2 ** 159, L)]
NWIN16_EDGES = [0, 1, 7, 8, 15, 16, 2 ** 128 - 1, 2 ** 131, L - 1]
HALFSIZE_EDGES = [0, 1, 2, 3, 2 ** 64, 2 ** 127, 2 ** 128 - 1, 2 ** 128, 2 ** 128 + 1, L - 1, L - 2,
                  N8L // 3, N8L // 2 ** 20, N8L // 2 ** 31, N8L // 2 ** 32, N8L // 2 ** 33, N8L // 2 ** 60,
                  2 ** 200, 2 ** 252, (2 ** 252) | 1]
LP_HALFSIZE_EDGES = [0, 1, 2 ** 64, 2 ** 128 - 1, 2 ** 128, 2 ** 131 + 5, L - 1, N8L // 3, N8L // 2 ** 33, 2 ** 252]
WIDE_RECODE_TOO_LARGE = [2 ** 253, 2 ** 255 + 12345, 2 ** 256 - 1]  # rejected before any point arithmetic
# operand widths the group formulas produce: LR products, sums of two (2^27.13), differences
# with 2p (2^27.6) on either side, and the doubling's uncarried E (2^28.4) against H or F
LP_MUL_COMBOS = [(26.01, 26.01), (27.13, 27.13), (27.6, 27.6), (28.4, 27.13), (28.4, 26.01)]
LP_MUL_DUAL_COMBOS = [(26.01, 26.01), (27.13, 27.13), (27.6, 26.6)]


def wide_recode_edges(w):
    return [0, 1, L - 1, L, 2 ** 252, 2 ** 253 - 1, (1 << (w - 1)), (1 << w) - 1]


def split_edges():
    out = list(HALFSIZE_EDGES)
    out += [k for k in LP_HALFSIZE_EDGES if k not in out]
    return out


def rand_limbs(rng, bound_bits):
    """Limbs below 2^bound_bits (even) / 2^(bound_bits - 1) (odd): odd limbs are 25 bits wide, so
    every value the formulas form (sums, differences with 2p or 4p) keeps them half as large."""
    return [rng.randrange(int(2 ** (bound_bits - (i & 1)))) for i in range(10)]


def max_limbs(bound_bits):
    return [int(2 ** (bound_bits - (i & 1))) - 1 for i in range(10)]


# ---------------------------------------------------------------- conversions
def words(vals, nw):
    """Integers -> (n, nw) little-endian uint32 words."""
    buf = b"".join(int(v).to_bytes(4 * nw, "little") for v in vals)
    return np.frombuffer(buf, "<u4").reshape(len(vals), nw).copy()


def enc_words(encs):
    """32-byte strings -> (n, 8) words."""
    return np.frombuffer(b"".join(encs), "<u4").reshape(len(encs), 8).copy()


def ints(arr):
    """(n, nw) words -> integers."""
    a = np.ascontiguousarray(arr, "<u4")
    return [int.from_bytes(row.tobytes(), "little") for row in a]


def limb_rows(rows):
    return np.array(rows, dtype=np.uint32).reshape(len(rows), -1)


# ---------------------------------------------------------------- curve helpers (RFC 8032, affine)
def decode_xy(enc):
    """(x, y) with x's parity = bit 255 for an encoding whose y^2 - 1 over d y^2 + 1 is a square, else
    None. y is taken mod p (a non-canonical y decodes as libsodium's frombytes takes it)."""
    y = (int.from_bytes(enc, "little") & (2 ** 255 - 1)) % P
    s = enc[31] >> 7
    u, v = (y * y - 1) % P, (D * y * y + 1) % P
    x = u * pow(v, 3, P) * pow(u * pow(v, 7, P), (P - 5) // 8, P) % P
    if v * x * x % P != u:
        x = x * SQRTM1 % P
        if v * x * x % P != u:
            return None
    if x & 1 != s:
        x = (P - x) % P
    return x, y


def pt_add(p, q):
    (x1, y1), (x2, y2) = p, q
    t = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + x2 * y1) * pow(1 + t, P - 2, P) % P, (y1 * y2 + x1 * x2) * pow(1 - t, P - 2, P) % P)


def pt_mul(s, p):
    acc = (0, 1)
    while s:
        if s & 1:
            acc = pt_add(acc, p)
        p = pt_add(p, p)
        s >>= 1
    return acc


BASE = decode_xy((4 * pow(5, P - 2, P) % P).to_bytes(32, "little"))


def ext_rows(pt):
    x, y = pt
    return to_limbs(x) + to_limbs(y) + to_limbs(1) + to_limbs(x * y % P)


def affine_of_rows(rows40):
    X, Y, Z, T = (from_limbs(rows40[10 * r:10 * r + 10]) % P for r in range(4))
    zi = pow(Z, P - 2, P)
    assert X * Y % P == T * Z % P  # T consistent
    return X * zi % P, Y * zi % P


# ---------------------------------------------------------------- inputs
def _unit_limb(i, v):
    return [v if j == i else 0 for j in range(10)]


def fe_mul_pairs():
    """(f, g) limb pairs: the extremes first, then 3000 random below the mul bound and 3000 below p."""
    rng = random.Random(7)
    mx = max_mul_input()
    pairs = [(mx, mx)] + wide_f_operand_pairs()
    for i in range(10):  # one maximal limb, the rest zero: separates the columns' terms
        pairs += [(_unit_limb(i, mx[i]), mx), (mx, _unit_limb(i, mx[i]))]
    for i in range(10):
        for j in range(10):
            pairs.append((_unit_limb(i, mx[i]), _unit_limb(j, mx[j])))
    for i in range(10):  # f may be any limb < 2^31
        pairs.append((_unit_limb(i, 2 ** 31 - 1), mx))
    special = [to_limbs_wide(v) for v in (0, 1, P - 1, P, 2 * P - 1)]
    pairs += [(a, b) for a in special for b in special]
    for _ in range(3000):
        f = [rng.randrange(3 * (1 << w) + (1 << 18)) for w in W]
        g = [rng.randrange(3 * (1 << w) + (1 << 18)) for w in W]
        pairs.append((f, g))
        pairs.append((to_limbs(rng.randrange(P)), to_limbs(rng.randrange(P))))
    return pairs


def fe_sq_inputs():
    return [f for f, _ in fe_mul_pairs() if max(f) < PV_GMAX]


def fe_carry_inputs():
    out = [f for f, _ in fe_mul_pairs()[:170]]
    out += [[0xFFFFFFFF] * 10] + [_unit_limb(i, 0xFFFFFFFF) for i in range(10)]
    rng = random.Random(71)
    out += [[rng.getrandbits(32) for _ in range(10)] for _ in range(500)]
    return out


def fe_tobytes_inputs():
    out = [to_limbs(v) for v in TOBYTES_EDGES]
    for v in TOBYTES_UNNORMALISED:  # non-normalised representations
        lim = to_limbs(v % 2 ** 255)
        lim[0] += v - from_limbs(lim)
        if lim[0] < 2 ** 31:
            out.append(lim)
    rng = random.Random(72)
    out += [[rng.randrange(3 * (1 << w) + (1 << 18)) for w in W] for _ in range(300)]
    return out


def fe_chain_inputs():
    rng = random.Random(8)
    return [1, 2, P - 1] + [rng.randrange(1, P) for _ in range(40)]


def point_encodings():
    """Blacklist (with and without bit 255), x = 0 (y = 1, p - 1; with bit 255 the sign bit on x = 0),
    non-canonical y in [p, p + 18], 64 off-curve y, 400 random strings. Returns (encodings, index of the
    first random one)."""
    from adversarial_batch import _offcurve_ys
    from vectors import BLACKLIST
    encs = []
    for b in BLACKLIST:
        for top in (0, 0x80):
            e = bytearray(b)
            e[31] |= top
            encs.append(bytes(e))
    for y in (1, P - 1):
        for top in (0, 1):
            encs.append((y | (top << 255)).to_bytes(32, "little"))
    for y in range(P, P + 19):
        for top in (0, 1):
            encs.append((y | (top << 255)).to_bytes(32, "little"))
    for y in _offcurve_ys(np.random.default_rng(51), 64):
        encs.append(y.to_bytes(32, "little"))
    rng = random.Random(52)
    first_random = len(encs)
    encs += [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(400)]
    return encs, first_random


def p2_inputs():
    rng = random.Random(53)
    out = [(0, 1, 1), (1, 0, 1), (P - 1, P - 1, 1), (5, 7, P - 1)]
    out += [(rng.randrange(P), rng.randrange(P), rng.randrange(1, P)) for _ in range(200)]
    return out


def hash_records():
    """(sm, pk) for every smlen in 64..364 (message lengths 0..300: every residue mod 128)."""
    rng = random.Random(54)
    return [(bytes(rng.getrandbits(8) for _ in range(n)), bytes(rng.getrandbits(8) for _ in range(32)))
            for n in range(64, 365)]


def sc_reduce_inputs():
    rng = random.Random(9)
    return SC_REDUCE_EDGES + [rng.getrandbits(512) for _ in range(2000)]


def sc_canonical_inputs():
    rng = random.Random(91)
    return SC_CANONICAL_EDGES + [rng.getrandbits(256) for _ in range(1000)] + [rng.getrandbits(253) for _ in range(1000)]


def sc_recode_inputs():
    """(values, n_exact): the first n_exact are < 2^253 (digit sums are exact), the rest any 256 bits."""
    rng = random.Random(92)
    exact = SC_RECODE_EDGES + [rng.randrange(L) for _ in range(2000)]
    return exact + SC_RECODE_ANY_EDGES + [rng.getrandbits(256) for _ in range(2000)], len(exact)


def sc_mul_inputs(na):
    rng = random.Random(42)
    if na == 8:
        return SC_MUL_EDGES + [(rng.getrandbits(256), rng.getrandbits(256)) for _ in range(2000)]
    return SC_MUL5_EDGES + [(rng.getrandbits(160), rng.getrandbits(256)) for _ in range(2000)]


def wide_recode_inputs(w):
    """(values, n_exact): the last ones are >= 2^253 (digit ranges only)."""
    rng = random.Random(31 + w)
    exact = wide_recode_edges(w) + [rng.randrange(L) for _ in range(1500)] + [rng.getrandbits(253) for _ in range(500)]
    return exact + WIDE_RECODE_TOO_LARGE, len(exact)


def nwin16_inputs():
    rng = random.Random(43)
    return NWIN16_EDGES + [rng.randrange(L) for _ in range(2000)]


def split_random():
    rng = random.Random(41)
    return [rng.randrange(L) for _ in range(4000)], [rng.getrandbits(253) for _ in range(200)]


def split_inputs():
    """(scalars, index of the first random one): edges, 4000 random below L, 200 random 253-bit."""
    e = split_edges()
    a, b = split_random()
    return e + a + b, len(e)


def lp_mul_inputs():
    rng = random.Random(3)
    fs, gs = [], []
    for it in range(600):
        fb, gb = LP_MUL_COMBOS[it % len(LP_MUL_COMBOS)]
        f = [rand_limbs(rng, fb) for _ in range(4)]
        g = [rand_limbs(rng, gb) for _ in range(4)]
        if it < len(LP_MUL_COMBOS):
            f = [max_limbs(fb)] * 4
            g = [max_limbs(gb)] * 4
        fs.append(sum(f, []))
        gs.append(sum(g, []))
    for _ in range(200):
        fs.append(sum((to_limbs(rng.randrange(P)) for _ in range(4)), []))
        gs.append(sum((to_limbs(rng.randrange(P)) for _ in range(4)), []))
    return fs, gs


def lp_mul_dual_inputs():
    rng = random.Random(5)
    fs, gs = [], []
    for it in range(400):
        fb, gb = LP_MUL_DUAL_COMBOS[it % 3]
        f = [rand_limbs(rng, fb) for _ in range(2)]
        g = [rand_limbs(rng, gb) for _ in range(2)]
        if it < 3:
            f = [max_limbs(fb)] * 2
            g = [max_limbs(gb)] * 2
        fs.append(sum(f + f, []))
        gs.append(sum(g + g, []))
    return fs, gs


def lp_chain_inputs(dual, seed, n_reduced, n_wide):
    """Rows for lp_invert / lp_pow22523: reduced nonzero values, then unreduced limbs as the products that
    feed them leave them (< 2^26 + 2^23). dual: rows 2, 3 repeat rows 0, 1."""
    rng = random.Random(seed)
    out = []
    nrow = 2 if dual else 4
    for it in range(n_reduced + n_wide):
        if it < n_reduced:
            rows = [to_limbs(rng.randrange(1, P)) for _ in range(nrow)]
        else:
            rows = [rand_limbs(rng, 26.1) for _ in range(nrow)]
        out.append(sum(rows + rows if dual else rows, []))
    return out


def lp_points():
    rng = random.Random(55)
    from vectors import ORDER8
    pts = [pt_mul(rng.randrange(1, L), BASE) for _ in range(6)]
    return pts + [decode_xy(ORDER8), (0, 1), (0, P - 1)]  # small order, identity, order 2


def ydbl_inputs():
    """(a encodings, r encodings, doubling counts) of test_lp_ydbl_chain_matches_doublings."""
    rng = random.Random(46)
    encs = [(1).to_bytes(32, "little"), (P - 1).to_bytes(32, "little")]
    encs += [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(400)]
    a, r, nd = [], [], []
    for i, e in enumerate(encs):
        for n in ((68,) if i % 8 else (1, 2, 68)):
            a.append(e)
            r.append(encs[(i * 7 + 3) % len(encs)])
            nd.append(n)
    return a, r, nd


def table_parts_inputs():
    rng = random.Random(47)
    return [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(300)]


# ---------------------------------------------------------------- backends
def _ptr(a, i=0):
    return ctypes.c_void_p(a.ctypes.data + i * a.strides[0])


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


class HostBackend:
    """libhostcheck.so: one call per operand set."""
    name = "host"

    def __init__(self, lib):
        self.lib = lib

    def _map(self, fn, n, outs, ins, ret=None):
        for i in range(n):
            r = fn(*[_ptr(o, i) for o in outs], *[_ptr(a, i) for a in ins])
            if ret is not None:
                ret[i] = r

    def _fe(self, name, wo, *ins):
        ins = [_u32(a) for a in ins]
        out = np.zeros((len(ins[0]), wo), np.uint32)
        self._map(getattr(self.lib, name), len(out), [out], ins)
        return out

    def fe_mul(self, f, g): return self._fe("hc_fe_mul", 10, f, g)
    def fe_mul_pre(self, f, g): return self._fe("hc_fe_mul_pre", 10, f, g)
    def fe_sq(self, f): return self._fe("hc_fe_sq", 10, f)
    def fe_carry(self, f): return self._fe("hc_fe_carry", 10, f)
    def fe_tobytes(self, f): return self._fe("hc_fe_tobytes", 8, f)
    def fe_frombytes(self, s): return self._fe("hc_fe_frombytes", 10, s)
    def fe_invert(self, f): return self._fe("hc_fe_invert", 10, f)
    def fe_pow22523(self, f): return self._fe("hc_fe_pow22523", 10, f)
    def sc_reduce64(self, x): return self._fe("hc_sc_reduce64", 8, x)

    def sc_is_canonical(self, s):
        s = _u32(s)
        out = np.zeros(len(s), np.int32)
        self._map(self.lib.hc_sc_is_canonical, len(s), [], [s], out)
        return out

    def sc_mul(self, a, b, na): return self._fe("hc_sc_mul" if na == 8 else "hc_sc_mul5", 8, a, b)
    def sc_recode(self, a, radix): return self._fe("hc_sc_recode%d" % radix, 8, a)

    def sc_recode_w(self, a, w):
        a = _u32(a)
        out = np.zeros((len(a), 16), np.int32)
        for i in range(len(a)):
            assert self.lib.hc_sc_recode_w(w, _ptr(out, i), _ptr(a, i)) == {16: 16, 24: 11}[w]
        return out

    def sc_nwin16(self, a):
        a = _u32(a)
        out = np.zeros(len(a), np.int32)
        self._map(self.lib.hc_sc_nwin16, len(a), [], [a], out)
        return out

    def _split(self, fn, k):
        k = _u32(k)
        k1, k2 = np.zeros_like(k), np.zeros_like(k)
        flags = np.zeros((len(k), 2), np.int32)
        neg = ctypes.c_int()
        for i in range(len(k)):
            flags[i, 1] = fn(_ptr(k, i), _ptr(k1, i), _ptr(k2, i), ctypes.byref(neg))
            flags[i, 0] = neg.value
        return k1, k2, flags

    def sc_halfsize(self, k): return self._split(self.lib.hc_sc_halfsize, k)
    def lp_halfsize(self, k): return self._split(self.lib.hc_lp_halfsize, k)

    def enc_rules(self, s):
        s = _u32(s)
        out = np.zeros((len(s), 2), np.int32)
        for i in range(len(s)):
            out[i] = (self.lib.hc_has_small_order(_ptr(s, i)), self.lib.hc_ge_is_canonical(_ptr(s, i)))
        return out

    def ge_frombytes_negate(self, s):
        s = _u32(s)
        ok = np.zeros(len(s), np.int32)
        out = np.zeros((len(s), 40), np.uint32)
        self._map(self.lib.hc_ge_frombytes_negate, len(s), [out], [s], ok)
        return ok, out

    def ge_p2_tobytes(self, xyz): return self._fe("hc_ge_p2_tobytes", 8, xyz)

    def hash_k(self, records):
        out = np.zeros((len(records), 8), np.uint32)
        for i, (sm, pk) in enumerate(records):
            self.lib.hc_hash_k(_ptr(out, i), sm, ctypes.c_uint64(len(sm)), pk)
        return out

    _BIN = ("hc_lp_mul", "hc_lp_mul_dual", "hc_lp_add", "hc_lp_sub")
    _UN = ("hc_lp_invert", "hc_lp_invert_dual", "hc_lp_pow22523", "hc_lp_pow22523_dual", "hc_lp_dbl")

    def lp_binary(self, f, g, op): return self._fe(self._BIN[op], 40, f, g)
    def lp_unary(self, f, op): return self._fe(self._UN[op], 40, f)

    def lp_decompress_ar(self, a, r):
        a, r = _u32(a), _u32(r)
        flags = np.zeros((len(a), 3), np.int32)
        xy = np.zeros((len(a), 80), np.uint32)
        self._map(self.lib.hc_lp_decompress_ar, len(a), [flags, xy], [a, r])
        return flags, xy

    def lp_ydbl_check(self, a, r, nd):
        a, r = _u32(a), _u32(r)
        out = np.zeros(len(a), np.int32)
        for i in range(len(a)):
            out[i] = self.lib.hc_lp_ydbl_check(_ptr(a, i), _ptr(r, i), int(nd[i]))
        return out

    def lp_table_parts_check(self, enc):
        enc = _u32(enc)
        out = np.zeros(len(enc), np.int32)
        self._map(self.lib.hc_lp_table_parts_check, len(enc), [], [enc], out)
        return out


class DeviceError(AssertionError):
    pass


class DevBackend:
    """libdevcheck.so: operand set i on thread i (per-lane units, blocks of 64 lanes) or on wave i
    (limb-parallel units), in launches of at most LANE_CHUNK lanes / WAVE_CHUNK waves. A wrapper that
    returns a HIP error raises."""
    name = "device"

    def __init__(self, lib):
        self.lib = lib
        self.launches = 0

    def _run(self, name, chunk, outs, ins, *scalars):
        """outs / ins: arrays with one row per operand set; scalars go between the pointers and n."""
        n = len(ins[0])
        fn = getattr(self.lib, name)
        for lo in range(0, n, chunk):
            m = min(chunk, n - lo)
            rc = fn(*[_ptr(o, lo) for o in outs], *[_ptr(a, lo) for a in ins], *scalars, ctypes.c_int(m))
            self.launches += 1
            if rc != 0:
                raise DeviceError("%s returned HIP error %d" % (name, rc))

    def _fe(self, name, wo, *ins, scalars=(), chunk=LANE_CHUNK, dtype=np.uint32):
        ins = [_u32(a) for a in ins]
        out = np.zeros((len(ins[0]), wo), dtype)
        self._run(name, chunk, [out], ins, *scalars)
        return out

    def fe_mul(self, f, g): return self._fe("dc_fe_mul", 10, f, g)
    def fe_mul_pre(self, f, g): return self._fe("dc_fe_mul_pre", 10, f, g)
    def fe_sq(self, f): return self._fe("dc_fe_sq", 10, f)
    def fe_carry(self, f): return self._fe("dc_fe_carry", 10, f)
    def fe_tobytes(self, f): return self._fe("dc_fe_tobytes", 8, f)
    def fe_frombytes(self, s): return self._fe("dc_fe_frombytes", 10, s)
    def fe_invert(self, f): return self._fe("dc_fe_invert", 10, f)
    def fe_pow22523(self, f): return self._fe("dc_fe_pow22523", 10, f)
    def sc_reduce64(self, x): return self._fe("dc_sc_reduce64", 8, x)
    def sc_is_canonical(self, s): return self._fe("dc_sc_is_canonical", 1, s, dtype=np.int32)[:, 0]
    def sc_mul(self, a, b, na): return self._fe("dc_sc_mul", 8, a, b, scalars=(ctypes.c_int(na),))
    def sc_recode(self, a, radix): return self._fe("dc_sc_recode", 8, a, scalars=(ctypes.c_int(radix),))
    def sc_recode_w(self, a, w): return self._fe("dc_sc_recode_w", 16, a, scalars=(ctypes.c_int(w),), dtype=np.int32)
    def sc_nwin16(self, a): return self._fe("dc_sc_nwin16", 1, a, dtype=np.int32)[:, 0]

    def _split(self, name, chunk, k):
        k = _u32(k)
        k1, k2 = np.zeros_like(k), np.zeros_like(k)
        flags = np.zeros((len(k), 2), np.int32)
        self._run(name, chunk, [k1, k2, flags], [k])
        return k1, k2, flags

    def sc_halfsize(self, k): return self._split("dc_sc_halfsize", LANE_CHUNK, k)
    def lp_halfsize(self, k): return self._split("dc_lp_halfsize", WAVE_CHUNK, k)
    def enc_rules(self, s): return self._fe("dc_enc_rules", 2, s, dtype=np.int32)

    def ge_frombytes_negate(self, s):
        s = _u32(s)
        ok = np.zeros((len(s), 1), np.int32)
        out = np.zeros((len(s), 40), np.uint32)
        self._run("dc_ge_frombytes_negate", LANE_CHUNK, [ok, out], [s])
        return ok[:, 0], out

    def ge_p2_tobytes(self, xyz): return self._fe("dc_ge_p2_tobytes", 8, xyz)

    def hash_k(self, records):
        n = len(records)
        stride = max(len(sm) for sm, _ in records) + 256  # the slack pv_hash_k may read, zeroed
        blob = np.zeros((n, stride), np.uint8)
        for i, (sm, _) in enumerate(records):
            blob[i, :len(sm)] = np.frombuffer(sm, np.uint8)
        lens = np.array([[len(sm)] for sm, _ in records], np.uint64)
        pks = enc_words([pk for _, pk in records])
        out = np.zeros((n, 8), np.uint32)
        rc = self.lib.dc_hash_k(_ptr(out), _ptr(blob), ctypes.c_uint64(stride), _ptr(lens), _ptr(pks), ctypes.c_int(n))
        self.launches += 1
        if rc != 0:
            raise DeviceError("dc_hash_k returned HIP error %d" % rc)
        return out

    def lp_binary(self, f, g, op):
        return self._fe("dc_lp_binary", 40, f, g, scalars=(ctypes.c_int(op),), chunk=WAVE_CHUNK)

    def lp_unary(self, f, op):
        return self._fe("dc_lp_unary", 40, f, scalars=(ctypes.c_int(op),), chunk=WAVE_CHUNK)

    def lp_decompress_ar(self, a, r):
        a, r = _u32(a), _u32(r)
        flags = np.zeros((len(a), 3), np.int32)
        xy = np.zeros((len(a), 80), np.uint32)
        self._run("dc_lp_decompress_ar", WAVE_CHUNK, [flags, xy], [a, r])
        return flags, xy

    def lp_ydbl_check(self, a, r, nd):
        a, r = _u32(a), _u32(r)
        nd = np.ascontiguousarray(np.array(nd, np.int32).reshape(-1, 1))
        out = np.zeros((len(a), 1), np.int32)
        self._run("dc_lp_ydbl_check", WAVE_CHUNK, [out], [a, r, nd])
        return out[:, 0]

    def lp_table_parts_check(self, enc):
        return self._fe("dc_lp_table_parts_check", 1, enc, chunk=WAVE_CHUNK, dtype=np.int32)[:, 0]


# ---------------------------------------------------------------- checkers
def check_limb_bound(h, slack_bits=17, what="limb"):
    """Every limb < 2^width + 2^slack_bits: the "R" bound (17) the next operation's column bound depends
    on, which the device build cannot assert itself; 23 for lp_mul's output."""
    h = np.asarray(h, dtype=np.uint64).reshape(-1, 10)
    bound = np.array([(1 << w) + (1 << slack_bits) for w in W], np.uint64)
    bad = np.nonzero((h >= bound).any(axis=1))[0]
    assert len(bad) == 0, "%s bound 2^w + 2^%d exceeded at element %d: %s" % (what, slack_bits, bad[0], list(h[bad[0]]))


def check_values(h, want, what="value"):
    """from_limbs(h[i]) == want[i] (mod p)."""
    h = np.asarray(h).reshape(-1, 10)
    assert len(h) == len(want)
    for i, w in enumerate(want):
        got = from_limbs(h[i]) % P
        assert got == w % P, "%s %d: got %x, want %x" % (what, i, got, w % P)


def check_field(h, want, slack_bits=17, what="field result"):
    check_values(h, want, what)
    check_limb_bound(h, slack_bits, what)


def check_equal(a, b, what):
    """Word-for-word equality of two backends' outputs (limbs, not only values)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.nonzero(a != b)
    assert len(bad[0]) == 0, "%s: %d words differ, first at %s: %r != %r" % (
        what, len(bad[0]), tuple(int(x[0]) for x in bad), a[tuple(x[0] for x in bad)], b[tuple(x[0] for x in bad)])


def recode_reference(a, w):
    """The digit-by-digit carry loop the closed-form recodings replaced (top digit unreduced)."""
    out, carry, n = 0, 0, 256 // w
    for i in range(n):
        v = ((a >> (w * i)) & ((1 << w) - 1)) + carry
        carry = 0 if i == n - 1 else (v + (1 << (w - 1))) >> w
        out |= ((v - (carry << w)) & ((1 << w) - 1)) << (w * i)
    return out


def check_recode(vals, n_exact, out, radix):
    w = {16: 4, 256: 8, 65536: 16}[radix]
    half, full, n = 1 << (w - 1), 1 << w, 256 // w
    for i, (a, o) in enumerate(zip(vals, ints(out))):
        assert o == recode_reference(a, w), (radix, hex(a))
        if i < n_exact:
            dig = [(o >> (w * j)) & (full - 1) for j in range(n)]
            sd = [d - full if d >= half else d for d in dig]
            assert sum(d * full ** j for j, d in enumerate(sd)) == a, (radix, hex(a))
            assert all(-half <= d <= half for d in sd)


def check_recode_w(vals, n_exact, out, w):
    npos = {16: 16, 24: 11}[w]
    top = 253 - w * (npos - 1)
    for i, s in enumerate(vals):
        d = [int(x) for x in out[i][:npos]]
        assert all(int(x) == 0 for x in out[i][npos:])
        if i < n_exact:
            assert sum(x << (w * j) for j, x in enumerate(d)) == s, (w, s)
        assert all(-(1 << (w - 1)) <= x < (1 << (w - 1)) for x in d[:-1]), (w, s)
        assert 0 <= d[-1] <= (1 << top), (w, s)


def nwin16_reference(a):
    d, c = [], 0
    for i in range(64):
        v = ((a >> (4 * i)) & 15) + c
        c = 0 if i == 63 else (v + 8) >> 4
        d.append(v - 16 * c)
    nz = [i for i, v in enumerate(d) if v]
    return nz[-1] + 1 if nz else 1


def split_results(k1, k2, flags):
    """[(signed k1, k2, fallback)] from a split's outputs."""
    return [((-a if f[0] else a), b, bool(f[1])) for a, b, f in zip(ints(k1), ints(k2), np.asarray(flags))]


def check_split(ks, first_random, k1, k2, flags):
    """The contract of sc_halfsize / lp_halfsize: k1 == k k2 (mod 8L), k2 odd and > 0, |k1| < 2^128 and
    k2 < 2^160 unless the (k, 1) fallback was taken, fallback => (k1, k2) = (k, 1), no random scalar falls
    back, max(bitlen) <= 140; words 5..7 of k2 are zero unless fallback (sc_mul<5> relies on it)."""
    bits = []
    k2w = np.asarray(k2)
    for i, (k, (a, b, fb)) in enumerate(zip(ks, split_results(k1, k2, flags))):
        assert (a - k * b) % N8L == 0, k
        assert b > 0 and b & 1, k
        if fb:
            assert (a, b) == (k, 1), k
            assert i < first_random, "random scalar %d fell back" % k
        else:
            assert abs(a) < 2 ** 128 and b < 2 ** 160, k
            bits.append(max(abs(a).bit_length(), b.bit_length()))
        assert not k2w[i, 5:].any(), k
    assert max(bits) <= 140


def check_decompress(a_encs, r_encs, flags, xy):
    """lp_decompress_ar: ok flags against RFC 8032 decompression, row 0 = -A, row 1 = R with x's parity
    = bit 255, x_r_zero, Y rows = the encodings' y; every limb within lp_mul's output bound."""
    xy = np.asarray(xy)
    for i, (ea, er) in enumerate(zip(a_encs, r_encs)):
        pa, pr = decode_xy(ea), decode_xy(er)
        ok_a, ok_r, xz = (int(v) for v in flags[i])
        assert ok_a == (pa is not None) and ok_r == (pr is not None), i
        X, Y = xy[i, :40], xy[i, 40:]
        ya = int.from_bytes(ea, "little") & (2 ** 255 - 1)
        yr = int.from_bytes(er, "little") & (2 ** 255 - 1)
        assert from_limbs(Y[0:10]) == ya and from_limbs(Y[10:20]) == yr, i
        if pa is not None:
            assert from_limbs(X[0:10]) % P == (P - pa[0]) % P, i
        if pr is not None:
            assert from_limbs(X[10:20]) % P == pr[0], i
            assert xz == (pr[0] == 0), i
    check_limb_bound(xy, 23, "lp_decompress_ar")


# ---------------------------------------------------------------- units
class Unit:
    """inputs() -> tuple (cached); run(backend, inputs) -> tuple of arrays; check(inputs, outputs);
    count = operand sets. exact: the device output must equal the host output word for word."""

    def __init__(self, name, inputs, run, check, exact=True):
        self.name, self._inputs, self.run, self.check, self.exact = name, inputs, run, check, exact
        self._cache = None

    def inputs(self):
        if self._cache is None:
            self._cache = self._inputs()
        return self._cache

    def count(self):
        return len(self.inputs()[0])


def _mk_fe_mul(method):
    def inputs():
        pairs = fe_mul_pairs()
        return limb_rows([f for f, _ in pairs]), limb_rows([g for _, g in pairs])

    def check(ins, outs):
        f, g = ins
        check_field(outs[0], [from_limbs(a) * from_limbs(b) for a, b in zip(f, g)], 17, method)
    return Unit(method, inputs, lambda be, ins: (getattr(be, method)(*ins),), check)


def _mk_fe_unary(name, inputs, want):
    def check(ins, outs):
        check_field(outs[0], [want(from_limbs(f)) for f in ins[0]], 17, name)
    return Unit(name, lambda: (limb_rows(inputs()),), lambda be, ins: (getattr(be, name)(ins[0]),), check)


def _check_tobytes(ins, outs):
    for f, got in zip(ins[0], ints(outs[0])):
        assert got == from_limbs(f) % P, list(f)


def _frombytes_inputs():
    encs, _ = point_encodings()
    encs = encs + [v.to_bytes(32, "little") for v in (0, 1, P - 1, P, 2 ** 255 - 1, 2 ** 256 - 1, 2 ** 255)]
    return (enc_words(encs),)


def _check_frombytes(ins, outs):
    for v, h in zip(ints(ins[0]), outs[0]):
        assert [int(x) for x in h] == to_limbs(v & (2 ** 255 - 1)), hex(v)


def _mk_scalar(name, vals, nw, run, want):
    def check(ins, outs):
        got = ints(outs[0]) if outs[0].ndim == 2 else [int(x) for x in outs[0]]
        for v, g in zip(ints(ins[0]), got):
            assert g == want(v), (name, hex(v))
        assert len(got) == len(ins[0])
    return Unit(name, lambda: (words(vals(), nw),), lambda be, ins: (run(be, ins[0]),), check)


def _mk_sc_mul(na):
    name = "sc_mul" if na == 8 else "sc_mul<5>"

    def inputs():
        pairs = sc_mul_inputs(na)
        return words([a for a, _ in pairs], 8), words([b for _, b in pairs], 8)

    def check(ins, outs):
        assert ints(outs[0]) == [a * b % L for a, b in zip(ints(ins[0]), ints(ins[1]))], name
    return Unit(name, inputs, lambda be, ins: (be.sc_mul(ins[0], ins[1], na),), check)


def _mk_recode(radix):
    def inputs():
        vals, n_exact = sc_recode_inputs()
        return words(vals, 8), n_exact

    def check(ins, outs):
        check_recode(ints(ins[0]), ins[1], outs[0], radix)
    return Unit("sc_recode%d" % radix, inputs, lambda be, ins: (be.sc_recode(ins[0], radix),), check)


def _mk_recode_w(w):
    def inputs():
        vals, n_exact = wide_recode_inputs(w)
        return words(vals, 8), n_exact

    def check(ins, outs):
        check_recode_w(ints(ins[0]), ins[1], outs[0], w)
    return Unit("sc_recode_w<%d>" % w, inputs, lambda be, ins: (be.sc_recode_w(ins[0], w),), check)


def _mk_split(method):
    def inputs():
        ks, first_random = split_inputs()
        return words(ks, 8), first_random

    def check(ins, outs):
        check_split(ints(ins[0]), ins[1], *outs)
    return Unit(method, inputs, lambda be, ins: getattr(be, method)(ins[0]), check, exact=False)


def _enc_inputs():
    encs, first_random = point_encodings()
    return enc_words(encs), encs, first_random


def _check_enc_rules(ins, outs):
    from vectors import BLACKLIST
    for e, (small, canon) in zip(ins[1], outs[0]):
        y = int.from_bytes(e, "little") & (2 ** 255 - 1)
        assert bool(small) == (y.to_bytes(32, "little") in BLACKLIST), e.hex()
        assert bool(canon) == (y < P), e.hex()
    assert int(outs[0][:, 0].sum()) >= 14  # the seven blacklisted encodings, with and without bit 255


def _check_frombytes_negate(ins, outs):
    ok, out = outs
    for i, e in enumerate(ins[1]):
        pt = decode_xy(e)
        assert bool(ok[i]) == (pt is not None), e.hex()
        if pt is None:
            continue
        X, Y, Z, T = (from_limbs(out[i, 10 * r:10 * r + 10]) % P for r in range(4))
        assert (X, Y, Z) == ((P - pt[0]) % P, pt[1], 1) and T == X * Y % P, e.hex()
        check_limb_bound(out[i], 17, "ge_frombytes_negate")
    assert int(np.asarray(ok)[ins[2]:].sum()) >= 150  # about half of the random strings decompress


def _p2_unit_inputs():
    pts = p2_inputs()
    return limb_rows([to_limbs(x) + to_limbs(y) + to_limbs(z) for x, y, z in pts]), pts


def _check_p2(ins, outs):
    for (x, y, z), got in zip(ins[1], ints(outs[0])):
        zi = pow(z, P - 2, P)
        xa, ya = x * zi % P, y * zi % P
        assert got == ya | ((xa & 1) << 255), (x, y, z)


def _check_hash(ins, outs):
    for (sm, pk), got in zip(ins[0], ints(outs[0])):
        want = int.from_bytes(hashlib.sha512(sm[:32] + pk + sm[64:]).digest(), "little") % L
        assert got == want, len(sm)


def _rows_values(rows40):
    return [from_limbs(rows40[10 * r:10 * r + 10]) for r in range(4)]


def _mk_lp_mul(name, op, inputs):
    def check(ins, outs):
        want = [a * b for f, g in zip(*ins) for a, b in zip(_rows_values(f), _rows_values(g))]
        check_field(outs[0], want, 23, name)
    return Unit(name, lambda: tuple(limb_rows(x) for x in inputs()), lambda be, ins: (be.lp_binary(ins[0], ins[1], op),), check)


def _mk_lp_chain(name, op, dual, seed, n_reduced, n_wide, exponent):
    def check(ins, outs):
        want = [pow(v % P, exponent, P) for f in ins[0] for v in _rows_values(f)]
        check_field(outs[0], want, 23, name)
    return Unit(name, lambda: (limb_rows(lp_chain_inputs(dual, seed, n_reduced, n_wide)),),
                lambda be, ins: (be.lp_unary(ins[0], op),), check)


def _lp_point_pairs():
    pts = lp_points()
    pairs = [(p, q) for p in pts for q in pts]
    return limb_rows([ext_rows(p) for p, _ in pairs]), limb_rows([ext_rows(q) for _, q in pairs]), pairs


def _check_lp_dbl(ins, outs):
    for p, h in zip(ins[1], outs[0]):
        assert affine_of_rows(h) == pt_add(p, p)
    check_limb_bound(outs[0], 23, "lp_dbl")


def _mk_lp_add(name, op):
    def check(ins, outs):
        for (p, q), h in zip(ins[2], outs[0]):
            q2 = q if op == 2 else ((P - q[0]) % P, q[1])
            assert affine_of_rows(h) == pt_add(p, q2), name
        check_limb_bound(outs[0], 23, name)
    return Unit(name, _lp_point_pairs, lambda be, ins: (be.lp_binary(ins[0], ins[1], op),), check)


def _decompress_inputs():
    encs, _ = point_encodings()
    r = [encs[(i * 7 + 3) % len(encs)] for i in range(len(encs))]
    return enc_words(encs), enc_words(r), encs, r


def _ydbl_unit_inputs():
    a, r, nd = ydbl_inputs()
    return enc_words(a), enc_words(r), nd, a, r


def _check_ydbl(ins, outs):
    tested = 0
    for i, got in enumerate(outs[0]):
        both = decode_xy(ins[3][i]) is not None and decode_xy(ins[4][i]) is not None
        assert int(got) == (3 if both else -1), (i, ins[2][i])
        tested += both
    assert tested >= 50


def _table_parts_unit_inputs():
    encs = table_parts_inputs()
    return enc_words(encs), encs


def _check_table_parts(ins, outs):
    tested = 0
    for e, got in zip(ins[1], outs[0]):
        ok = decode_xy(e) is not None
        assert int(got) == (1 if ok else -1), e.hex()
        tested += ok
    assert tested >= 50


def _build_units():
    inv = lambda x: pow(x, P - 2, P)  # noqa: E731
    u = [
        _mk_fe_mul("fe_mul"),
        _mk_fe_mul("fe_mul_pre"),
        _mk_fe_unary("fe_sq", fe_sq_inputs, lambda x: x * x),
        _mk_fe_unary("fe_carry", fe_carry_inputs, lambda x: x),
        Unit("fe_tobytes", lambda: (limb_rows(fe_tobytes_inputs()),), lambda be, ins: (be.fe_tobytes(ins[0]),), _check_tobytes),
        Unit("fe_frombytes", _frombytes_inputs, lambda be, ins: (be.fe_frombytes(ins[0]),), _check_frombytes),
        _mk_fe_unary("fe_invert", lambda: [to_limbs(x) for x in fe_chain_inputs()], inv),
        _mk_fe_unary("fe_pow22523", lambda: [to_limbs(x) for x in fe_chain_inputs()], lambda x: pow(x, (P - 5) // 8, P)),
        _mk_scalar("sc_reduce64", sc_reduce_inputs, 16, lambda be, x: be.sc_reduce64(x), lambda v: v % L),
        _mk_scalar("sc_is_canonical", sc_canonical_inputs, 8, lambda be, x: be.sc_is_canonical(x), lambda v: int(v < L)),
        _mk_sc_mul(8),
        _mk_sc_mul(5),
        _mk_recode(16),
        _mk_recode(256),
        _mk_recode(65536),
        _mk_recode_w(16),
        _mk_recode_w(24),
        _mk_scalar("sc_nwin16", nwin16_inputs, 8, lambda be, x: be.sc_nwin16(x), nwin16_reference),
        _mk_split("sc_halfsize"),
        Unit("enc_rules", _enc_inputs, lambda be, ins: (be.enc_rules(ins[0]),), _check_enc_rules),
        Unit("ge_frombytes_negate", _enc_inputs, lambda be, ins: be.ge_frombytes_negate(ins[0]), _check_frombytes_negate),
        Unit("ge_p2_tobytes", _p2_unit_inputs, lambda be, ins: (be.ge_p2_tobytes(ins[0]),), _check_p2),
        Unit("pv_hash_k", lambda: (hash_records(),), lambda be, ins: (be.hash_k(ins[0]),), _check_hash),
        _mk_lp_mul("lp_mul", 0, lp_mul_inputs),
        _mk_lp_mul("lp_mul_dual", 1, lp_mul_dual_inputs),
        _mk_lp_chain("lp_invert", 0, False, 41, 4, 2, P - 2),
        _mk_lp_chain("lp_invert<true>", 1, True, 43, 3, 1, P - 2),
        _mk_lp_chain("lp_pow22523", 2, False, 4, 5, 2, (P - 5) // 8),
        _mk_lp_chain("lp_pow22523<true>", 3, True, 44, 4, 1, (P - 5) // 8),
        Unit("lp_dbl", lambda: (limb_rows([ext_rows(p) for p in lp_points()]), lp_points()),
             lambda be, ins: (be.lp_unary(ins[0], 4),), _check_lp_dbl),
        _mk_lp_add("lp_add_cached", 2),
        _mk_lp_add("lp_add_cached(neg)", 3),
        _mk_split("lp_halfsize"),
        Unit("lp_decompress_ar", _decompress_inputs, lambda be, ins: be.lp_decompress_ar(ins[0], ins[1]),
             lambda ins, outs: check_decompress(ins[2], ins[3], *outs)),
        Unit("lp_ydbl_chain", _ydbl_unit_inputs, lambda be, ins: (be.lp_ydbl_check(ins[0], ins[1], ins[2]),), _check_ydbl),
        Unit("lp_table_parts", _table_parts_unit_inputs, lambda be, ins: (be.lp_table_parts_check(ins[0]),), _check_table_parts),
    ]
    return {x.name: x for x in u}


UNITS = _build_units()


# ---------------------------------------------------------------- lane layouts for the per-lane split
def split_lane_layouts():
    """Layouts that make neighbouring lanes of a wave leave sc_halfsize's block loop and step loop at
    different iterations. pool: the edge scalars and 64 random ones; `uniform`: every pool scalar 64
    times (one wave each); `mixed`: 4096 + 37 lanes (a partial last wave), every wave starting with k = 0,
    k = 1 (no block, no step), L - 1 (one block, then the (k, 1) fallback) and a random scalar (several
    blocks and steps) side by side, the rest drawn from the pool in seeded order."""
    rnd = split_random()[0][:64]
    pool = split_edges() + rnd
    uniform = [k for k in pool for _ in range(64)]
    rng = random.Random(48)
    mixed = []
    for i in range(4096 + 37):
        lead = (0, 1, L - 1, rnd[(i // 64) % 64])
        mixed.append(lead[i % 64] if i % 64 < 4 else pool[rng.randrange(len(pool))])
    return pool, uniform, mixed
