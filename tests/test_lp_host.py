"""The latency path's limb-parallel arithmetic (indy-plenum_amd/csrc/lp25519.h) on the HOST: the
64 lanes of a wave simulated exactly (DPP row broadcast / rotate / shift and the gfx950 permlane
swaps as specified), every lp_mul column recomputed in 128 bits and bound-checked (PV_BOUNDS_CHECK),
against Python big integers, the C oracle, the golden libsodium verdicts and libsodium itself.
A pass here proves the limb-parallel algorithms and their bounds on a MODEL of the lane instructions
(row_newbcast / row_ror / row_shr / row_shl with bound_ctrl, permlane16_swap, permlane32_swap,
readlane, ballot); whether the model matches the hardware is checked by tests/test_gpu_devarith.py,
which runs the device forms on the GPU with the same operands and compares them with this simulation
limb for limb (shared vectors: tests/devarith_cases.py). tests/test_gpu_parity.py runs the whole
latency path on the GPU (PV_PATH_LATENCY)."""
import ctypes
import json
import os
import random

import pytest

from devarith_cases import LP_MUL_COMBOS, LP_MUL_DUAL_COMBOS, rand_limbs
from test_native_host import HERE, L, P, W, from_limbs, hc, to_limbs  # noqa: F401

A40 = ctypes.c_uint32 * 40
D = (-121665 * pow(121666, P - 2, P)) % P


def rows_in(vals):
    out = []
    for v in vals:
        out += v if isinstance(v, list) else to_limbs(v)
    return A40(*out)


def rows_out(a):
    a = list(a)
    return [a[10 * r:10 * r + 10] for r in range(4)]


def test_lp_mul_random_and_bounds(hc):
    rng = random.Random(3)
    h = A40()
    # operand widths the group formulas produce: LR products, sums of two (2^27.13), differences
    # with 2p (2^27.6) on either side, and the doubling's uncarried E (2^28.4) against H or F
    combos = LP_MUL_COMBOS
    for it in range(600):
        fb, gb = combos[it % len(combos)]
        f = [rand_limbs(rng, fb) for _ in range(4)]
        g = [rand_limbs(rng, gb) for _ in range(4)]
        if it < len(combos):
            f = [[int(2 ** (fb - (i & 1))) - 1 for i in range(10)]] * 4
            g = [[int(2 ** (gb - (i & 1))) - 1 for i in range(10)]] * 4
        hc.hc_lp_mul(h, rows_in(f), rows_in(g))
        for r, hr in enumerate(rows_out(h)):
            assert from_limbs(hr) % P == from_limbs(f[r]) * from_limbs(g[r]) % P, (it, r)
            for k, x in enumerate(hr):
                assert x < (1 << W[k]) + (1 << 23)
    for _ in range(200):
        f = [rng.randrange(P) for _ in range(4)]
        g = [rng.randrange(P) for _ in range(4)]
        hc.hc_lp_mul(h, rows_in(f), rows_in(g))
        for r, hr in enumerate(rows_out(h)):
            assert from_limbs(hr) % P == f[r] * g[r] % P


def test_lp_pow22523(hc):
    rng = random.Random(4)
    h = A40()
    for _ in range(5):
        z = [rng.randrange(P) for _ in range(4)]
        hc.hc_lp_pow22523(h, rows_in(z))
        for r, hr in enumerate(rows_out(h)):
            assert from_limbs(hr) % P == pow(z[r], (P - 5) // 8, P)


def test_lp_invert(hc):
    """lp_invert (the encode kernel's wave-wide inversion, PvWaveInvert): 1 / z in every row, for
    reduced inputs and for limbs at the lp_mul output bound."""
    rng = random.Random(41)
    h = A40()
    for it in range(6):
        if it < 4:
            z = [rng.randrange(1, P) for _ in range(4)]
            hc.hc_lp_invert(h, rows_in(z))
        else:  # unreduced limbs as the products that feed it leave them (< 2^26 + 2^23)
            limbs = [rand_limbs(rng, 26.1) for _ in range(4)]
            z = [from_limbs(l) % P or 1 for l in limbs]
            arr = A40(*[v for l in limbs for v in l])
            hc.hc_lp_invert(h, arr)
        for r, hr in enumerate(rows_out(h)):
            assert from_limbs(hr) % P == pow(z[r], P - 2, P), (it, r)


def test_lp_invert_dual(hc):
    """lp_invert<true> (the form the encode's wave inversion uses): two values in rows 0, 1, repeated in
    rows 2, 3 (the wave tree's two products), 1 / z in every row."""
    rng = random.Random(43)
    h = A40()
    for it in range(4):
        if it < 3:
            z = [rng.randrange(1, P) for _ in range(2)]
            hc.hc_lp_invert_dual(h, rows_in(z + z))
        else:
            limbs = [rand_limbs(rng, 26.1) for _ in range(2)]
            z = [from_limbs(l) % P or 1 for l in limbs]
            hc.hc_lp_invert_dual(h, A40(*[v for l in limbs + limbs for v in l]))
        for r, hr in enumerate(rows_out(h)):
            assert from_limbs(hr) % P == pow(z[r & 1], P - 2, P), (it, r)


def test_lp_mul_dual_matches_lp_mul(hc):
    """lp_mul_dual (the decompression chain's product: rows 0, 1 sum column terms 0..4, rows 2, 3 terms
    5..9 on operands pre-rotated by five limbs, halves added across with v_permlane32_swap) gives
    lp_mul's limbs exactly, in all four rows, at the operand widths the chain forms; the dual
    z^((p-5)/8) matches Python."""
    rng = random.Random(5)
    h, h2 = A40(), A40()
    for it in range(400):
        fb, gb = LP_MUL_DUAL_COMBOS[it % 3]
        f = [rand_limbs(rng, fb) for _ in range(2)]
        g = [rand_limbs(rng, gb) for _ in range(2)]
        if it < 3:
            f = [[int(2 ** (fb - (i & 1))) - 1 for i in range(10)]] * 2
            g = [[int(2 ** (gb - (i & 1))) - 1 for i in range(10)]] * 2
        fr, gr = rows_in(f + f), rows_in(g + g)
        hc.hc_lp_mul(h, fr, gr)
        hc.hc_lp_mul_dual(h2, fr, gr)
        want = rows_out(h)
        assert rows_out(h2) == [want[0], want[1], want[0], want[1]], it
    for _ in range(4):
        z = [rng.randrange(P) for _ in range(2)]
        hc.hc_lp_pow22523_dual(h, rows_in(z + z))
        for r, hr in enumerate(rows_out(h)):
            assert from_limbs(hr) % P == pow(z[r & 1], (P - 5) // 8, P)


def _decode(enc):
    """(x, y) of an Ed25519 encoding (RFC 8032 decompression)."""
    y = int.from_bytes(enc, "little") & (2 ** 255 - 1)
    s = enc[31] >> 7
    u, v = (y * y - 1) % P, (D * y * y + 1) % P
    x = u * pow(v, 3, P) * pow(u * pow(v, 7, P), (P - 5) // 8, P) % P
    if v * x * x % P != u:
        x = x * pow(2, (P - 1) // 4, P) % P
    if x & 1 != s:
        x = P - x
    return x, y


def _ext(pt):
    x, y = pt
    return [x, y, 1, x * y % P]


def _affine(rows):
    X, Y, Z, T = (from_limbs(r) % P for r in rows)
    zi = pow(Z, P - 2, P)
    assert X * Y % P == T * Z % P  # T consistent
    return X * zi % P, Y * zi % P


def _add(p, q):
    (x1, y1), (x2, y2) = p, q
    t = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + x2 * y1) * pow(1 + t, P - 2, P) % P, (y1 * y2 + x1 * x2) * pow(1 - t, P - 2, P) % P)


def test_lp_group_ops(hc, oracle):
    rng = random.Random(5)
    out = A40()
    from vectors import ORDER8
    pts = [_decode(oracle.scalarmult_base(rng.randrange(1, L).to_bytes(32, "little"))) for _ in range(6)]
    pts += [_decode(ORDER8), (0, 1), (0, P - 1)]  # small order, identity, order 2
    for p in pts:
        hc.hc_lp_dbl(out, rows_in(_ext(p)))
        assert _affine(rows_out(out)) == _add(p, p)
        for q in pts:
            hc.hc_lp_add(out, rows_in(_ext(p)), rows_in(_ext(q)))
            assert _affine(rows_out(out)) == _add(p, q)
            hc.hc_lp_sub(out, rows_in(_ext(p)), rows_in(_ext(q)))
            assert _affine(rows_out(out)) == _add(p, ((P - q[0]) % P, q[1]))


def _lp_open(hc, sm, pk):
    return bool(hc.hc_lp_sign_open(sm, ctypes.c_uint64(len(sm)), pk))


def test_lp_path_golden_verdicts(hc):
    with open(os.path.join(HERE, "golden", "verdicts.json")) as f:
        cases = json.load(f)
    # every class, a bounded sample (each host-simulated verification runs ~900 lp products)
    seen = {}
    for c in cases:
        seen.setdefault((c["cls"], c["ok"]), []).append(c)
    for key, cs in sorted(seen.items()):
        for c in cs[:3]:
            sm, pk = bytes.fromhex(c["sm"]), bytes.fromhex(c["pk"])
            assert _lp_open(hc, sm, pk) == c["ok"], key


@pytest.mark.slow
def test_lp_path_vs_libsodium(hc, sodium, oracle):
    from vectors import VectorGen
    g = VectorGen(sodium, oracle, seed=23)
    for cls in VectorGen.CLASSES:
        for _ in range(3):
            sm, pk = g.make(cls)
            assert _lp_open(hc, sm, pk) == sodium.sign_open_ok(sm, pk), cls


def test_lp_cached_key_path_golden_verdicts(hc):
    """The key-cache branch of the latency kernel (32 comb-table additions for [k](-A))."""
    with open(os.path.join(HERE, "golden", "verdicts.json")) as f:
        cases = json.load(f)
    seen = {}
    for c in cases:
        seen.setdefault((c["cls"], c["ok"]), []).append(c)
    for key, cs in sorted(seen.items()):
        for c in cs[:2]:
            sm, pk = bytes.fromhex(c["sm"]), bytes.fromhex(c["pk"])
            assert bool(hc.hc_lp_sign_open_cached(sm, ctypes.c_uint64(len(sm)), pk)) == c["ok"], key


def test_lp_key_chain_matches_per_lane_chain(hc, oracle):
    """pv_key_chain_lp_kernel's chain (lp doublings, then a carry to reduced limbs) stores the same
    bases [256^i](-A), [16], [32], [64] multiples as the per-lane chain the fill kernel was built on."""
    rng = random.Random(8)
    from vectors import ORDER8
    keys = [oracle.scalarmult_base(rng.randrange(1, L).to_bytes(32, "little")) for _ in range(3)]
    keys.append(oracle.point_add(keys[0], ORDER8))  # mixed-order key
    for pk in keys:
        assert hc.hc_lp_chain_check(pk) == 0


def test_lp_key_chain_in_parts(hc, oracle):
    """The chain kernel's [lo, hi) form (the keyed launch runs one part; in parts, each resumes from the
    previous part's stored, carried P_lo) stores the same points as the per-lane chain, with consistent T,
    for 1, 2, 4 and 8 parts."""
    rng = random.Random(9)
    from vectors import ORDER8
    keys = [oracle.scalarmult_base(rng.randrange(1, L).to_bytes(32, "little")) for _ in range(2)]
    keys.append(oracle.point_add(keys[0], ORDER8))
    for pk in keys:
        for parts in (1, 2, 4, 8):
            assert hc.hc_lp_chain_parts_check(pk, parts) == 0, parts


def test_lp4_path_vs_libsodium(hc, sodium, oracle):
    """The four-wave latency form (pv_lat4_kernel's arithmetic: the half-size split, each scalar cut
    at window 17 with the high part on [2^68]-multiples) against golden verdicts of every class and
    libsodium on every adversarial class, mixed-order A and R included; split points 1 and 40 too
    (one scalar part empty / a split beyond the window count)."""
    from vectors import VectorGen
    with open(os.path.join(HERE, "golden", "verdicts.json")) as f:
        cases = json.load(f)
    seen = {}
    for c in cases:
        seen.setdefault((c["cls"], c["ok"]), []).append(c)
    for key, cs in sorted(seen.items()):
        c = cs[0]
        sm, pk = bytes.fromhex(c["sm"]), bytes.fromhex(c["pk"])
        assert bool(hc.hc_lp4_sign_open(sm, ctypes.c_uint64(len(sm)), pk, 17)) == c["ok"], key
    g = VectorGen(sodium, oracle, seed=29)
    for cls in VectorGen.CLASSES:
        for split in (17, 1, 40):
            sm, pk = g.make(cls)
            assert bool(hc.hc_lp4_sign_open(sm, ctypes.c_uint64(len(sm)), pk, split)) == sodium.sign_open_ok(sm, pk), (cls, split)
