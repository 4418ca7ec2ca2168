"""The kernels' own arithmetic (indy-plenum_amd/csrc/*.h), compiled for the HOST with bound
assertions enabled (tests/native/hostcheck.hip), against Python big integers, the oracle, the
golden libsodium verdicts and libsodium itself. A pass here proves the algorithms, the limb bounds
and every line the host and device builds share. It does NOT prove the branches the headers take only
under __HIP_DEVICE_COMPILE__ (fe_mul_pre / fe_sq's inline-asm product columns, dbl32, v_rcp_f32 and
__all in sc_halfsize, sha512.h's alignbit / bitop3 / perm): the host build compiles the plain C on the
other side of each switch. tests/test_gpu_devarith.py runs those branches on the GPU with the same edge
inputs (tests/devarith_cases.py holds the shared vectors); tests/test_gpu_parity.py checks them end
to end."""
import ctypes
import json
import os
import random
import subprocess

import pytest

from devarith_cases import (HALFSIZE_EDGES, L, LP_HALFSIZE_EDGES, N8L, NWIN16_EDGES, P, SC_CANONICAL_EDGES,  # noqa: F401
                            SC_MUL_EDGES, SC_RECODE_ANY_EDGES, SC_RECODE_EDGES, SC_REDUCE_EDGES, TOBYTES_EDGES,
                            TOBYTES_UNNORMALISED, W, WIDE_RECODE_TOO_LARGE, from_limbs, max_mul_input, to_limbs,
                            wide_f_operand_pairs, wide_recode_edges)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(HERE, "native", "libhostcheck.so")
A10 = ctypes.c_uint32 * 10


def build_hostcheck():
    # -O1: the host simulation of the limb-parallel code compiles in ~5 min instead of ~16 at -O2,
    # and the whole host suite still runs in seconds
    src = os.path.join(HERE, "native", "hostcheck.hip")
    cmd = ["/opt/rocm/bin/hipcc", "-O1", "-fPIC", "-shared", "-pthread", "--offload-arch=gfx950", "--offload-host-only",
           "-I" + os.path.join(ROOT, "indy-plenum_amd", "csrc"), src, "-o", LIB]
    subprocess.check_call(cmd)


@pytest.fixture(scope="module")
def hc():
    srcs = [os.path.join(ROOT, "indy-plenum_amd", "csrc", f)
            for f in os.listdir(os.path.join(ROOT, "indy-plenum_amd", "csrc")) if f.endswith(".h")]
    srcs.append(os.path.join(HERE, "native", "hostcheck.hip"))
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in srcs):
        build_hostcheck()
    return ctypes.CDLL(LIB)


def test_fe_mul_sq_random_and_extreme(hc):
    rng = random.Random(7)
    cases = [(max_mul_input(), max_mul_input())]
    for _ in range(3000):
        f = [rng.randrange(3 * (1 << w) + (1 << 18)) for w in W]
        g = [rng.randrange(3 * (1 << w) + (1 << 18)) for w in W]
        cases.append((f, g))
        cases.append((to_limbs(rng.randrange(P)), to_limbs(rng.randrange(P))))
    h = A10()
    for f, g in cases:
        hc.hc_fe_mul(h, A10(*f), A10(*g))
        assert from_limbs(list(h)) % P == from_limbs(f) * from_limbs(g) % P
        hc.hc_fe_sq(h, A10(*f))
        assert from_limbs(list(h)) % P == from_limbs(f) ** 2 % P


def test_fe_mul_wide_f_operand_bounds(hc):
    """The f side of fe_mul may be an uncarried value (ge_p2_dbl's r.X = S + 4p - r.Y, the niels
    F = 2Z + 2p - c): at those maxima, against the largest g each call site passes, every
    product column still fits 64 bits (the bounds build asserts it) and the product is right."""
    h = A10()
    for f, g in wide_f_operand_pairs():  # (dbl_rx, R), (niels_f, G3), (G3, G3)
        hc.hc_fe_mul(h, A10(*f), A10(*g))
        assert from_limbs(list(h)) % P == from_limbs(f) * from_limbs(g) % P
        assert all(v < (1 << w) + (1 << 19) for v, w in zip(h, W))


def test_fe_tobytes_canonical_edges(hc):
    s = ctypes.create_string_buffer(32)
    for v in TOBYTES_EDGES:
        hc.hc_fe_tobytes(s, A10(*to_limbs(v)))
        assert int.from_bytes(s.raw, "little") == v % P, v
    for v in TOBYTES_UNNORMALISED:  # non-normalised representations
        lim = to_limbs(v % 2 ** 255)
        lim[0] += v - from_limbs(lim)
        if lim[0] < 2 ** 31:
            hc.hc_fe_tobytes(s, A10(*lim))
            assert int.from_bytes(s.raw, "little") == v % P, v


def test_fe_invert_pow(hc):
    rng = random.Random(8)
    h = A10()
    for _ in range(40):
        x = rng.randrange(1, P)
        hc.hc_fe_invert(h, A10(*to_limbs(x)))
        assert from_limbs(list(h)) * x % P == 1
        hc.hc_fe_pow22523(h, A10(*to_limbs(x)))
        assert from_limbs(list(h)) % P == pow(x, (P - 5) // 8, P)


def test_scalar_reduce_canonical_recode(hc):
    rng = random.Random(9)
    r = ctypes.create_string_buffer(32)
    for x in SC_REDUCE_EDGES + [rng.getrandbits(512) for _ in range(5000)]:
        hc.hc_sc_reduce64(r, x.to_bytes(64, "little"))
        assert int.from_bytes(r.raw, "little") == x % L
    for s in SC_CANONICAL_EDGES + [rng.getrandbits(256) for _ in range(2000)]:
        assert hc.hc_sc_is_canonical(s.to_bytes(32, "little")) == (s < L)
    for a in SC_RECODE_EDGES + [rng.randrange(L) for _ in range(2000)]:
        hc.hc_sc_recode16(r, a.to_bytes(32, "little"))
        nib = [(r.raw[i // 2] >> (4 * (i % 2))) & 15 for i in range(64)]
        assert sum((n - 16 if n >= 8 else n) * 16 ** i for i, n in enumerate(nib)) == a
        assert all(-8 <= (n - 16 if n >= 8 else n) <= 8 for n in nib)
        hc.hc_sc_recode256(r, a.to_bytes(32, "little"))
        assert sum((b - 256 if b >= 128 else b) * 256 ** i for i, b in enumerate(r.raw)) == a
        hc.hc_sc_recode65536(r, a.to_bytes(32, "little"))
        hw = [int.from_bytes(r.raw[2 * i:2 * i + 2], "little") for i in range(16)]
        assert sum((h - 65536 if h >= 32768 else h) * 65536 ** i for i, h in enumerate(hw)) == a
    # the closed-form recodings ((a + M) xor M) against the digit-by-digit carry loop they replaced,
    # for any 256-bit input (the top digit unreduced)
    for a in SC_RECODE_ANY_EDGES + [rng.getrandbits(256) for _ in range(2000)]:
        for w, fn in ((4, hc.hc_sc_recode16), (8, hc.hc_sc_recode256), (16, hc.hc_sc_recode65536)):
            out, carry, n = 0, 0, 256 // w
            for i in range(n):
                v = ((a >> (w * i)) & ((1 << w) - 1)) + carry
                carry = 0 if i == n - 1 else (v + (1 << (w - 1))) >> w
                out |= ((v - (carry << w)) & ((1 << w) - 1)) << (w * i)
            fn(r, a.to_bytes(32, "little"))
            assert int.from_bytes(r.raw, "little") == out, (w, hex(a))


def test_small_order_and_canonical_rules(hc):
    from vectors import BLACKLIST
    for b in BLACKLIST:
        for top in (0, 0x80):
            e = bytearray(b)
            e[31] |= top
            assert hc.hc_has_small_order(bytes(e)) == 1
    assert hc.hc_has_small_order(bytes([2]) + bytes(31)) == 0
    for y in range(P - 3, 2 ** 255):
        assert hc.hc_ge_is_canonical(y.to_bytes(32, "little")) == (y < P)


def test_base_point_table(hc, oracle):
    tab = (ctypes.c_uint32 * (129 * 32))()
    hc.hc_build_b_table(tab)
    d = (-121665 * pow(121666, P - 2, P)) % P
    for j in [0, 1, 2, 3, 64, 127, 128]:
        e = tab[j * 32:(j + 1) * 32]
        ypx, ymx, xy2d = from_limbs(e[0:10]), from_limbs(e[10:20]), from_limbs(e[20:30])
        y = (ypx + ymx) * pow(2, P - 2, P) % P
        x = (ypx - ymx) * pow(2, P - 2, P) % P
        assert xy2d == 2 * d * x * y % P
        enc = bytearray(y.to_bytes(32, "little"))
        enc[31] |= (x & 1) << 7
        want = oracle.scalarmult_base(j.to_bytes(32, "little")) if j else (1).to_bytes(32, "little")
        assert bytes(enc) == want, j


def test_pipeline_matches_golden_verdicts(hc):
    with open(os.path.join(HERE, "golden", "verdicts.json")) as f:
        cases = json.load(f)
    for c in cases:
        sm, pk = bytes.fromhex(c["sm"]), bytes.fromhex(c["pk"])
        assert bool(hc.hc_sign_open(sm, ctypes.c_uint64(len(sm)), pk)) == c["ok"], c["cls"]


def test_pipeline_vs_libsodium(hc, sodium, oracle):
    from vectors import VectorGen
    g = VectorGen(sodium, oracle, seed=21)
    for cls in VectorGen.CLASSES:
        for _ in range(10):
            sm, pk = g.make(cls)
            assert bool(hc.hc_sign_open(sm, ctypes.c_uint64(len(sm)), pk)) == sodium.sign_open_ok(sm, pk), cls


@pytest.mark.parametrize("form", ["default", "two_groups_16"])
def test_encode_batch_shared_inversion(hc, form):
    """pv_encode_batch (one inversion per PV_ENC_BATCH points) and the 16-point two-group form
    (pv_encode_batch_stream_b<16>) == per-point x/z, y/z encoding; a point with its use flag clear or
    Z = 0 does not disturb the others."""
    m = hc.hc_enc_batch_size() if form == "default" else 16
    encode = hc.hc_encode_batch if form == "default" else hc.hc_encode_batch16
    rng = random.Random(11)
    for trial in range(200):
        pts, use, want = [], [], []
        for t in range(m):
            x, y, z = (rng.randrange(P) for _ in range(3))
            z = z or 1
            kind = rng.randrange(6)
            u = 1
            if kind == 0:
                z, u = 0, 1          # Z = 0 must be dropped by the zero check
            elif kind == 1:
                u = 0                # flagged out by the caller
            pts += to_limbs(x) + to_limbs(y) + to_limbs(z)
            use.append(u)
            if u and z:
                zi = pow(z, P - 2, P)
                xa, ya = x * zi % P, y * zi % P
                want.append((ya | ((xa & 1) << 255)).to_bytes(32, "little"))
            else:
                want.append(None)
        xyz = (ctypes.c_uint32 * (30 * m))(*pts)
        u_arr = (ctypes.c_int * m)(*use)
        out = ctypes.create_string_buffer(32 * m)
        encode(out, xyz, u_arr)
        for t in range(m):
            assert bool(u_arr[t]) == (want[t] is not None)
            if want[t] is not None:
                assert out.raw[32 * t:32 * t + 32] == want[t], (trial, t)


def test_comb_path_matches_golden_verdicts(hc):
    """The keyed comb arithmetic (comb.h: key chain, table fill, 64-addition accumulation, batched
    encoding), host-compiled with bound checks, against every golden libsodium verdict."""
    with open(os.path.join(HERE, "golden", "verdicts.json")) as f:
        cases = json.load(f)
    for c in cases:
        sm, pk = bytes.fromhex(c["sm"]), bytes.fromhex(c["pk"])
        assert bool(hc.hc_sign_open_comb(sm, ctypes.c_uint64(len(sm)), pk)) == c["ok"], c["cls"]


def test_comb_path_vs_libsodium(hc, sodium, oracle):
    from vectors import VectorGen
    g = VectorGen(sodium, oracle, seed=22)
    for cls in VectorGen.CLASSES:
        for _ in range(3):
            sm, pk = g.make(cls)
            assert bool(hc.hc_sign_open_comb(sm, ctypes.c_uint64(len(sm)), pk)) == sodium.sign_open_ok(sm, pk), cls


def _recode_w(hc, w, s):
    out = (ctypes.c_int32 * 16)()
    p = hc.hc_sc_recode_w(w, out, s.to_bytes(32, "little"))
    return list(out[:p])


def test_wide_comb_recode(hc):
    """sc_recode_w<W, P> (the wide fixed-base comb's digits of S): sum d_j 2^(W j) == S for every
    S < 2^253, d_j in [-2^(W-1), 2^(W-1)) below the top, top in [0, 2^TOP]; S >= 2^253 (rejected by
    the S < L check before any point arithmetic) keeps every digit inside its table row."""
    rng = random.Random(31)
    for w, npos in ((16, 16), (20, 13), (22, 12), (24, 11)):
        top = 253 - w * (npos - 1)
        vals = wide_recode_edges(w) + \
               [rng.randrange(L) for _ in range(1500)] + [rng.getrandbits(253) for _ in range(500)]
        for s in vals:
            d = _recode_w(hc, w, s)
            assert len(d) == npos
            assert sum(x << (w * j) for j, x in enumerate(d)) == s, (w, s)
            assert all(-(1 << (w - 1)) <= x < (1 << (w - 1)) for x in d[:-1])
            assert 0 <= d[-1] <= (1 << top)
        for s in WIDE_RECODE_TOO_LARGE:
            d = _recode_w(hc, w, s)
            assert all(-(1 << (w - 1)) <= x < (1 << (w - 1)) for x in d[:-1]) and 0 <= d[-1] <= (1 << top)


def test_wide_comb_build_run_matches_table(hc):
    """pv_bc2_build_run (the device build of the wide comb, one run per thread: double-and-add start,
    P-steps, one batched inversion) gives exactly the entries of the host-built radix-65536 table at
    W = 16, including d = 0 (identity) and a run that ends at the row's last entry."""
    tab = hc.hc_bcomb_table
    tab.restype = ctypes.POINTER(ctypes.c_uint32)
    base = tab()
    ent, stride = 32769, 32
    for j, d0, cnt in ((0, 0, 64), (0, 4096, 64), (5, 12345, 64), (15, 32704, 65), (9, 1000, 7)):
        out = (ctypes.c_uint32 * (cnt * stride))()
        hc.hc_bc2_build_run16(out, j, ctypes.c_uint32(d0), ctypes.c_uint32(cnt))
        want = base[(j * ent + d0) * stride:(j * ent + d0 + cnt) * stride]
        assert list(out) == list(want), (j, d0)


def test_wide_comb_path_vs_libsodium(hc, sodium, oracle):
    """[S]B through pv_comb_b_acc_w (entry conversion at the top position + niels additions, the
    device comb_b code) over the radix-65536 table, then the per-key comb: every golden verdict and
    every adversarial class against libsodium."""
    from vectors import VectorGen
    with open(os.path.join(HERE, "golden", "verdicts.json")) as f:
        for c in json.load(f):
            sm, pk = bytes.fromhex(c["sm"]), bytes.fromhex(c["pk"])
            assert bool(hc.hc_sign_open_comb_wide16(sm, ctypes.c_uint64(len(sm)), pk)) == c["ok"], c["cls"]
    g = VectorGen(sodium, oracle, seed=23)
    for cls in VectorGen.CLASSES:
        for _ in range(3):
            sm, pk = g.make(cls)
            assert bool(hc.hc_sign_open_comb_wide16(sm, ctypes.c_uint64(len(sm)), pk)) == sodium.sign_open_ok(sm, pk), cls


def test_affine_cached_rows_vs_libsodium(hc, sodium, oracle):
    """The key cache's affine rows (comb.h pv_comb_row_to_affine: every entry of a 129-entry row divided
    by its Z with one batched inversion) and the comb loop's affine mode (D = 2 Z1, no Z1 Z2 product,
    words 20..27 unread) -- the device path of a cached key in the comb kernels: every golden verdict
    and every adversarial class against libsodium, under the bound assertions."""
    from vectors import VectorGen
    with open(os.path.join(HERE, "golden", "verdicts.json")) as f:
        for c in json.load(f):
            sm, pk = bytes.fromhex(c["sm"]), bytes.fromhex(c["pk"])
            assert bool(hc.hc_sign_open_comb_affine16(sm, ctypes.c_uint64(len(sm)), pk)) == c["ok"], c["cls"]
    g = VectorGen(sodium, oracle, seed=29)
    for cls in VectorGen.CLASSES:
        for _ in range(3):
            sm, pk = g.make(cls)
            assert bool(hc.hc_sign_open_comb_affine16(sm, ctypes.c_uint64(len(sm)), pk)) == sodium.sign_open_ok(sm, pk), cls


def test_wide_cached_rows_vs_libsodium(hc, sodium, oracle):
    """A cached key's radix-65536 rows (comb.h PV_KW_*: [d 65536^q](-A), d <= 32896, built with the
    wide fixed-base comb's pv_bc2_build_run from the chain's P_{2q}) and the niels loop that runs the
    fixed base's positions and the key's 16 in one pass (digits e_{2q} + 256 e_{2q+1}) -- the device's
    pv_comb_bw_acc: three keys, each with a valid signature, bit flips in R, S and M, S + L and an
    empty message, against libsodium, under the bound assertions."""
    import random
    rnd = random.Random(31)
    for _ in range(3):
        pk, sk = sodium.seed_keypair(bytes(rnd.getrandbits(8) for _ in range(32)))
        for m in (b"", bytes(rnd.getrandbits(8) for _ in range(rnd.randrange(1, 400)))):
            sm = sodium.sign_detached(m, sk) + m
            cases = [sm]
            for pos in (3, 40, 64 + len(m) // 2 if m else 10):
                t = bytearray(sm)
                t[pos % len(t)] ^= 1 << rnd.randrange(8)
                cases.append(bytes(t))
            s_big = (int.from_bytes(sm[32:64], "little") + 2 ** 252 + 27742317777372353535851937790883648493)
            cases.append(sm[:32] + (s_big % 2 ** 256).to_bytes(32, "little") + sm[64:])
            for c in cases:
                assert bool(hc.hc_sign_open_comb_kw16(c, ctypes.c_uint64(len(c)), pk)) == sodium.sign_open_ok(c, pk)


def test_straus_wide_b_vs_libsodium(hc, sodium, oracle):
    """The full-length Straus path with [S]B from the wide comb: the loop over k's radix-16 digits
    with the [j](-A) table only, then one addition of [S]B from pv_comb_b_acc_w -- every golden
    verdict and every adversarial class against libsodium."""
    from vectors import VectorGen
    with open(os.path.join(HERE, "golden", "verdicts.json")) as f:
        for c in json.load(f):
            sm, pk = bytes.fromhex(c["sm"]), bytes.fromhex(c["pk"])
            assert bool(hc.hc_sign_open_straus_wide16(sm, ctypes.c_uint64(len(sm)), pk)) == c["ok"], c["cls"]
    g = VectorGen(sodium, oracle, seed=24)
    for cls in VectorGen.CLASSES:
        for _ in range(3):
            sm, pk = g.make(cls)
            assert bool(hc.hc_sign_open_straus_wide16(sm, ctypes.c_uint64(len(sm)), pk)) == sodium.sign_open_ok(sm, pk), cls


def test_comb_sparse_fill_matches_full_fill(hc, oracle):
    """pv_comb_fill_sparse (small-chunk table fill: [r] P by steps, the [16 q] P from the chain's
    multiples, every other needed entry as T[16 q] + T[r]) builds exactly the points of the full fill
    for every needed entry, at sparse and dense need sets, for prime-order and mixed-order keys."""
    from vectors import ORDER8
    rng = random.Random(12)
    keys = [oracle.scalarmult_base(rng.randrange(1, L).to_bytes(32, "little")) for _ in range(2)]
    keys.append(oracle.point_add(keys[0], ORDER8))
    for j, pk in enumerate(keys):
        for density in (0.05, 0.3, 1.0):
            assert hc.hc_comb_fill_sparse_check(pk, ctypes.c_uint32(j * 7 + 1), ctypes.c_double(density)) == 0, density


def _halfsize(hc, k):
    k1 = ctypes.create_string_buffer(32)
    k2 = ctypes.create_string_buffer(32)
    neg = ctypes.c_int()
    fb = hc.hc_sc_halfsize(k.to_bytes(32, "little"), k1, k2, ctypes.byref(neg))
    a, b = int.from_bytes(k1.raw, "little"), int.from_bytes(k2.raw, "little")
    return (-a if neg.value else a), b, bool(fb)


def test_halfsize_split_invariants(hc):
    """sc_halfsize (the half-size Straus path's split of k): k1 == k k2 (mod 8L), k2 odd and > 0,
    |k1| < 2^128 and k2 < 2^160 unless the (k, 1) fallback was taken; random scalars never fall back,
    and the edge scalars (0, tiny, 2^128 boundary, huge first quotients, L - 1) stay exact."""
    rng = random.Random(41)
    edges = HALFSIZE_EDGES
    fallbacks, bits = 0, []
    for k in edges + [rng.randrange(L) for _ in range(20000)]:
        k1, k2, fb = _halfsize(hc, k)
        assert (k1 - k * k2) % N8L == 0, k
        assert k2 > 0 and k2 & 1, k
        if fb:
            assert (k1, k2) == (k, 1)
            fallbacks += k not in edges
        else:
            assert abs(k1) < 2 ** 128 and k2 < 2 ** 160, k
            bits.append(max(abs(k1).bit_length(), k2.bit_length()))
    assert fallbacks == 0
    assert max(bits) <= 140 and sum(bits) / len(bits) < 129


def test_sc_mul_mod_l(hc):
    rng = random.Random(42)
    r = ctypes.create_string_buffer(32)
    for a, b in SC_MUL_EDGES + \
            [(rng.getrandbits(256), rng.getrandbits(256)) for _ in range(3000)]:
        hc.hc_sc_mul(r, a.to_bytes(32, "little"), b.to_bytes(32, "little"))
        assert int.from_bytes(r.raw, "little") == a * b % L


def test_nwin16(hc):
    rng = random.Random(43)
    for a in NWIN16_EDGES + [rng.randrange(L) for _ in range(500)]:
        d, c = [], 0
        for i in range(64):
            v = ((a >> (4 * i)) & 15) + c
            c = 0 if i == 63 else (v + 8) >> 4
            d.append(v - 16 * c)
        nz = [i for i, v in enumerate(d) if v]
        assert hc.hc_sc_nwin16(a.to_bytes(32, "little")) == (nz[-1] + 1 if nz else 1), a


def test_straus_half_vs_libsodium(hc, sodium, oracle):
    """The half-size Straus path (sc_halfsize split, [j](+-A) and [j](-R') tables, ~33 windows of both
    scalars, + [k2 S]B + R', encoding compared with R) against every golden verdict and every
    adversarial class -- mixed-order A and R included, where a split modulo L alone (or an even k2)
    would change libsodium's cofactorless verdict -- with the normal split, with the (k, 1) fallback,
    and with extra leading zero windows (a wave whose maximum window count exceeds the lane's)."""
    from vectors import VectorGen
    with open(os.path.join(HERE, "golden", "verdicts.json")) as f:
        for c in json.load(f):
            sm, pk = bytes.fromhex(c["sm"]), bytes.fromhex(c["pk"])
            for fb, extra in ((0, 0), (1, 0), (0, 3)):
                got = hc.hc_sign_open_straus_half16(sm, ctypes.c_uint64(len(sm)), pk, fb, extra)
                assert bool(got) == c["ok"], (c["cls"], fb, extra)
    g = VectorGen(sodium, oracle, seed=44)
    for cls in VectorGen.CLASSES:
        for i in range(4):
            sm, pk = g.make(cls)
            want = sodium.sign_open_ok(sm, pk)
            got = hc.hc_sign_open_straus_half16(sm, ctypes.c_uint64(len(sm)), pk, 0, i % 2)
            assert bool(got) == want, cls


def test_lp_halfsize_matches_per_lane_split(hc):
    """lp_halfsize (the latency path's limb-parallel split: the multiword state across the lanes of
    a wave, matrix updates as lane products + DPP carry passes) gives exactly sc_halfsize's split."""
    rng = random.Random(45)
    edges = LP_HALFSIZE_EDGES
    for k in edges + [rng.randrange(L) for _ in range(3000)] + [rng.getrandbits(253) for _ in range(200)]:
        b = k.to_bytes(32, "little")
        outs = []
        for fn in (hc.hc_sc_halfsize, hc.hc_lp_halfsize):
            k1 = ctypes.create_string_buffer(32)
            k2 = ctypes.create_string_buffer(32)
            neg = ctypes.c_int()
            fb = fn(b, k1, k2, ctypes.byref(neg))
            outs.append((k1.raw, k2.raw, neg.value, fb))
        assert outs[0] == outs[1], k


def test_lp_ydbl_chain_matches_doublings(hc):
    """The four-wave latency kernel's [2^68] chains run on y alone (lp_ydbl_chain: y' and the x ratio
    as functions of y) and take x at the end (lp_ydbl_finish): the same point as 68 lp_dbl steps of the
    decompressed -A and R, with the limb bounds asserted, at random points and at x = 0 (y = +-1)."""
    rng = random.Random(46)
    encs = [(1).to_bytes(32, "little"), (P - 1).to_bytes(32, "little")]
    encs += [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(400)]
    tested = 0
    for i, a in enumerate(encs):
        r = encs[(i * 7 + 3) % len(encs)]
        for n in ((68,) if i % 8 else (1, 2, 68)):
            got = hc.hc_lp_ydbl_check(a, r, n)
            if got == -1:
                break
            assert got == 3, (i, n)
            tested += 1
    assert tested >= 50


def test_lp_table_parts_match_full_table(hc):
    """The four-wave kernel builds R''s [j] table in three parts on three waves (entries 0..4 by one
    doubling and additions, 5-6 from [4]P, 7-8 from [8]P and [8]P - P): every entry is the same point
    as lp_build_a_table's."""
    rng = random.Random(47)
    tested = 0
    for _ in range(300):
        got = hc.hc_lp_table_parts_check(bytes(rng.getrandbits(8) for _ in range(32)))
        if got == -1:
            continue
        assert got == 1
        tested += 1
    assert tested >= 50

