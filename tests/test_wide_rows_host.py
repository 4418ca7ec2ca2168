"""The radix-2^11 rows of a resident comb table (indy-plenum_amd/csrc/comb.h PV_KR_*: the code
pv_dir_widen_kernel runs per (position, run of 64 entries), and sc25519.h sc_recode_w_packed) compiled for
the HOST under the bound assertions (tests/native/widecheck.hip): the digits against Python integers, the
bases against plain doublings, the rows against an independent double-and-add, [S]B + [k](-A) through the
one niels loop against libsodium, and once as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes
import json
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "indy-plenum_amd", "csrc")
SRC = os.path.join(HERE, "native", "widecheck.hip")
LIB = os.path.join(HERE, "native", "libwidecheck.so")
HIPCC = ["/opt/rocm/bin/hipcc", "-O1", "-pthread", "--offload-arch=gfx950", "--offload-host-only", "-I" + CSRC]

L = 2 ** 252 + 27742317777372353535851937790883648493
POS, W = 23, 11


def build_widecheck():
    subprocess.check_call(HIPCC + ["-fPIC", "-shared", SRC, "-o", LIB])


def widecheck_lib():
    srcs = [os.path.join(CSRC, f) for f in ("comb.h", "btable.h", "verify_core.h", "fe25519.h", "ge25519.h",
                                            "sc25519.h", "sha512.h")]
    srcs.append(SRC)
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in srcs):
        build_widecheck()
    return ctypes.CDLL(LIB)


@pytest.fixture(scope="module")
def wc():
    return widecheck_lib()


@pytest.fixture(scope="module")
def keys(sodium):
    rnd = random.Random(47)
    return [sodium.seed_keypair(bytes(rnd.getrandbits(8) for _ in range(32)))[0] for _ in range(3)]


def _digits(wc, k):
    out = (ctypes.c_int16 * POS)()
    wc.wc_digits(k.to_bytes(32, "little"), out)
    return list(out)


def test_digits(wc):
    """Exactly 23 digits, |d| <= 1024, top digit >= 0, sum d_q 2^(11 q) = k, for every k < L tried: the
    edges of a digit, of the top digit and of the group; all 23 raw digits 1023 (no carry anywhere); the 22
    raw digits below the top all 1024 (every one becomes -1024 and carries), with a top raw digit of 0 and
    of 1023, which the carry takes to 1024, the last entry of the top row (all 23 raw digits 1024 is above
    L: its bits 252 and 241 are set); and 2,000 seeded random scalars."""
    low_1024 = sum(1024 << (W * q) for q in range(POS - 1))
    rnd = random.Random(53)
    ks = [0, 1, 1023, 1024, 1025, 2 ** 242 - 1, 2 ** 252 - 1, 2 ** 252, L - 1,
          sum(1023 << (W * q) for q in range(POS)), low_1024, low_1024 + (1023 << (W * (POS - 1)))]
    assert _digits(wc, ks[-1])[-1] == 1024 and _digits(wc, 2 ** 252)[-1] == 1024
    ks += [rnd.randrange(L) for _ in range(2000)]
    for k in ks:
        assert 0 <= k < L
        d = _digits(wc, k)
        assert len(d) == POS
        assert all(abs(x) <= 1024 for x in d), (hex(k), d)
        assert d[-1] >= 0, (hex(k), d)
        assert sum(x << (W * q) for q, x in enumerate(d)) == k, (hex(k), d)


def test_bases_from_the_narrow_table(wc, keys):
    """Entry (11 q / 8, 2^(11 q mod 8)) of the radix-256 table, in cached form and converted in place to
    affine rows, is [2^(11 q)](-A) by plain doublings (and a consistent extended point) for all 23 q."""
    for pk in keys:
        assert wc.wc_base_mismatches(pk, 0) == 0
        assert wc.wc_base_mismatches(pk, 1) == 0


def test_rows_against_double_and_add(wc, keys):
    """The product's builder over the in-place-affine table: for every q the entries d in {0, 1, 2, 63, 64,
    65, 1023, 1024} (run boundaries and both ends) plus 200 random (q, d) equal, word for word, the canonical
    affine niels form of [d 2^(11 q)](-A) from an independent double-and-add; over the whole table words 30
    and 31 are zero and every entry was written."""
    rnd = random.Random(59)
    pairs = [(q, d) for q in range(POS) for d in (0, 1, 2, 63, 64, 65, 1023, 1024)]
    pairs += [(rnd.randrange(POS), rnd.randrange(1025)) for _ in range(200)]
    qs = (ctypes.c_int32 * len(pairs))(*[p[0] for p in pairs])
    ds = (ctypes.c_int32 * len(pairs))(*[p[1] for p in pairs])
    for pk in keys:
        assert wc.wc_row_mismatches(pk, qs, ds, len(pairs)) == 0


def test_keys_that_fail_the_checks_are_refused(wc):
    from vectors import BLACKLIST, P
    qs, ds = (ctypes.c_int32 * 1)(0), (ctypes.c_int32 * 1)(1)
    for pk in (bytes(BLACKLIST[0]), (P + 1).to_bytes(32, "little")):
        assert wc.wc_row_mismatches(pk, qs, ds, 1) == -1
        assert wc.wc_base_mismatches(pk, 1) == -1


def test_wide_rows_loop_vs_libsodium(wc, sodium, oracle):
    """[S]B + [k](-A) in one niels loop of 16 + 23 positions over the wide rows: every golden verdict and
    three of every adversarial class against libsodium."""
    from vectors import VectorGen
    with open(os.path.join(HERE, "golden", "verdicts.json")) as f:
        for c in json.load(f):
            sm, pk = bytes.fromhex(c["sm"]), bytes.fromhex(c["pk"])
            assert bool(wc.wc_sign_open_wide(sm, ctypes.c_uint64(len(sm)), pk)) == c["ok"], c["cls"]
    g = VectorGen(sodium, oracle, seed=61)
    for cls in VectorGen.CLASSES:
        for _ in range(3):
            sm, pk = g.make(cls)
            assert bool(wc.wc_sign_open_wide(sm, ctypes.c_uint64(len(sm)), pk)) == sodium.sign_open_ok(sm, pk), cls


def test_standalone_program_clean_under_sanitizers(tmp_path):
    """The same routines as a program of its own (widecheck.hip's main), built with ASan and UBSan: two
    keys' bases and rows, four scalars' digits, no report, exit status 0."""
    exe = str(tmp_path / "widecheck_san")
    # -O0 after HIPCC's -O1: the instrumented build compiles in ~10 s instead of minutes, the run takes ~5 s
    subprocess.check_call(HIPCC + ["-O0", "-DWC_MAIN", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                                   "-Xarch_host", "-fno-sanitize-recover=all", SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert r.stdout.count("0 0 mismatching bases, 0 mismatching entries") == 2, r.stdout
    assert "all checks passed" in r.stdout, r.stdout
