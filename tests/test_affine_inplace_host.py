"""The in-place affine-row conversion of a resident comb table (indy-plenum_amd/csrc/comb.h
pv_comb_row_to_affine_inplace, the code pv_dir_affine_kernel runs per (position, segment)) compiled
for the HOST under the bound assertions (tests/native/affinecheck.hip): word for word against the
out-of-place pv_comb_row_to_affine on real tables, through the comb loop's affine mode against
libsodium, and once as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes
import json
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "indy-plenum_amd", "csrc")
SRC = os.path.join(HERE, "native", "affinecheck.hip")
LIB = os.path.join(HERE, "native", "libaffinecheck.so")
HIPCC = ["/opt/rocm/bin/hipcc", "-O1", "-pthread", "--offload-arch=gfx950", "--offload-host-only", "-I" + CSRC]


def build_affinecheck():
    subprocess.check_call(HIPCC + ["-fPIC", "-shared", SRC, "-o", LIB])


def affinecheck_lib():
    srcs = [os.path.join(CSRC, f) for f in ("comb.h", "btable.h", "verify_core.h", "fe25519.h", "ge25519.h",
                                            "sc25519.h", "sha512.h")]
    srcs.append(SRC)
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in srcs):
        build_affinecheck()
    return ctypes.CDLL(LIB)


@pytest.fixture(scope="module")
def ac():
    return affinecheck_lib()


def test_inplace_equals_out_of_place(ac, sodium):
    """All 32 rows of real keys' tables (row 0's entry 0 is the identity, as is every row's), cut into
    the kernel's four segments: every word equals pv_comb_row_to_affine's output, words 20..29 are 0."""
    rnd = random.Random(41)
    for _ in range(3):
        pk, _sk = sodium.seed_keypair(bytes(rnd.getrandbits(8) for _ in range(32)))
        assert ac.ac_inplace_mismatches(pk) == 0


def test_keys_that_fail_the_checks_are_not_converted(ac):
    from vectors import BLACKLIST, P
    for pk in (bytes(BLACKLIST[0]), (P + 1).to_bytes(32, "little")):
        assert ac.ac_inplace_mismatches(pk) == -1


def test_affine_inplace_rows_vs_libsodium(ac, sodium, oracle):
    """[S]B + [k](-A) through pv_comb_a_xyz_staged in affine mode over the table converted in place:
    every golden verdict and every adversarial class against libsodium."""
    from vectors import VectorGen
    with open(os.path.join(HERE, "golden", "verdicts.json")) as f:
        for c in json.load(f):
            sm, pk = bytes.fromhex(c["sm"]), bytes.fromhex(c["pk"])
            assert bool(ac.ac_sign_open_affine_inplace(sm, ctypes.c_uint64(len(sm)), pk)) == c["ok"], c["cls"]
    g = VectorGen(sodium, oracle, seed=43)
    for cls in VectorGen.CLASSES:
        for _ in range(3):
            sm, pk = g.make(cls)
            assert bool(ac.ac_sign_open_affine_inplace(sm, ctypes.c_uint64(len(sm)), pk)) == \
                sodium.sign_open_ok(sm, pk), cls


def test_standalone_program_clean_under_sanitizers(tmp_path):
    """The same routine as a program of its own (affinecheck.hip's main), built with ASan and UBSan:
    three tables converted both ways, no report, exit status 0."""
    exe = str(tmp_path / "affinecheck_san")
    # -O0 after HIPCC's -O1: the instrumented build compiles in ~10 s instead of minutes, the run takes ~2 s
    subprocess.check_call(HIPCC + ["-O0", "-DAC_MAIN", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                                   "-Xarch_host", "-fno-sanitize-recover=all", SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert r.stdout.count("0 mismatching words") == 3, r.stdout
