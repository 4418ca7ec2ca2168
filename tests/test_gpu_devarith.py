"""The DEVICE branches of the arithmetic headers on the GPU, unit by unit, at edge inputs.

The host check libraries compile the headers with --offload-host-only, so they take the `#else` side of
every `__HIP_DEVICE_COMPILE__` switch: the C loop instead of fe_mul_pre / fe_sq's inline-asm product
columns, a 64-lane simulation instead of lp25519.h's DPP / permlane / readlane / ballot forms, the
exact 1.0f / x and a one-lane pv_wave_all in the splits, plain C instead of sha512.h's alignbit /
bitop3 / perm. tests/native/devcheck.hip wraps the same units in small gfx950 kernels; this module
pushes the vectors of tests/devarith_cases.py through them and asserts

  (a) every wrapper returns 0,
  (b) the pure-Python checkers pass (values mod p, % L, digit sums, hashlib, the limb bounds the device
      build cannot assert itself),
  (c) for every unit but the two splits, the device output equals the host library's output word for
      word (both sides compute the same integer column sums; a difference means the asm columns, or
      the host simulation's model of a lane instruction, do not match the hardware).

The splits (sc_halfsize, lp_halfsize) use floating point, so their contract is check_split's
invariants; the device's two splits must agree with each other, and with the host's.

Not covered: each product kernel's own register allocation and scheduling around these units; the
end-to-end parity tests (tests/test_gpu_parity.py) remain the check of those."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import devarith_cases as dv

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "indy-plenum_amd", "csrc")
SRC = os.path.join(HERE, "native", "devcheck.hip")
LIB = os.path.join(HERE, "native", "libdevcheck.so")


def build_devcheck():
    # the product Makefile's flags: the device branches as the product kernels compile them
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-fPIC", "-shared", "-I" + CSRC,
                           SRC, "-o", LIB])


def devcheck_lib():
    """libdevcheck.so, rebuilt when older than its sources. Loading needs no GPU; calling into it does."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [SRC]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in srcs):
        build_devcheck()
    return ctypes.CDLL(LIB)


@pytest.fixture(scope="module")
def dev():
    return dv.DevBackend(devcheck_lib())


@pytest.fixture(scope="module")
def host():
    from test_native_host import LIB as HOSTLIB, build_hostcheck
    if not os.path.exists(HOSTLIB):
        build_hostcheck()
    return dv.HostBackend(ctypes.CDLL(HOSTLIB))


@pytest.mark.parametrize("name", [n for n, u in dv.UNITS.items() if u.exact])
def test_unit_on_device(dev, host, name):
    u = dv.UNITS[name]
    ins = u.inputs()
    got = u.run(dev, ins)           # (a): a HIP error raises
    u.check(ins, got)               # (b)
    want = u.run(host, ins)
    for j, (a, b) in enumerate(zip(got, want)):  # (c)
        dv.check_equal(a, b, "%s output %d, device vs host" % (name, j))


@pytest.fixture(scope="module")
def device_splits(dev):
    ins = dv.UNITS["sc_halfsize"].inputs()
    return ins, dev.sc_halfsize(ins[0]), dev.lp_halfsize(ins[0])


def test_split_invariants_on_device(device_splits):
    ins, per_lane, per_wave = device_splits
    ks = dv.ints(ins[0])
    dv.check_split(ks, ins[1], *per_lane)
    dv.check_split(ks, ins[1], *per_wave)


def test_lp_halfsize_equals_sc_halfsize_on_device(device_splits):
    """Both use the same quotient estimate (v_rcp_f32), so the splits are equal on every scalar."""
    _, per_lane, per_wave = device_splits
    for a, b in zip(per_lane, per_wave):
        dv.check_equal(a, b, "lp_halfsize vs sc_halfsize on the device")


def test_device_split_equals_host_split(device_splits, host):
    """v_rcp_f32 (1 ulp) against the host's exact 1.0f / x, and the device's software double division:
    the estimate is corrected exactly, so the split is the same on every scalar."""
    ins, per_lane, _ = device_splits
    for a, b in zip(per_lane, host.sc_halfsize(ins[0])):
        dv.check_equal(a, b, "sc_halfsize, device vs host")


def test_split_in_divergent_waves(dev):
    """sc_halfsize's loops break wave-uniformly (pv_wave_all) and `continue` per lane: a lane's result
    must not depend on its neighbours. Every pool scalar in a wave of 64 copies gives the reference; the
    mixed layout (k = 0, k = 1, a fallback scalar and L - 1 side by side in every wave, edge and random
    scalars interleaved, a partial last wave) must give each lane the same words."""
    pool, uniform, mixed = dv.split_lane_layouts()
    u1, u2, uf = dev.sc_halfsize(dv.words(uniform, 8))
    ref = {}
    for j, k in enumerate(pool):
        rows = slice(64 * j, 64 * j + 64)
        for arr in (u1, u2, uf):
            assert (arr[rows] == arr[64 * j]).all(), "lanes of a uniform wave differ for k = %d" % k
        ref[k] = (u1[64 * j].tobytes(), u2[64 * j].tobytes(), uf[64 * j].tobytes())
    dv.check_split(pool, len(dv.split_edges()), u1[::64], u2[::64], uf[::64])
    m1, m2, mf = dev.sc_halfsize(dv.words(mixed, 8))
    assert any(int(f) for f in mf[:64, 1]) and not all(int(f) for f in mf[:64, 1])
    for i, k in enumerate(mixed):
        assert (m1[i].tobytes(), m2[i].tobytes(), mf[i].tobytes()) == ref[k], (i, k)


def test_launch_shapes(dev):
    """No per-lane launch above 4160 lanes, no per-wave launch above 700 waves (the backend splits)."""
    assert dv.LANE_CHUNK == 4160 and dv.WAVE_CHUNK == 700
    n = dv.LANE_CHUNK + 37
    f = np.zeros((n, 10), np.uint32)
    f[:, 0] = np.arange(n)
    before = dev.launches
    h = dev.fe_carry(f)
    assert dev.launches - before == 2 and (h == f).all()
