"""Every vector of tests/devarith_cases.py through libhostcheck.so, the bounds-checked HOST build of
the arithmetic headers, with the module's pure-Python checkers. A pass shows that every vector
respects its unit's preconditions (PV_BOUNDS_CHECK aborts otherwise) and that the checkers accept
correct results; tests/test_gpu_devarith.py then runs the same vectors and checkers on the headers'
DEVICE branches. The self-test shows that the checkers and the limb comparison reject a result that is
wrong in one limb."""
import ctypes

import numpy as np
import pytest

import devarith_cases as dv
from test_native_host import hc  # noqa: F401


@pytest.fixture(scope="module")
def host(hc):  # noqa: F811
    return dv.HostBackend(hc)


@pytest.mark.parametrize("name", list(dv.UNITS))
def test_unit_on_host_backend(host, name):
    u = dv.UNITS[name]
    ins = u.inputs()
    u.check(ins, u.run(host, ins))


def test_coverage_counts(host):
    """The counts a test may not fall below, with the chosen seeds: random encodings that decompress
    (>= 150 of 400), y-only doubling chains and table-part inputs actually tested (>= 50 each)."""
    u = dv.UNITS["ge_frombytes_negate"]
    ins = u.inputs()
    ok, _ = u.run(host, ins)
    assert len(ins[1]) - ins[2] == 400 and int(ok[ins[2]:].sum()) >= 150
    a, r, nd = dv.ydbl_inputs()
    assert sum(dv.decode_xy(x) is not None and dv.decode_xy(y) is not None for x, y in zip(a, r)) >= 50
    assert sum(dv.decode_xy(e) is not None for e in dv.table_parts_inputs()) >= 50


def test_host_splits_agree(host):
    """lp_halfsize gives exactly sc_halfsize's split on the host (both use the exact 1.0f / x there)."""
    u = dv.UNITS["sc_halfsize"]
    ins = u.inputs()
    for a, b in zip(host.sc_halfsize(ins[0]), host.lp_halfsize(ins[0])):
        dv.check_equal(a, b, "lp_halfsize vs sc_halfsize")


def test_split_lane_layouts_cover_the_exits(host):
    """The mixed lane layout puts a fallback scalar, first-iteration exits and full-length runs into
    every wave."""
    pool, uniform, mixed = dv.split_lane_layouts()
    assert len(uniform) == 64 * len(pool) and len(mixed) == 4096 + 37
    _, _, flags = host.sc_halfsize(dv.words(mixed[:4], 8))
    assert [int(f) for f in flags[:, 1]] == [0, 0, 1, 0]  # L - 1 falls back
    stats = (ctypes.c_uint32 * 3)()
    counts = []
    for k in mixed[:4]:
        host.lib.hc_lp_halfsize_stats(k.to_bytes(32, "little"), stats)
        counts.append(list(stats))
    assert counts[0] == counts[1] == [0, 0, 0]      # k = 0, 1: neither loop runs
    assert counts[2][0] == 1 and counts[3][0] >= 3  # Lehmer blocks: one, then several


def _perturbations(h):
    """One change in one limb, in turn: +1, -1, the top-limb wrap (+2^25 in limb 9 and -19 in limb 0,
    which keeps the value mod p), a swap of two limbs."""
    out = []
    for name in ("plus1", "minus1", "wrap", "swap"):
        g = np.array(h, dtype=np.uint32, copy=True)
        if name == "plus1":
            g[0, 3] += 1
        elif name == "minus1":
            g[0, 6] -= 1
        elif name == "wrap":
            g[0, 9] += 1 << 25
            g[0, 0] -= 19
        else:
            g[0, 2], g[0, 7] = h[0, 7], h[0, 2]
        out.append((name, g))
    return out


def test_checkers_reject_one_limb_errors(host):
    """A correct fe_mul result (host backend) with one limb changed: the value checker, the bound
    checker or the limb-for-limb comparison rejects each perturbation. The wrap keeps the value (the
    value checker alone would accept it): the "R" bound and the limb comparison catch it."""
    rng = np.random.default_rng(5)
    f = dv.limb_rows([dv.to_limbs(int.from_bytes(rng.bytes(32), "little") % dv.P) for _ in range(3)])
    g = dv.limb_rows([dv.to_limbs(int.from_bytes(rng.bytes(32), "little") % dv.P) for _ in range(3)])
    h = host.fe_mul(f, g)
    want = [dv.from_limbs(a) * dv.from_limbs(b) for a, b in zip(f, g)]
    dv.check_field(h, want)
    assert h[0, 0] >= 19 and h[0, 6] >= 1 and h[0, 2] != h[0, 7]
    for name, bad in _perturbations(h):
        rejected = {}
        for what, fn in (("value", lambda: dv.check_values(bad, want)), ("bound", lambda: dv.check_limb_bound(bad)),
                         ("limbs", lambda: dv.check_equal(bad, h, "perturbed"))):
            try:
                fn()
                rejected[what] = False
            except AssertionError:
                rejected[what] = True
        assert rejected["limbs"], name
        assert rejected["value"] or rejected["bound"], (name, rejected)
        if name == "wrap":
            assert not rejected["value"] and rejected["bound"]
