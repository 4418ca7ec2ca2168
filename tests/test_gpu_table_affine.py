"""GPU: affine rows for resident comb tables (pv_table_affine). A chunk of more than 65,536 requests that
reads a listed table which such a chunk has read once before (the table's second hit: converting costs
as much as ten warm chunks save, measured, so a table that comes back once is left alone) converts it,
behind its own kernels, to affine rows in place (pv_dir_affine_kernel); every later chunk reads it with
the comb loop's affine mode. Verdicts stay libsodium's throughout; the
counters say which form each chunk read. Shapes, signers, bad keys and tampering are those of
tests/test_gpu_table_reuse.py: 64 keys x 1,100 requests = 70,400 (the smallest listing chunk has
65,537), 1,100 is no multiple of 64 so waves straddle keys, and the three keys that fail libsodium's
key checks must never be converted."""
import numpy as np
import pytest

from test_gpu_table_reuse import K1, K2, NKEYS, _batch, _run, signers  # noqa: F401  (signers: fixture)

pytestmark = pytest.mark.gpu

GOOD = NKEYS - 3  # signers of a batch: the keys whose tables may be converted


@pytest.fixture(scope="module")
def nat():
    from plenum_amd import _native
    _native.ensure_device()
    _native.set_path(_native.PV_PATH_AUTO)
    yield _native
    _native.set_path(_native.PV_PATH_AUTO)
    _native.table_affine(True)
    _native.table_reuse(True, _native.PV_TABLE_REUSE_CAP)


@pytest.fixture()
def fresh(nat):
    """Reuse and affine rows on, default capacity, nothing kept from earlier tests."""
    nat.table_affine(True)
    nat.table_reuse(False)
    nat.table_reuse(True, nat.PV_TABLE_REUSE_CAP)
    return nat


class _Stats:
    """Deltas of (converted, affine_reads) and (hits, built, resets) since the last call."""

    def __init__(self, nat):
        self.nat = nat
        self.a, self.r = nat.table_affine_stats(), nat.table_reuse_stats()

    def step(self):
        a, r = self.nat.table_affine_stats(), self.nat.table_reuse_stats()
        out = (tuple(int(x - y) for x, y in zip(a, self.a)), tuple(int(x - y) for x, y in zip(r, self.r)))
        self.a, self.r = a, r
        return out


def _promote(nat, b):
    _run(nat, b, "build")
    _run(nat, b, "first hit")
    _run(nat, b, "second hit: promote")


def test_build_promote_read(fresh, signers):
    nat = fresh
    b = _batch(signers, K1)
    s = _Stats(nat)
    _run(nat, b, "build")
    assert s.step() == ((0, 0), (0, NKEYS, 0))
    _run(nat, b, "first hit")
    assert s.step() == ((0, 0), (NKEYS, 0, 0))
    _run(nat, b, "promote")  # reads cached form, converts the 61 checked keys behind the chunk
    assert s.step() == ((GOOD, 0), (NKEYS, 0, 0))
    _run(nat, b, "read affine")
    assert s.step() == ((0, GOOD), (NKEYS, 0, 0))


def test_mixed_forms_in_one_chunk(fresh, signers):
    nat = fresh
    _promote(nat, _batch(signers, K1))
    # 32 of K1's keys (29 signers, affine by now, and its 3 bad keys) and 32 new signers
    half = _batch(signers, K1[:29] + list(range(200, 232)), seed=1)
    s = _Stats(nat)
    _run(nat, half, "affine and new")
    assert s.step() == ((0, 29), (32, 32, 0))
    _run(nat, half, "first hit of the new half")
    assert s.step() == ((0, 29), (64, 0, 0))
    _run(nat, half, "promotes the new half only")
    assert s.step() == ((32, 29), (64, 0, 0))
    _run(nat, half, "all affine")
    assert s.step() == ((0, 61), (64, 0, 0))


@pytest.mark.parametrize("how", ["full", "off_on", "kc_put"])
def test_rebuilt_slot_reads_projective(fresh, signers, how):
    """The affine bit must not outlive the table it describes: after a reset by a chunk that does not
    fit, after the directory was emptied by a control call, and after a key-cache put that built its
    tables over the directory, the same slots hold new cached-form tables."""
    nat = fresh
    a, b = _batch(signers, K1), _batch(signers, K2, bad=1, seed=6)
    kc = nat.KeyCache
    try:
        if how == "full":
            nat.table_reuse(True, 96)
        elif how == "kc_put":
            nat.table_reuse(True, 16384 - 4)  # a put of more than 4 keys builds over the directory
            kc.configure(128)
        _promote(nat, a)
        s = _Stats(nat)
        if how == "off_on":
            nat.table_reuse(False)
            nat.table_reuse(True)
        elif how == "kc_put":
            kc.put([signers.records(i, 1)[0] for i in range(500, 508)])
        _run(nat, b, "K2 into K1's slots")
        assert s.step() == ((0, 0), (0, NKEYS, 1 if how == "full" else 0))
        _run(nat, b, "K2 hit once")
        assert s.step() == ((0, 0), (NKEYS, 0, 0))
        _run(nat, b, "K2 promoted")
        assert s.step() == ((GOOD, 0), (NKEYS, 0, 0))
        _run(nat, b, "K2 affine")
        assert s.step() == ((0, GOOD), (NKEYS, 0, 0))
    finally:
        kc.configure(0)
        nat.table_reuse(True, nat.PV_TABLE_REUSE_CAP)


def test_small_chunk_reads_never_converts(fresh, signers):
    nat = fresh
    dense = _batch(signers, K1)
    small = _batch(signers, K1, per_key=100, seed=8)  # 6,400 requests: pv_comb_b_kernel + pv_comb_a_kernel
    assert len(small[3]) == 6400
    _run(nat, dense, "build")
    s = _Stats(nat)
    _run(nat, small, "small on unpromoted tables")
    assert s.step() == ((0, 0), (NKEYS, 0, 0))
    _run(nat, small, "small again: its hits do not count towards promotion")
    assert s.step() == ((0, 0), (NKEYS, 0, 0))
    _run(nat, dense, "first dense hit")
    assert s.step() == ((0, 0), (NKEYS, 0, 0))
    _run(nat, dense, "promote")
    assert s.step() == ((GOOD, 0), (NKEYS, 0, 0))
    _run(nat, small, "small on affine tables")
    assert s.step() == ((0, GOOD), (NKEYS, 0, 0))


def test_off_switch(fresh, signers):
    nat = fresh
    b = _batch(signers, K1)
    try:
        nat.table_affine(False)
        s = _Stats(nat)
        for rep in range(4):
            _run(nat, b, ("off", rep))
        assert s.step() == ((0, 0), (3 * NKEYS, NKEYS, 0))
        nat.table_affine(True)  # starts from an empty directory
        _run(nat, b, "on: build")
        assert s.step() == ((0, 0), (0, NKEYS, 0))
        _run(nat, b, "on: first hit")
        _run(nat, b, "on: promote")
        assert s.step() == ((GOOD, 0), (2 * NKEYS, 0, 0))
    finally:
        nat.table_affine(True)


def test_device_calls_back_to_back(fresh, signers):
    """Ordering between chunks: device-buffer calls on the same keys enqueued with nothing between
    them (the chunk limit of one call cannot be lowered from outside). Call 1 builds, call 2 is the
    first hit, call 3 reads cached form and converts behind itself, call 4 reads affine rows."""
    from test_gpu_robustness import _Dev
    nat = fresh
    blob, off, pks, want = _batch(signers, K1)
    d = _Dev(nat, blob, off, pks)
    try:
        vers = [d.ver, d.alloc(d.words * 8), d.alloc(d.words * 8), d.alloc(d.words * 8)]
        s = _Stats(nat)
        for v in vers:
            nat.check(nat.lib().pv_verify_batch_device(d.blob, d.off, d.n, d.pk, v, None), "pv_verify_batch_device")
        for k, v in enumerate(vers):
            d.ver = v
            got = d.verdicts()
            assert np.array_equal(got, want), (k, np.nonzero(got != want)[0][:10])
        assert s.step() == ((GOOD, GOOD), (3 * NKEYS, NKEYS, 0))
    finally:
        d.free()
