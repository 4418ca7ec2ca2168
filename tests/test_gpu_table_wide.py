"""GPU: radix-2^11 rows for resident comb tables (pv_table_wide). A chunk of more than 65,536 requests that
reads a listed table in affine form (the table's third hit by such a chunk) builds, behind its own kernels,
23 rows of 1,025 affine niels entries for that key in the wide pool (pv_dir_widen_kernel); every later keyed
chunk that hits the table computes [k](-A) from them in the niels loop of [S]B, 23 additions instead of
32. Verdicts stay libsodium's throughout; the counters say which form each chunk read. Signers, bad keys,
tampering and the 70,400-request shape are those of tests/test_gpu_table_reuse.py.

Shapes: 64 keys x 1,100 = 70,400 requests through the host-buffer call (the smallest listing chunk has
65,537; the split kernels pv_comb_b_kernel + pv_comb_a_kernel; 1,100 is no multiple of 64, so waves
straddle keys); 64 keys x 4,100 = 262,400 through the device-buffer call (the smallest fused chunk has
262,145: pv_comb_ab_kernel); 64 keys x 100 = 6,400, a small chunk that reads wide tables and never widens."""
import numpy as np
import pytest

from test_gpu_table_reuse import K1, K2, NKEYS, _batch, _run, signers  # noqa: F401  (signers: fixture)

pytestmark = pytest.mark.gpu

GOOD = NKEYS - 3  # signers of a batch: the keys whose tables may be widened
FUSED_PER_KEY = 4100


@pytest.fixture(scope="module")
def nat():
    from plenum_amd import _native
    _native.ensure_device()
    _native.set_path(_native.PV_PATH_AUTO)
    yield _native
    _native.set_path(_native.PV_PATH_AUTO)
    _native.table_affine(True)
    _native.table_wide(_native.PV_TABLE_WIDE_CAP)
    _native.table_reuse(True, _native.PV_TABLE_REUSE_CAP)


@pytest.fixture()
def fresh(nat):
    """Reuse, affine rows and wide rows on at their defaults, nothing kept from earlier tests."""
    nat.table_affine(True)
    nat.table_wide(nat.PV_TABLE_WIDE_CAP)
    nat.table_reuse(False)
    nat.table_reuse(True, nat.PV_TABLE_REUSE_CAP)
    return nat


class _Stats:
    """Deltas of (widened, wide_reads), (converted, affine_reads) and (hits, built, resets) since the last call."""

    def __init__(self, nat):
        self.nat = nat
        self.v = self._read()

    def _read(self):
        return self.nat.table_wide_stats(), self.nat.table_affine_stats(), self.nat.table_reuse_stats()

    def step(self):
        v = self._read()
        out = tuple(tuple(int(x - y) for x, y in zip(a, b)) for a, b in zip(v, self.v))
        self.v = v
        return out


def _to_wide(nat, b, s=None, resets=0):
    """build -> first hit -> affine -> widen (the chunk itself reads affine rows) -> read wide, the counters
    checked at every step when s is given."""
    steps = [("build", ((0, 0), (0, 0), (0, NKEYS, resets))),
             ("first hit", ((0, 0), (0, 0), (NKEYS, 0, 0))),
             ("second hit: affine rows behind it", ((0, 0), (GOOD, 0), (NKEYS, 0, 0))),
             ("third hit: reads affine rows, widened behind it", ((GOOD, 0), (0, GOOD), (NKEYS, 0, 0))),
             ("reads wide rows", ((0, GOOD), (0, GOOD), (NKEYS, 0, 0)))]
    for what, want in steps:
        _run(nat, b, what)
        if s is not None:
            assert s.step() == want, what


def test_sequence(fresh, signers):
    """The three bad keys, each with a table of its own, are never widened (61 of 64 are); a small chunk
    reads wide rows; the fused kernel reads them too."""
    nat = fresh
    b = _batch(signers, K1)
    small = _batch(signers, K1, per_key=100, seed=8)
    assert len(b[3]) == 70400 and len(small[3]) == 6400
    s = _Stats(nat)
    _to_wide(nat, b, s)
    _run(nat, small, "small chunk on wide tables")
    assert s.step() == ((0, GOOD), (0, GOOD), (NKEYS, 0, 0))
    _run(nat, b, "wide again: nothing left to widen")
    assert s.step() == ((0, GOOD), (0, GOOD), (NKEYS, 0, 0))


def test_small_chunk_never_widens(fresh, signers):
    nat = fresh
    dense = _batch(signers, K1)
    small = _batch(signers, K1, per_key=100, seed=8)
    for what in ("build", "first hit", "affine"):
        _run(nat, dense, what)
    s = _Stats(nat)
    for rep in range(2):
        _run(nat, small, ("small on affine tables", rep))
        assert s.step() == ((0, 0), (0, GOOD), (NKEYS, 0, 0))
    _run(nat, dense, "the dense chunk widens")
    assert s.step() == ((GOOD, 0), (0, GOOD), (NKEYS, 0, 0))
    _run(nat, small, "small on wide tables")
    assert s.step() == ((0, GOOD), (0, GOOD), (NKEYS, 0, 0))


def test_mixed_forms_in_one_chunk(fresh, signers):
    """One chunk with keys in all four states. W has been in four dense chunks (wide), A in three (affine), C
    in two (cached form, hit once), N in none; the chunk's three bad keys are new as well."""
    nat = fresh
    W, A, C, N = K1[:15], K1[15:30], K1[30:45], K1[45:61]
    F = list(range(400, 446))  # fillers that keep every earlier chunk at 61 keys x 1,100 = 67,100 requests
    _run(nat, _batch(signers, W + F, bad=None, seed=11), "W built")
    _run(nat, _batch(signers, W + A + F[:31], bad=None, seed=12), "W hit, A built")
    b3 = _batch(signers, W + A + C + F[:16], bad=None, seed=13)
    _run(nat, b3, "W affine, A hit, C built")
    _run(nat, b3, "W widened, A affine, C hit")
    m = _batch(signers, W + A + C + N, bad=2, seed=14)
    assert len(m[3]) == 70400
    s = _Stats(nat)
    _run(nat, m, "wide, affine, cached form and new in one chunk")
    assert s.step() == ((15, 15), (15, 30), (45, 19, 0))
    _run(nat, m, "W and A wide, C affine and widened behind it, N hit once")
    assert s.step() == ((15, 30), (0, 45), (NKEYS, 0, 0))
    _run(nat, m, "W, A and C wide, N converted behind it")
    assert s.step() == ((0, 45), (16, 45), (NKEYS, 0, 0))


@pytest.mark.parametrize("how", ["full", "off_on", "kc_put"])
def test_wide_flag_does_not_outlive_its_table(fresh, signers, how):
    """After a reset by a chunk that does not fit, after the directory was emptied by a control call, and
    after a key-cache put that built its tables over the directory, the same slots hold new tables in
    cached form, and they are widened again later. The pool holds 64 tables here: K2's 61 find room only
    because the pool was emptied with the directory."""
    nat = fresh
    a, b = _batch(signers, K1), _batch(signers, K2, bad=1, seed=6)
    kc = nat.KeyCache
    try:
        nat.table_wide(64)
        if how == "full":
            nat.table_reuse(True, 96)
        elif how == "kc_put":
            nat.table_reuse(True, 16384 - 4)  # a put of more than 4 keys builds over the directory
            kc.configure(128)
        _to_wide(nat, a)
        s = _Stats(nat)
        if how == "off_on":
            nat.table_reuse(False)
            nat.table_reuse(True)
        elif how == "kc_put":
            kc.put([signers.records(i, 1)[0] for i in range(500, 508)])
        _to_wide(nat, b, s, resets=1 if how == "full" else 0)
    finally:
        kc.configure(0)
        nat.table_wide(nat.PV_TABLE_WIDE_CAP)
        nat.table_reuse(True, nat.PV_TABLE_REUSE_CAP)


def test_pool_full(fresh, signers):
    nat = fresh
    b = _batch(signers, K1)
    try:
        nat.table_wide(32)
        for what in ("build", "first hit", "affine"):
            _run(nat, b, what)
        s = _Stats(nat)
        _run(nat, b, "32 of the 61 find room")
        assert s.step() == ((32, 0), (0, GOOD), (NKEYS, 0, 0))
        for rep in range(2):
            _run(nat, b, ("32 wide, 29 affine, nothing more widens", rep))
            assert s.step() == ((0, 32), (0, GOOD), (NKEYS, 0, 0))
    finally:
        nat.table_wide(nat.PV_TABLE_WIDE_CAP)


def test_off_switch(fresh, signers):
    nat = fresh
    b = _batch(signers, K1)
    try:
        nat.table_wide(0)
        s = _Stats(nat)
        for rep in range(6):
            _run(nat, b, ("off", rep))
        assert s.step() == ((0, 0), (GOOD, 3 * GOOD), (5 * NKEYS, NKEYS, 0))
    finally:
        nat.table_wide(nat.PV_TABLE_WIDE_CAP)


def test_device_calls_back_to_back(fresh, signers):
    """Ordering between the widening kernel and the next chunk's reads: five device-buffer calls of the fused
    shape on the same keys enqueued with nothing between them. Call 1 builds, 2 is the first hit, 3 converts
    behind itself, 4 reads affine rows and widens behind itself, 5 reads wide rows."""
    from test_gpu_robustness import _Dev
    nat = fresh
    blob, off, pks, want = _batch(signers, K1, per_key=FUSED_PER_KEY, seed=9)
    assert len(want) == 262400
    d = _Dev(nat, blob, off, pks)
    try:
        vers = [d.ver] + [d.alloc(d.words * 8) for _ in range(4)]
        s = _Stats(nat)
        for v in vers:
            nat.check(nat.lib().pv_verify_batch_device(d.blob, d.off, d.n, d.pk, v, None), "pv_verify_batch_device")
        for k, v in enumerate(vers):
            d.ver = v
            got = d.verdicts()
            assert np.array_equal(got, want), (k, np.nonzero(got != want)[0][:10])
        assert s.step() == ((GOOD, GOOD), (GOOD, 2 * GOOD), (4 * NKEYS, NKEYS, 0))
        nat.check(nat.lib().pv_verify_batch_device(d.blob, d.off, d.n, d.pk, vers[0], None), "pv_verify_batch_device")
        d.ver = vers[0]
        assert np.array_equal(d.verdicts(), want)
        assert s.step() == ((0, GOOD), (0, GOOD), (NKEYS, 0, 0))
    finally:
        d.free()
