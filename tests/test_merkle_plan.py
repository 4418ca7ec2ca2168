"""The ledger Merkle plan (indy-plenum_amd/csrc/merkle_plan.h: the chunks of an append-like call and where a
chunk's outputs lie, the reply window of a catch-up chunk, the chunks of the proof checks and of proof generation,
the argument checks of the eleven entries), compiled with g++ exactly as the library includes it, under
AddressSanitizer and UBSan, and run as a stand-alone program (tests/native/merkle_plan_check.cpp). A sweep against
a Python model that transcribes the expressions as they stood inside mk_enqueue, mk_host_entry_device,
mk_verify_enqueue and mk_consistency_enqueue before the plan had a file of its own (pv_merkle.hip:469-480, 528-557,
575-577 and 590-592 of the parent commit), the properties themselves, the byte bound at 100 bytes (the library's
is 2^30, which no test stages), and every check function on each side of its condition. What the plan leads to
on the device is checked by tests/test_gpu_merkle.py, test_gpu_consistency.py, test_gpu_prove.py and
test_gpu_host_staging.py. CPU only."""
import bisect
import functools
import json
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "merkle_plan_check.cpp")
STUB = os.path.join(HERE, "native", "stub_hip")
CSRC = os.path.join(HERE, "..", "indy-plenum_amd", "csrc")
BIN = os.path.join(HERE, "native", "merkle_plan_check")

CHUNK_BYTES = 1 << 30
SWEEP_S0 = (0, 1, 1023, 1024, 1025, 2 ** 20 + 12345, 2 ** 48 - 2000)
SWEEP_N = (1, 63, 64, 65, 1000, 1024, 1025, 5000)
SWEEP_BOUND = (1, 50, 64, 1000, 1024, 2 ** 20)
SPAN_BOUND = (1, 50, 63, 64, 65, 1000)
SPAN_N = (1, 63, 64, 65, 1000, 1025)


def popcount(x):
    return bin(x).count("1")


def node_count(s):
    """pv_merkle_node_count: CompactMerkleTree.get_expected_node_count."""
    return s - popcount(s)


@functools.lru_cache(maxsize=None)
def popc_sum(x):
    """pv_merkle_popc_sum: the sum of popcount(j) over 0 <= j < x, bit by bit."""
    total = 0
    for b in range(49):
        half = 1 << b
        rem = x & (2 * half - 1)
        total += (x >> (b + 1)) * half + max(0, rem - half)
    return total


def model_chunks(s0, n, chunk, off=None, byte_bound=CHUNK_BYTES, strict=True, pbase_from=0):
    """The chunk walk of mk_enqueue (off None) and of mk_host_entry_device as the parent commit wrote them out.
    strict=False and pbase_from=1: deliberately wrong variants."""
    nodes0, paths0 = node_count(s0), popc_sum(s0)
    rows, c0 = [], 0
    while c0 < n:
        m = min(chunk, n - c0)
        if off is not None and off[c0 + m] - off[c0] > byte_bound:  # the longest prefix within it, at least one leaf
            cut = bisect.bisect_right if strict else bisect.bisect_left  # std::upper_bound
            e = cut(off, off[c0] + byte_bound, c0 + 1, c0 + m + 1)
            m = max(1, (e - c0) - 1)
        s = s0 + c0
        pbase = popc_sum(s + pbase_from) - paths0
        is_last = c0 + m == n
        n_nodes, n_path = node_count(s + m) - node_count(s), popc_sum(s + m) - popc_sum(s)  # pv_merkle_plan_core
        rows.append([c0, m, s, pbase, node_count(s) - nodes0, n_nodes, n_path, int(is_last)])
        c0 += m
    return rows


def sweep_lens(n):
    return [(i * 37 + 11) % 90 for i in range(n)]


def sweep_jobs():
    for s0 in SWEEP_S0:
        for n in SWEEP_N:
            for bound in SWEEP_BOUND:
                for with_off in (0, 1):
                    yield [1, s0, n, bound, with_off, CHUNK_BYTES] + sweep_lens(n)


def byte_cases():
    """(leaf bound, record lengths) at a byte bound of 100."""
    rng = np.random.default_rng(2025)
    cases = [(64, [int(x) for x in rng.integers(0, 151, 300)]), (1000, [int(x) for x in rng.integers(0, 151, 300)]),
             (5, [int(x) for x in rng.integers(0, 151, 100)])]
    cases += [(64, [0] * 200 + [50, 50, 1] + [0] * 70),   # runs of zero-length records, longer than the leaf bound
              (64, [100]), (64, [101]),                   # a record of exactly the bound, and one byte more
              (64, [40, 60, 1]), (64, [60, 41]),          # a record that ends exactly on the bound; one byte past it
              (64, [0, 0, 101, 0, 0]), (64, [100, 0, 0, 1]), (64, [150, 150, 150]), (64, [99, 1, 0, 0, 1, 100, 101, 100]),
              (2, [10, 10, 10, 10, 100, 0, 0])]
    return cases


def window_cases():
    """(s0, n, leaf bound, reply ends): chunks (1000, 2000], (2000, 3000], (3000, 3500]."""
    s0, n, bound = 1000, 2500, 1000
    special = [1001, 2000, 2001, 3000, 3001, 3500]  # a chunk's first leaf, its last leaf, one past it
    rng = np.random.default_rng(2026)
    cases = [(s0, n, bound, [e]) for e in special]
    for R in (63, 64, 65, 200):
        fill = [int(x) for x in rng.choice(np.arange(s0 + 1, s0 + n + 1), R, replace=False)]
        ends = sorted(set(special) | set(fill))
        while len(ends) > R:  # drop fills, keep the special ends
            ends.remove(next(e for e in ends if e not in special))
        cases.append((s0, n, bound, ends))
    # 64 replies, one verdict word, that straddle three chunks
    cases.append((s0, n, bound, list(range(1990, 2010)) + list(range(2990, 3012)) + list(range(3400, 3422))))
    # every reply in the last chunk, and every reply in the first
    cases.append((s0, n, bound, list(range(3100, 3300))))
    cases.append((s0, n, bound, list(range(1001, 1201))))
    # one reply per leaf of a small call in chunks of 50
    cases.append((7, 130, 50, list(range(8, 138))))
    return cases


OUTPUT_CALLS = [(1023, 1025, 50), (0, 65, 64), (2 ** 20 + 12345, 1000, 64), (5, 3, 1000)]
OUTPUT_MASKS = (63, 0, 8, 2, 32, 61)  # all, none, the root only, the nodes only, the paths only, all but the nodes


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    deps = [SRC, os.path.join(HERE, "..", "include", "plenum_verify.h")] + [
        os.path.join(CSRC, h) for h in ("merkle_plan.h", "merkle_core.h", "workspace.h")]
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-I", STUB, "-o", BIN, SRC])
    jobs = {"sweep": list(sweep_jobs()),
            "bytes": [[1, 77, len(lens), bound, 1, 100] + lens for bound, lens in byte_cases()],
            "windows": [[2, s0, n, bound, len(ends)] + ends for s0, n, bound, ends in window_cases()],
            "outputs": [[3, s0, n, bound, mask] for s0, n, bound in OUTPUT_CALLS for mask in OUTPUT_MASKS]}
    path = str(tmp_path_factory.mktemp("merkle_plan") / "jobs.bin")
    with open(path, "wb") as f:
        for group in jobs.values():
            for j in group:
                f.write(np.array(j, np.uint64).tobytes())
    out = subprocess.run([BIN, path], check=True, capture_output=True, text=True, timeout=120).stdout
    rep = json.loads(out)
    results = iter(rep.pop("jobs"))
    for name, group in jobs.items():
        rep[name] = [(j, next(results)) for j in group]
    assert next(results, None) is None
    return rep


def test_the_byte_bound_is_the_parents(report):
    assert report["MK_CHUNK_BYTES"] == CHUNK_BYTES


# --------------------------------------------------------------------------------------------- append chunks

def offsets(lens):
    return [7] + [7 + int(x) for x in np.cumsum(lens)]


def first_difference(rows, **wrong):
    for j, got in rows:
        _, s0, n, bound, with_off, byte_bound = j[:6]
        want = model_chunks(s0, n, bound, offsets(j[6:]) if with_off else None, byte_bound, **wrong)
        if got != want:
            return s0, n, bound, with_off
    return None


def check_properties(s0, n, got):
    """The chunks tile [0, n) in order, each holds a leaf, exactly the last one says so, a chunk's outputs start
    where the previous chunk's end, and the sums are pv_merkle_plan of the whole call."""
    at, pbase, node_off = 0, 0, 0
    for k, (c0, m, s, pb, no, n_nodes, n_path, is_last) in enumerate(got):
        assert c0 == at and m >= 1 and s == s0 + c0, (s0, n, k)
        assert (pb, no) == (pbase, node_off), (s0, n, k)
        assert is_last == int(k == len(got) - 1), (s0, n, k)
        at, pbase, node_off = at + m, pbase + n_path, node_off + n_nodes
    assert at == n
    assert node_off == node_count(s0 + n) - node_count(s0)
    assert pbase == sum(popcount(s0 + i) for i in range(n))


def test_append_chunk_sweep_matches_the_former_expressions(report):
    """Seven tree sizes x eight batch sizes x six leaf bounds, with and without offsets (whose bytes stay far
    below 2^30: both walks agree)."""
    rows = report["sweep"]
    assert len(rows) == 7 * 8 * 6 * 2
    assert first_difference(rows) is None
    counts = set()
    for j, got in rows:
        _, s0, n, bound = j[:4]
        check_properties(s0, n, got)
        assert len(got) == -(-n // bound) and all(r[1] == bound for r in got[:-1])
        counts.add(len(got))
    assert {1, 2, 5, 5000} <= counts
    for (ja, a), (jb, b) in zip(rows[0::2], rows[1::2]):
        assert (ja[4], jb[4]) == (0, 1) and a == b


@pytest.mark.parametrize("wrong", [{"pbase_from": 1}, {"strict": False}])
def test_the_comparison_notices_a_wrong_model(report, wrong):
    """The checker bites: a path base one leaf late, and a byte bound that leaves out a record ending exactly on it."""
    assert first_difference(report["sweep"] + report["bytes"], **wrong) is not None


def test_the_byte_bound_at_100_bytes(report):
    """A chunk is the longest prefix of at most 100 data bytes and at most `bound` leaves, and at least one leaf:
    a record above the bound is a chunk of its own, a record that ends on the bound closes its chunk, and
    zero-length records ride along up to the leaf bound."""
    rows = report["bytes"]
    assert first_difference(rows) is None
    seen = set()
    for j, got in rows:
        _, s0, n, bound, _, byte_bound = j[:6]
        lens = j[6:]
        check_properties(s0, n, got)
        for c0, m, *_ in got:
            size = sum(lens[c0:c0 + m])
            assert m <= bound
            assert size <= byte_bound or m == 1, (lens, c0, m)
            if c0 + m < n and m < bound:  # not cut by the call's end or the leaf bound: the next record did not fit
                assert size + lens[c0 + m] > byte_bound, (lens, c0, m)
            seen.add("over" if size > byte_bound else "exact" if size == byte_bound else "leaves" if m == bound else "under")
    assert seen == {"over", "exact", "leaves", "under"}
    named = {tuple(j[6:]): [r[:2] for r in got] for j, got in rows}
    assert named[(100,)] == [[0, 1]] and named[(101,)] == [[0, 1]]
    assert named[(40, 60, 1)] == [[0, 2], [2, 1]] and named[(60, 41)] == [[0, 1], [1, 1]]
    assert named[(0, 0, 101, 0, 0)] == [[0, 2], [2, 1], [3, 2]]
    assert named[(100, 0, 0, 1)] == [[0, 3], [3, 1]]
    assert named[(150, 150, 150)] == [[0, 1], [1, 1], [2, 1]]
    assert named[(99, 1, 0, 0, 1, 100, 101, 100)] == [[0, 4], [4, 1], [5, 1], [6, 1], [7, 1]]
    assert named[(10, 10, 10, 10, 100, 0, 0)] == [[0, 2], [2, 2], [4, 2], [6, 1]]
    zeros = named[tuple([0] * 200 + [50, 50, 1] + [0] * 70)]
    assert zeros == [[0, 64], [64, 64], [128, 64], [192, 10], [202, 64], [266, 7]]


# --------------------------------------------------------------------------------------------- reply windows

def test_reply_windows(report):
    """Lines 553-557 of the parent: r0 the first reply that ends above s, rounded down to a verdict word, r1 the
    first that ends above s + m. Every reply lies in the window of the chunk its end lies in, the windows meet,
    and r0 is a whole word."""
    rows = report["windows"]
    assert sorted({len(j[5:]) for j, _ in rows}) == [1, 63, 64, 65, 130, 200]
    for j, got in rows:
        _, s0, n, bound, R = j[:5]
        ends = j[5:]
        assert [r[:8] for r in got] == model_chunks(s0, n, bound)
        prev_r1, owner = 0, {}
        for k, (c0, m, s, *_, r0, r1) in enumerate(got):
            first = bisect.bisect_right(ends, s)
            assert (r0, r1) == (first & ~63, bisect.bisect_right(ends, s + m)), (ends, k)
            assert r0 % 64 == 0 and r0 <= first == prev_r1 <= r1 <= R
            assert all(s < e <= s + m for e in ends[first:r1])
            assert not any(s < e <= s + m for e in ends[:first] + ends[r1:])
            for r in range(first, r1):
                owner[r] = k
            prev_r1 = r1
        assert prev_r1 == R and sorted(owner) == list(range(R))
    straddle = next(got for j, got in rows if j[5:5 + 2] == [1990, 1991])
    assert [r[8:] for r in straddle] == [[0, 11], [0, 31], [0, 64]]  # one word, launched for each of three chunks
    per_leaf = next(got for j, got in rows if j[1] == 7)
    assert [r[8:] for r in per_leaf] == [[0, 50], [0, 100], [64, 130]]
    last_only = next(got for j, got in rows if j[5] == 3100)
    assert [r[8:] for r in last_only] == [[0, 0], [0, 0], [0, 200]]  # the first two chunks launch nothing


# -------------------------------------------------------------------------------------------- chunk outputs

def test_chunk_outputs_lie_inside_the_callers_arrays(report):
    """Arrays of exactly the call's size (AddressSanitizer guards their ends, UBSan the pointer arithmetic): a
    chunk's part starts at c0 leaves, node_off nodes and pbase path hashes, ends inside the array, the root and
    the frontier go to the last chunk only, and an output the caller does not take stays null whatever the chunk
    is (the parent formed node_hash + 32 * ... from a null node_hash)."""
    rows = report["outputs"]
    assert len(rows) == len(OUTPUT_CALLS) * len(OUTPUT_MASKS)
    for j, got in rows:
        _, s0, n, bound, mask = j
        assert [r[:8] for r in got] == model_chunks(s0, n, bound)
        total_nodes, total_path = node_count(s0 + n) - node_count(s0), popc_sum(s0 + n) - popc_sum(s0)
        for c0, m, s, pbase, node_off, n_nodes, n_path, is_last, leaf, node, roots, path, poff, root, frontier in got:
            assert leaf == (c0 if mask & 1 else -1) and roots == (c0 if mask & 16 else -1)
            assert node == (node_off if mask & 2 else -1)
            assert (path, poff) == ((pbase, c0) if mask & 32 else (-1, -1))
            assert root == (0 if mask & 8 and is_last else -1) and frontier == (0 if mask & 4 and is_last else -1)
            assert c0 + m <= n and node_off + n_nodes <= total_nodes and pbase + n_path <= total_path
            assert c0 + m + 1 <= n + 1  # the chunk's m + 1 path offsets


# ---------------------------------------------------------------------------------------------------- spans

def test_verdict_word_chunks_and_spans(report):
    """Lines 575-577 and 590-592 of the parent (the proof checks: the leaf bound rounded up to whole verdict
    words) and 602-603 (proof generation: the bound as it is)."""
    rows = report["spans"]
    assert [(r[0], r[1]) for r in rows] == [(b, n) for b in SPAN_BOUND for n in SPAN_N]
    for bound, n, vchunk, words, plain in rows:
        assert vchunk == (bound + 63) & ~63 and vchunk % 64 == 0 and bound <= vchunk < bound + 64
        for chunk, got in ((vchunk, words), (bound, plain)):
            assert got == [[c0, min(chunk, n - c0)] for c0 in range(0, n, chunk)]
            assert sum(m for _, m in got) == n
        assert all(c0 % 64 == 0 for c0, _ in words)
    assert {r[0]: r[2] for r in rows} == {1: 64, 50: 64, 63: 64, 64: 64, 65: 128, 1000: 1024}
    # a body's non-zero return ends either walk at once and is what the walk returns
    assert report["stops"] == [-7, 3, -9, 3]


# --------------------------------------------------------------------------------------------------- checks

SIZES = "tree_size + n must stay below 2^48"
FRONTIER = "a tree of size > 0 needs its frontier"
POFF = "proof offsets must be non-decreasing over a proof array"
ENDS = "reply ends must increase strictly within (tree_size, tree_size + n]"
ALIGNED = "hash arrays must be 16-byte aligned"


def test_every_check_on_each_side_of_its_condition(report):
    assert report["checks"] == {
        # 2^48: each of a, b and a + b; the wording may be the entry's own
        "sizes_below": None, "sizes_sum": SIZES, "sizes_a": SIZES, "sizes_b": SIZES, "sizes_a_max": None,
        "sizes_own_wording": "the store must stay below 2^48 leaves", "sizes_wrap": SIZES,
        "count_below": None, "count_at": "more than 2^32 - 1 proofs",
        # the append arguments of a host-buffer entry, in the order of the checks
        "host_ok": None, "host_sizes": SIZES, "host_sizes_before_frontier": SIZES, "host_frontier": FRONTIER,
        "host_frontier_given": None, "host_null_offsets": "null offsets", "host_no_leaves_no_offsets": None,
        "host_decreasing": "offsets must be non-decreasing", "host_null_data": "null data",
        "host_null_data_empty_records": None, "host_offsets_before_data": "offsets must be non-decreasing",
        # ... and of a device-buffer entry
        "dev_ok": None, "dev_sizes": SIZES, "dev_frontier": FRONTIER, "dev_null_data": "null pointer",
        "dev_null_off": "null pointer", "dev_no_leaves": None,
        "out_null": "null output struct", "out_empty": None, "out_path_alone": "path and path_off go together",
        "out_pair": None, "out_path_off_alone": "path and path_off go together",
        "poff_ok": None, "poff_decreasing": POFF, "poff_null_proof": POFF, "poff_null_proof_no_hashes": None,
        "ends_ok": None, "ends_at_tree_size": ENDS, "ends_equal": ENDS, "ends_decreasing": ENDS, "ends_past": ENDS,
        "ends_one_last": None, "ends_one_past": ENDS,
        "aligned_0_16_null": None, "aligned_8": ALIGNED, "aligned_8_first": ALIGNED, "aligned_1": ALIGNED,
        "aligned_none": None, "append_aligned": None, "append_frontier_8": ALIGNED,
        "append_out_8_0": ALIGNED, "append_out_8_1": ALIGNED, "append_out_8_2": ALIGNED, "append_out_8_3": ALIGNED,
        "append_out_8_4": ALIGNED, "append_out_8_5": ALIGNED, "append_path_off_8": None}
