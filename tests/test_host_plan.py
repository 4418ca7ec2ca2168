"""The host-buffer call plan (indy-plenum_amd/csrc/host_plan.h: the staging layout, the sub-batch bounds, the form
of a staged call and what follows from it, the key-repeat answer behind AUTO's host-side hint, the zero-copy slot
format) and the admission sample (csrc/kc_admit.h admit_sample), compiled with g++ exactly as the library includes
them, under AddressSanitizer and UBSan, and run as a stand-alone program (tests/native/host_plan_check.cpp). Named
calls with bounds worked out by hand, then a sweep on either side of every threshold against a Python model that
transcribes the expressions as they stood inside stage_and_launch, pv_keyed_hint, pv_verify_batch and
kc_auto_after_batch before the plan had a file of its own. What the plan leads to on the device is checked by
tests/test_gpu_host_path.py. CPU only."""
import json
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "host_plan_check.cpp")
STUB = os.path.join(HERE, "native", "stub_hip")
CSRC = os.path.join(HERE, "..", "indy-plenum_amd", "csrc")
BIN = os.path.join(HERE, "native", "host_plan_check")

AUTO, STRAUS, COMB, LATENCY = 0, 1, 2, 3  # PV_PATH_*
ONE_DMA, PIPELINED = 0, 1  # pvhost::Form
SUB, END, PIPE_MAX, MIN_BLOB, SLACK = 262144, 131072, 64, 8 << 20, 256
ALLCOMB_KEYS, KC_AUTO_MAX_BATCH = 2048, 4096
ZC_PK_WORD, ZC_REC_WORD, ZC_SLACK, ZC_MAX_STRIDE = 4, 12, 160, 2048
REC = 363  # bytes per record the program gives a named call
M64 = (1 << 64) - 1


def key_sets():
    """Seeded key sets for few_distinct_keys and what numpy.unique over the first 16 bytes says of each: on both
    sides of 3 * distinct <= n, on both sides of PV_ALLCOMB_KEYS distinct keys, and keys that differ only in bytes
    16..31."""
    rng = np.random.default_rng(2024)
    sets = []

    def repeated(distinct, n):
        keys = rng.integers(0, 256, (distinct, 32), dtype=np.uint8)
        idx = np.concatenate([np.arange(distinct), rng.integers(0, distinct, n - distinct)])
        return keys[rng.permutation(idx)]

    for distinct, n in ((1000, 3000), (1000, 2999), (1001, 3000), (1, 3), (1, 2), (1365, 4096), (1366, 4096),
                        (683, 2049), (684, 2049), (2048, 6144), (2049, 6147), (2048, 8192), (2049, 8192), (2047, 8192), (3000, 8000)):
        sets.append(repeated(distinct, n))
    # two keys that differ only in bytes 16..31 count as one: 3 requests, 2 full keys, 1 counted
    a = rng.integers(0, 256, 32, dtype=np.uint8)
    b = a.copy()
    b[16:] ^= 0xFF
    sets.append(np.stack([a, b, a]))
    # ... and a difference in byte 15 counts: 3 requests, 2 counted
    c = a.copy()
    c[15] ^= 1
    sets.append(np.stack([a, c, a]))
    # 1,000 keys with one 16-byte prefix each and distinct tails everywhere: 1,000 counted among 3,000 full keys
    k = repeated(1000, 3000)
    k[:, 16:] = rng.integers(0, 256, (3000, 16), dtype=np.uint8)
    sets.append(k)
    # a first word of zero (the table marks an empty entry with (0, 0): the count ORs 1 into the word)
    z = repeated(10, 30)
    z[:, :8] = 0
    sets.append(z)
    return sets


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    deps = [SRC, os.path.join(HERE, "..", "include", "plenum_verify.h")] + [
        os.path.join(CSRC, h) for h in ("host_plan.h", "kc_admit.h", "chunk_plan.h", "pv_internal.h", "stage.h",
                                        "workspace.h")]
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-I", STUB, "-o", BIN, SRC])
    sets = key_sets()
    path = str(tmp_path_factory.mktemp("host_plan") / "keys.bin")
    with open(path, "wb") as f:
        for s in sets:
            f.write(np.uint64(len(s)).tobytes())
            f.write(np.ascontiguousarray(s, np.uint8).tobytes())
    out = subprocess.run([BIN, path], check=True, capture_output=True, text=True, timeout=120).stdout
    rep = json.loads(out)
    rep["key_sets"] = sets
    return rep


def test_the_constants_are_the_ones_the_model_uses(report):
    """The program was compiled with the header's defaults, which are the parent's values. PV_PIPE_SUB from the
    environment is cut to a multiple of 64 and raised to 8,192."""
    assert report["constants"] == {
        "PV_PIPE_SUB": SUB, "PV_PIPE_END_DEFAULT": END, "PV_PIPE_MAX": PIPE_MAX, "PV_PIPE_MIN_BLOB": MIN_BLOB,
        "PV_KC_AUTO_MAX_BATCH": KC_AUTO_MAX_BATCH, "PV_BLOB_SLACK": SLACK, "PV_ALLCOMB_KEYS": ALLCOMB_KEYS,
        "PV_LATENCY_MAX": 4096, "PV_ZC_MAX_REQ": 2048, "PV_ZC_MAX_STRIDE": ZC_MAX_STRIDE, "PV_ZC_PK_WORD": ZC_PK_WORD,
        "PV_ZC_REC_WORD": ZC_REC_WORD, "PV_ZC_SLACK": ZC_SLACK, "pipe_end_req": END, "pipe_sub_default": SUB,
        "pipe_sub_of_1": 8192, "pipe_sub_of_8255": 8192, "pipe_sub_of_8256": 8256}


# --------------------------------------------------------------------------------------------------- pieces

def model_pieces(n, blob, sub, end_req, halves_from=3, floor_mid=False):
    """pv_host.hip:307-325 of the parent commit with PV_PIPE_HALF_ENDS at its default. halves_from / floor_mid:
    deliberately wrong variants."""
    bnd = [0]
    if blob >= MIN_BLOB and n >= halves_from * sub:
        h = min(end_req, sub) // 64 * 64
        mid = n - 2 * h
        k = min(PIPE_MAX - 2, max(1, (mid + (0 if floor_mid else sub // 2)) // sub))
        bnd.append(h)
        for j in range(1, k):
            bnd.append(h + (mid * j // k) // 64 * 64)
        bnd.append((n - h) & ~63)
    elif blob >= MIN_BLOB:
        k = min(PIPE_MAX, max(1, n // sub))
        for j in range(1, k):
            bnd.append((n * j // k) & ~63)
    bnd.append(n)
    return bnd


def test_named_calls(report):
    """The sizes the GPU tests and the bench use. At the default sub-batch of 262,144 a call pipelines from 524,288
    requests on: 400,000, 263,143 and 322,144 are one piece. A blob just under 8 MB is one piece whatever n is. At
    PV_PIPE_SUB=8192 the GPU test's 30,001 requests are a first, two middle and a ragged last sub-batch."""
    got = {(n, blob, sub): bnd for n, blob, sub, _, bnd in report["named"]}
    assert len(got) == len(report["named"]) == 11 and all(end == END for _, _, _, end, _ in report["named"])
    assert got[(400000, 400000 * REC, SUB)] == [0, 400000]
    assert got[(263143, 263143 * REC, SUB)] == [0, 263143]
    assert got[(322144, 322144 * REC, SUB)] == [0, 322144]
    assert got[(524288, 524288 * REC, SUB)] == [0, 262144, 524288]
    assert got[(1048576, 1048576 * REC, SUB)] == [0, 131072, 393216, 655360, 917504, 1048576]
    for n in (1, 30001, 1048576, 70 * 262144):
        assert got[(n, MIN_BLOB - 1, 8192)] == [0, n]
    assert got[(30001, 30001 * REC, 8192)] == [0, 8192, 14976, 21760, 30001]
    assert got[(40037, 40037 * REC, 8192)] == [0, 8192, 16064, 23936, 31808, 40037]


def sweep_inputs():
    for sub in (8192, 65536, 262144):
        for n in (1, 63, 64, 65, sub - 1, sub, sub + 1, 2 * sub - 1, 2 * sub, 2 * sub + 1, 3 * sub - 1, 3 * sub,
                  64 * sub, 70 * sub):
            for blob in (MIN_BLOB - 1, MIN_BLOB, n * REC):
                for end_req in (8192, sub // 2, sub, 2 * sub):
                    yield n, blob, sub, end_req


def first_difference(rows, **wrong):
    for n, blob, sub, end_req, bnd in rows:
        if bnd != model_pieces(n, blob, sub, end_req, **wrong):
            return n, blob, sub, end_req, bnd, model_pieces(n, blob, sub, end_req, **wrong)
    return None


def test_pieces_sweep_matches_the_former_expressions(report):
    """n on both sides of every threshold x the blob on both sides of 8 MB (and a realistic one) x three sub-batch
    sizes x four end sizes: the bounds are the parent's, start at 0, end at n, increase strictly, are whole verdict
    words inside, and are at most PV_PIPE_MAX pieces."""
    rows = report["sweep"]
    assert [tuple(r[:4]) for r in rows] == list(sweep_inputs()) and len(rows) == 3 * 14 * 3 * 4
    assert first_difference(rows) is None
    shapes = set()
    for n, blob, sub, end_req, bnd in rows:
        assert bnd[0] == 0 and bnd[-1] == n, (n, blob, sub, end_req, bnd)
        assert all(a < b for a, b in zip(bnd, bnd[1:])), (n, blob, sub, end_req, bnd)
        assert all(b % 64 == 0 for b in bnd[1:-1]), (n, blob, sub, end_req, bnd)
        assert 1 <= len(bnd) - 1 <= PIPE_MAX, (n, blob, sub, end_req, bnd)
        if blob < MIN_BLOB:
            assert bnd == [0, n]
        shapes.add(len(bnd) - 1)
    assert {1, 2, 3, 4, PIPE_MAX} <= shapes  # one piece, equal pieces, half-size ends, and the cap


@pytest.mark.parametrize("wrong", [{"halves_from": 2}, {"floor_mid": True}])
def test_the_comparison_notices_a_wrong_model(report, wrong):
    """The checker bites: half-size ends from two sub-batches on, and a middle count rounded down, each differ."""
    assert first_difference(report["sweep"], **wrong) is not None


# --------------------------------------------------------------------------------------------------- layout

def test_layout_is_the_former_rounding(report):
    """pv_host.hip:294-298, 332-333 of the parent: pk, offsets and verdict words each rounded up to 256 bytes, the
    blob and its slack behind them unrounded. The sections are aligned, in order, and hold what they are for."""
    def up(x):
        return (x + 255) & ~255

    assert len(report["layout"]) == 14 * 5
    for n, blob, pk, off, ver, blob_off, vwords, ver_bytes, total in report["layout"]:
        pk_bytes, off_bytes, vw = up(n * 32), up((n + 1) * 8), (n + 63) // 64
        v_bytes = up(vw * 8)
        assert (pk, off, ver, blob_off) == (0, pk_bytes, pk_bytes + off_bytes, pk_bytes + off_bytes + v_bytes), n
        assert (vwords, ver_bytes) == (vw, v_bytes), n
        assert total == pk_bytes + off_bytes + v_bytes + blob + SLACK, (n, blob)
        assert all(x % 256 == 0 for x in (pk, off, ver, blob_off))
        assert pk + n * 32 <= off and off + (n + 1) * 8 <= ver and ver + vw * 8 <= blob_off
        assert blob_off + blob + SLACK == total


# ---------------------------------------------------------------------------------------------------- calls

def test_form_host_bytes_sharing_and_injection_point(report):
    """All eight pinned combinations x one piece, four pieces, two pieces x the four paths: one DMA only for one
    piece with nothing pinned (pv_host.hip:345); no host staging only when all three inputs are pinned (:328); tables
    may be shared by more than one piece under AUTO or COMB (:434); an injected failure fires before piece
    min(1, np - 1)'s kernels (:450)."""
    rows = report["calls"]
    assert len(rows) == 3 * 8 * 4
    assert {(r[0], r[1], r[2], r[3]) for r in rows} == {(np_, a, b, c) for np_ in (1, 4, 2) for a in (0, 1)
                                                         for b in (0, 1) for c in (0, 1)}
    for np_, pin_sm, pin_pk, pin_off, path, total, form, host_bytes, may_share, inject_at, all_pin, kept in rows:
        any_pin, all_ = pin_sm or pin_pk or pin_off, pin_sm and pin_pk and pin_off
        assert form == (ONE_DMA if np_ == 1 and not any_pin else PIPELINED)
        assert host_bytes == (0 if all_ else total)
        assert may_share == int(np_ > 1 and path in (AUTO, COMB))
        assert inject_at == min(1, np_ - 1)
        assert all_pin == all_ and kept == 1


# ----------------------------------------------------------------------------------------------------- keys

def test_key_repeat_answer_against_numpy_unique(report):
    """few_distinct_keys(pk, n) is distinct <= PV_ALLCOMB_KEYS and 3 * distinct <= n, distinct counted over the keys'
    first 16 bytes."""
    sets = report["key_sets"]
    assert len(report["keys"]) == len(sets)
    seen = set()
    for ans, s in zip(report["keys"], sets):
        distinct, n = len(np.unique(s[:, :16], axis=0)), len(s)
        assert ans == int(distinct <= ALLCOMB_KEYS and 3 * distinct <= n), (distinct, n)
        seen.add((distinct <= ALLCOMB_KEYS, 3 * distinct <= n))
    assert seen == {(True, True), (True, False), (False, True), (False, False)}
    want = [(1000, 3000, 1), (1000, 2999, 0), (1001, 3000, 0), (1, 3, 1), (1, 2, 0), (1365, 4096, 1), (1366, 4096, 0),
            (683, 2049, 1), (684, 2049, 0), (2048, 6144, 1), (2049, 6147, 0), (2048, 8192, 1), (2049, 8192, 0),
            (2047, 8192, 1), (3000, 8000, 0)]
    for (distinct, n, ans), s, got in zip(want, sets, report["keys"]):
        assert (len(np.unique(s[:, :16], axis=0)), len(s), got) == (distinct, n, ans)
    tails, byte15, prefixes, zero_word = report["keys"][len(want):]
    assert len(np.unique(sets[len(want)], axis=0)) == 2 and tails == 1  # bytes 16..31 are not looked at
    assert byte15 == 0  # byte 15 is
    assert len(np.unique(sets[len(want) + 2], axis=0)) == 3000 and prefixes == 1
    assert zero_word == 1


# ------------------------------------------------------------------------------------------------------- zc

def test_zero_copy_slots(report):
    """zc_stride is pv_host.hip:505 of the parent; a slot is the record's length in word 0 and zeros up to the key,
    the key from word 4, the record from word 12, zeros to the end of the slot (at least PV_ZC_SLACK). Filled into a
    buffer of exactly n x stride bytes under AddressSanitizer; slots outside [a, b) are not touched."""
    cases = report["zc"]
    assert [(c["lens"], c["a"], c["b"]) for c in cases] == [
        ([0, 0, 0], 0, 3), ([0, 1, 1, 0], 0, 4), ([1840, 5, 0, 1839], 0, 4), ([1841], 0, 1),
        ([100, 200, 300, 17], 1, 3), ([816], 0, 1)]
    assert [c["stride"] for c in cases] == [256, 256, 2048, 2112, 512, 1024]
    for c in cases:
        lens, stride = c["lens"], c["stride"]
        assert stride == (4 * ZC_REC_WORD + max(lens) + ZC_SLACK + 63) & ~63
        buf = np.frombuffer(bytes.fromhex(c["hex"]), np.uint8).reshape(len(lens), stride)
        off = np.concatenate([[5], 5 + np.cumsum(lens)])
        sm = ((np.arange(off[-1]) * 7 + 3) & 0xFF).astype(np.uint8)
        for i, ln in enumerate(lens):
            sl = buf[i]
            if not c["a"] <= i < c["b"]:
                assert (sl == 0xAA).all(), i
                continue
            assert sl[:4].view("<u4")[0] == ln and not sl[4:4 * ZC_PK_WORD].any(), i
            key = ((i * 37 + np.arange(32) * 11 + 1) & 0xFF).astype(np.uint8)
            assert np.array_equal(sl[4 * ZC_PK_WORD:4 * ZC_PK_WORD + 32], key), i
            assert 4 * ZC_PK_WORD + 32 == 4 * ZC_REC_WORD
            assert np.array_equal(sl[4 * ZC_REC_WORD:4 * ZC_REC_WORD + ln], sm[off[i]:off[i + 1]]), i
            tail = sl[4 * ZC_REC_WORD + ln:]
            assert len(tail) >= ZC_SLACK and not tail.any(), i
    # the longest record whose slot still fits PV_ZC_MAX_STRIDE is 1,840 bytes
    assert cases[2]["stride"] == ZC_MAX_STRIDE < cases[3]["stride"]


# --------------------------------------------------------------------------------------------------- sample

def test_admission_sample(report):
    """pv_host.hip:212-217 of the parent: no sample up to PV_KC_AUTO_MAX_BATCH requests (every request is counted);
    above, one request from each block of ceil(n / 4,096), inside its block, at the hashed position."""
    got = dict((n, idx) for n, idx in report["sample"])
    assert sorted(got) == [1, 4095, 4096, 4097, 8191, 8192, 8193, 30001, 100000, 1048576, 1048583]
    for n, idx in got.items():
        if n <= KC_AUTO_MAX_BATCH:
            assert idx == [], n
            continue
        stride = (n + KC_AUTO_MAX_BATCH - 1) // KC_AUTO_MAX_BATCH
        blocks = list(range(0, n, stride))
        assert len(idx) == len(blocks) <= KC_AUTO_MAX_BATCH, n
        for t, (b, i) in enumerate(zip(blocks, idx)):
            assert b <= i < min(b + stride, n), (n, t)
            assert i == b + (((t * 0x9E3779B97F4A7C15) & M64) >> 40) % min(stride, n - b), (n, t)
    assert len(got[1048576]) == 4096 and len(got[4097]) == 2049 and len(got[8193]) == 2731
