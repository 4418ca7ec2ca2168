"""The launch plan (indy-plenum_amd/csrc/chunk_plan.h: the path of a batch, and per chunk the path, the views a key
is looked up in, the KeyWork scalars, the launch shape, the grids, the follow-up kernels, the clears the dirty flags
force; the wide pool's allocation trigger), compiled with g++ exactly as the library includes it, under
AddressSanitizer and UBSan, and run as a stand-alone program (tests/native/chunk_plan_check.cpp). Scenarios with
plans worked out by hand, then every combination of the inputs on either side of each threshold against a Python
model that transcribes the conditions as they stood inside launch_chunk and launch_chunks before the plan had a file
of its own, and the zero-copy gate of pv_verify_batch against the expression it used to spell out. What the plan
leads to on the device is read back by the GPU tests through pv_last_path, pv_last_split and the reuse, affine and
wide counters (tests/test_gpu_*.py). CPU only."""
import json
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "chunk_plan_check.cpp")
STUB = os.path.join(HERE, "native", "stub_hip")
CSRC = os.path.join(HERE, "..", "indy-plenum_amd", "csrc")
BIN = os.path.join(HERE, "native", "chunk_plan_check")

AUTO, STRAUS, COMB, LATENCY = 0, 1, 2, 3  # PV_PATH_*
NONE, NODE, NODE_THEN_XT, XT_ONLY = 0, 1, 2, 3  # pvhost::Lookup
M = 1 << 20

# the thresholds as the library compiles them by default; the program reports what it was compiled with
LATENCY_MAX, KEYED_HINT_MIN, KEYED_MIN, XT_KEYS, KEY_CAP, NSEG = 4096, 2049, 4097, 2048, 16384, 8
COMB_MIN_REQ, SPARSE_CHUNK, FUSED_MIN_REQ, KEY_SEED, SIDE_GRID_PER_CU = 48, 65536, 262144, 4096, 2
LP_CHAIN_BLOCKS, ENC_SMALL_B, ENC16_MIN, INS_REQS, BLOCK, FILL_ITEMS_PER_KEY = 2048, 8, 0xFFFFFFFF, 4096, 256, 256
DIR_CAP, KC_WCAP = 14336, 1024  # what the program's inputs hold fixed

IN_BITS = ["hint_set", "keyed_hint", "cache", "xt_fill", "xt_use", "dir_on", "aff_on", "slots_dirty", "dir_dirty"]
OUT_BITS = ["latency", "dev_choice", "gate", "keyed", "kc_on", "dir_on", "dir_pub", "aff_conv", "wide_conv",
            "lat_choice", "dense_only", "dir_use", "direct_fill", "fused", "enc16", "clear_slots", "clear_dir",
            "mark_dir_dirty", "run_probe", "run_xtab_publish", "run_dir_publish", "run_affine", "run_widen",
            "run_dev_latency"]
OUT_WORDS = ["lookup", "min_req", "kc_wcap", "dir_cap", "wide_cap", "chunk_n", "seg_cap", "kcap", "seed_reqs",
             "req_grid", "ins_grid", "probe_grid", "chain_blocks", "fill_grid", "side_grid", "enc_grid", "pub_grid"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    deps = [SRC, os.path.join(CSRC, "chunk_plan.h"), os.path.join(HERE, "..", "include", "plenum_verify.h")]
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                               "-I", STUB, "-o", BIN, SRC])
    sweep = str(tmp_path_factory.mktemp("chunk_plan") / "sweep.u32")
    out = subprocess.run([BIN, sweep], check=True, capture_output=True, text=True, timeout=120).stdout
    rep = json.loads(out)
    rep["rows"] = np.fromfile(sweep, dtype="<u4").reshape(-1, rep["sweep_words"]).tolist()
    return rep


def test_the_thresholds_are_the_ones_the_model_uses(report):
    """The program was compiled with the header's defaults, which are the parent's values."""
    assert report["constants"] == {
        "PV_LATENCY_MAX": LATENCY_MAX, "PV_KEYED_HINT_MIN": KEYED_HINT_MIN, "PV_KEYED_MIN": KEYED_MIN,
        "PV_ALLCOMB_KEYS": 2048, "PV_XT_KEYS": XT_KEYS, "PV_KEY_CAP": KEY_CAP, "PV_NSEG": NSEG,
        "PV_COMB_MIN_REQ": COMB_MIN_REQ, "PV_SPARSE_CHUNK": SPARSE_CHUNK, "PV_FUSED_MIN_REQ": FUSED_MIN_REQ,
        "PV_KEY_SEED": KEY_SEED, "PV_SIDE_GRID_PER_CU": SIDE_GRID_PER_CU, "PV_LP_CHAIN_BLOCKS": LP_CHAIN_BLOCKS,
        "PV_ENC_SMALL_B": ENC_SMALL_B, "PV_ENC16_MIN": ENC16_MIN, "PV_INS_REQS": INS_REQS, "PV_BLOCK": BLOCK,
        "PV_FILL_ITEMS_PER_KEY": FILL_ITEMS_PER_KEY}


def expect(plan, **want):
    got = {k: plan[k] for k in want}
    assert got == want


# ------------------------------------------------------------------------------------------------ scenarios
# Inputs unless a scenario says otherwise: AUTO, a device-buffer call (no hint), no node cache, no pipelined
# call, the directory on with 14,336 slots, affine rows on, the wide pool configured and present with 2,048
# tables, 16,384 comb keys, 256 CUs, nothing dirty.

def test_headline_chunk(report):
    """2^20 requests under AUTO: above PV_KEYED_MIN so keyed; above PV_SPARSE_CHUNK so the fill follows the chain
    (direct_fill), the tables are whole and listed (dir_pub), hit tables are converted (aff_conv) and, the pool being
    there, widened (wide_conv); above PV_FUSED_MIN_REQ so the fused comb kernel; above 16 x PV_KEY_SEED so a seed
    pre-pass of 4,096 requests. 4,096 request workgroups, 256 insert workgroups of 4,096 requests, 16,384 waves in 8
    segments of 2,048 waves = 131,072 ids each, probed by 4,096 workgroups; 2,048 chain waves; the fill capped at
    4,096 workgroups; 2 x 256 side workgroups; 2,048 requests per encode workgroup; 16,384 / 256 publish workgroups."""
    expect(report["scenarios"]["headline"], latency=0, dev_choice=0, keyed=1, lookup=NONE, min_req=48, kc_on=1,
           dir_on=1, dir_cap=DIR_CAP, dir_pub=1, aff_conv=1, wide_cap=2048, wide_conv=1, chunk_n=M, seg_cap=131072,
           lat_choice=0, dense_only=0, kcap=KEY_CAP, direct_fill=1, fused=1, seed_reqs=4096, enc16=0, req_grid=4096,
           ins_grid=256, probe_grid=4096, chain_blocks=2048, fill_grid=4096, side_grid=512, enc_grid=512, pub_grid=64,
           clear_slots=0, clear_dir=0, mark_dir_dirty=1, run_probe=1, run_xtab_publish=0, run_dir_publish=1,
           run_affine=1, run_widen=1, run_dev_latency=0)


def test_host_call_of_3072_with_a_keyed_hint(report):
    """The host counted few keys: not latency although n <= PV_LATENCY_MAX, no device choice (hint_set), keyed by the
    hint. 3,072 <= PV_SPARSE_CHUNK: the fill goes to the fill stream where the sparse fill follows, nothing is
    listed, the two-kernel comb form, no seed. The directory is still consulted (dir_on, the probe runs)."""
    expect(report["scenarios"]["host_3072_keyed_hint"], latency=0, dev_choice=0, keyed=1, direct_fill=0, fused=0,
           seed_reqs=0, dir_on=1, kc_on=1, dir_pub=0, aff_conv=0, wide_conv=0, run_probe=1, run_dir_publish=0,
           run_affine=0, run_widen=0, run_dev_latency=0, lat_choice=0, chunk_n=3072, seg_cap=384, req_grid=12,
           ins_grid=1, probe_grid=12, side_grid=12, enc_grid=2)


def test_device_call_of_3072_decides_on_the_device(report):
    """No hint and an empty cache between PV_KEYED_HINT_MIN and PV_LATENCY_MAX: the keyed kernels run with
    lat_choice, and the latency launch follows them, gated by the scan's choice."""
    expect(report["scenarios"]["device_3072_empty_cache"], latency=0, dev_choice=1, keyed=1, lat_choice=1,
           run_dev_latency=1, direct_fill=0, fused=0, seed_reqs=0, dir_pub=0)


def test_device_call_of_3072_with_a_cache_takes_the_latency_path(report):
    """A non-empty key cache keeps the latency path: no device choice."""
    expect(report["scenarios"]["device_3072_cache"], latency=1, dev_choice=0, lookup=NODE)


def test_sub_batch_0_of_a_pipelined_call(report):
    """xt_fill at 262,144 requests: the tables go to the call's store, so the directory is bypassed (dir_on, dir_pub,
    wide_cap 0; dir_dirty is neither set nor cleared), at most PV_XT_KEYS = 2,048 comb keys (the key stream's grids
    follow: 2,048 fill workgroups, 8 publish workgroups), never a sparse fill, and the tables are published. With no
    cache and no directory there is nothing to probe. 262,144 is not above PV_FUSED_MIN_REQ."""
    expect(report["scenarios"]["pipelined_sub0"], latency=0, keyed=1, lookup=NONE, dir_use=0, dir_on=0, kc_on=0,
           dir_pub=0, aff_conv=0, wide_cap=0, wide_conv=0, kcap=2048, dense_only=1, run_xtab_publish=1, run_probe=0,
           mark_dir_dirty=0, clear_dir=0, run_dir_publish=0, direct_fill=1, fused=0, chain_blocks=2048,
           fill_grid=2048, pub_grid=8, seed_reqs=4096)


def test_later_sub_batch_with_the_node_cache(report):
    """xt_use with a node cache: the cache first, the call's store as the second view; the cache's wide rows stay
    readable. A later sub-batch goes through the directory like any chunk."""
    expect(report["scenarios"]["pipelined_later_node_cache"], keyed=1, lookup=NODE_THEN_XT, kc_on=1, kc_wcap=KC_WCAP,
           dir_on=1, dir_pub=1, dense_only=0, kcap=KEY_CAP, run_xtab_publish=0, run_probe=1)


def test_later_sub_batch_without_the_node_cache(report):
    """xt_use alone: the call's store is the only view, in the node cache's place, and it has no wide rows
    (kc_wcap 0). The chunk counts as one with an active cache: kc_on and the probe."""
    expect(report["scenarios"]["pipelined_later"], keyed=1, lookup=XT_ONLY, kc_on=1, kc_wcap=0, dir_on=1, dir_pub=1,
           dense_only=0, kcap=KEY_CAP, run_xtab_publish=0, run_probe=1)


def test_forced_paths(report):
    """Forced COMB at one request: keyed, every key a comb key (min_req 1), one workgroup of each per-request
    kernel. Forced STRAUS at 2^20: not keyed, no key kernel and no follow-up. Forced LATENCY at 2^20: latency."""
    expect(report["scenarios"]["forced_comb_1"], latency=0, dev_choice=0, keyed=1, min_req=1, req_grid=1, ins_grid=1,
           side_grid=1, enc_grid=1, seg_cap=64, probe_grid=2, seed_reqs=0, direct_fill=0, fused=0)
    expect(report["scenarios"]["forced_straus_1m"], latency=0, dev_choice=0, keyed=0, min_req=48, clear_slots=0,
           clear_dir=0, mark_dir_dirty=0, run_probe=0, run_xtab_publish=0, run_dir_publish=0, run_affine=0,
           run_widen=0, run_dev_latency=0, req_grid=4096, enc_grid=512)
    expect(report["scenarios"]["forced_latency_1m"], latency=1, dev_choice=0)


def test_wide_pool_is_attempted_by_the_fourth_dense_chunk_and_never_after_a_failure(report):
    """Dense keyed chunks with no pool: the first three only count, the fourth attempts the allocation. The attempt
    fails (wide_failed): no later chunk attempts or counts."""
    assert report["wide_run"] == [[0, 1], [0, 2], [0, 3], [1, 4], [0, 4], [0, 4], [0, 4]]


def test_wide_pool_trigger_matches_the_former_condition(report):
    """pv_engine.hip:1876 of the parent: keyed && kw.dir_pub && !wide_failed && d_wide.cap < wide_want &&
    ++wide_dense >= 4, the increment reached only when everything before it holds (and wrapping at 2^32)."""
    assert len(report["wide"]) == 2 * 2 * 2 * 5 * 6
    for keyed, pub, failed, have, want, dense, attempt, dense_next in report["wide"]:
        att = False
        if keyed and pub and not failed and have < want:
            dense = (dense + 1) & 0xFFFFFFFF
            att = dense >= 4
        assert (attempt, dense_next) == (int(att), dense), (keyed, pub, failed, have, want)


# ---------------------------------------------------------------------------------------------------- sweep

def model(i, wide_cap, pool, cus, m, n, sparse_ge=False, dir_during_fill=False):
    """launch_chunks (pv_engine.hip:2085-2089) and launch_chunk (pv_engine.hip:1834-1909, the conditions around the
    launches in 1910-2068) of the parent commit, condition by condition; the encode grid from 2032-2039. i: the inputs
    named in IN_BITS and the path. sparse_ge / dir_during_fill: deliberately wrong variants."""
    path = i["path"]
    # launch_chunks
    kc_nonempty = i["cache"]
    dev_choice = path == AUTO and not i["hint_set"] and not kc_nonempty and KEYED_HINT_MIN <= n <= LATENCY_MAX
    latency = path == LATENCY or (path == AUTO and n <= LATENCY_MAX and not i["keyed_hint"] and not dev_choice)
    # pv_host.hip:505-507, with pv_keyed_hint's answer as the input
    gate = path == LATENCY or (path == AUTO and n <= LATENCY_MAX and not i["keyed_hint"])
    # launch_chunk: the views (1834-1852)
    node_kc = i["cache"]
    kcv_hmask, xtv_hmask, xt_only = node_kc, False, False
    if i["xt_use"]:
        if node_kc:
            xtv_hmask = True
        else:
            kcv_hmask, xt_only = True, True
    kc_active = kcv_hmask
    lookup = XT_ONLY if xt_only else NODE_THEN_XT if xtv_hmask else NODE if node_kc else NONE
    keyed = path == COMB or (path == AUTO and (m >= KEYED_MIN or i["keyed_hint"] or dev_choice or kc_active))
    # the KeyWork scalars (1860-1907)
    min_req = 1 if path == COMB else COMB_MIN_REQ
    dir_use = i["dir_on"] and (dir_during_fill or not i["xt_fill"])
    dense = m >= SPARSE_CHUNK if sparse_ge else m > SPARSE_CHUNK
    dir_pub = dir_use and dense
    aff_conv = dir_pub and i["aff_on"]
    kw_wide_cap = min(wide_cap, pool) if dir_use else 0
    wide_conv = dir_pub and kw_wide_cap != 0
    seg_cap = (((m + 63) // 64) + NSEG - 1) // NSEG * 64
    kcap = min(KEY_CAP, XT_KEYS) if i["xt_fill"] else KEY_CAP
    limit = kcap
    direct_fill = dense
    # the key stage (1910-1970)
    seed = min(m, KEY_SEED) if KEY_SEED > 0 and m > 16 * KEY_SEED else 0
    grid = (m + BLOCK - 1) // BLOCK
    items = limit * 32 * 8  # PV_COMB_POS * PV_COMB_BLOCKS
    enc16 = m >= ENC16_MIN
    eb = 16 if enc16 else ENC_SMALL_B
    bits = dict(
        latency=latency, dev_choice=dev_choice, gate=gate, keyed=keyed, kc_on=kc_active or dir_use, dir_on=dir_use,
        dir_pub=dir_pub, aff_conv=aff_conv, wide_conv=wide_conv, lat_choice=dev_choice, dense_only=i["xt_fill"],
        dir_use=dir_use, direct_fill=direct_fill, fused=m > FUSED_MIN_REQ, enc16=enc16,
        clear_slots=keyed and i["slots_dirty"], clear_dir=keyed and dir_use and i["dir_dirty"],
        mark_dir_dirty=keyed and not i["xt_fill"], run_probe=keyed and (kc_active or dir_use),
        run_xtab_publish=keyed and i["xt_fill"], run_dir_publish=keyed and dir_use and dir_pub,
        run_affine=keyed and dir_use and aff_conv, run_widen=keyed and dir_use and wide_conv,
        run_dev_latency=keyed and dev_choice)
    words = dict(
        lookup=lookup, min_req=min_req, kc_wcap=0 if xt_only else KC_WCAP, dir_cap=DIR_CAP, wide_cap=kw_wide_cap,
        chunk_n=m, seg_cap=seg_cap, kcap=kcap, seed_reqs=seed, req_grid=grid, ins_grid=(m + INS_REQS - 1) // INS_REQS,
        probe_grid=(NSEG * seg_cap + BLOCK - 1) // BLOCK, chain_blocks=min(limit, LP_CHAIN_BLOCKS),
        fill_grid=min((items + BLOCK - 1) // BLOCK, 4096),
        side_grid=min(grid, max(1, SIDE_GRID_PER_CU * max(1, cus))),
        enc_grid=(m + BLOCK * eb - 1) // (BLOCK * eb), pub_grid=(limit + BLOCK - 1) // BLOCK)
    ob = 0
    for k, name in enumerate(OUT_BITS):
        ob |= int(bool(bits[name])) << k
    return [ob] + [words[w] for w in OUT_WORDS]


def inputs_of(row):
    i = {name: (row[0] >> k) & 1 for k, name in enumerate(IN_BITS)}
    i["path"] = row[0] >> 16
    return i


def describe(row, want):
    out = {name: (row[6] >> k) & 1 for k, name in enumerate(OUT_BITS)}
    out.update(zip(OUT_WORDS, row[7:]))
    exp = {name: (want[0] >> k) & 1 for k, name in enumerate(OUT_BITS)}
    exp.update(zip(OUT_WORDS, want[1:]))
    return "inputs %s wide_cap %d pool %d cus %d m %d n %d: %s" % (
        inputs_of(row), row[1], row[2], row[3], row[4], row[5],
        {k: (out[k], exp[k]) for k in out if out[k] != exp[k]})


def first_difference(rows, **wrong):
    for row in rows:
        want = model(inputs_of(row), *row[1:6], **wrong)
        if row[6:] != want:
            return describe(row, want)
    return None


MS = [1, 63, 64, 65, 2048, 2049, 4096, 4097, 65536, 65537, 262144, 262145, M]


def test_every_combination_matches_the_former_conditions(report):
    """359,424 combinations: path x hint_set x keyed_hint x cache active x (xt_fill, xt_use) in {(0,0), (1,0), (0,1)}
    x dir_on x aff_on x configured wide capacity {0, 1, 2048} x pool size {0, 1, 2048, 4096} tables x CUs {0, 1, 256}
    x the 13 chunk sizes on either side of every threshold x (a one-chunk call, n = m; the tail chunk of a two-chunk
    call, n = 2^20 + m), the dirty flags cycling through their four pairs. Every output of the batch plan and the
    chunk plan, and the zero-copy gate's answer, equal the model's."""
    rows = report["rows"]
    assert len(rows) == report["sweep_rows"] == 4 * 2 * 2 * 2 * 3 * 2 * 2 * 3 * 4 * 3 * 13 * 2 == 359424
    seen = set()
    for row in rows:
        i = inputs_of(row)
        assert (i["xt_fill"], i["xt_use"]) != (1, 1) and row[5] in (row[4], M + row[4])
        seen.add((row[0] & ~0x180, row[1], row[2], row[3], row[4], row[5]))  # all but the dirty flags
    assert len(seen) == len(rows)  # no combination twice, so each of the product's once
    assert {row[4] for row in rows} == set(MS) and {row[0] >> 16 for row in rows} == {AUTO, STRAUS, COMB, LATENCY}
    assert {(row[1], row[2], row[3]) for row in rows} == {(w, p, c) for w in (0, 1, 2048) for p in (0, 1, 2048, 4096)
                                                          for c in (0, 1, 256)}
    # the dirty flags meet keyed and unkeyed chunks, inside and outside the directory, in all four pairs
    keyed_bit, dir_use_bit = OUT_BITS.index("keyed"), OUT_BITS.index("dir_use")
    assert len({((row[6] >> keyed_bit) & 1, (row[6] >> dir_use_bit) & 1, (row[0] >> 7) & 3) for row in rows}) == 16
    assert all(row[6] >> 31 == 0 for row in rows)  # the 0/1 scalars are 0 or 1
    assert first_difference(rows) is None


def test_zero_copy_gate_is_the_batch_plan(report):
    """pv_verify_batch's zero-copy gate asks plan_batch with hint_set and the hint it has just counted. Over the same
    combinations the answer is the expression the gate used to spell out (PV_PATH_LATENCY, or AUTO with
    n <= PV_LATENCY_MAX and no hint), whatever the cache's state: with hint_set there is no device choice."""
    gate_bit = OUT_BITS.index("gate")
    for row in report["rows"]:
        i, n = inputs_of(row), row[5]
        old = i["path"] == LATENCY or (i["path"] == AUTO and n <= LATENCY_MAX and not i["keyed_hint"])
        assert (row[6] >> gate_bit) & 1 == int(old), (i, n)


@pytest.mark.parametrize("wrong", ["sparse_ge", "dir_during_fill"])
def test_the_comparison_notices_a_wrong_model(report, wrong):
    """The checker bites: a model with >= for > at PV_SPARSE_CHUNK, and one that consults the directory during
    xt_fill, each differ from the header."""
    assert first_difference(report["rows"], **{wrong: True}) is not None
