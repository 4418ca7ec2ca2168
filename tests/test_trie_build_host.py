"""The device trie builder's passes without a GPU (indy-plenum_amd/csrc/trie_build.h: the per-item functions the
kernels of kern_trie_build.h run one lane each), compiled with g++ as the library includes the header, under
AddressSanitizer and UBSan, and run in plain loops by a stand-alone program (tests/native/trie_build_check.cpp),
one loop per kernel pass. The root it builds is compared against (a) the roots recorded from the reference
(tests/golden/state.json) for every case whose keys have one length of 1 .. 64 bytes, and (b) the host
structural path, pv_trie_host_build + pv_trie_host_hash from the blank root, on seeded random sets and on the
shapes that embed nodes; the sizing bound (no node below 32 bytes holds more than six leaves) is asserted on all
of them. What the kernels make of the same source is checked by tests/test_gpu_trie_build.py. CPU only."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import trie_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "trie_build_check.cpp")
CSRC = os.path.join(HERE, "..", "indy-plenum_amd", "csrc")
BIN = os.path.join(HERE, "native", "trie_build_check")

VALUE_LENGTHS = (1, 2, 30, 31, 32, 33, 54, 55, 56, 150, 255, 256)


def uniform_golden():
    """The golden cases the builder takes: all keys of one length between 1 and 64."""
    out = []
    for c in R.load_golden():
        lens = {len(k) for k, _ in c["sets"]}
        if len(lens) == 1 and 1 <= next(iter(lens)) <= 64:
            out.append(c)
    return out


GOLDEN = uniform_golden()


def random_case(rng, n, key_len, wrap, lengths=VALUE_LENGTHS, dup=0.1):
    keys = [rng.bytes(key_len) for _ in range(n)]
    for i in range(1, n):
        if rng.random() < dup:
            keys[i] = keys[int(rng.integers(0, i))]  # an overwrite: the later entry wins
    choice = list(lengths) + ([0] if wrap else [])
    vals = [rng.bytes(int(rng.choice(choice))) for _ in range(n)]
    vals = [bytes([v[0] & 0x7F]) if len(v) == 1 and i % 2 else v for i, v in enumerate(vals)]  # single bytes below 0x80 too
    return keys, vals, wrap


def shaped_cases():
    """name -> (keys, values, wrap): the embedded shapes of the sizing argument and the structure edges."""
    rng = np.random.default_rng(7)
    out = {}
    # one branch embedded in an extension: keys 10 00, 10 01 with empty values beside 20 00 with 40 bytes
    out["ext_embeds_branch"] = ([b"\x10\x00", b"\x10\x01", b"\x20\x00"], [b"", b"", b"v" * 40], 1)
    # 16 embedded branches: the one-byte keys {a + 0, a + 1 : a = 00, 10, .., f0} with empty values
    out["sixteen_embedded_branches"] = ([bytes([a | b]) for a in range(0, 256, 16) for b in (0, 1)], [b""] * 32, 1)
    # three-byte leaves (an empty path and a value that is its own encoding): six make a branch of 30 bytes, seven of 32
    out["six_embedded_leaves"] = ([bytes([7, b]) for b in range(6)] + [b"\x90\x00"], [b"\x05"] * 6 + [b"w" * 50], 0)
    out["seven_leaves_not_embedded"] = ([bytes([7, b]) for b in range(7)] + [b"\x90\x00"], [b"\x05"] * 7 + [b"w" * 50], 0)
    out["all_one_byte_keys"] = ([bytes([b]) for b in range(256)] + [bytes([int(b)]) for b in rng.integers(0, 256, 100)],
                                [rng.bytes(3) for _ in range(356)], 0)
    dense = sorted(set(int(x) for x in rng.integers(0, 65536, 6000)))[:5000]
    out["dense_two_byte_keys"] = ([struct.pack(">H", x) for x in dense], [bytes([x & 0x7F]) for x in dense], 0)
    out["last_nibble"] = ([b"\xab" * 7 + bytes([0xC0 | x]) for x in range(16)], [b"x" * 33] * 16, 1)
    out["first_nibble"] = ([bytes([(x << 4) | 5]) + b"\xcd" * 7 for x in range(16)], [b"x" * 33] * 16, 1)
    out["long_extension"] = ([b"\x55" * 63 + bytes([x]) for x in (1, 2, 0x31, 0xF0)], [b"y" * 40] * 4, 1)
    comb, cur = [], bytearray(rng.bytes(64))
    for i in range(64):  # key i shares exactly i bytes with key i + 1
        comb.append(bytes(cur))
        cur[i] ^= 0x80
    out["comb"] = (comb, [rng.bytes(150) for _ in range(64)], 1)
    srt = sorted(rng.bytes(8) for _ in range(300))
    out["sorted"] = (srt, [rng.bytes(40) for _ in range(300)], 1)
    out["reverse_sorted"] = (srt[::-1], [rng.bytes(40) for _ in range(300)], 1)
    out["one_key_1000_times"] = ([b"samekey!"] * 1000, [b"%d" % i for i in range(1000)], 1)
    out["single_short_value"] = ([b"\x01"], [b"\x05"], 0)
    out["long_value"] = ([rng.bytes(9) for _ in range(5)], [rng.bytes(70000)] + [b"z"] * 4, 1)
    return out


def job_bytes(jobs):
    parts = [struct.pack("<I", len(jobs))]
    for keys, vals, wrap in jobs:
        kl = len(keys[0])
        assert all(len(k) == kl for k in keys) and len(keys) == len(vals)
        off = np.zeros(len(vals) + 1, np.uint64)
        np.cumsum([len(v) for v in vals], out=off[1:])
        blob = b"".join(vals)
        parts += [struct.pack("<IIIQ", kl, len(keys), wrap, len(blob)), b"".join(keys), off.tobytes(), blob]
    return b"".join(parts)


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    deps = [SRC, os.path.join(HERE, "..", "include", "plenum_verify.h")] + [
        os.path.join(CSRC, h) for h in ("trie_build.h", "trie_core.h", "trie_host.h", "trie_host.cpp", "keccak.h")]
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-pthread",
                               "-o", BIN, SRC, os.path.join(CSRC, "trie_host.cpp")])
    rng = np.random.default_rng(2027)
    groups = {"golden": [([k for k, _ in c["sets"]], [v for _, v in c["sets"]], 1) for c in GOLDEN],
              "random": [random_case(rng, n, kl, wrap) for n in (1, 2, 3, 63, 64, 65, 257, 1500)
                         for kl in (1, 2, 3, 8, 9, 32, 64) for wrap in (0, 1)],
              "shaped": list(shaped_cases().values()),
              "bad": [([b"ab"], [b""], 0)]}  # an empty value without the wrapping: the error word
    path = str(tmp_path_factory.mktemp("trie_build") / "jobs.bin")
    with open(path, "wb") as f:
        f.write(job_bytes([j for g in groups.values() for j in g]))
    out = subprocess.run([BIN, path], check=True, capture_output=True, text=True, timeout=300).stdout
    results = iter(json.loads(out))
    rep = {name: [(j, next(results)) for j in g] for name, g in groups.items()}
    assert next(results, None) is None
    return rep


def test_the_golden_roots_recorded_from_the_reference(report):
    assert len(GOLDEN) >= 20
    names = {c["name"] for c in GOLDEN}
    assert {"leaf_lengths_56", "leaf_lengths_256", "leaf_length_sweep", "branch_lengths", "full_branch_embedded",
            "same_key_twice", "uniform_1000"} <= names, sorted(names)
    for c, (_, got) in zip(GOLDEN, report["golden"]):
        assert got["err"] == 0 and got["root"] == c["final"], c["name"]
        assert got["n_keys"] == len({k for k, _ in c["sets"]}), c["name"]


def check_against_host(rows):
    for (keys, vals, wrap), got in rows:
        what = (len(keys), len(keys[0]), wrap)
        assert got["err"] == 0 and got["host_ok"] == 1, what
        assert got["root"] == got["host_root"], what
        assert (got["n_records"], got["arena_bytes"]) == (got["host_records"], got["host_arena_bytes"]), what
        assert got["n_keys"] == len(set(keys)) and got["n_nodes"] >= got["n_records"], what
        assert got["small_leaves"] <= 6, what


def test_random_sets_against_the_host_structural_path(report):
    rows = report["random"]
    assert len(rows) == 8 * 7 * 2
    check_against_host(rows)
    assert any(got["n_keys"] < len(keys) for (keys, _, _), got in rows)  # overwrites happened


def test_embedded_shapes_and_structure_edges(report):
    rows = report["shaped"]
    check_against_host(rows)
    by = {name: got for name, (_, got) in zip(shaped_cases(), rows)}
    assert by["ext_embeds_branch"]["n_nodes"] == 6 and by["ext_embeds_branch"]["n_records"] == 2
    assert by["sixteen_embedded_branches"]["n_nodes"] == 49 and by["sixteen_embedded_branches"]["n_records"] == 1
    assert by["six_embedded_leaves"]["small_leaves"] == 6
    assert by["seven_leaves_not_embedded"]["small_leaves"] < 6
    assert by["dense_two_byte_keys"]["small_leaves"] >= 2
    assert by["comb"]["max_depth"] > 64 and by["comb"]["depths"] > 64
    assert by["one_key_1000_times"]["n_keys"] == 1 and by["one_key_1000_times"]["n_nodes"] == 1
    assert by["all_one_byte_keys"]["n_keys"] == 256 and by["all_one_byte_keys"]["n_nodes"] == 256 + 17
    assert by["long_extension"]["max_depth"] >= 2


def test_the_error_word(report):
    (_, got), = report["bad"]
    assert got["err"] == 1
