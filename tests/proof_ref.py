"""Shared helpers of the state-proof tests: which tries, keys and prefixes the golden file
(tests/golden/state_proof.json, recorded from the reference by tests/golden/make_state_proof_golden.py) covers,
and the corruption classes, built the same way by the generator (which asks the reference) and by the tests
(which ask the package). Everything here works on RLP bytes, so it needs neither side's decoder: a proof is the
list of its nodes' encodings, sorted, plus the root node's, and what is verified is always the serialized form."""
import hashlib
import json
import os

import trie_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
TRIES = ("blank", "single", "empty_key", "prefix_short_first", "anchor_small", "full_branch_embedded",
         "full_branch_hashed", "value_70000", "ascii_300")


def sha3(b):
    return hashlib.sha3_256(b).digest()


def proofcheck_lib():
    """tests/native/proofcheck.hip compiled for the host (built when missing or older than its sources)."""
    import ctypes
    import subprocess
    csrc = os.path.join(os.path.dirname(HERE), "indy-plenum_amd", "csrc")
    lib = os.path.join(HERE, "native", "libproofcheck.so")
    srcs = [os.path.join(csrc, f) for f in ("keccak.h", "sha512.h", "fe25519.h", "trie_core.h")]
    srcs.append(os.path.join(HERE, "native", "proofcheck.hip"))
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(f) for f in srcs):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-fPIC", "-shared", "--offload-arch=gfx950",
                               "--offload-host-only", "-I" + csrc, srcs[-1], "-o", lib])
    return ctypes.CDLL(lib)


def _prefix(n, base):
    if n < 56:
        return bytes([base + n])
    be = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([base + 55 + len(be)]) + be


def rlp_str(b):
    return b if len(b) == 1 and b[0] < 0x80 else _prefix(len(b), 0x80) + b


def rlp_list(raw_items):
    """The list whose items are already encoded."""
    body = b"".join(raw_items)
    return _prefix(len(body), 0xC0) + body


def split_list(enc):
    """The encoded items of a canonical list."""
    def head(pos):
        b0 = enc[pos]
        if b0 < 0x80:
            return pos, pos + 1
        v = b0 - (0xC0 if b0 >= 0xC0 else 0x80)
        if v < 56:
            return pos + 1, pos + 1 + v
        start = pos + 1 + v - 55
        return start, start + int.from_bytes(enc[pos + 1:start], "big")
    pos, end = head(0)
    assert enc[0] >= 0xC0 and end == len(enc)
    out = []
    while pos < end:
        _, e = head(pos)
        out.append(enc[pos:e])
        pos = e
    return out


def serialized(node_rlps):
    return rlp_list(node_rlps)


def trie_sets(name):
    return next(c for c in R.load_golden() if c["name"] == name)["sets"]


def final_map(sets):
    out = {}
    for k, v in sets:
        out[k] = v
    return out


def query_keys(sets):
    """(present keys, absent keys): a handful of each, the same for the generator and the tests."""
    keys = sorted(final_map(sets))
    present = keys if len(keys) <= 6 else keys[::max(1, len(keys) // 5)][:6]
    absent = [b"zz-absent"]
    if keys:
        k = keys[len(keys) // 2]
        absent.append(k[:-1] + bytes([k[-1] ^ 0x01]) if k else b"\x01")
        absent.append(k + b"\x00")
        if len(k) > 1:
            absent.append(k[:-1])
    have = set(keys)
    return present, [a for a in dict.fromkeys(absent) if a not in have]


def prefixes(sets):
    """The empty prefix, prefixes that end inside a leaf's or an extension's path, a whole key, and one no key has."""
    keys = sorted(final_map(sets))
    out = [b""]
    for k in keys[:1] + keys[-1:]:
        out += [k[:1], k[:len(k) // 2], k[:max(len(k) - 1, 0)], k, k + b"x"]
    return list(dict.fromkeys(out))


def sibling_sets(sets):
    """The same keys with one value changed: a trie whose nodes look alike and hash differently."""
    if not sets:
        return [(b"other", b"trie")]
    return list(sets[:-1]) + [(sets[-1][0], sets[-1][1] + b"'")]


def noncanonical(node_rlp):
    """The node with its first short string (prefix 0x81 .. 0xb7) written in long form (0xb8, length), or None."""
    if node_rlp[0] < 0xC0:
        return None
    items = split_list(node_rlp)
    for i, it in enumerate(items):
        if 0x81 <= it[0] <= 0xB7:
            items[i] = b"\xb8" + bytes([it[0] - 0x80]) + it[1:]
            return rlp_list(items)
    return None


def build_state(make_state, sets):
    st = make_state()
    for k, v in sets:
        st.set(k, v)
    return st


def proof_of(st, rlp_encode, key, prefix=False):
    """(sorted RLPs of the nodes below the root, the root node's RLP, serialized length, value or value map)
    of the state's own proof for a key or a prefix."""
    gen = st.generate_state_proof_for_keys_with_prefix if prefix else st.generate_state_proof
    nodes, value = gen(key, get_value=True)
    return sorted(rlp_encode(n) for n in nodes[:-1]), rlp_encode(nodes[-1]), len(gen(key, serialize=True)), value


def base_of(st, sibling, rlp_encode, sets):
    """What corruptions() needs, from a state and its sibling (sibling_sets)."""
    present, absent = query_keys(sets)
    key = present[0] if present else b"abc"
    nodes, rn, _, raw = proof_of(st, rlp_encode, key)
    a_nodes = proof_of(st, rlp_encode, absent[0])[0]
    s_nodes, s_rn = proof_of(sibling, rlp_encode, key)[:2]
    return {"root": st.headHash, "key": key, "value": final_map(sets).get(key), "nodes": nodes, "root_node": rn,
            "absent_key": absent[0], "absent_nodes": a_nodes, "sibling_nodes": s_nodes, "sibling_root_node": s_rn}


CANONICAL_CLASSES = ("honest", "wrong_value", "value_for_absent_key", "none_for_present_key", "absent_expected_absent",
                     "path_node_dropped", "root_node_dropped", "sibling_substituted", "wrong_root", "key_nibble_off",
                     "duplicated_nodes", "extra_unrelated_nodes", "nodes_reordered")
DEFER_CLASSES = ("noncanonical_node", "node_of_3_items", "child_of_5_bytes")


def corruptions(base):
    """class -> (root, key, value, serialized proof). base: root, key, value (None = absent), nodes (sorted RLPs
    below the root), root_node (RLP), absent_key, absent_nodes, sibling_nodes, sibling_root_node."""
    root, key, value = base["root"], base["key"], base["value"]
    nodes, rn = list(base["nodes"]), base["root_node"]
    full = nodes + [rn]
    out = {"honest": (root, key, value, serialized(full)),
           "wrong_value": (root, key, (value or b"") + b"x", serialized(full)),
           "value_for_absent_key": (root, base["absent_key"], b"v", serialized(base["absent_nodes"] + [rn])),
           "absent_expected_absent": (root, base["absent_key"], None, serialized(base["absent_nodes"] + [rn])),
           "none_for_present_key": (root, key, None, serialized(full)),
           "root_node_dropped": (root, key, value, serialized(nodes)),
           "wrong_root": (sha3(b"wrong root"), key, value, serialized(full)),
           "root_of_0_bytes": (b"", key, value, serialized(full)),
           "root_of_31_bytes": (root[:31], key, value, serialized(full)),
           "root_of_33_bytes": (root + b"\x00", key, value, serialized(full)),
           "key_nibble_off": (root, key[:-1] + bytes([key[-1] ^ 0x01]) if key else b"\x01", value, serialized(full)),
           "duplicated_nodes": (root, key, value, serialized(full + full)),
           "extra_unrelated_nodes": (root, key, value, serialized(
               base["sibling_nodes"] + [base["sibling_root_node"], rlp_list([b"\x20", b"a", b"b"])] + full)),
           "nodes_reordered": (root, key, value, serialized(full[::-1])),
           "serialized_truncated": (root, key, value, serialized(full)[:-1]),
           "serialized_c1": (root, key, value, b"\xc1"),
           "serialized_empty": (root, key, value, b"")}
    if nodes:
        out["path_node_dropped"] = (root, key, value, serialized(nodes[1:] + [rn]))
        out["sibling_substituted"] = (root, key, value, serialized([base["sibling_root_node"]] + nodes[1:] + [rn]))
    else:
        out["sibling_substituted"] = (root, key, value, serialized([base["sibling_root_node"]]))
    flip = bytearray(full[0])
    flip[len(flip) // 2] ^= 0x01
    out["node_byte_flipped"] = (root, key, value, serialized([bytes(flip)] + full[1:]))
    bad = noncanonical(rn)
    if bad is not None:  # the reference re-encodes what it decodes, so the root still matches
        out["noncanonical_node"] = (root, key, value, serialized(nodes + [bad]))
    three = rlp_list([b"\x20", b"a", b"b"])
    out["node_of_3_items"] = (sha3(three), key, value, serialized(nodes + [three]))
    if key:
        branch = [b"\x80"] * 17
        branch[key[0] >> 4] = rlp_str(b"short")
        five = rlp_list(branch)
        out["child_of_5_bytes"] = (sha3(five), key, value, serialized(nodes + [five]))
    return out


def multi_cases(root, values, all_nodes, root_node):
    """case -> (root, {key: value}, serialized proof): values is the whole mapping, all_nodes the empty-prefix proof."""
    ser = serialized(list(all_nodes) + [root_node])
    keys = sorted(values)
    right = {k: values[k] for k in keys[:40]}
    wrong = dict(right)
    wrong[keys[0]] = values[keys[0]] + b"!"
    absent = dict(right)
    absent[b"zz-absent"] = None
    absent_wrong = dict(right)
    absent_wrong[b"zz-absent"] = b"there"
    return {"all_right": (root, right, ser), "one_wrong": (root, wrong, ser), "one_absent_expected_absent": (root, absent, ser),
            "one_absent_expected_present": (root, absent_wrong, ser)}


def build_tries(S):
    """name -> (state, sets, corruptions of the first key's proof, multi cases) over the package's classes."""
    make = lambda: S.PruningState(S.KeyValueStorageInMemory())  # noqa: E731
    out = {}
    for name in TRIES:
        sets = trie_sets(name)
        st, sib = build_state(make, sets), build_state(make, sibling_sets(sets))
        multi = {}
        if sets:
            nodes, rn = proof_of(st, S.rlp_encode, b"", prefix=True)[:2]
            multi = multi_cases(st.headHash, final_map(sets), nodes, rn)
        out[name] = (st, sets, corruptions(base_of(st, sib, S.rlp_encode, sets)), multi)
    return out


def all_corruptions(tries, skip=()):
    return [(name, c, a) for name in TRIES for c, a in tries[name][2].items() if c not in skip]


def stored(S, value):
    """The value as the trie stores it; None (absent) as the empty string."""
    return S.rlp_encode([value]) if value is not None else b""


def native_statuses(N, S, cases):
    """The library's statuses for [(root, key, value, serialized proof)], every proof split by the library; a
    proof the split refuses counts as deferred, which is what the Python layer does with it."""
    import numpy as np
    blob, first, off, lens, ok = N.trie_proof_split([a[3] for a in cases])
    status = N.trie_verify_proofs(blob, off, lens, np.arange(len(lens)), first, np.arange(len(cases)), [a[0] for a in cases],
                                  [a[1] for a in cases], [stored(S, a[2]) for a in cases])
    status[ok == 0] = N.PV_PROOF_DEFER
    return status


ROOT_LENGTH_CLASSES = ("root_of_0_bytes", "root_of_31_bytes", "root_of_33_bytes")  # settled in Python
UNSPLITTABLE = ("serialized_truncated", "serialized_c1", "serialized_empty")      # refused by the split


def outcome(f):
    """'true', 'false' or the exception's class name."""
    try:
        return "true" if f() else "false"
    except Exception as e:  # noqa: BLE001 - the class is the recorded result
        return type(e).__name__


def forms(rlps):
    return [R.form(x) for x in rlps]


def value_forms(values):
    m = {k.hex(): R.form(v) for k, v in values.items()}
    return m if len(m) <= 100 else R.digest(m)


def load_proof_golden():
    with open(os.path.join(HERE, "golden", "state_proof.json")) as f:
        return {t["name"]: t for t in json.load(f)["tries"]}
