"""Shared helpers of the state-trie tests: the golden file (tests/golden/state.json, recorded from the
reference by tests/golden/make_state_golden.py) and its value forms, hashlib as the SHA3-256 reference,
node builders for malformed-input cases, and the store properties a batch must keep."""
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHA3_LENGTHS = (0, 1, 31, 32, 134, 135, 136, 137, 271, 272, 273, 408, 600, 70003)
LONG = 64  # values and store entries above this many bytes are recorded as "#<length>:<sha256 hex>"


def det(tag, n):
    out = b"".join(hashlib.sha256(b"state golden %s %d" % (tag.encode(), k)).digest() for k in range(n // 32 + 1))
    return out[:n]


class Det(bytes):
    """det(tag, n) that remembers its rule: the golden file records it as "@<n>:<tag>"."""
    spec = None


def detv(tag, n):
    b = Det(det(tag, n))
    b.spec = "@%d:%s" % (n, tag)
    return b


# sets too long to write out: the golden file names the rule, the anchors below pin the result
RULES = {
    "ascii_300": lambda: [(b"did:sov:namespace/%04d/attr/%s" % (i % 75, (b"name", b"endpoint", b"role", b"verkey")[i // 75]),
                           b'{"seq":%d}' % i) for i in range(300)],
    "uniform_1000": lambda: [(hashlib.sha256(b"k%d" % i).digest(), (b'{"v":%d}' % i) * 5) for i in range(1000)],
}


def form(b):
    b = bytes(b)
    return b.hex() if len(b) <= LONG else "#%d:%s" % (len(b), hashlib.sha256(b).hexdigest())


def digest(mapping):
    h = hashlib.sha256()
    for k in sorted(mapping):
        h.update(k.encode() + b"\0" + mapping[k].encode() + b"\n")
    return {"count": len(mapping), "digest": h.hexdigest()}


def heads_recorded(heads, like):
    """The hex head hashes after every set, in the form the golden file recorded them in: the list, or for
    more than 16 sets its length and the SHA-256 of its lines (one differing step changes it)."""
    if isinstance(like, list):
        return heads
    return {"count": len(heads), "digest": hashlib.sha256("\n".join(heads).encode()).hexdigest()}


def recorded(mapping, like):
    """{bytes: bytes} in the form the golden file recorded `like` in (a dict of forms, or its digest)."""
    forms = {bytes(k).hex(): form(v) for k, v in mapping.items()}
    return digest(forms) if set(like) == {"count", "digest"} else forms


def load_golden():
    with open(os.path.join(HERE, "golden", "state.json")) as f:
        cases = json.load(f)["cases"]
    for c in cases:
        sets = RULES[c["rule"]]() if "rule" in c else []
        for k, v in c.get("sets", ()):
            if v.startswith("@"):
                n, tag = v[1:].split(":")
                v = det(tag, int(n))
            else:
                v = bytes.fromhex(v)
            sets.append((bytes.fromhex(k), v))
        c["sets"] = sets
    return cases


def sha3(b):
    return hashlib.sha3_256(b).digest()


def pack(items, lead=0):
    """Records behind `lead` bytes of filler -> (uint8 blob, uint64 offsets)."""
    off = np.zeros(len(items) + 1, np.uint64)
    np.cumsum([len(x) for x in items], out=off[1:])
    off += np.uint64(lead)
    return np.frombuffer(b"\xa5" * lead + b"".join(items) + b"\x5a" * 3, np.uint8), off


def split(sets, parts):
    n = len(sets)
    return [sets[n * p // parts:n * (p + 1) // parts] for p in range(parts)]


def reachable(trie_mod, kv, root_hash):
    """Every hash reachable from root_hash; raises KeyError when a node is not in the store."""
    seen = set()
    if root_hash == trie_mod.BLANK_ROOT:
        return seen

    def walk(ref):
        if ref == b"":
            return
        if isinstance(ref, list):
            node = ref
        else:
            seen.add(ref)
            enc = kv.get(ref)
            assert trie_mod.sha3(enc) == ref
            node = trie_mod.rlp_decode(enc)
        if len(node) == 17:
            for c in node[:16]:
                walk(c)
        elif not trie_mod.hp_unpack(node[0])[1]:
            walk(node[1])
    walk(root_hash)
    return seen


def malformed_nodes(S):
    """name -> bytes no encoder of trie nodes writes; each must be rejected, none read past."""
    enc = S.rlp_encode
    h = bytes(range(32))
    leaf = enc([S.hp_pack([1, 2, 3], True), b"value"])
    out = {
        "empty": b"",
        "a_string": enc(b"just a string, no list at all"),
        "truncated_list_length": b"\xf8",
        "truncated_list_length_2": b"\xf9\x01",
        "list_length_past_buffer": b"\xc5\x80\x80",
        "long_list_length_past_buffer": b"\xf8\x50" + b"\x80" * 17,
        "item_length_past_list": b"\xc3\x20\x85ab"[:4],
        "item_truncated_length": b"\xc2\x20\xb8",
        "item_long_length_past_list": b"\xc4\x20\xb9\x01\x00",
        "trailing_bytes": leaf + b"\x00",
        "short_by_one": leaf[:-1],
        "list_of_0": enc([]),
        "list_of_1": enc([b"\x20"]),
        "list_of_3": enc([b"\x20", b"a", b"b"]),
        "list_of_16": enc([b""] * 16),
        "list_of_18": enc([b""] * 18),
        "branch_child_31_bytes": enc([h[:31]] + [b""] * 16),
        "branch_child_33_bytes": enc([h + b"x"] + [b""] * 16),
        "branch_value_is_list": enc([b""] * 16 + [[b"x"]]),
        "extension_child_short": enc([S.hp_pack([1, 2], False), b"short"]),
        "extension_child_blank": enc([S.hp_pack([1, 2], False), b""]),
        "extension_without_path": enc([S.hp_pack([], False), h]),
        "path_is_list": enc([[b"\x20"], b"v"]),
        "path_empty": enc([b"", b"v"]),
        "path_flags_4": enc([b"\x41", b"v"]),
        "path_padding_set": enc([b"\x25", b"v"]),
        "leaf_value_empty": enc([b"\x20", b""]),
        "leaf_value_is_list": enc([b"\x20", [b"v"]]),
        "non_minimal_long_form": b"\xc4\x20\xb8\x01\x90",
        "single_byte_with_prefix": b"\xc3\x20\x81\x05",
        "length_with_leading_zero": b"\xf9\x00\x40" + b"\x80" * 64,
        "nested_embedded_truncated": enc([S.hp_pack([1, 2], False), b""])[:-1] + b"\xc5\x20",
    }
    return out
