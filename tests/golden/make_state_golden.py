"""Generate tests/golden/state.json by running the REFERENCE's own PruningState over its in-memory store.

TEST INFRASTRUCTURE, run only where the reference is checked out (the tests read the JSON alone):
    python tests/golden/make_state_golden.py
The reference (swcurran/indy-plenum, checked out beside this repository) is imported, never copied; its
`rlp` dependency is the stand-in of tests/golden/_shims/rlp. Output (JSON, data only, one case per line), per
case: the ordered sets [key hex, value], headHash after each set, the final store and as_dict. To keep the
file small (the forms are tests/trie_ref.py's, which the tests apply to their own results):
  - a value or store entry longer than 64 bytes is written "#<length>:<sha256 hex>"; a set value
    "@<length>:<tag>" stands for det(tag, length); the two long cases name their RULES entry instead of sets;
  - a store above 1 KB of hex, and an as_dict of more than 100 keys, are recorded as
    {"count": n, "digest": sha256 over the sorted key || 0x00 || value-form lines}; more than 16 heads as
    their count and the SHA-256 of their lines.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = os.environ.get("PLENUM_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
sys.path[:0] = [REF, os.path.join(HERE, "_shims"), os.path.dirname(HERE)]

from state.pruning_state import PruningState  # noqa: E402
from storage.kv_in_memory import KeyValueStorageInMemory  # noqa: E402
from trie_ref import RULES, det, detv, digest, form, heads_recorded  # noqa: E402

def cases():
    v = lambda i, n=6: detv("v%d" % i, n)  # noqa: E731
    out = [("blank", []),
           ("single", [(b"abc", b"value1")]),
           ("empty_key_alone", [(b"", b"v-empty")]),
           ("empty_key", [(b"", b"v-empty"), (b"a", b"1"), (b"", b"v2"), (b"\x00", b"z")]),
           ("diverge_first", [(bytes.fromhex("123456"), v(1)), (bytes.fromhex("923456"), v(2))]),
           ("diverge_middle", [(bytes.fromhex("123456"), v(1)), (bytes.fromhex("123956"), v(2))]),
           ("diverge_last", [(bytes.fromhex("123456"), v(1)), (bytes.fromhex("123457"), v(2))]),
           ("prefix_short_first", [(b"ab", v(1)), (b"abcd", v(2, 40)), (b"abc", v(3))]),
           ("prefix_long_first", [(b"abcd", v(2, 40)), (b"ab", v(1)), (b"abc", v(3))]),
           ("leaf_split", [(b"abcdef", v(1, 30)), (b"abcxyz", v(2, 30)), (b"abcdeg", v(3, 3))]),
           ("anchor_small", [(b"a", b"1"), (b"ab", b"2"), (b"abc", b"3"), (b"b", b"x" * 40)])]
    base = [(b"aaaa1", v(1, 33)), (b"aaaa2", v(2, 33))]
    out += [("ext_split_start", base + [(b"\x10aaa", v(3))]),
            ("ext_split_middle", base + [(b"aa\x00", v(3))]),
            ("ext_split_end", base + [(b"aaaa\x40", v(3))]),
            ("ext_split_one_left", base + [(b"aaa\x61", v(3)), (b"aaaq", v(4, 35))]),
            ("ext_key_ends_inside", base + [(b"aa", v(3)), (b"aaa", v(4, 50))]),
            ("overwrite_same", base + [(b"aaaa1", v(1, 33))]),
            ("overwrite_other", base + [(b"aaaa1", v(9, 34)), (b"aaaa2", b"")]),
            ("same_key_twice", [(b"k1", v(1)), (b"k2", v(2, 40)), (b"k1", v(3, 41)), (b"k1", v(4, 2))])]
    lens = (0, 1, 28, 29, 30, 31, 32)
    for kl in (1, 2, 32):
        sets = [(bytes([17 * i + 3]) + det("key%d" % i, kl - 1), v(i, n)) for i, n in enumerate(lens)]
        sets += [(bytes([17 * (i + 7)]) + det("key%d" % i, kl - 1), bytes([b])) for i, b in enumerate((0, 0x7F, 0x80, 0xFF))]
        out.append(("value_lengths_key%d" % kl, sets))
        # the same first nibble twice: leaves one level down, shorter paths
        out.append(("value_lengths_deep_key%d" % kl,
                    [(bytes([0x30 + i]) + det("key%d" % i, kl - 1), v(i, n)) for i, n in enumerate(lens)]))
    out.append(("leaf_lengths_56", [(bytes([17 * i]), v(i, 40 + i)) for i in range(16)]))
    out.append(("leaf_lengths_256", [(bytes([17 * i]), v(i, 236 + i)) for i in range(16)]))
    out.append(("leaf_length_sweep", [(b"k", v(n, n)) for n in list(range(44, 60)) + list(range(240, 256))]))
    out.append(("branch_lengths", [(bytes([16 * i + j]), v(16 * i + j, 1 + (i + j) % 3)) for i in range(16) for j in range(3)]))
    out.append(("value_70000", [(b"big", "@70000:big"), (b"bit", v(1)), (b"small", v(2, 3))]))
    out.append(("full_branch_embedded", [(bytes([17 * i]), bytes([i + 1])) for i in range(16)]))
    out.append(("full_branch_hashed", [(bytes([17 * i]) + b"tail", v(i, 48)) for i in range(16)] + [(b"", v(99, 5))]))
    out += [(name, name) for name in sorted(RULES)]  # the sets come from tests/trie_ref.py RULES
    return out


def main():
    lines = []
    for name, sets in cases():
        kv = KeyValueStorageInMemory()
        st = PruningState(kv)
        heads, rec, rule = [], [], None
        if isinstance(sets, str):
            rule, sets = sets, RULES[sets]()
        for k, val in sets:
            if isinstance(val, str):
                n, tag = val[1:].split(":")
                rec.append([k.hex(), val])
                val = det(tag, int(n))
            else:
                rec.append([k.hex(), val.spec if getattr(val, "spec", None) and len(val) > 16 else val.hex()])
            st.set(k, bytes(val))
            heads.append(st.headHash.hex())
        store = {bytes(k).hex(): form(x) for k, x in kv._dict.items()}
        asd = {bytes(k).hex(): form(x) for k, x in st.as_dict.items()}
        case = {"name": name, "heads": heads_recorded(heads, heads if len(heads) <= 16 else {}), "final": st.headHash.hex(),
                "store": store if sum(len(x) for x in store.values()) <= 1024 else digest(store),
                "as_dict": asd if len(asd) <= 100 else digest(asd)}
        case.update({"rule": rule} if rule else {"sets": rec})
        lines.append(json.dumps(case, sort_keys=True))
    path = os.path.join(HERE, "state.json")
    with open(path, "w") as f:
        f.write('{"cases": [\n' + ",\n".join(lines) + "]}\n")
    print("wrote %s: %d cases, %d bytes" % (path, len(lines), os.path.getsize(path)))


if __name__ == "__main__":
    main()
