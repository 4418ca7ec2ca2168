"""Generate tests/golden/state_proof.json by running the REFERENCE's own PruningState: its proofs for keys and
prefixes, and what its verify_state_proof / verify_state_proof_multi answer for every corruption class.

TEST INFRASTRUCTURE, run only where the reference is checked out (the tests read the JSON alone):
    python tests/golden/make_state_proof_golden.py
The reference is imported as tests/golden/make_state_golden.py imports it, never copied. The tries are cases of
tests/golden/state.json; which keys, prefixes and corruptions are recorded is decided by tests/proof_ref.py, which
the tests use in the same way on the package's own classes. Output (JSON, data only), per trie:
  keys         per present and absent key: the proof as the sorted RLPs of its nodes below the root plus the
               root node's RLP (the reference returns the former in a set's order), the serialized length, the
               raw value returned (null: absent);
  prefixes     the same per prefix, with the map {key: raw value};
  corruptions  class -> "true", "false" or the exception's class name, for PruningState.verify_state_proof of
               the serialized proof that proof_ref.corruptions builds from the first key's proof;
  multi        case -> the same for verify_state_proof_multi.
Byte strings above 64 bytes are written "#<length>:<sha256 hex>" (tests/trie_ref.py form)."""
import contextlib
import io
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = os.environ.get("PLENUM_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
sys.path[:0] = [REF, os.path.join(HERE, "_shims"), os.path.dirname(HERE)]

from state.pruning_state import PruningState  # noqa: E402
from state.trie.pruning_trie import rlp_encode  # noqa: E402
from storage.kv_in_memory import KeyValueStorageInMemory  # noqa: E402
import proof_ref as P  # noqa: E402
from trie_ref import form  # noqa: E402


def quiet(f):
    """The reference prints the exceptions it catches."""
    with contextlib.redirect_stdout(io.StringIO()):
        return P.outcome(f)


def main():
    make = lambda: PruningState(KeyValueStorageInMemory())  # noqa: E731
    lines = []
    for name in P.TRIES:
        sets = P.trie_sets(name)
        st, sib = P.build_state(make, sets), P.build_state(make, P.sibling_sets(sets))
        present, absent = P.query_keys(sets)
        rec = {"name": name, "root": st.headHash.hex(), "keys": [], "prefixes": []}
        for key in present + absent:
            nodes, rn, ser_len, value = P.proof_of(st, rlp_encode, key)
            rec["keys"].append({"key": key.hex(), "nodes": P.forms(nodes), "root_node": form(rn), "ser_len": ser_len,
                                "value": form(value) if value is not None else None})
        for prefix in P.prefixes(sets):
            nodes, rn, ser_len, values = P.proof_of(st, rlp_encode, prefix, prefix=True)
            rec["prefixes"].append({"prefix": prefix.hex(), "nodes": P.forms(nodes), "root_node": form(rn),
                                    "ser_len": ser_len, "values": P.value_forms(values)})
        base = P.base_of(st, sib, rlp_encode, sets)
        rec["corruptions"] = {c: quiet(lambda a=a: PruningState.verify_state_proof(a[0], a[1], a[2], a[3], serialized=True))
                              for c, a in P.corruptions(base).items()}
        rec["multi"] = {}
        values = P.final_map(sets)
        if values:
            all_nodes, rn = P.proof_of(st, rlp_encode, b"", prefix=True)[:2]
            rec["multi"] = {c: quiet(lambda a=a: PruningState.verify_state_proof_multi(a[0], a[1], a[2], serialized=True))
                            for c, a in P.multi_cases(st.headHash, values, all_nodes, rn).items()}
        lines.append(json.dumps(rec, sort_keys=True))
    path = os.path.join(HERE, "state_proof.json")
    with open(path, "w") as f:
        f.write('{"tries": [\n' + ",\n".join(lines) + "]}\n")
    print("wrote %s: %d tries, %d bytes" % (path, len(lines), os.path.getsize(path)))


if __name__ == "__main__":
    main()
