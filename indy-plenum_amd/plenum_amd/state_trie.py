"""The state's Patricia trie with batched updates.

The interface of the reference's state/trie/pruning_trie.py (Trie), state/pruning_state.py (PruningState)
and its in-memory key-value store, implemented independently: a node is a list of byte strings (leaf
[hp(path + terminator), value], extension [hp(path), child], branch of 16 children and a value), a child is
b'' (blank), the 32-byte SHA3-256 of the child's RLP, or the child itself when its RLP is shorter than 32
bytes; an update rebuilds the nodes on the key's path, leaf to root. The store is content-addressed
(hash -> RLP) and never pruned, as the reference's (state/db/persistent_db.py:26-30). Added: one library
call chain for a whole batch.

    Trie.update_batch(items)         n updates          (pruning_trie.py:1006-1027 Trie.update)
    PruningState.set_batch(items)    n sets             (pruning_state.py:60-61; update_state over a 3PC batch)
    PruningState.root_of(items)      the root of a mapping built from empty, nothing stored (state rebuild,
                                     catch-up check); root_of_arrays the same from numpy arrays

The batch calls go through libplenum_verify (pv_trie_update_batch): the structure in C++ on the host, the
SHA3-256 of every new node on the GPU or, for small batches and without one, on host threads. root_of with
keys of one length (1 to 64 bytes) goes through pv_trie_root, which on the device path builds the structure
with kernels as well; any other root_of goes where it went before.

State proofs (pruning_trie.py:1043-1170, pruning_state.py:104-128): generate_state_proof and its prefix form,
verify_state_proof and verify_state_proof_multi, and for many proofs at once

    Trie.verify_spv_proof_batch(items)             n x Trie.verify_spv_proof
    PruningState.verify_state_proof_batch(items)   n x PruningState.verify_state_proof
    PruningState.generate_state_proof_batch(keys)  n x generate_state_proof, one decoded-node cache

The batch verification goes through pv_trie_verify_proofs: one SHA3-256 per proof node and one walk per query,
on the GPU or on host threads. The library answers ACCEPT, REJECT or DEFER per query; a deferred query (a proof
record that is not canonical RLP, a malformed node on the path) goes through the sequential method here, which
decodes as leniently as the reference does. Generation hashes nothing (the nodes come out of a content-addressed
store) and stays in Python.

Node order of a generated proof: the hashed nodes below the root in the order the walk loaded them, each once,
then the root last. (The reference returns the nodes below the root in a set's order; the root is last there too.)
An embedded node (RLP under 32 bytes) travels inside its parent and is no proof node of its own.

Not here: remove / delete, prefix iteration, persistent stores."""
import hashlib

import numpy as np

from . import _native

BLANK_NODE = b""
NIBBLE_TERMINATOR = 16


def sha3(data):
    return hashlib.sha3_256(data).digest()


# ---------------------------------------------------------------------------------------------- RLP
def _length_prefix(n, base):
    if n < 56:
        return bytes([base + n])
    be = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([base + 55 + len(be)]) + be


def rlp_encode(item):
    """RLP of a byte string or a (nested) list of byte strings."""
    if isinstance(item, (bytes, bytearray)):
        if len(item) == 1 and item[0] < 0x80:
            return bytes(item)
        return _length_prefix(len(item), 0x80) + bytes(item)
    body = b"".join(rlp_encode(x) for x in item)
    return _length_prefix(len(body), 0xC0) + body


def _rlp_item(data, pos):
    """(is_list, payload start, payload end) of the item at pos."""
    b0 = data[pos]
    if b0 < 0x80:
        return False, pos, pos + 1
    is_list = b0 >= 0xC0
    v = b0 - (0xC0 if is_list else 0x80)
    if v < 56:
        start, n = pos + 1, v
    else:
        ll = v - 55
        start = pos + 1 + ll
        n = int.from_bytes(data[pos + 1:start], "big")
    if start + n > len(data):
        raise ValueError("RLP item runs past its buffer")
    return is_list, start, start + n


def rlp_decode(data):
    """The byte string or nested list that `data` encodes."""
    def item(pos):
        is_list, a, b = _rlp_item(data, pos)
        if not is_list:
            return bytes(data[a:b]), b
        out = []
        while a < b:
            x, a = item(a)
            out.append(x)
        return out, b
    return item(0)[0]


def _lenient_prefix(data, pos):
    """(is_list, payload length, payload start) of the prefix at pos, nothing checked: a length field cut short
    by the end of the data counts the bytes that are there."""
    b0 = data[pos]
    if b0 < 0x80:
        return False, 1, pos
    is_list = b0 >= 0xC0
    v = b0 - (0xC0 if is_list else 0x80)
    if v < 56:
        return is_list, v, pos + 1
    start = pos + 1 + v - 55
    return is_list, int.from_bytes(data[pos + 1:start], "big"), start


def rlp_decode_lenient(data):
    """What the reference's proof deserializer (state/util/fast_rlp.py:34-71) makes of `data`: no bounds, no
    minimal-length and no trailing-byte checks. A list runs to the end of the bytes it was given, whatever its
    length field says; an item that runs past them is cut off there. IndexError on empty input."""
    is_list, n, pos = _lenient_prefix(data, 0)
    if not is_list:
        return bytes(data[pos:pos + n])
    out = []
    while pos < len(data):
        _, n, start = _lenient_prefix(data, pos)
        out.append(rlp_decode_lenient(data[pos:start + n]))
        pos = start + n
    return out


BLANK_ROOT = sha3(rlp_encode(BLANK_NODE))


# ------------------------------------------------------------------------------------- nibble paths
def bin_to_nibbles(key):
    out = []
    for b in bytes(key):
        out.append(b >> 4)
        out.append(b & 15)
    return out


def nibbles_to_bin(nibbles):
    if len(nibbles) % 2:
        raise ValueError("nibbles must be of even numbers")
    return bytes(16 * nibbles[i] + nibbles[i + 1] for i in range(0, len(nibbles), 2))


def hp_pack(nibbles, terminator):
    """Hex-prefix packing: flags nibble (2 = terminator, 1 = odd length), a padding nibble when even."""
    flags = (2 if terminator else 0) | (len(nibbles) & 1)
    seq = [flags] + ([] if len(nibbles) & 1 else [0]) + list(nibbles)
    return bytes(16 * seq[i] + seq[i + 1] for i in range(0, len(seq), 2))


def hp_unpack(packed):
    """(nibbles, terminator) of a packed path."""
    flags = packed[0] >> 4
    nib = bin_to_nibbles(packed)
    return nib[1:] if flags & 1 else nib[2:], bool(flags & 2)


def _common(a, b):
    n = 0
    for x, y in zip(a, b):
        if x != y:
            break
        n += 1
    return n


def _to_bytes(x, what):
    if isinstance(x, str):
        return x.encode()
    if not isinstance(x, (bytes, bytearray)):
        raise Exception("%s must be string" % what)
    return bytes(x)


class KeyValueStorageInMemory:
    """A dict as key-value store: get raises KeyError for an absent key. Trie and PruningState ask no more
    of any store than get, put and __contains__."""

    def __init__(self):
        self._dict = {}
        self.closed = False

    def get(self, key):
        return self._dict[_to_bytes(key, "key")]

    def put(self, key, value):
        self._dict[_to_bytes(key, "key")] = _to_bytes(value, "value")

    def __contains__(self, key):
        return _to_bytes(key, "key") in self._dict

    def close(self):
        self.closed = True

    @property
    def size(self):
        return len(self._dict)


class Trie:
    def __init__(self, db, root_hash=BLANK_ROOT):
        self._db = db
        self.set_root_hash(root_hash)

    # ------------------------------------------------------------------------------------- storage
    def _ref(self, node, is_root=False):
        """What a parent holds for `node`: the node itself below 32 bytes of RLP, else its hash, stored."""
        if node == BLANK_NODE:
            return BLANK_NODE
        enc = rlp_encode(node)
        if len(enc) < 32 and not is_root:
            return node
        key = sha3(enc)
        self._db.put(key, enc)
        return key

    def _load(self, ref):
        if ref == BLANK_NODE or isinstance(ref, list):
            return ref
        return rlp_decode(bytes(self._db.get(ref)))

    @property
    def root_hash(self):
        if self.root_node == BLANK_NODE:
            return BLANK_ROOT
        return sha3(rlp_encode(self.root_node))

    @root_hash.setter
    def root_hash(self, value):
        self.set_root_hash(value)

    def set_root_hash(self, root_hash):
        if not isinstance(root_hash, (bytes, bytearray)):
            raise TypeError("root_hash must be bytes")
        if len(root_hash) not in (0, 32):
            raise ValueError("root_hash must be 0 or 32 bytes long")
        self.root_node = BLANK_NODE if root_hash == BLANK_ROOT else self._load(bytes(root_hash))

    def replace_root_hash(self, old_node, new_node):
        self._ref(new_node, is_root=True)
        self.root_node = new_node

    # --------------------------------------------------------------------------------------- reads
    def _get(self, node, path):
        while True:
            if node == BLANK_NODE:
                return BLANK_NODE
            if len(node) == 17:
                if not path:
                    return node[16]
                node, path = self._load(node[path[0]]), path[1:]
                continue
            cur, term = hp_unpack(node[0])
            if term:
                return node[1] if cur == path else BLANK_NODE
            if path[:len(cur)] != cur:
                return BLANK_NODE
            node, path = self._load(node[1]), path[len(cur):]

    def get(self, key):
        return self._get(self.root_node, bin_to_nibbles(_to_bytes(key, "Key")))

    def get_at(self, root_node, key):
        return self._get(root_node, bin_to_nibbles(_to_bytes(key, "Key")))

    def __contains__(self, key):
        return self.get(key) != BLANK_NODE

    def _walk(self, node, prefix, out):
        if node == BLANK_NODE:
            return
        if len(node) == 17:
            for i in range(16):
                self._walk(self._load(node[i]), prefix + [i], out)
            if node[16]:
                out[nibbles_to_bin(prefix)] = node[16]
            return
        cur, term = hp_unpack(node[0])
        if term:
            out[nibbles_to_bin(prefix + cur)] = node[1]
        else:
            self._walk(self._load(node[1]), prefix + cur, out)

    def to_dict(self, node=None):
        out = {}
        self._walk(node or self.root_node, [], out)
        return out

    # -------------------------------------------------------------------------------------- proofs
    def _recorder(self, cache=None):
        """(load, seen): load(ref) is _load that notes every node it fetches by hash in `seen`, an insertion-
        ordered {RLP: node}. Recording is local to the call that asked for it; `cache` ({hash: (RLP, node)})
        lets several calls share the decoding."""
        seen = {}

        def load(ref):
            if ref == BLANK_NODE or isinstance(ref, list):
                return ref
            hit = cache.get(ref) if cache is not None else None
            if hit is None:
                enc = bytes(self._db.get(ref))
                hit = (enc, rlp_decode(enc))
                if cache is not None:
                    cache[bytes(ref)] = hit
            seen.setdefault(hit[0], hit[1])
            return hit[1]
        return load, seen

    @staticmethod
    def _get_with(node, path, load):
        """_get over load(ref), with the reference's answer for a list that is no node (pruning_trie.py:359-407:
        neither 2 nor 17 items gives None, which equals no expected value)."""
        while True:
            if node == BLANK_NODE:
                return BLANK_NODE
            if len(node) == 17:
                if not path:
                    return node[16]
                node, path = load(node[path[0]]), path[1:]
                continue
            if len(node) != 2:
                return None
            cur, term = hp_unpack(node[0])
            if term:
                return node[1] if cur == path else BLANK_NODE
            if path[:len(cur)] != cur:
                return BLANK_NODE
            node, path = load(node[1]), path[len(cur):]

    @staticmethod
    def _last_node_for_prefix(node, prefix, seen_prefix, load):
        """The node below which every key with `prefix` lies (pruning_trie.py:409-458); seen_prefix collects the
        nibbles consumed above it, not the node's own path."""
        while True:
            if node == BLANK_NODE:
                return BLANK_NODE
            if len(node) == 17:
                if not prefix:
                    return node
                seen_prefix.append(prefix[0])
                node, prefix = load(node[prefix[0]]), prefix[1:]
                continue
            cur, term = hp_unpack(node[0])
            if term or len(prefix) <= len(cur):
                return node if cur[:len(prefix)] == prefix else BLANK_NODE
            if prefix[:len(cur)] != cur:
                return BLANK_NODE
            seen_prefix.extend(cur)
            node, prefix = load(node[1]), prefix[len(cur):]

    def _collect(self, node, prefix, out, load):
        """_walk over load(ref): {nibble tuple: raw value} of everything below node."""
        if node == BLANK_NODE:
            return
        if len(node) == 17:
            for i in range(16):
                self._collect(load(node[i]), prefix + [i], out, load)
            if node[16]:
                out[tuple(prefix)] = node[16]
            return
        cur, term = hp_unpack(node[0])
        if term:
            out[tuple(prefix + cur)] = node[1]
        else:
            self._collect(load(node[1]), prefix + cur, out, load)

    def produce_spv_proof(self, key, root=None, get_value=False, _cache=None):
        """The nodes fetched by hash on key's path below `root` (a node; default the current root), in the order
        loaded, each once. The root itself is not among them. With get_value: (nodes, the raw stored value or None)."""
        root = root if root is not None else self.root_node
        load, seen = self._recorder(_cache)
        rv = self._get_with(root, bin_to_nibbles(_to_bytes(key, "Key")), load)
        nodes = list(seen.values())
        return (nodes, rv if rv != BLANK_NODE else None) if get_value else nodes

    def produce_spv_proof_for_keys_with_prefix(self, key_prfx, root=None, get_value=False, _cache=None):
        """The nodes fetched by hash on the way to the prefix and in the whole subtree below it. With get_value:
        (nodes, {full key: raw stored value})."""
        root = root if root is not None else self.root_node
        load, seen = self._recorder(_cache)
        seen_prefix = []
        node = self._last_node_for_prefix(root, bin_to_nibbles(_to_bytes(key_prfx, "Key")), seen_prefix, load)
        found = {}
        self._collect(node, [], found, load)
        nodes = list(seen.values())
        if not get_value:
            return nodes
        values = {}
        for k, v in found.items():
            nib = seen_prefix + list(k)
            values[nibbles_to_bin(nib[1:] if len(nib) % 2 else nib)] = v
        return nodes, values

    def _generate_state_proof(self, path, func, root, serialize, **kw):
        root = root if root is not None else self.root_node
        rv = func(path, root, **kw)
        has_val = isinstance(rv, tuple)
        nodes = rv[0] if has_val else rv
        nodes.append(list(root) if isinstance(root, list) else root)  # the root last; b'' for the blank root
        if serialize:
            nodes = self.serialize_proof(nodes)
        return (nodes, rv[1]) if has_val else nodes

    def generate_state_proof(self, key, root=None, serialize=False, get_value=False, _cache=None):
        return self._generate_state_proof(key, self.produce_spv_proof, root, serialize, get_value=get_value, _cache=_cache)

    def generate_state_proof_for_keys_with_prefix(self, key_prfx, root=None, serialize=False, get_value=False):
        return self._generate_state_proof(key_prfx, self.produce_spv_proof_for_keys_with_prefix, root, serialize,
                                          get_value=get_value)

    @staticmethod
    def serialize_proof(proof_nodes):
        return rlp_encode(proof_nodes)

    @staticmethod
    def deserialize_proof(ser_proof):
        return rlp_decode_lenient(bytes(ser_proof))

    @staticmethod
    def get_new_trie_with_proof_nodes(proof_nodes):
        """A trie over a fresh store holding every proof node under the SHA3-256 of its (re-)encoding."""
        trie = Trie(KeyValueStorageInMemory())
        for node in proof_nodes:
            enc = rlp_encode(node)
            trie._db.put(sha3(enc), enc)
        return trie

    @staticmethod
    def verify_spv_proof(root, key, value, proof_nodes, serialized=False):
        """Does the trie under the root hash `root` hold `value` (as stored; b'' = nothing) for `key`, by these
        nodes alone? Deserializing and storing the nodes may raise; everything after gives False."""
        if serialized:
            proof_nodes = Trie.deserialize_proof(proof_nodes)
        trie = Trie.get_new_trie_with_proof_nodes(proof_nodes)
        try:
            trie.root_hash = root
            return trie._get_with(trie.root_node, bin_to_nibbles(_to_bytes(key, "Key")), trie._load) == value
        except Exception:
            return False

    @staticmethod
    def verify_spv_proof_multi(root, key_values, proof_nodes, serialized=False):
        """verify_spv_proof for every key -> value of `key_values` against one pool of nodes."""
        if serialized:
            proof_nodes = Trie.deserialize_proof(proof_nodes)
        trie = Trie.get_new_trie_with_proof_nodes(proof_nodes)
        try:
            trie.root_hash = root
            for k, v in key_values.items():
                if trie._get_with(trie.root_node, bin_to_nibbles(_to_bytes(k, "Key")), trie._load) != v:
                    return False
            return True
        except Exception:
            return False

    @staticmethod
    def _proof_statuses(queries, proofs, serialized):
        """The library's status per query, or None where Python decides alone. queries: (proof index, root, key,
        value); proofs: per proof the list of nodes or, serialized, the bytes. None for a root that is not 32
        bytes or blank, a key or value that is no byte string or above the library's limits, a proof of more
        than 1,024 nodes, one whose nodes cannot be encoded and a serialized one whose outer list is not
        canonical RLP."""
        out = [None] * len(queries)
        records = [None] * len(proofs)  # per proof: (start, end) into node_off, once it is known to be usable
        blob, off, lens = b"", [], None
        if serialized:
            try:
                sers = [bytes(p) for p in proofs]
            except TypeError:
                return out
            blob, first, off, lens, ok = _native.trie_proof_split(sers)
            for p in range(len(proofs)):
                if ok[p] and first[p + 1] - first[p] <= _native.PV_PROOF_MAX_NODES:
                    records[p] = (int(first[p]), int(first[p + 1]))
        else:
            parts, at = [], 0
            for p, nodes in enumerate(proofs):
                try:
                    encs = [rlp_encode(n) for n in nodes]
                except Exception:
                    continue  # the sequential method raises what it raises
                if len(encs) > _native.PV_PROOF_MAX_NODES:
                    continue
                records[p] = (len(off), len(off) + len(encs))
                for e in encs:
                    off.append(at)
                    at += len(e)
                parts += encs
            off.append(at)
            blob = b"".join(parts)
        sent, proof_of, first = [], {}, [0]
        node_idx = []
        roots, keys, vals, qp = [], [], [], []
        for i, (p, root, key, value) in enumerate(queries):
            if records[p] is None or not isinstance(root, (bytes, bytearray)) or len(root) != 32 or root == BLANK_ROOT:
                continue
            if isinstance(key, str):
                key = key.encode()
            if not isinstance(key, (bytes, bytearray)) or not isinstance(value, (bytes, bytearray)):
                continue
            if len(key) > _native.PV_TRIE_MAX_KEY or len(value) > _native.PV_TRIE_MAX_VALUE:
                continue
            if p not in proof_of:
                proof_of[p] = len(first) - 1
                node_idx.extend(range(*records[p]))
                first.append(len(node_idx))
            sent.append(i)
            qp.append(proof_of[p])
            roots.append(bytes(root))
            keys.append(bytes(key))
            vals.append(bytes(value))
        if sent:
            status = _native.trie_verify_proofs(blob, off, lens, node_idx, first, qp, roots, keys, vals)
            for i, s in zip(sent, status):
                out[i] = int(s)
        return out

    @staticmethod
    def verify_spv_proof_batch(items, serialized=False):
        """[verify_spv_proof(root, key, value, proof_nodes, serialized) for each of items], the hashing and the
        walks as one library call. What the library defers or cannot take goes through the sequential method,
        which may raise as it does on its own."""
        items = list(items)
        status = Trie._proof_statuses([(i, r, k, v) for i, (r, k, v, _) in enumerate(items)], [it[3] for it in items],
                                      serialized)
        return [Trie.verify_spv_proof(r, k, v, pn, serialized) if s is None or s == _native.PV_PROOF_DEFER
                else s == _native.PV_PROOF_ACCEPT for s, (r, k, v, pn) in zip(status, items)]

    @staticmethod
    def verify_spv_proof_multi_batch(root, key_values, proof_nodes, serialized=False):
        """verify_spv_proof_multi as one proof with many queries in one library call."""
        if key_values:
            status = Trie._proof_statuses([(0, root, k, v) for k, v in key_values.items()], [proof_nodes], serialized)
            if _native.PV_PROOF_REJECT in status:
                return False  # that pair alone makes the sequential answer False
            if all(s == _native.PV_PROOF_ACCEPT for s in status):
                return True
        return Trie.verify_spv_proof_multi(root, key_values, proof_nodes, serialized)

    # -------------------------------------------------------------------------------------- update
    def _leaf_ref(self, path, value):
        return self._ref([hp_pack(path, True), value])

    def _insert(self, node, path, value):
        """The node that replaces `node` once path -> value is set below it."""
        if node == BLANK_NODE:
            return [hp_pack(path, True), value]
        if len(node) == 17:
            new = list(node)
            if not path:
                new[16] = value
            else:
                new[path[0]] = self._ref(self._insert(self._load(node[path[0]]), path[1:], value))
            return new
        cur, term = hp_unpack(node[0])
        m = _common(cur, path)
        if m == len(cur) and (not term or m == len(path)):
            if term:
                return [node[0], value]
            return [node[0], self._ref(self._insert(self._load(node[1]), path[m:], value))]
        # the two paths part after m nibbles: a branch there, under an extension when m > 0
        branch = [BLANK_NODE] * 17
        rest = cur[m:]
        if term:
            if rest:
                branch[rest[0]] = self._leaf_ref(rest[1:], node[1])
            else:
                branch[16] = node[1]
        else:
            branch[rest[0]] = node[1] if len(rest) == 1 else self._ref([hp_pack(rest[1:], False), node[1]])
        mine = path[m:]
        if mine:
            branch[mine[0]] = self._leaf_ref(mine[1:], value)
        else:
            branch[16] = value
        return [hp_pack(cur[:m], False), self._ref(branch)] if m else branch

    def update(self, key, value):
        key, value = _to_bytes(key, "Key"), _to_bytes(value, "Value")
        new_root = self._insert(self.root_node, bin_to_nibbles(key), value)
        self.replace_root_hash(self.root_node, new_root)

    def update_batch(self, items):
        """update(key, value) for every (key, value) of `items`, in order, as one library call chain: the
        library is told the root, answers with the hashes of the existing nodes the batch reaches, gets them
        from the store, and returns the final trie's new nodes, which are stored. Afterwards root_hash, every
        get and every node reachable from the root are what the sequential updates leave; each key written
        to the store holds the bytes the sequential run writes under it. The intermediate roots of the batch
        (after its first, second, ... update) are NOT produced, and the nodes only they reach are not stored."""
        items = [(_to_bytes(k, "Key"), _to_bytes(v, "Value")) for k, v in items]
        if not items:
            return
        if any(len(k) > _native.PV_TRIE_MAX_KEY or not v or len(v) > _native.PV_TRIE_MAX_VALUE for k, v in items):
            for k, v in items:  # outside the library's limits: the sequential method
                self.update(k, v)
            return
        self._ref(self.root_node, is_root=True)  # the library starts from the stored root
        root, nodes = _native.trie_update(self.root_hash, self._db.get, [k for k, _ in items], [v for _, v in items])
        for h, enc in nodes:
            self._db.put(h, enc)
        self.root_node = rlp_decode(nodes[-1][1])

    def delete(self, key):
        raise NotImplementedError("the trie has no delete yet (branch normalisation, pruning_trie.py:706-744)")


class PruningState:
    """The state over a key-value store; the committed root hash is kept in the store under rootHashKey
    and moves only on commit, so batches in flight are forgotten by a restart."""

    rootHashKey = b"\x88\xc8\x88 \x9a\xa7\x89\x1b"

    def __init__(self, keyValueStorage):
        self._kv = keyValueStorage
        if self.rootHashKey in self._kv:
            root_hash = bytes(self._kv.get(self.rootHashKey))
        else:
            root_hash = BLANK_ROOT
            self._kv.put(self.rootHashKey, BLANK_ROOT)
        self._trie = Trie(self._kv, root_hash)

    @property
    def head(self):
        return self._trie.root_node

    @property
    def committedHead(self):
        return self._hash_to_node(self.committedHeadHash)

    def get_head_by_hash(self, root_hash):
        return self._hash_to_node(root_hash)

    def _hash_to_node(self, node_hash):
        if node_hash == BLANK_ROOT:
            return BLANK_NODE
        return self._trie._load(bytes(node_hash))

    @staticmethod
    def _stored(value):
        return rlp_encode([_to_bytes(value, "Value")])

    @staticmethod
    def get_decoded(encoded):
        return rlp_decode(encoded)[0]

    def set(self, key, value):
        self._trie.update(key, self._stored(value))

    def set_batch(self, items):
        """set(key, value) for every (key, value) of `items`, in order, as one Trie.update_batch: headHash,
        every get under the new head and every node reachable from it are what the set calls leave. The
        intermediate roots of the batch are not produced."""
        self._trie.update_batch([(k, self._stored(v)) for k, v in items])

    @staticmethod
    def root_of(items):
        """headHash of a state built from empty by set(key, value) for every (key, value) of `items`; no
        store is written (rebuilding state from the ledger, the catch-up check)."""
        items = [(_to_bytes(k, "Key"), _to_bytes(v, "Value")) for k, v in items]
        key_len = len(items[0][0]) if items else 0
        if (1 <= key_len <= _native.PV_TRIE_BUILD_MAX_KEY and all(len(k) == key_len for k, _ in items)
                and all(len(v) <= _native.PV_TRIE_MAX_VALUE - 8 for _, v in items)):
            # one key length: the from-empty entry, which builds the structure on the device too and wraps each value
            # as rlp([value]) while it writes the leaf
            val_blob, val_off = _native._blob([v for _, v in items])
            keys = np.frombuffer(b"".join(k for k, _ in items), np.uint8).reshape(len(items), key_len)
            return _native.trie_root(keys, val_blob, val_off, wrap=True)
        items = [(k, PruningState._stored(v)) for k, v in items]
        if any(len(k) > _native.PV_TRIE_MAX_KEY or len(v) > _native.PV_TRIE_MAX_VALUE for k, v in items):
            trie = Trie(KeyValueStorageInMemory())
            for k, v in items:
                trie.update(k, v)
            return trie.root_hash
        if not items:
            return BLANK_ROOT
        return _native.trie_update(BLANK_ROOT, None, [k for k, _ in items], [v for _, v in items])[0]

    @staticmethod
    def root_of_arrays(keys, val_blob, val_off):
        """root_of for callers that hold arrays: keys a (n, key_len) uint8 array with key_len 1 .. 64, value i the
        bytes val_blob[val_off[i]:val_off[i + 1]] as given to set (the library wraps them). One library call, no
        per-item Python."""
        return _native.trie_root(keys, val_blob, val_off, wrap=True)

    def get(self, key, isCommitted=True):
        if not isCommitted:
            val = self._trie.get(key)
        else:
            val = self._trie.get_at(self.committedHead, key)
        if val:
            return self.get_decoded(val)

    def get_for_root_hash(self, root_hash, key):
        val = self._trie.get_at(self._hash_to_node(root_hash), key)
        if val:
            return self.get_decoded(val)

    def get_all_leaves_for_root_hash(self, root_hash):
        return self._trie.to_dict(self._hash_to_node(root_hash))

    def remove(self, key):
        self._trie.delete(key)

    # -------------------------------------------------------------------------------------- proofs
    def generate_state_proof(self, key, root=None, serialize=False, get_value=False):
        """The proof for `key` under `root` (a node, as get_head_by_hash gives it; default the head): the hashed
        nodes on its path in the order loaded, then the root. serialize: as one RLP list. get_value: with the
        raw stored value (rlp([value])) or None."""
        return self._trie.generate_state_proof(key, root, serialize, get_value=get_value)

    def generate_state_proof_for_keys_with_prefix(self, key_prfx, root=None, serialize=False, get_value=False):
        return self._trie.generate_state_proof_for_keys_with_prefix(key_prfx, root, serialize, get_value=get_value)

    def generate_state_proof_batch(self, keys, root=None, serialize=False, get_value=False):
        """[generate_state_proof(key, root, serialize, get_value) for key in keys]; a node that several paths
        share (the top of the trie) is fetched and decoded once for the call."""
        cache = {}
        return [self._trie.generate_state_proof(k, root, serialize, get_value=get_value, _cache=cache) for k in keys]

    @staticmethod
    def encode_kv_for_verification(key, value):
        return key.encode() if isinstance(key, str) else key, rlp_encode([value]) if value is not None else b""

    @staticmethod
    def verify_state_proof(root, key, value, proof_nodes, serialized=False):
        key, value = PruningState.encode_kv_for_verification(key, value)
        return Trie.verify_spv_proof(root, key, value, proof_nodes, serialized)

    @staticmethod
    def verify_state_proof_multi(root, key_values, proof_nodes, serialized=False):
        encoded = dict(PruningState.encode_kv_for_verification(k, v) for k, v in key_values.items())
        return Trie.verify_spv_proof_multi_batch(root, encoded, proof_nodes, serialized)

    @staticmethod
    def verify_state_proof_batch(items, serialized=False):
        """[verify_state_proof(root, key, value, proof_nodes, serialized) for each of items] as one library call."""
        return Trie.verify_spv_proof_batch(
            [(r,) + PruningState.encode_kv_for_verification(k, v) + (pn,) for r, k, v, pn in items], serialized)

    def commit(self, rootHash=None, rootNode=None):
        if rootNode:
            rootHash = self._trie._ref(rootNode, is_root=True)
        elif rootHash:
            if isinstance(rootHash, str):
                rootHash = rootHash.encode()
            try:
                if len(rootHash) == 64:
                    rootHash = bytes.fromhex(rootHash.decode())
            except (ValueError, UnicodeDecodeError):
                pass
        else:
            rootHash = self.headHash
        self._kv.put(self.rootHashKey, rootHash)

    def revertToHead(self, headHash=None):
        self._trie.replace_root_hash(self._trie.root_node, self._hash_to_node(headHash))

    @property
    def as_dict(self):
        return {k: self.get_decoded(v) for k, v in self._trie.to_dict().items()}

    @property
    def headHash(self):
        return self._trie.root_hash

    @property
    def committedHeadHash(self):
        return bytes(self._kv.get(self.rootHashKey))

    @property
    def closed(self):
        return not self._kv or self._kv.closed

    @property
    def isEmpty(self):
        return bool(self._kv) and self.committedHeadHash == BLANK_ROOT

    def close(self):
        if self._kv:
            self._kv.close()
            self._kv = None
