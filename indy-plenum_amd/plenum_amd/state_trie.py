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
                                     catch-up check)

The batch calls go through libplenum_verify (pv_trie_update_batch): the structure in C++ on the host, the
SHA3-256 of every new node on the GPU or, for small batches and without one, on host threads. Not here:
remove / delete, state proofs, prefix iteration, persistent stores."""
import hashlib

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
        items = [(_to_bytes(k, "Key"), PruningState._stored(v)) for k, v in items]
        if any(len(k) > _native.PV_TRIE_MAX_KEY or len(v) > _native.PV_TRIE_MAX_VALUE for k, v in items):
            trie = Trie(KeyValueStorageInMemory())
            for k, v in items:
                trie.update(k, v)
            return trie.root_hash
        if not items:
            return BLANK_ROOT
        return _native.trie_update(BLANK_ROOT, None, [k for k, _ in items], [v for _, v in items])[0]

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

    def remove(self, key):
        self._trie.delete(key)

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
