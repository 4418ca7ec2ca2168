"""The key cache's host index (indy-plenum_amd/csrc/kc_index.h: which slot a key gets, which key is evicted, the
rollback of a failed put, the fold of the launches' stamps into the LRU, the packing of a put into build batches, the
fill of the open-addressing table), compiled with g++ exactly as the library includes it, under AddressSanitizer
and UBSan, and run as a stand-alone program (tests/native/kc_index_check.cpp). The table the host fills is read
back there with the library's own pv_kc_hash / pv_kc_lookup (csrc/keycache.h). Scenarios with outcomes worked out
by hand, then 2,000 seeded random operations per capacity against a Python model of the loops as they stood in
pv_engine.hip before the index had a file of its own. The GPU side is tests/test_gpu_keycache.py. CPU only."""
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "kc_index_check.cpp")
STUB = os.path.join(HERE, "native", "stub_hip")
CSRC = os.path.join(HERE, "..", "indy-plenum_amd", "csrc")
BIN = os.path.join(HERE, "native", "kc_index_check")

E = 0xFFFFFFFF  # PV_KC_EMPTY


@pytest.fixture(scope="module")
def report():
    deps = [SRC, os.path.join(CSRC, "kc_index.h"), os.path.join(CSRC, "keycache.h"),
            os.path.join(STUB, "hip", "hip_runtime.h")]
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                               "-I", STUB, "-o", BIN, SRC])
    out = subprocess.run([BIN], check=True, capture_output=True, text=True, timeout=120).stdout
    return json.loads(out)


def r(a, b):
    return list(range(a, b))


def down(a, b):
    """a, a - 1, ..., b"""
    return list(range(a, b - 1, -1))


def checked(s):
    assert s["invariants"] is True and s["lookups"] is True, s
    return s


def lru_slots(s):
    return [slot for slot, _ in s["lru"]]


def test_forty_keys_into_sixteen_slots_then_four_old_ones(report):
    """One put of 40 distinct keys at capacity 16: slots 0..15 go out in ascending order, keys 16..31 evict keys
    0..15 from those slots, keys 32..39 evict keys 16..23 from slots 0..7. The last 16 keys remain; the first 24
    have nothing left to build; one batch at kcap 16 holds exactly the 16 built keys with their slots. Then keys
    0..3 take the slots of the four least recent survivors, keys 24..27."""
    s0 = checked(report["s0"])
    assert s0["lru"] == [] and s0["free"] == down(15, 0) and s0["size"] == 0 and s0["capacity"] == 16
    s1 = checked(report["s1"])
    assert s1["fresh"] == r(0, 40)
    assert s1["fresh_slot"] == [E] * 24 + r(8, 16) + r(0, 8)
    assert s1["touched"] == r(0, 16) + r(0, 16) + r(0, 8)
    assert s1["evicted"] == r(0, 24)
    assert s1["packs"] == [[0, 40, 16, r(24, 40), r(8, 16) + r(0, 8)]]
    assert s1["lru"] == [[s, 32 + s] for s in down(7, 0)] + [[s, 16 + s] for s in down(15, 8)]
    assert s1["free"] == [] and s1["size"] == 16
    s2 = checked(report["s2"])
    assert s2["fresh"] == r(0, 4) and s2["fresh_slot"] == r(8, 12) and s2["evicted"] == r(24, 28)
    assert s2["lru"] == [[11, 3], [10, 2], [9, 1], [8, 0]] + s1["lru"][:8] + [[s, 16 + s] for s in down(15, 12)]
    assert s2["size"] == 16


def test_duplicates_in_one_put_after_a_clear(report):
    """keys[:10] + keys[:10] after a clear: ten fresh entries in slots 0..9 in order, the second ten only refresh.
    needs_fold counts the call's keys, duplicates included, and never asks for a fold of an empty LRU."""
    c = checked(report["s3_cleared"])
    assert c["lru"] == [] and c["free"] == down(15, 0) and c["size"] == 0 and c["capacity"] == 16
    assert c["needs_fold_20"] is False
    s3 = checked(report["s3"])
    assert s3["fresh"] == r(0, 10) and s3["fresh_slot"] == r(0, 10) and s3["touched"] == r(0, 10)
    assert s3["evicted"] == [] and s3["size"] == 10
    assert s3["lru"] == [[s, s] for s in down(9, 0)] and s3["free"] == down(15, 10)
    assert s3["needs_fold_6"] is False and s3["needs_fold_7"] is True


def test_rollback_frees_what_the_put_assigned_and_nothing_else(report):
    """16 keys, then a put of 8 more that is rolled back: the 8 untouched keys keep slots 8..15, the 8 slots the put
    had taken (and whose former keys it had evicted) are free and go out next, last freed first; a put of 11 keys
    fills them and evicts the three least recent of the untouched keys."""
    rb = checked(report["s4_rolled_back"])
    assert rb["fresh"] == r(16, 24) and rb["fresh_slot"] == r(0, 8) and rb["evicted"] == r(0, 8)
    assert rb["size"] == 8 and rb["lru"] == [[s, s] for s in down(15, 8)] and rb["free"] == r(0, 8)
    p = checked(report["s4_put_11"])
    assert p["fresh_slot"] == down(7, 0) + [8, 9, 10] and p["evicted"] == [8, 9, 10]
    assert p["size"] == 16 and p["free"] == []
    assert sorted(k for _, k in p["lru"]) == r(11, 16) + r(24, 35)


def test_rollback_frees_a_slot_assigned_twice_once(report):
    """Five keys into two slots: slot 0 is handed out three times and slot 1 twice in one put. Rolled back, each
    is free once and the index is empty."""
    a = checked(report["s5_assigned"])
    assert a["fresh_slot"] == [E, E, E, 1, 0] and a["touched"] == [0, 1, 0, 1, 0] and a["evicted"] == [0, 1, 2]
    assert a["lru"] == [[0, 4], [1, 3]]
    rb = checked(report["s5_rolled_back"])
    assert rb["lru"] == [] and rb["free"] == [0, 1] and rb["size"] == 0 and rb["capacity"] == 2
    p = checked(report["s5_put_2"])
    assert p["fresh_slot"] == [1, 0] and p["evicted"] == [] and p["free"] == []


def test_fold_orders_the_lru_by_the_age_of_the_stamps(report):
    """Capacity 4, keys 0..3 put in order (slot i holds key i, slot 0 least recent), one fold, then four evictions.
    Only slot 0 newer than the fold epoch (slot 1 equal to it, slot 2 one below it, which wraps negative): the next
    eviction takes the key put second. Equal ages keep their order. The largest age ends most recent. An age of
    2^31 - 1 is taken and one of 2^31 is not. The same across the wrap of the epoch."""
    s6 = report["s6"]
    want = {
        "only_slot_0_newer": ([0, 3, 2, 1], [1, 2, 3, 0]),
        "equal_ages": ([1, 0, 3, 2], [2, 3, 0, 1]),
        "largest_age_most_recent": ([0, 2, 1, 3], [3, 1, 2, 0]),
        "half_range_ahead": ([1, 3, 2, 0], [0, 2, 3, 1]),
        "epoch_wrapped": ([1, 3, 2, 0], [0, 2, 3, 1]),
    }
    assert s6["folds"] == len(want)
    for name, (lru, evicted) in want.items():
        s = checked(s6[name])
        assert lru_slots(s) == lru and s["lru"] == [[x, x] for x in lru], (name, s)
        assert s["evicted_next"] == evicted, (name, s)


def test_packing_skips_holes_at_batch_boundaries(report):
    """21 fresh entries at kcap 5, holes (slot PV_KC_EMPTY) before, between and after three full batches: every
    built key appears exactly once with its slot, no batch exceeds kcap, and the last batch is holes only."""
    packs = report["s7"]["packs"]
    assert packs == [[0, 6, 5, r(101, 106), r(10, 15)], [6, 13, 5, r(108, 113), r(15, 20)],
                     [13, 19, 5, r(114, 119), r(20, 25)], [19, 21, 0, [], []]]
    assert report["pack_bytes_ok"] is True


class Model:
    """The index as pv_engine.hip kept it inside kc_put_locked, kc_fold_hits, pv_key_cache_configure and
    pv_key_cache_clear: a map key -> slot, the LRU as a list of slots (most recent first), slot_key, and the
    free slots, taken from the back. evict_front / free_descending: deliberately wrong variants."""

    def __init__(self, cap, evict_front=False, free_descending=False):
        self.cap, self.evict_front, self.free_descending = cap, evict_front, free_descending
        self.clear()

    def clear(self):
        self.index, self.lru, self.slot_key = {}, [], [None] * self.cap
        self.free = list(range(self.cap)) if self.free_descending else list(range(self.cap - 1, -1, -1))

    def needs_fold(self, n):
        return len(self.free) < n and len(self.lru) > 0

    def assign(self, keys):
        fresh, fresh_slot, touched, evicted = [], [], [], []
        for key in keys:
            if key in self.index:
                self.lru.remove(self.index[key])
                self.lru.insert(0, self.index[key])
                continue
            if self.free:
                slot = self.free.pop()
            else:
                slot = self.lru.pop(0) if self.evict_front else self.lru.pop()
                del self.index[self.slot_key[slot]]
                evicted.append(self.slot_key[slot])
                for f in range(len(fresh)):
                    if fresh_slot[f] == slot:
                        fresh_slot[f] = E
            self.lru.insert(0, slot)
            self.index[key] = slot
            self.slot_key[slot] = key
            fresh.append(key)
            fresh_slot.append(slot)
            touched.append(slot)
        return fresh, fresh_slot, touched, evicted

    def rollback(self, touched):
        seen = [False] * self.cap
        for slot in touched:
            if seen[slot]:
                continue
            seen[slot] = True
            if self.index.get(self.slot_key[slot]) == slot:
                self.lru.remove(slot)
                del self.index[self.slot_key[slot]]
            self.slot_key[slot] = None
            self.free.append(slot)

    def fold(self, stamps, fold_epoch):
        used = []
        for slot in reversed(self.lru):
            age = (stamps[slot] - fold_epoch) & 0xFFFFFFFF
            if 0 < age < 1 << 31:
                used.append((age, slot))
        used.sort(key=lambda u: u[0])  # stable
        for _, slot in used:
            if self.index.get(self.slot_key[slot]) == slot:
                self.lru.remove(slot)
                self.lru.insert(0, slot)

    @staticmethod
    def packs(fresh, fresh_slot, kcap):
        out, f0 = [], 0
        while f0 < len(fresh):
            keys, slots, f = [], [], f0
            while f < len(fresh) and len(keys) < kcap:
                if fresh_slot[f] != E:
                    keys.append(fresh[f])
                    slots.append(fresh_slot[f])
                f += 1
            out.append([f0, f, len(keys), keys, slots])
            f0 = f
        return out


def first_difference(run, **wrong):
    """Replays a capacity's operations on the model; the index of the first operation after which the program and
    the model differ, or None."""
    m = Model(run["cap"], **wrong)
    touched = None
    for i, op in enumerate(run["ops"]):
        if op["op"] == "assign":
            if m.needs_fold(len(op["keys"])) != op["needs_fold"]:
                return i
            fresh, fresh_slot, touched, evicted = m.assign(op["keys"])
            if [fresh, fresh_slot, touched, evicted] != [op["fresh"], op["fresh_slot"], op["touched"], op["evicted"]]:
                return i
            if Model.packs(fresh, fresh_slot, run["kcap"]) != op["packs"]:
                return i
        elif op["op"] == "rollback":
            m.rollback(touched)
        elif op["op"] == "fold":
            m.fold(op["stamps"], op["epoch"])
        else:
            assert op["op"] == "clear", op
            m.clear()
        if [[s, m.slot_key[s]] for s in m.lru] != op["lru"] or m.free != op["free"] or len(m.index) != op["size"]:
            return i
    return None


def test_random_operations_match_the_former_loops(report):
    """Capacities 1, 2, 7 and 64, 2,000 operations each: after every operation the results of the put, its build
    batches, the LRU order, each key's slot and the free list in order equal the model's; the program's own checks
    (slots partitioned between free list and LRU, index and slot_key consistent, the filled table resolving every
    indexed key to its slot through pv_kc_lookup and no other key) hold; every built key is packed exactly once."""
    assert [run["cap"] for run in report["random"]] == [1, 2, 7, 64]
    for run in report["random"]:
        ops = run["ops"]
        assert len(ops) == 2000
        kinds = [op["op"] for op in ops]
        assert all(kinds.count(k) >= 50 for k in ("assign", "rollback", "fold", "clear")), run["cap"]
        assert first_difference(run) is None, run["cap"]
        assert run["pack_bytes_ok"] is True
        for op in ops:
            assert op["invariants"] is True and op["lookups"] is True and op["capacity"] == run["cap"], (run["cap"], op)
            if op["op"] == "assign":
                built = [(k, s) for k, s in zip(op["fresh"], op["fresh_slot"]) if s != E]
                packed = [(k, s) for p in op["packs"] for k, s in zip(p[3], p[4])]
                assert packed == built and all(p[2] == len(p[3]) <= run["kcap"] for p in op["packs"])
        # the cases the scenarios name occur here too (but for a batch of holes only: a put's last fresh key is
        # never evicted by the same put)
        assert any(op["op"] == "assign" and E in op["fresh_slot"] for op in ops)
        if run["cap"] > 1:
            assert any(op["op"] == "assign" and E in op["fresh_slot"] and len(op["packs"]) >= 2 for op in ops)
            assert any(op["op"] == "assign" and len(op["keys"]) != len(set(op["keys"])) for op in ops)


@pytest.mark.parametrize("wrong", ["evict_front", "free_descending"])
def test_the_comparison_notices_a_wrong_model(report, wrong):
    """The checker bites: a model that evicts the most recent key, and one that hands out the highest free slot
    first, each differ from the program."""
    for run in report["random"]:
        if run["cap"] == 1:
            continue  # one slot: both orders are the same
        assert first_difference(run, **{wrong: True}) is not None, (wrong, run["cap"])
