// CPU check of the ledger Merkle plan (csrc/merkle_plan.h, the header the library compiles). Reads the jobs of
// the file named by argv[1], a sequence of u64 words written by tests/test_merkle_plan.py:
//   [1, s0, n, leaf_bound, with_off, byte_bound, len[n]]   an append-like call; its records' offsets start at 7
//   [2, s0, n, leaf_bound, R, end[R]]                       a catch-up with device data and R reply ends
//   [3, s0, n, leaf_bound, mask]                            the outputs of a call, mask bit k = output k is taken
// and prints one JSON object:
//   jobs    per job the chunks of for_each_append_chunk, [c0, m, s, pbase, node_off, n_nodes, n_path, is_last],
//           for job 2 followed by the chunk's reply_window [r0, r1], for job 3 by chunk_outputs as element
//           offsets into arrays of exactly the call's size [leaf, node, roots, path, path_off, root, frontier]
//           (-1: null)
//   spans   [leaf_bound, n, verdict_chunk, for_each_span at verdict_chunk, for_each_span at leaf_bound]
//   checks  every check function on each side of its condition: name -> reason or null
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../indy-plenum_amd/csrc/merkle_plan.h"

using namespace pvhost;

int pv_fail(int code, const std::string&) { return code; }  // workspace.h declares it

static std::string num(int64_t v) { return std::to_string(v); }
static std::string list(const std::vector<int64_t>& v) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); i++) s += (i ? ", " : "") + num(v[i]);
    return s + "]";
}
struct Rows {
    std::string s = "[";
    bool first = true;
    void add(const std::string& row) {
        s += (first ? "" : ", ") + row;
        first = false;
    }
    std::string done() const { return s + "]"; }
};
static std::vector<int64_t> chunk_row(const MkChunk& c) {
    return {(int64_t)c.c0, (int64_t)c.m, (int64_t)c.s, (int64_t)c.pbase, (int64_t)c.node_off, (int64_t)c.n_nodes,
            (int64_t)c.n_path, c.is_last};
}

static std::string job(const uint64_t*& w) {
    const uint64_t type = w[0], s0 = w[1], n = w[2], bound = w[3];
    Rows rows;
    if (type == 1) {
        const bool with_off = w[4];
        const uint64_t byte_bound = w[5];
        uint64_t* off = new uint64_t[n + 1];  // exactly sized
        off[0] = 7;
        for (uint64_t i = 0; i < n; i++) off[i + 1] = off[i] + w[6 + i];
        for_each_append_chunk(s0, n, bound, with_off ? off : nullptr, byte_bound, [&](const MkChunk& c) {
            rows.add(list(chunk_row(c)));
            return 0;
        });
        delete[] off;
        w += 6 + n;
    } else if (type == 2) {
        const uint64_t R = w[4];
        uint64_t* end = new uint64_t[R];
        for (uint64_t r = 0; r < R; r++) end[r] = w[5 + r];
        for_each_append_chunk(s0, n, bound, nullptr, 0, [&](const MkChunk& c) {
            const MkWindow x = reply_window(end, R, c.s, c.m);
            std::vector<int64_t> row = chunk_row(c);
            row.push_back((int64_t)x.r0);
            row.push_back((int64_t)x.r1);
            rows.add(list(row));
            return 0;
        });
        delete[] end;
        w += 5 + R;
    } else {
        const uint64_t mask = w[4];
        uint64_t n_nodes, n_front, n_path;
        pv_merkle_plan_core(s0, n, &n_nodes, &n_front, &n_path);
        std::vector<uint8_t> leaf(32 * n), node(32 * n_nodes + 1), front(2048), root(32), roots(32 * n), path(32 * n_path + 1);
        std::vector<uint64_t> poff(n + 1);
        PvMerkleOut out{};
        if (mask & 1) out.leaf_hash = leaf.data();
        if (mask & 2) out.node_hash = node.data();
        if (mask & 4) out.frontier = front.data();
        if (mask & 8) out.root = root.data();
        if (mask & 16) out.roots = roots.data();
        if (mask & 32) out.path = path.data(), out.path_off = poff.data();
        for_each_append_chunk(s0, n, bound, nullptr, 0, [&](const MkChunk& c) {
            const PvMerkleOut o = chunk_outputs(out, c);
            std::vector<int64_t> row = chunk_row(c);
            row.push_back(o.leaf_hash ? (o.leaf_hash - leaf.data()) / 32 : -1);
            row.push_back(o.node_hash ? (o.node_hash - node.data()) / 32 : -1);
            row.push_back(o.roots ? (o.roots - roots.data()) / 32 : -1);
            row.push_back(o.path ? (o.path - path.data()) / 32 : -1);
            row.push_back(o.path_off ? o.path_off - poff.data() : -1);
            row.push_back(o.root ? o.root - root.data() : -1);
            row.push_back(o.frontier ? o.frontier - front.data() : -1);
            rows.add(list(row));
            return 0;
        });
        w += 5;
    }
    return rows.done();
}

static std::string spans(uint64_t n, uint64_t chunk) {
    Rows r;
    const int rc = for_each_span(n, chunk, [&](uint64_t c0, uint64_t m) {
        r.add(list({(int64_t)c0, (int64_t)m}));
        return 0;
    });
    return rc ? "null" : r.done();
}

struct Checks {
    std::string s = "{";
    void add(const char* name, const char* why) {
        s += std::string(s.size() > 1 ? ", " : "") + "\"" + name + "\": " + (why ? "\"" + std::string(why) + "\"" : "null");
    }
};

int main(int argc, char** argv) {
    std::vector<uint64_t> words;
    if (argc > 1) {
        FILE* fp = fopen(argv[1], "rb");
        if (!fp) {
            fprintf(stderr, "cannot read %s\n", argv[1]);
            return 1;
        }
        uint64_t x;
        while (fread(&x, 8, 1, fp) == 1) words.push_back(x);
        fclose(fp);
    }
    std::string o = "{\"MK_CHUNK_BYTES\": " + num((int64_t)MK_CHUNK_BYTES) + ", ";
    Rows jobs;
    for (const uint64_t* w = words.data(); w < words.data() + words.size();) jobs.add(job(w));
    o += "\"jobs\": " + jobs.done() + ", ";

    Rows sp;
    for (uint64_t bound : {1ull, 50ull, 63ull, 64ull, 65ull, 1000ull})
        for (uint64_t n : {1ull, 63ull, 64ull, 65ull, 1000ull, 1025ull})
            sp.add("[" + num(bound) + ", " + num(n) + ", " + num(verdict_chunk(bound)) + ", " + spans(n, verdict_chunk(bound)) +
                   ", " + spans(n, bound) + "]");
    o += "\"spans\": " + sp.done() + ", ";
    // a body's refusal ends the walk and is returned
    int calls = 0;
    const int rc = for_each_span(1000, 64, [&](uint64_t c0, uint64_t) { return ++calls, c0 == 128 ? -7 : 0; });
    int chunks = 0;
    const int rc2 = for_each_append_chunk(5, 1000, 64, nullptr, 0, [&](const MkChunk& c) { return ++chunks, c.c0 == 128 ? -9 : 0; });
    o += "\"stops\": " + list({rc, calls, rc2, chunks}) + ", ";

    Checks k;
    const uint64_t B48 = 1ull << 48, B32 = 1ull << 32;
    k.add("sizes_below", check_sizes(B48 - 2, 1));
    k.add("sizes_sum", check_sizes(B48 - 1, 1));
    k.add("sizes_a", check_sizes(B48, 0));
    k.add("sizes_b", check_sizes(0, B48));
    k.add("sizes_a_max", check_sizes(B48 - 1, 0));
    k.add("sizes_own_wording", check_sizes(B48, 0, "the store must stay below 2^48 leaves"));
    k.add("sizes_wrap", check_sizes(~0ull, 1));
    k.add("count_below", check_count(B32 - 1, "more than 2^32 - 1 proofs"));
    k.add("count_at", check_count(B32, "more than 2^32 - 1 proofs"));

    const uint64_t good[3] = {0, 4, 8}, dec[3] = {0, 8, 4}, flat[3] = {5, 5, 5};
    const uint8_t blob[16] = {0};
    k.add("host_ok", check_append_host(0, nullptr, blob, good, 2));
    k.add("host_sizes", check_append_host(B48 - 1, blob, blob, good, 2));
    k.add("host_sizes_before_frontier", check_append_host(B48, nullptr, blob, good, 0));
    k.add("host_frontier", check_append_host(5, nullptr, blob, good, 2));
    k.add("host_frontier_given", check_append_host(5, blob, blob, good, 2));
    k.add("host_null_offsets", check_append_host(0, nullptr, blob, nullptr, 2));
    k.add("host_no_leaves_no_offsets", check_append_host(0, nullptr, nullptr, nullptr, 0));
    k.add("host_decreasing", check_append_host(0, nullptr, blob, dec, 2));
    k.add("host_null_data", check_append_host(0, nullptr, nullptr, good, 2));
    k.add("host_null_data_empty_records", check_append_host(0, nullptr, nullptr, flat, 2));
    k.add("host_offsets_before_data", check_append_host(0, nullptr, nullptr, dec, 2));
    k.add("dev_ok", check_append_device(0, nullptr, blob, good, 2));
    k.add("dev_sizes", check_append_device(B48, blob, blob, good, 0));
    k.add("dev_frontier", check_append_device(5, nullptr, blob, good, 2));
    k.add("dev_null_data", check_append_device(0, nullptr, nullptr, good, 2));
    k.add("dev_null_off", check_append_device(0, nullptr, blob, nullptr, 2));
    k.add("dev_no_leaves", check_append_device(5, blob, nullptr, nullptr, 0));

    PvMerkleOut out{};
    uint8_t h[32];
    uint64_t po[3];
    k.add("out_null", check_out(nullptr));
    k.add("out_empty", check_out(&out));
    out.path = h;
    k.add("out_path_alone", check_out(&out));
    out.path_off = po;
    k.add("out_pair", check_out(&out));
    out.path = nullptr;
    k.add("out_path_off_alone", check_out(&out));

    k.add("poff_ok", check_proof_offsets(blob, good, 2));
    k.add("poff_decreasing", check_proof_offsets(blob, dec, 2));
    k.add("poff_null_proof", check_proof_offsets(nullptr, good, 2));
    k.add("poff_null_proof_no_hashes", check_proof_offsets(nullptr, flat, 2));

    const uint64_t e_ok[2] = {11, 13}, e_first[2] = {10, 13}, e_eq[2] = {12, 12}, e_dec[2] = {13, 12}, e_past[2] = {11, 14},
                   e_one[1] = {13};
    k.add("ends_ok", check_reply_ends(e_ok, 2, 10, 3));
    k.add("ends_at_tree_size", check_reply_ends(e_first, 2, 10, 3));
    k.add("ends_equal", check_reply_ends(e_eq, 2, 10, 3));
    k.add("ends_decreasing", check_reply_ends(e_dec, 2, 10, 3));
    k.add("ends_past", check_reply_ends(e_past, 2, 10, 3));
    k.add("ends_one_last", check_reply_ends(e_one, 1, 10, 3));
    k.add("ends_one_past", check_reply_ends(e_one, 1, 10, 2));

    alignas(16) uint8_t a[48];
    k.add("aligned_0_16_null", check_aligned({a, a + 16, nullptr, a + 32}));
    k.add("aligned_8", check_aligned({a, a + 8}));
    k.add("aligned_8_first", check_aligned({a + 8, a}));
    k.add("aligned_1", check_aligned({a + 1}));
    k.add("aligned_none", check_aligned({}));
    PvMerkleOut d{};
    d.leaf_hash = a, d.node_hash = a + 16, d.root = a + 32;
    k.add("append_aligned", check_append_aligned(a, d));
    k.add("append_frontier_8", check_append_aligned(a + 8, d));
    int field = 0;
    for (uint8_t** f : {&d.leaf_hash, &d.node_hash, &d.frontier, &d.root, &d.roots, &d.path}) {
        uint8_t* keep = *f;
        *f = a + 8;
        k.add(("append_out_8_" + num(field++)).c_str(), check_append_aligned(a, d));
        *f = keep;
    }
    d.path_off = reinterpret_cast<uint64_t*>(a + 8);  // offsets are 8-byte words: not a hash array
    k.add("append_path_off_8", check_append_aligned(a, d));
    o += "\"checks\": " + k.s + "}}";
    printf("%s\n", o.c_str());
    return 0;
}
