// CPU check of the launch plan (csrc/chunk_plan.h, the header the library compiles): the batch plan, the
// chunk plan and the wide pool's trigger. Prints one JSON object for tests/test_chunk_plan.py:
//   constants  the thresholds the rules read, as compiled
//   scenarios  named inputs whose expected plan the Python file states by hand, every field of the plan
//   wide_run   the dense-chunk counter and the attempt over five dense chunks, a failed attempt, two more
//   wide       the trigger over a small product of its inputs
// and writes the sweep to the file named by argv[1]: one row of SWEEP_WORDS uint32 per combination of the
// inputs (words 0..5 the inputs, the rest every output of plan_batch and plan_chunk, the zero-copy gate's
// answer among them), bools packed into bit words in the order of IN_BITS / OUT_BITS in the Python file.
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../indy-plenum_amd/csrc/chunk_plan.h"

using namespace pvhost;

static ChunkFacts default_facts(uint64_t m) {
    ChunkFacts f{};
    f.m = m;
    f.path = PV_PATH_AUTO;
    f.kc_wcap = 1024;
    f.dir_on = true;
    f.dir_cap = PV_KEY_CAP - PV_ALLCOMB_KEYS;
    f.aff_on = true;
    f.wide_cap = 2048;
    f.wide_have = 2048;
    f.kcap = PV_KEY_CAP;
    f.cus = 256;
    return f;
}

static std::string kv(const char* k, uint64_t v, bool last = false) {
    return std::string("\"") + k + "\": " + std::to_string(v) + (last ? "" : ", ");
}
static std::string plan_json(const BatchPlan& b, const ChunkPlan& p) {
    std::string s = "{";
    s += kv("latency", b.latency) + kv("dev_choice", b.dev_choice) + kv("keyed", p.keyed) + kv("lookup", p.lookup);
    s += kv("min_req", p.min_req) + kv("kc_on", p.kc_on) + kv("kc_wcap", p.kc_wcap) + kv("dir_on", p.dir_on);
    s += kv("dir_cap", p.dir_cap) + kv("dir_pub", p.dir_pub) + kv("aff_conv", p.aff_conv) + kv("wide_cap", p.wide_cap);
    s += kv("wide_conv", p.wide_conv) + kv("chunk_n", p.chunk_n) + kv("seg_cap", p.seg_cap);
    s += kv("lat_choice", p.lat_choice) + kv("dense_only", p.dense_only) + kv("kcap", p.kcap);
    s += kv("dir_use", p.dir_use) + kv("direct_fill", p.direct_fill) + kv("fused", p.fused);
    s += kv("seed_reqs", p.seed_reqs) + kv("enc16", p.enc16) + kv("req_grid", p.req_grid) + kv("ins_grid", p.ins_grid);
    s += kv("probe_grid", p.probe_grid) + kv("chain_blocks", p.chain_blocks) + kv("fill_grid", p.fill_grid);
    s += kv("side_grid", p.side_grid) + kv("enc_grid", p.enc_grid) + kv("pub_grid", p.pub_grid);
    s += kv("clear_slots", p.clear_slots) + kv("clear_dir", p.clear_dir) + kv("mark_dir_dirty", p.mark_dir_dirty);
    s += kv("run_probe", p.run_probe) + kv("run_xtab_publish", p.run_xtab_publish);
    s += kv("run_dir_publish", p.run_dir_publish) + kv("run_affine", p.run_affine) + kv("run_widen", p.run_widen);
    s += kv("run_dev_latency", p.run_dev_latency, true);
    return s + "}";
}
// one call of n requests whose chunk under test has f.m of them
static std::string scenario(const char* name, uint64_t n, bool hint_set, bool kc_active, const ChunkFacts& f) {
    const BatchPlan b = plan_batch({f.path, n, hint_set, f.keyed_hint, kc_active});
    return std::string("\"") + name + "\": " + plan_json(b, plan_chunk(b, f));
}

static constexpr int SWEEP_WORDS = 24;
static void sweep_row(std::vector<uint32_t>& out, int path, bool hint_set, bool keyed_hint, bool cache, bool xt_fill,
                      bool xt_use, bool dir_on, bool aff_on, uint32_t wide_cap, uint32_t pool, int cus, uint64_t m,
                      uint64_t n, bool slots_dirty, bool dir_dirty) {
    ChunkFacts f = default_facts(m);
    f.path = path;
    f.keyed_hint = keyed_hint;
    f.node_kc = cache;
    f.xt_fill = xt_fill;
    f.xt_use = xt_use;
    f.dir_on = dir_on;
    f.aff_on = aff_on;
    f.wide_cap = wide_cap;
    f.wide_have = pool;
    f.cus = cus;
    f.slots_dirty = slots_dirty;
    f.dir_dirty = dir_dirty;
    const BatchPlan b = plan_batch({path, n, hint_set, keyed_hint, cache});
    const ChunkPlan p = plan_chunk(b, f);
    // the zero-copy gate of pv_verify_batch: a host-buffer call with the hint it counted
    const bool gate = plan_batch({path, n, true, keyed_hint, cache}).latency;
    const bool in_bits[] = {hint_set, keyed_hint, cache, xt_fill, xt_use, dir_on, aff_on, slots_dirty, dir_dirty};
    const bool out_bits[] = {b.latency,      b.dev_choice,     gate,           p.keyed,           p.kc_on != 0,
                             p.dir_on != 0,  p.dir_pub != 0,   p.aff_conv != 0, p.wide_conv != 0,  p.lat_choice != 0,
                             p.dense_only != 0, p.dir_use,     p.direct_fill,  p.fused,           p.enc16,
                             p.clear_slots,  p.clear_dir,      p.mark_dir_dirty, p.run_probe,     p.run_xtab_publish,
                             p.run_dir_publish, p.run_affine,  p.run_widen,    p.run_dev_latency};
    uint32_t ib = 0, ob = 0;
    for (size_t i = 0; i < sizeof(in_bits); i++) ib |= (uint32_t)in_bits[i] << i;
    for (size_t i = 0; i < sizeof(out_bits); i++) ob |= (uint32_t)out_bits[i] << i;
    // every 0/1 scalar of the plan is 0 or 1 exactly
    const uint32_t flags01[] = {p.kc_on, p.dir_on, p.dir_pub, p.aff_conv, p.wide_conv, p.lat_choice, p.dense_only};
    for (uint32_t v : flags01)
        if (v > 1) ob |= 1u << 31;
    const uint32_t row[SWEEP_WORDS] = {
        ib | (uint32_t)path << 16, wide_cap, pool, (uint32_t)cus, (uint32_t)m, (uint32_t)n,
        ob, (uint32_t)p.lookup, p.min_req, p.kc_wcap, p.dir_cap, p.wide_cap, p.chunk_n, p.seg_cap, p.kcap,
        (uint32_t)p.seed_reqs, p.req_grid, p.ins_grid, p.probe_grid, p.chain_blocks, p.fill_grid, p.side_grid,
        p.enc_grid, p.pub_grid};
    out.insert(out.end(), row, row + SWEEP_WORDS);
}

int main(int argc, char** argv) {
    std::string o = "{";
    o += "\"constants\": {" + kv("PV_LATENCY_MAX", PV_LATENCY_MAX) + kv("PV_KEYED_HINT_MIN", PV_KEYED_HINT_MIN) +
         kv("PV_KEYED_MIN", PV_KEYED_MIN) + kv("PV_ALLCOMB_KEYS", PV_ALLCOMB_KEYS) + kv("PV_XT_KEYS", PV_XT_KEYS) +
         kv("PV_KEY_CAP", PV_KEY_CAP) + kv("PV_NSEG", PV_NSEG) + kv("PV_COMB_MIN_REQ", PV_COMB_MIN_REQ) +
         kv("PV_SPARSE_CHUNK", PV_SPARSE_CHUNK) + kv("PV_FUSED_MIN_REQ", PV_FUSED_MIN_REQ) +
         kv("PV_KEY_SEED", PV_KEY_SEED) + kv("PV_SIDE_GRID_PER_CU", PV_SIDE_GRID_PER_CU) +
         kv("PV_LP_CHAIN_BLOCKS", PV_LP_CHAIN_BLOCKS) + kv("PV_ENC_SMALL_B", PV_ENC_SMALL_B) +
         kv("PV_ENC16_MIN", PV_ENC16_MIN) + kv("PV_INS_REQS", PV_INS_REQS) + kv("PV_BLOCK", PV_BLOCK) +
         kv("PV_FILL_ITEMS_PER_KEY", PV_FILL_ITEMS_PER_KEY, true) + "}, ";

    o += "\"scenarios\": {";
    const uint64_t M = 1ull << 20;
    o += scenario("headline", M, false, false, default_facts(M)) + ", ";
    {
        ChunkFacts f = default_facts(3072);
        f.keyed_hint = true;
        o += scenario("host_3072_keyed_hint", 3072, true, false, f) + ", ";
    }
    o += scenario("device_3072_empty_cache", 3072, false, false, default_facts(3072)) + ", ";
    {
        ChunkFacts f = default_facts(3072);
        f.node_kc = true;
        o += scenario("device_3072_cache", 3072, false, true, f) + ", ";
    }
    {
        ChunkFacts f = default_facts(262144);
        f.xt_fill = true;
        o += scenario("pipelined_sub0", 262144, true, false, f) + ", ";
        f.xt_fill = false;
        f.xt_use = true;
        o += scenario("pipelined_later", 262144, true, false, f) + ", ";
        f.node_kc = true;
        o += scenario("pipelined_later_node_cache", 262144, true, true, f) + ", ";
    }
    {
        ChunkFacts f = default_facts(1);
        f.path = PV_PATH_COMB;
        o += scenario("forced_comb_1", 1, false, false, f) + ", ";
        f = default_facts(M);
        f.path = PV_PATH_STRAUS;
        o += scenario("forced_straus_1m", M, false, false, f) + ", ";
        f.path = PV_PATH_LATENCY;
        o += scenario("forced_latency_1m", M, false, false, f);
    }
    o += "}, ";

    // five dense chunks with no pool yet, the fourth's attempt failing; then two more dense chunks
    o += "\"wide_run\": [";
    {
        uint32_t dense = 0;
        bool failed = false;
        const uint64_t want = 2048ull * 3017600;
        for (int i = 0; i < 7; i++) {
            const WideTrigger t = plan_wide_pool(true, true, failed, 0, want, dense);
            dense = t.dense;
            if (t.attempt) failed = true;
            o += std::string(i ? ", " : "") + "[" + std::to_string(t.attempt) + ", " + std::to_string(t.dense) + "]";
        }
    }
    o += "], \"wide\": [";
    {
        const uint64_t sizes[][2] = {{0, 0}, {0, 8}, {4, 8}, {8, 8}, {16, 8}};
        const uint32_t counts[] = {0, 1, 2, 3, 4, 0xFFFFFFFFu};
        bool first = true;
        for (int keyed = 0; keyed < 2; keyed++)
            for (int pub = 0; pub < 2; pub++)
                for (int failed = 0; failed < 2; failed++)
                    for (const auto& sz : sizes)
                        for (uint32_t dense : counts) {
                            const WideTrigger t = plan_wide_pool(keyed, pub, failed, sz[0], sz[1], dense);
                            o += std::string(first ? "" : ", ") + "[" + std::to_string(keyed) + ", " +
                                 std::to_string(pub) + ", " + std::to_string(failed) + ", " + std::to_string(sz[0]) +
                                 ", " + std::to_string(sz[1]) + ", " + std::to_string(dense) + ", " +
                                 std::to_string(t.attempt) + ", " + std::to_string(t.dense) + "]";
                            first = false;
                        }
    }
    o += "], ";

    std::vector<uint32_t> rows;
    const int paths[] = {PV_PATH_AUTO, PV_PATH_STRAUS, PV_PATH_COMB, PV_PATH_LATENCY};
    const bool xts[][2] = {{false, false}, {true, false}, {false, true}};  // (xt_fill, xt_use)
    const uint32_t wide_caps[] = {0, 1, 2048}, pools[] = {0, 1, 2048, 4096};
    const int cuss[] = {0, 1, 256};
    const uint64_t ms[] = {1, 63, 64, 65, 2048, 2049, 4096, 4097, 65536, 65537, 262144, 262145, M};
    uint32_t count = 0;
    for (int path : paths)
        for (int hint_set = 0; hint_set < 2; hint_set++)
            for (int keyed_hint = 0; keyed_hint < 2; keyed_hint++)
                for (int cache = 0; cache < 2; cache++)
                    for (const auto& xt : xts)
                        for (int dir_on = 0; dir_on < 2; dir_on++)
                            for (int aff_on = 0; aff_on < 2; aff_on++)
                                for (uint32_t wide_cap : wide_caps)
                                    for (uint32_t pool : pools)
                                        for (int cus : cuss)
                                            for (uint64_t m : ms)
                                                for (int two = 0; two < 2; two++) {
                                                    // the dirty flags: the four pairs in turn, one per (cus, m)
                                                    const uint32_t k = count++ / 2;
                                                    sweep_row(rows, path, hint_set, keyed_hint, cache, xt[0], xt[1],
                                                              dir_on, aff_on, wide_cap, pool, cus, m, two ? M + m : m,
                                                              k & 1, (k >> 1) & 1);
                                                }
    o += kv("sweep_words", SWEEP_WORDS) + kv("sweep_rows", rows.size() / SWEEP_WORDS, true) + "}";
    if (argc > 1) {
        FILE* fp = fopen(argv[1], "wb");
        if (!fp || fwrite(rows.data(), 4, rows.size(), fp) != rows.size() || fclose(fp) != 0) {
            fprintf(stderr, "cannot write %s\n", argv[1]);
            return 1;
        }
    }
    printf("%s\n", o.c_str());
    return 0;
}
