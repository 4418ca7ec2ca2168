// TEST INFRASTRUCTURE: host-compiled build of the in-place affine-row conversion of a resident comb
// table (indy-plenum_amd/csrc/comb.h pv_comb_row_to_affine_inplace, the code pv_dir_affine_kernel
// runs) with PV_BOUNDS_CHECK, against the out-of-place pv_comb_row_to_affine and, through the affine
// mode of pv_comb_a_xyz_staged, against libsodium. Not part of the product library.
// With -DAC_MAIN it is a stand-alone program (for a sanitizer build): it converts the tables of a few
// fixed keys both ways and exits 0 when they agree.
#define PV_BOUNDS_CHECK 1
#include "verify_core.h"
#include "btable.h"
#include "comb.h"
#include <stdio.h>
#include <string.h>
#include <thread>
#include <vector>

namespace {

struct HostBases {
    ge_p3* b;  // [32][PV_COMB_PTS]
    void store(int i, int m, const ge_p3& p) const { b[i * PV_COMB_PTS + m] = p; }
};
struct HostBasePts {
    const ge_p3* b;
    void load(int m, ge_p3& p) const { p = b[m]; }
};
struct HostCombRow {  // [129][40], cached form
    uint32_t* r;
    void store(int d, const ge_cached& c) const { ge_cached_store_words(r + 40 * d, c); }
    void load(int d, ge_cached& c) const { ge_cached_load_words(c, r + 40 * d); }
    void load_half(int d, int h, uint32_t w[20]) const { memcpy(w, r + 40 * d + 20 * h, 80); }
    // the in-place conversion's view of the same row
    void load_z2(int d, fe& z) const { memcpy(z.v, r + 40 * d + 20, 40); }
    void store_affine(int d, const fe& ypx, const fe& ymx, const fe& xy2d) const {
        uint32_t* e = r + 40 * d;
        memcpy(e, ypx.v, 40);
        memcpy(e + 10, ymx.v, 40);
        memset(e + 20, 0, 40);
        memcpy(e + 30, xy2d.v, 40);
    }
};
struct HostCombRows {
    uint32_t* base;
    HostCombRow row(int i) const { return HostCombRow{base + (size_t)i * PV_COMB_ENT * 40}; }
};
struct HostAffineRowDst {
    uint32_t* r;
    uint32_t* e(int d) const { return r + 40 * d; }
};
struct HostScr {
    fe* z;  // PV_AFF_SEG products
    void store(int k, const fe& f) const { z[k] = f; }
    void load(int k, fe& f) const { f = z[k]; }
};
struct HostBRow {
    const uint32_t* r;
    void load_part(int d, int part, uint32_t w[20]) const {
        memcpy(w, r + d * PV_BCOMB_STRIDE + 20 * part, part ? 40 : 80);
    }
};
struct HostBRows {
    const uint32_t* base;
    HostBRow row(int i) const { return HostBRow{base + (size_t)i * PV_BCOMB_ENT * PV_BCOMB_STRIDE}; }
};
struct HostMsg {
    const uint8_t* sm;
    uint64_t operator()(uint64_t q) const { uint64_t v; memcpy(&v, sm + 8 * q, 8); return v; }
};

// a key's whole table as the engine builds it: the chain, then every fill block
void build_table(std::vector<uint32_t>& ctab, const ge_p3& negA) {
    std::vector<ge_p3> bases(PV_COMB_POS * PV_COMB_PTS);
    pv_comb_chain(HostBases{bases.data()}, negA);
    ctab.assign((size_t)PV_COMB_POS * PV_COMB_ENT * 40, 0u);
    for (int pos = 0; pos < PV_COMB_POS; pos++)
        for (int b = 0; b < PV_COMB_BLOCKS; b++)
            pv_comb_fill_block(HostCombRow{ctab.data() + (size_t)pos * PV_COMB_ENT * 40},
                               HostBasePts{bases.data() + pos * PV_COMB_PTS}, b);
}

// every row in place, cut into the kernel's segments (one thread each there, one after another here)
void convert_inplace(std::vector<uint32_t>& tab) {
    fe scr[PV_AFF_SEG];
    for (int pos = 0; pos < PV_COMB_POS; pos++)
        for (int seg = 0; seg < PV_AFF_SEGS; seg++) {
            const int d0 = seg * PV_AFF_SEG, d1 = d0 + PV_AFF_SEG < PV_COMB_ENT ? d0 + PV_AFF_SEG : PV_COMB_ENT;
            pv_comb_row_to_affine_inplace(HostCombRow{tab.data() + (size_t)pos * PV_COMB_ENT * 40}, HostScr{scr}, d0,
                                          d1);
        }
}

// words that differ between the in-place table and pv_comb_row_to_affine's, plus nonzero words 20..29
int inplace_mismatches(const ge_p3& negA) {
    std::vector<uint32_t> ctab, atab;
    build_table(ctab, negA);
    atab.resize(ctab.size());
    for (int pos = 0; pos < PV_COMB_POS; pos++)
        pv_comb_row_to_affine(HostCombRow{ctab.data() + (size_t)pos * PV_COMB_ENT * 40},
                              HostAffineRowDst{atab.data() + (size_t)pos * PV_COMB_ENT * 40});
    convert_inplace(ctab);
    int bad = 0;
    for (size_t w = 0; w < ctab.size(); w++) {
        bad += ctab[w] != atab[w];
        if (w % 40 >= 20 && w % 40 < 30) bad += ctab[w] != 0;
    }
    return bad;
}

#ifndef AC_MAIN
const std::vector<uint32_t>& host_bcomb() {
    static std::vector<uint32_t> bcomb;
    if (bcomb.empty()) {
        bcomb.resize((size_t)PV_BCOMB_POS * PV_BCOMB_ENT * PV_BCOMB_STRIDE);
        ge_p3 base[PV_BCOMB_POS];
        pv_bcomb_bases(base);
        std::vector<std::thread> th;
        for (int j = 0; j < PV_BCOMB_POS; j++)
            th.emplace_back(pv_bcomb_build_position, bcomb.data() + (size_t)j * PV_BCOMB_ENT * PV_BCOMB_STRIDE,
                            std::cref(base[j]));
        for (auto& t : th) t.join();
    }
    return bcomb;
}

#endif

}  // namespace

extern "C" {

// -1: the key fails libsodium's key checks (such a table is never converted); else the mismatch count
int ac_inplace_mismatches(const uint8_t* pk) {
    uint32_t A[8];
    memcpy(A, pk, 32);
    ge_p3 negA;
    if (!pv_key_ok_negate(negA, A)) return -1;
    return inplace_mismatches(negA);
}

#ifndef AC_MAIN  // the stand-alone program runs the conversion alone
// crypto_sign_open with [k](-A) from the key's table converted IN PLACE and read in affine mode (what a
// chunk does with a promoted resident table); a key that fails the checks keeps its cached-form table,
// as in the engine, and its verdict is 0 through the key flag.
int ac_sign_open_affine_inplace(const uint8_t* sm, uint64_t smlen, const uint8_t* pk) {
    const std::vector<uint32_t>& bcomb = host_bcomb();
    std::vector<uint8_t> buf(smlen + 256, 0);  // PV_BLOB_SLACK
    memcpy(buf.data(), sm, smlen);
    pv_sig_words in;
    memcpy(in.R, buf.data(), 32);
    memcpy(in.S, buf.data() + 32, 32);
    memcpy(in.A, pk, 32);
    HostMsg mw{buf.data()};
    bool ok = pv_sig_ok(in, smlen);
    ge_p3 negA;
    const bool key_ok = pv_key_ok_negate(negA, in.A);
    ok &= key_ok;
    uint32_t k[8];
    pv_hash_k(k, in, smlen, mw);
    std::vector<uint32_t> ctab;
    build_table(ctab, negA);
    if (key_ok) convert_inplace(ctab);
    pv_dig_regs dig;
    sc_recode256(dig.e, k);
    int32_t fb[16];
    sc_recode_w<16, 16>(fb, in.S);
    HostBRows brows{bcomb.data()};
    ge_p3 acc;
    pv_comb_b_acc_w<16>(acc, PvRowsStageB<HostBRows>{brows, 0, 0}, [&](int j) { return fb[j]; });
    HostCombRows arows{ctab.data()};
    fe X[PV_ENC_BATCH], Y[PV_ENC_BATCH], Z[PV_ENC_BATCH];
    bool use[PV_ENC_BATCH];
    pv_comb_a_xyz_staged(X[0], Y[0], Z[0], acc, PvRowsStageA<HostCombRows>{arows, 0, 0, key_ok}, dig);
    use[0] = ok;
    for (int t = 1; t < PV_ENC_BATCH; t++) { X[t] = X[0]; Y[t] = Y[0]; Z[t] = Z[0]; use[t] = false; }
    uint32_t enc[PV_ENC_BATCH][8];
    pv_encode_batch(enc, X, Y, Z, use);
    return use[0] && pv_words_equal(enc[0], in.R);
}
#endif

}  // extern "C"

#ifdef AC_MAIN
int main() {
    // keys: the base point, then the first few y = 3, 4, ... that decompress to a point passing the checks
    int done = 0, bad = 0;
    uint8_t pk[32];
    memcpy(pk, PV_B_ENC, 32);
    for (uint32_t y = 2; done < 3; y++) {
        const int r = ac_inplace_mismatches(pk);
        if (r >= 0) {
            printf("key %d: %d mismatching words\n", done, r);
            bad += r;
            done++;
        }
        memset(pk, 0, 32);
        memcpy(pk, &y, 4);
    }
    return bad ? 1 : 0;
}
#endif
