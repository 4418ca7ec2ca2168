// TEST INFRASTRUCTURE: host-compiled build of the radix-2^11 rows of a resident comb table
// (indy-plenum_amd/csrc/comb.h PV_KR_*: pv_kr_base, pv_kr_build_run, the code pv_dir_widen_kernel runs per
// (position, run); sc25519.h sc_recode_w_packed) with PV_BOUNDS_CHECK: the digits, the bases read from the
// radix-256 table, the rows against an independent double-and-add, and [S]B + [k](-A) through the niels
// loop (pv_comb_b_acc_w with 16 + 23 positions) against libsodium. Not part of the product library.
// With -DWC_MAIN it is a stand-alone program (for a sanitizer build): it builds the rows of a few fixed
// keys, checks a sample of entries and digits, and exits 0 when they agree.
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
struct HostCombRow {  // [129][40], cached form; the in-place conversion's view of the same row
    uint32_t* r;
    void store(int d, const ge_cached& c) const { ge_cached_store_words(r + 40 * d, c); }
    void load(int d, ge_cached& c) const { ge_cached_load_words(c, r + 40 * d); }
    void load_z2(int d, fe& z) const { memcpy(z.v, r + 40 * d + 20, 40); }
    void store_affine(int d, const fe& ypx, const fe& ymx, const fe& xy2d) const {
        uint32_t* e = r + 40 * d;
        memcpy(e, ypx.v, 40);
        memcpy(e + 10, ymx.v, 40);
        memset(e + 20, 0, 40);
        memcpy(e + 30, xy2d.v, 40);
    }
};
struct HostScr {
    fe* z;
    void store(int k, const fe& f) const { z[k] = f; }
    void load(int k, fe& f) const { f = z[k]; }
};
struct HostMsg {
    const uint8_t* sm;
    uint64_t operator()(uint64_t q) const { uint64_t v; memcpy(&v, sm + 8 * q, 8); return v; }
};

// a key's radix-256 table as the engine builds it, then (affine) converted in place as pv_dir_affine_kernel does
void build_table(std::vector<uint32_t>& ctab, const ge_p3& negA, bool affine) {
    std::vector<ge_p3> bases(PV_COMB_POS * PV_COMB_PTS);
    pv_comb_chain(HostBases{bases.data()}, negA);
    ctab.assign((size_t)PV_COMB_POS * PV_COMB_ENT * 40, 0u);
    for (int pos = 0; pos < PV_COMB_POS; pos++)
        for (int b = 0; b < PV_COMB_BLOCKS; b++)
            pv_comb_fill_block(HostCombRow{ctab.data() + (size_t)pos * PV_COMB_ENT * 40},
                               HostBasePts{bases.data() + pos * PV_COMB_PTS}, b);
    if (!affine) return;
    fe scr[PV_AFF_SEG];
    for (int pos = 0; pos < PV_COMB_POS; pos++)
        for (int seg = 0; seg < PV_AFF_SEGS; seg++) {
            const int d0 = seg * PV_AFF_SEG, d1 = d0 + PV_AFF_SEG < PV_COMB_ENT ? d0 + PV_AFF_SEG : PV_COMB_ENT;
            pv_comb_row_to_affine_inplace(HostCombRow{ctab.data() + (size_t)pos * PV_COMB_ENT * 40}, HostScr{scr}, d0,
                                          d1);
        }
}

// the base of position q as the widening kernel reads it
void table_base(ge_p3& P, const std::vector<uint32_t>& ctab, int q, bool affine) {
    pv_kr_base(P, ctab.data() + ((size_t)pv_kr_base_row(q) * PV_COMB_ENT + pv_kr_base_ent(q)) * 40, affine);
}

// The wide rows [23][1025][32] by the product's routine, one run after another (one thread each on the device).
struct HostWideRow {
    uint32_t* r;
    size_t words;  // of the row, for the bound below
    uint32_t* e(uint32_t d) const {
        if ((size_t)(d + 1) * PV_BCOMB_STRIDE > words) abort();
        return r + (size_t)d * PV_BCOMB_STRIDE;
    }
};
struct HostWideScr {  // the products of the run in flight, indexed as DevWideScr does
    fe* z;
    void store(uint32_t d, const fe& f) const { z[(d - 1u) % PV_KR_RUN] = f; }
    void load(uint32_t d, fe& f) const { f = z[(d - 1u) % PV_KR_RUN]; }
};
void build_wide(std::vector<uint32_t>& wide, const std::vector<uint32_t>& atab) {
    const size_t row_words = (size_t)PV_KR_ENT * PV_BCOMB_STRIDE;
    wide.assign((size_t)PV_KR_POS * row_words, 0xA5A5A5A5u);  // every word must be written
    fe scr[PV_KR_RUN];
    for (int q = 0; q < PV_KR_POS; q++) {
        ge_p3 P;
        table_base(P, atab, q, true);
        for (uint32_t r = 0; r < PV_KR_RUNS; r++)
            pv_kr_build_run(HostWideRow{wide.data() + (size_t)q * row_words, row_words}, HostWideScr{scr}, P, r);
    }
}

void dbl(ge_p3& P) {
    ge_p1p1 t;
    ge_p2_dbl(t, P.X, P.Y, P.Z);
    ge_p1p1_to_p3(P, t);
}
// [d 2^(11 q)] P by plain doublings and a left-to-right double-and-add, nothing of the comb code
void ref_multiple(ge_p3& out, const ge_p3& P0, int q, uint32_t d) {
    ge_p3 P = P0;
    for (int i = 0; i < PV_KR_W * q; i++) dbl(P);
    ge_cached cP;
    ge_p3_to_cached(cP, P);
    ge_p3_identity(out);
    for (int b = 31; b >= 0; b--) {
        dbl(out);
        if ((d >> b) & 1u) {
            ge_p1p1 t;
            ge_add_cached(t, out, cP);
            ge_p1p1_to_p3(out, t);
        }
    }
}
// the affine niels entry of a point, canonical limbs, words 30 and 31 zero
void ref_entry(uint32_t e[PV_BCOMB_STRIDE], const ge_p3& P) {
    fe zi, x, y, t, d2, o;
    fe_invert(zi, P.Z);
    fe_mul(x, P.X, zi);
    fe_mul(y, P.Y, zi);
    fe_add(t, y, x);
    fe_canonical(o, t);
    memcpy(e, o.v, 40);
    fe_sub(t, y, x);
    fe_canonical(o, t);
    memcpy(e + 10, o.v, 40);
    fe_const(d2, PV_D2);
    fe_mul(t, x, y);
    fe_mul(t, t, d2);
    fe_canonical(o, t);
    memcpy(e + 20, o.v, 40);
    e[30] = e[31] = 0;
}

bool same_point(const ge_p3& a, const ge_p3& b) {
    uint32_t sa[8], sb[8];
    ge_p2_tobytes(sa, a.X, a.Y, a.Z);
    ge_p2_tobytes(sb, b.X, b.Y, b.Z);
    return memcmp(sa, sb, 32) == 0;
}

void digits_of(int16_t out[PV_KR_POS], const uint32_t k[8]) {
    uint32_t w[PV_KR_WORDS];
    sc_recode_w_packed<PV_KR_W, PV_KR_POS>(w, k);
    for (int q = 0; q < PV_KR_POS; q++) out[q] = (int16_t)pv_kr_digit(w[q >> 1], q);
}

struct HostBRow {
    const uint32_t* r;
    void load_part(int d, int part, uint32_t w[20]) const { memcpy(w, r + (size_t)d * PV_BCOMB_STRIDE + 20 * part, part ? 40 : 80); }
};
// the loop's rows as DevBWStage maps them: positions below 23 the key's wide rows, the rest the fixed base's
struct HostBWRows {
    const uint32_t* bcomb;
    const uint32_t* wide;
    HostBRow row(int j) const {
        if (j < PV_KR_POS) return HostBRow{wide + (size_t)j * PV_KR_ENT * PV_BCOMB_STRIDE};
        return HostBRow{bcomb + (size_t)(j - PV_KR_POS) * PV_BCOMB_ENT * PV_BCOMB_STRIDE};
    }
};

#ifndef WC_MAIN
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

// the 23 signed digits of a 32-byte scalar
void wc_digits(const uint8_t* k32, int16_t* out) {
    uint32_t k[8];
    memcpy(k, k32, 32);
    digits_of(out, k);
}

// positions whose base, read from the key's radix-256 table (affine: converted in place; else cached
// form), differs from [2^(11 q)](-A) by plain doublings; -1: the key fails libsodium's key checks
int wc_base_mismatches(const uint8_t* pk, int affine) {
    uint32_t A[8];
    memcpy(A, pk, 32);
    ge_p3 negA;
    if (!pv_key_ok_negate(negA, A)) return -1;
    std::vector<uint32_t> tab;
    build_table(tab, negA, affine != 0);
    int bad = 0;
    ge_p3 ref = negA;
    for (int q = 0; q < PV_KR_POS; q++) {
        ge_p3 P;
        table_base(P, tab, q, affine != 0);
        fe xy, zt;  // an extended point: X Y = Z T
        fe_mul(xy, P.X, P.Y);
        fe_mul(zt, P.Z, P.T);
        fe cx, cz;
        fe_canonical(cx, xy);
        fe_canonical(cz, zt);
        bad += !same_point(P, ref) || memcmp(cx.v, cz.v, 40) != 0;
        for (int i = 0; i < PV_KR_W; i++) dbl(ref);
    }
    return bad;
}

// The rows built by the product's routine from the in-place-affine table: of the n entries (qs[i], ds[i]),
// those that differ in any of their 32 words from the reference entry; plus, over the WHOLE table, entries
// with a nonzero word 30 or 31 or a word the builder did not write. -1: the key fails the checks and is refused.
int wc_row_mismatches(const uint8_t* pk, const int32_t* qs, const int32_t* ds, int n) {
    uint32_t A[8];
    memcpy(A, pk, 32);
    ge_p3 negA;
    if (!pv_key_ok_negate(negA, A)) return -1;
    std::vector<uint32_t> atab, wide;
    build_table(atab, negA, true);
    build_wide(wide, atab);
    int bad = 0;
    for (size_t e = 0; e < (size_t)PV_KR_POS * PV_KR_ENT; e++) {
        const uint32_t* w = wide.data() + e * PV_BCOMB_STRIDE;
        bool unwritten = false;
        for (int i = 0; i < 30; i++) unwritten |= w[i] == 0xA5A5A5A5u;  // a limb is below 2^26
        bad += unwritten || w[30] != 0 || w[31] != 0;
    }
    for (int i = 0; i < n; i++) {
        if (qs[i] < 0 || qs[i] >= PV_KR_POS || ds[i] < 0 || (uint32_t)ds[i] >= PV_KR_ENT) return -2;
        ge_p3 R;
        ref_multiple(R, negA, qs[i], (uint32_t)ds[i]);
        uint32_t want[PV_BCOMB_STRIDE];
        ref_entry(want, R);
        bad += memcmp(want, wide.data() + ((size_t)qs[i] * PV_KR_ENT + ds[i]) * PV_BCOMB_STRIDE, sizeof(want)) != 0;
    }
    return bad;
}

#ifndef WC_MAIN  // the stand-alone program checks digits, bases and rows alone
// crypto_sign_open with [S]B + [k](-A) in ONE niels loop of 16 + 23 positions (pv_comb_b_acc_w, the loop the
// comb kernels run for a key read from its wide rows). A key that fails the checks is never widened and
// its verdict is 0 through the key flag.
int wc_sign_open_wide(const uint8_t* sm, uint64_t smlen, const uint8_t* pk) {
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
    if (!pv_key_ok_negate(negA, in.A)) return 0;
    uint32_t k[8];
    pv_hash_k(k, in, smlen, mw);
    std::vector<uint32_t> atab, wide;
    build_table(atab, negA, true);
    build_wide(wide, atab);
    uint32_t kd[PV_KR_WORDS];
    sc_recode_w_packed<PV_KR_W, PV_KR_POS>(kd, k);
    int32_t fb[16];
    sc_recode_w<16, 16>(fb, in.S);
    HostBWRows rows{bcomb.data(), wide.data()};
    ge_p3 acc;
    pv_comb_b_acc_w<16>(
        acc, PvRowsStageB<HostBWRows>{rows, 0, 0},
        [&](int j) { return j < PV_KR_POS ? pv_kr_digit(kd[j >> 1], j) : (int)fb[j - PV_KR_POS]; }, 16 + PV_KR_POS);
    fe X[PV_ENC_BATCH], Y[PV_ENC_BATCH], Z[PV_ENC_BATCH];
    bool use[PV_ENC_BATCH];
    X[0] = acc.X;
    Y[0] = acc.Y;
    Z[0] = acc.Z;
    use[0] = ok;
    for (int t = 1; t < PV_ENC_BATCH; t++) { X[t] = X[0]; Y[t] = Y[0]; Z[t] = Z[0]; use[t] = false; }
    uint32_t enc[PV_ENC_BATCH][8];
    pv_encode_batch(enc, X, Y, Z, use);
    return use[0] && pv_words_equal(enc[0], in.R);
}
#endif

}  // extern "C"

#ifdef WC_MAIN
int main() {
    // keys: the base point, then the first few y = 2, 3, ... that decompress to a point passing the checks
    int done = 0, bad = 0;
    uint8_t pk[32];
    memcpy(pk, PV_B_ENC, 32);
    const int32_t qs[] = {0, 0, 0, 1, 7, 11, 22, 22, 22, 15}, ds[] = {0, 1, 1024, 64, 65, 1023, 0, 1, 1024, 513};
    for (uint32_t y = 2; done < 2; y++) {
        const int b0 = wc_base_mismatches(pk, 0), b1 = b0 < 0 ? -1 : wc_base_mismatches(pk, 1);
        if (b0 >= 0) {
            const int r = wc_row_mismatches(pk, qs, ds, 10);
            printf("key %d: %d %d mismatching bases, %d mismatching entries\n", done, b0, b1, r);
            bad += b0 + b1 + r;
            done++;
        }
        memset(pk, 0, 32);
        memcpy(pk, &y, 4);
    }
    // digits: sum d_q 2^(11 q) = k over a 64-bit window walk, for L - 1 and a few patterns
    const uint8_t Lm1[32] = {0xec, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14,
                             0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x10};
    uint8_t ks[4][32];
    memcpy(ks[0], Lm1, 32);
    memset(ks[1], 0, 32);
    memset(ks[2], 0xFF, 32);
    ks[2][31] = 0x0F;  // 2^252 - 1
    memset(ks[3], 0, 32);
    ks[3][31] = 0x10;  // 2^252
    for (int t = 0; t < 4; t++) {
        int16_t d[PV_KR_POS];
        wc_digits(ks[t], d);
        // sum d_q 2^(11 q) in 32-bit words with signed carries
        long long w[10] = {0};
        for (int q = 0; q < PV_KR_POS; q++) {
            w[(PV_KR_W * q) >> 5] += (long long)d[q] * (1LL << ((PV_KR_W * q) & 31));
            if (d[q] > 1024 || d[q] < -1024) bad++;
        }
        bool same = d[PV_KR_POS - 1] >= 0;
        for (int i = 0; i < 9; i++) {
            const long long c = w[i] >> 32;  // floor
            w[i] -= c * (1LL << 32);
            w[i + 1] += c;
            uint32_t kw = 0;
            if (i < 8) memcpy(&kw, ks[t] + 4 * i, 4);
            same &= (uint32_t)w[i] == kw;
        }
        if (!same) {
            printf("digits of scalar %d do not re-assemble\n", t);
            bad++;
        }
    }
    printf("%s\n", bad ? "FAILED" : "all checks passed");
    return bad ? 1 : 0;
}
#endif
