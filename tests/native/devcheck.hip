// TEST INFRASTRUCTURE: the device arithmetic headers (indy-plenum_amd/csrc/*.h) compiled for gfx950
// with the product library's flags and wrapped unit by unit in small kernels, so tests can drive the
// DEVICE branches of those headers (the inline-asm product columns of fe_mul_pre / fe_sq, the DPP /
// permlane / readlane / ballot forms of lp25519.h, v_rcp_f32 and __all in the splits, the alignbit /
// bitop3 / perm forms of sha512.h) with chosen operands. Same units and vectors as
// tests/native/hostcheck.hip (tests/devarith_cases.py); no PV_BOUNDS_CHECK: the device has no
// assertions, the tests check the output bounds. Not part of the product library, no dependency on it.
//
// Every dc_* entry takes host pointers and a count, allocates device buffers, copies in, launches,
// synchronises, copies out, frees, and returns the first HIP error (0 = success).
#include "verify_core.h"
#include "btable.h"
#include "comb.h"
#include "lp25519.h"
#include <string.h>
#include <vector>

namespace {

struct DcRun {
    struct Buf { void* d; void* h; size_t n; };
    std::vector<Buf> bufs;
    int rc = 0;
    void check(hipError_t e) { if (!rc && e != hipSuccess) rc = (int)e; }
    void* alloc(size_t n) {
        void* d = nullptr;
        if (!rc) check(hipMalloc(&d, n ? n : 4));
        return rc ? nullptr : d;
    }
    template <class T> const T* in(const T* h, size_t count) {
        const size_t n = count * sizeof(T);
        void* d = alloc(n);
        if (d) { bufs.push_back({d, nullptr, n}); if (n) check(hipMemcpy(d, h, n, hipMemcpyHostToDevice)); }
        return (const T*)d;
    }
    template <class T> T* out(T* h, size_t count) {
        const size_t n = count * sizeof(T);
        void* d = alloc(n);
        if (d) { bufs.push_back({d, h, n}); if (n) check(hipMemset(d, 0, n)); }
        return (T*)d;
    }
    bool ok() const { return rc == 0; }
    int finish() {
        check(hipGetLastError());
        check(hipDeviceSynchronize());
        for (const Buf& b : bufs)
            if (b.h && b.n) check(hipMemcpy(b.h, b.d, b.n, hipMemcpyDeviceToHost));
        for (const Buf& b : bufs) {
            const hipError_t e = hipFree(b.d);
            check(e);
        }
        return rc;
    }
};

inline unsigned blocks64(int n) { return (unsigned)((n + 63) / 64); }

__device__ __forceinline__ void ld_fe(fe& a, const uint32_t* p) {
#pragma unroll
    for (int i = 0; i < 10; i++) a.v[i] = p[i];
}
__device__ __forceinline__ void st_fe(uint32_t* p, const fe& a) {
#pragma unroll
    for (int i = 0; i < 10; i++) p[i] = a.v[i];
}
__device__ __forceinline__ void ld8(uint32_t w[8], const uint32_t* p) {
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = p[i];
}
__device__ __forceinline__ void st8(uint32_t* p, const uint32_t w[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) p[i] = w[i];
}

// ------------------------------------------------------------------ per-lane kernels: set i on thread i
#define DC_LANE int i = blockIdx.x * 64 + threadIdx.x; if (i >= n) return

__global__ void __launch_bounds__(64) k_fe_mul(uint32_t* h, const uint32_t* f, const uint32_t* g, int n) {
    DC_LANE;
    fe a, b, c; ld_fe(a, f + 10 * i); ld_fe(b, g + 10 * i);
    fe_mul(c, a, b);
    st_fe(h + 10 * i, c);
}
__global__ void __launch_bounds__(64) k_fe_mul_pre(uint32_t* h, const uint32_t* f, const uint32_t* g, int n) {
    DC_LANE;
    fe a, b, c; ld_fe(a, f + 10 * i); ld_fe(b, g + 10 * i);
    uint32_t g19[10];
    fe_mul19(g19, b);
    fe_mul_pre(c, a, b, g19);
    st_fe(h + 10 * i, c);
}
__global__ void __launch_bounds__(64) k_fe_sq(uint32_t* h, const uint32_t* f, int n) {
    DC_LANE;
    fe a, c; ld_fe(a, f + 10 * i);
    fe_sq(c, a);
    st_fe(h + 10 * i, c);
}
__global__ void __launch_bounds__(64) k_fe_carry(uint32_t* h, const uint32_t* f, int n) {
    DC_LANE;
    fe a, c; ld_fe(a, f + 10 * i);
    fe_carry(c, a);
    st_fe(h + 10 * i, c);
}
__global__ void __launch_bounds__(64) k_fe_tobytes(uint32_t* s, const uint32_t* f, int n) {
    DC_LANE;
    fe a; ld_fe(a, f + 10 * i);
    uint32_t w[8];
    fe_tobytes32(w, a);
    st8(s + 8 * i, w);
}
__global__ void __launch_bounds__(64) k_fe_frombytes(uint32_t* h, const uint32_t* s, int n) {
    DC_LANE;
    uint32_t w[8]; ld8(w, s + 8 * i);
    fe a;
    fe_frombytes32(a, w);
    st_fe(h + 10 * i, a);
}
__global__ void __launch_bounds__(64) k_fe_invert(uint32_t* h, const uint32_t* f, int n) {
    DC_LANE;
    fe a, c; ld_fe(a, f + 10 * i);
    fe_invert(c, a);
    st_fe(h + 10 * i, c);
}
__global__ void __launch_bounds__(64) k_fe_pow22523(uint32_t* h, const uint32_t* f, int n) {
    DC_LANE;
    fe a, c; ld_fe(a, f + 10 * i);
    fe_pow22523(c, a);
    st_fe(h + 10 * i, c);
}
__global__ void __launch_bounds__(64) k_sc_reduce64(uint32_t* r, const uint32_t* x, int n) {
    DC_LANE;
    uint32_t xw[16], rw[8];
#pragma unroll
    for (int j = 0; j < 16; j++) xw[j] = x[16 * i + j];
    sc_reduce64(rw, xw);
    st8(r + 8 * i, rw);
}
__global__ void __launch_bounds__(64) k_sc_is_canonical(int* out, const uint32_t* s, int n) {
    DC_LANE;
    uint32_t w[8]; ld8(w, s + 8 * i);
    out[i] = sc_is_canonical(w) ? 1 : 0;
}
template <int NA>
__global__ void __launch_bounds__(64) k_sc_mul(uint32_t* r, const uint32_t* a, const uint32_t* b, int n) {
    DC_LANE;
    uint32_t aw[8], bw[8], rw[8];
    ld8(aw, a + 8 * i); ld8(bw, b + 8 * i);
    sc_mul<NA>(rw, aw, bw);
    st8(r + 8 * i, rw);
}
// radix = 16, 256 or 65536
__global__ void __launch_bounds__(64) k_sc_recode(uint32_t* out, const uint32_t* a, int radix, int n) {
    DC_LANE;
    uint32_t w[8], o[8]; ld8(w, a + 8 * i);
    if (radix == 16) sc_recode16(o, w);
    else if (radix == 256) sc_recode256(o, w);
    else sc_recode65536(o, w);
    st8(out + 8 * i, o);
}
template <int W, int P>
__global__ void __launch_bounds__(64) k_sc_recode_w(int32_t* out, const uint32_t* a, int n) {
    DC_LANE;
    uint32_t w[8]; ld8(w, a + 8 * i);
    int32_t d[P];
    sc_recode_w<W, P>(d, w);
#pragma unroll
    for (int j = 0; j < 16; j++) out[16 * i + j] = j < P ? d[j < P ? j : 0] : 0;
}
__global__ void __launch_bounds__(64) k_sc_nwin16(int* out, const uint32_t* a, int n) {
    DC_LANE;
    uint32_t w[8], e[8]; ld8(w, a + 8 * i);
    sc_recode16(e, w);
    out[i] = sc_nwin16(e);
}
// flags: [2 i] = neg, [2 i + 1] = fallback
__global__ void __launch_bounds__(64) k_sc_halfsize(uint32_t* k1, uint32_t* k2, int* flags, const uint32_t* k, int n) {
    DC_LANE;
    uint32_t kw[8]; ld8(kw, k + 8 * i);
    pv_halfk h;
    sc_halfsize(h, kw);
    st8(k1 + 8 * i, h.k1);
    st8(k2 + 8 * i, h.k2);
    flags[2 * i] = h.neg ? 1 : 0;
    flags[2 * i + 1] = h.fallback ? 1 : 0;
}
// out[2 i] = pv_has_small_order, out[2 i + 1] = pv_ge_is_canonical
__global__ void __launch_bounds__(64) k_enc_rules(int* out, const uint32_t* s, int n) {
    DC_LANE;
    uint32_t w[8]; ld8(w, s + 8 * i);
    out[2 * i] = pv_has_small_order(w) ? 1 : 0;
    out[2 * i + 1] = pv_ge_is_canonical(w) ? 1 : 0;
}
__global__ void __launch_bounds__(64) k_ge_frombytes_negate(int* ok, uint32_t* out, const uint32_t* s, int n) {
    DC_LANE;
    uint32_t w[8]; ld8(w, s + 8 * i);
    ge_p3 p;
    ok[i] = ge_frombytes_negate(p, w) ? 1 : 0;
    st_fe(out + 40 * i, p.X); st_fe(out + 40 * i + 10, p.Y); st_fe(out + 40 * i + 20, p.Z); st_fe(out + 40 * i + 30, p.T);
}
__global__ void __launch_bounds__(64) k_ge_p2_tobytes(uint32_t* s, const uint32_t* xyz, int n) {
    DC_LANE;
    fe X, Y, Z; ld_fe(X, xyz + 30 * i); ld_fe(Y, xyz + 30 * i + 10); ld_fe(Z, xyz + 30 * i + 20);
    uint32_t w[8];
    ge_p2_tobytes(w, X, Y, Z);
    st8(s + 8 * i, w);
}
// little-endian bytes 8q..8q+7 of the record, loaded byte by byte (any alignment)
struct DcMsg {
    const uint8_t* sm;
    __device__ uint64_t operator()(uint64_t q) const {
        uint64_t v = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) v |= (uint64_t)sm[8 * q + j] << (8 * j);
        return v;
    }
};
// record i = sm + i * stride (stride >= smlen[i] + 256: the slack pv_hash_k may read), pk + 32 i
__global__ void __launch_bounds__(64) k_hash_k(uint32_t* kout, const uint8_t* sm, uint64_t stride, const uint64_t* smlen,
                                               const uint32_t* pk, int n) {
    DC_LANE;
    const uint8_t* rec = sm + (size_t)i * stride;
    pv_sig_words in;
    DcMsg mw{rec};
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint64_t r = mw(q), s = mw(4 + q);
        in.R[2 * q] = (uint32_t)r; in.R[2 * q + 1] = (uint32_t)(r >> 32);
        in.S[2 * q] = (uint32_t)s; in.S[2 * q + 1] = (uint32_t)(s >> 32);
    }
    ld8(in.A, pk + 8 * i);
    uint32_t k[8];
    pv_hash_k(k, in, smlen[i], mw);
    st8(kout + 8 * i, k);
}

// ------------------------------------------------------------------ per-wave kernels: set w on block w
// Rows in lanes 16 r + k; lanes 10..15 of each row get hostcheck.hip's hc_rows_in filler. The lane
// vectors are host structs in the host pass, so the bodies are device-only.
#if LP_DEVICE
__device__ __forceinline__ lu dc_rows_in(const uint32_t* x) {
    const int l = threadIdx.x;
    return (l & 15) < 10 ? x[10 * (l >> 4) + (l & 15)] : 0x1234567u + (uint32_t)l;
}
__device__ __forceinline__ void dc_rows_out(uint32_t* x, lu v) {
    const int l = threadIdx.x;
    if ((l & 15) < 10) x[10 * (l >> 4) + (l & 15)] = v;
}
#endif

// op: 0 lp_mul, 1 lp_mul_dual, 2 lp_add_cached(p, to_cached(q)), 3 the same with q negated
__global__ void __launch_bounds__(64) k_lp_binary(uint32_t* h, const uint32_t* f, const uint32_t* g, int op) {
#if LP_DEVICE
    const int w = blockIdx.x;
    const LpLane c = LpLane::make();
    const lu a = dc_rows_in(f + 40 * w), b = dc_rows_in(g + 40 * w);
    lu r;
    if (op == 0) r = lp_mul(c, a, b);
    else if (op == 1) r = lp_mul_dual(c, a, b);
    else {
        const LpConsts K = LpConsts::make(c);
        const lu q = lp_to_cached(c, b, K.d2);
        r = lp_add_cached(c, a, op == 2 ? q : lp_neg_cached(c, q));
    }
    dc_rows_out(h + 40 * w, r);
#endif
}
// op: 0 lp_invert, 1 lp_invert<true>, 2 lp_pow22523, 3 lp_pow22523<true>, 4 lp_dbl
__global__ void __launch_bounds__(64) k_lp_unary(uint32_t* h, const uint32_t* f, int op) {
#if LP_DEVICE
    const int w = blockIdx.x;
    const LpLane c = LpLane::make();
    const lu a = dc_rows_in(f + 40 * w);
    lu r;
    if (op == 0) r = lp_invert(c, a);
    else if (op == 1) r = lp_invert<true>(c, a);
    else if (op == 2) r = lp_pow22523(c, a);
    else if (op == 3) r = lp_pow22523<true>(c, a);
    else r = lp_dbl(c, a);
    dc_rows_out(h + 40 * w, r);
#endif
}
__global__ void __launch_bounds__(64) k_lp_halfsize(uint32_t* k1, uint32_t* k2, int* flags, const uint32_t* k) {
#if LP_DEVICE
    const int w = blockIdx.x;
    uint32_t kw[8]; ld8(kw, k + 8 * w);
    const LpLane c = LpLane::make();
    pv_halfk h;
    lp_halfsize(c, h, kw);
    if (threadIdx.x == 0) {
        st8(k1 + 8 * w, h.k1);
        st8(k2 + 8 * w, h.k2);
        flags[2 * w] = h.neg ? 1 : 0;
        flags[2 * w + 1] = h.fallback ? 1 : 0;
    }
#endif
}
// flags[3 w ..] = ok_a, ok_r, x_r_zero; xy[80 w ..] = the four rows of X, then of Y
__global__ void __launch_bounds__(64) k_lp_decompress_ar(int* flags, uint32_t* xy, const uint32_t* a_enc, const uint32_t* r_enc) {
#if LP_DEVICE
    const int w = blockIdx.x;
    uint32_t wa[8], wr[8];
    ld8(wa, a_enc + 8 * w); ld8(wr, r_enc + 8 * w);
    const LpLane c = LpLane::make();
    const LpConsts K = LpConsts::make(c);
    lu sw[8];
#pragma unroll
    for (int q = 0; q < 8; q++) sw[q] = lp_sel(lp_eq(c.row & 1u, 1u), wr[q], wa[q]);
    const LpDecomp d = lp_decompress_ar(c, K, sw);
    if (threadIdx.x == 0) {
        flags[3 * w] = d.ok_a ? 1 : 0;
        flags[3 * w + 1] = d.ok_r ? 1 : 0;
        flags[3 * w + 2] = d.x_r_zero ? 1 : 0;
    }
    dc_rows_out(xy + 80 * w, d.X);
    dc_rows_out(xy + 80 * w + 40, d.Y);
#endif
}
// hostcheck.hip's hc_lp_ydbl_check on the device: bit r of out[w] set when lp_ydbl_chain + lp_ydbl_finish
// give the point of nd[w] lp_dbl steps for row r (-A, R); -1 if either does not decompress
__global__ void __launch_bounds__(64) k_lp_ydbl_check(int* out, const uint32_t* a_enc, const uint32_t* r_enc, const int* nd) {
#if LP_DEVICE
    const int w = blockIdx.x;
    const int n = nd[w];
    uint32_t wa[8], wr[8];
    ld8(wa, a_enc + 8 * w); ld8(wr, r_enc + 8 * w);
    const LpLane c = LpLane::make();
    const LpConsts K = LpConsts::make(c);
    lu sw[8];
#pragma unroll
    for (int q = 0; q < 8; q++) sw[q] = lp_sel(lp_eq(c.row & 1u, 1u), wr[q], wa[q]);
    const LpDecomp dec = lp_decompress_ar(c, K, sw);
    int mask = 0;
    if (!dec.ok_a || !dec.ok_r) mask = -1;
    else
        for (int which = 0; which < 2; which++) {
            const lu P = lp_ext_from_xy(c, K, dec.X, dec.Y, which);
            lu Q = P;
            for (int j = 0; j < n; j++) Q = lp_dbl(c, Q);
            lu yw[8];
#pragma unroll
            for (int q = 0; q < 8; q++) yw[q] = which ? wr[q] : wa[q];
            const LpYChain ch = lp_ydbl_chain(c, K, lp_from_words(c, yw), n);
            lu x0, t1, t2, t3;
            lp_allrows(P, x0, t1, t2, t3);
            const lu R = lp_ydbl_finish(c, K, ch, x0);
            bool same = true;
            for (int r = 0; r < 4; r += (r == 1 ? 2 : 1)) {  // X, Y and T against Z
                fe a, b, d;
                fe_mul(a, lp_row_fe(Q, r), lp_row_fe(R, 2));
                fe_mul(b, lp_row_fe(R, r), lp_row_fe(Q, 2));
                fe_sub(d, a, b);
                same &= fe_iszero(d);
            }
            mask |= same ? 1 << which : 0;
        }
    if (threadIdx.x == 0) out[w] = mask;
#endif
}
// hostcheck.hip's hc_lp_table_parts_check on the device: 1 if lp_build_a_table_part's three parts give
// lp_build_a_table's points at every entry, 0 if not, -1 if the encoding does not decompress
__global__ void __launch_bounds__(64) k_lp_table_parts_check(int* out, const uint32_t* enc) {
#if LP_DEVICE
    const int w = blockIdx.x;
    uint32_t wa[8];
    ld8(wa, enc + 8 * w);
    const LpLane c = LpLane::make();
    const LpConsts K = LpConsts::make(c);
    lu sw[8];
#pragma unroll
    for (int q = 0; q < 8; q++) sw[q] = wa[q];
    const LpDecomp d = lp_decompress_ar(c, K, sw);
    int res = 1;
    if (!d.ok_a) res = -1;
    else {
        const lu P = lp_ext_from_xy(c, K, d.X, d.Y, 0);
        lu full[17], part[17];
        lp_build_a_table(c, K, P, [&](int j, const lu& q) { full[j + 8] = q; });
        for (int pt = 0; pt < 3; pt++) lp_build_a_table_part(c, K, P, pt, [&](int j, const lu& q) { part[j + 8] = q; });
        for (int e = 0; e < 17; e++)
            for (int r = 0; r < 3; r++) {  // cached rows [Y-X, Y+X, 2dT] against 2Z (row 3)
                fe a, b, dd;
                fe_mul(a, lp_row_fe(full[e], r), lp_row_fe(part[e], 3));
                fe_mul(b, lp_row_fe(part[e], r), lp_row_fe(full[e], 3));
                fe_sub(dd, a, b);
                if (!fe_iszero(dd)) res = 0;
            }
    }
    if (threadIdx.x == 0) out[w] = res;
#endif
}

// ------------------------------------------------------------------ host drivers
template <class K>
int run_fe2(K kern, uint32_t* h, const uint32_t* f, const uint32_t* g, int n) {
    if (n <= 0) return 0;
    DcRun r;
    const uint32_t* df = r.in(f, (size_t)10 * n);
    const uint32_t* dg = r.in(g, (size_t)10 * n);
    uint32_t* dh = r.out(h, (size_t)10 * n);
    if (r.ok()) kern<<<blocks64(n), 64>>>(dh, df, dg, n);
    return r.finish();
}
// one input of `wi` words and one output of `wo` words per set
template <class T, class K>
int run_1(K kern, T* out, int wo, const uint32_t* in, int wi, int n) {
    if (n <= 0) return 0;
    DcRun r;
    const uint32_t* di = r.in(in, (size_t)wi * n);
    T* d = r.out(out, (size_t)wo * n);
    if (r.ok()) kern<<<blocks64(n), 64>>>(d, di, n);
    return r.finish();
}

}  // namespace

extern "C" {

int dc_fe_mul(uint32_t* h, const uint32_t* f, const uint32_t* g, int n) { return run_fe2(k_fe_mul, h, f, g, n); }
int dc_fe_mul_pre(uint32_t* h, const uint32_t* f, const uint32_t* g, int n) { return run_fe2(k_fe_mul_pre, h, f, g, n); }
int dc_fe_sq(uint32_t* h, const uint32_t* f, int n) { return run_1(k_fe_sq, h, 10, f, 10, n); }
int dc_fe_carry(uint32_t* h, const uint32_t* f, int n) { return run_1(k_fe_carry, h, 10, f, 10, n); }
int dc_fe_tobytes(uint32_t* s, const uint32_t* f, int n) { return run_1(k_fe_tobytes, s, 8, f, 10, n); }
int dc_fe_frombytes(uint32_t* h, const uint32_t* s, int n) { return run_1(k_fe_frombytes, h, 10, s, 8, n); }
int dc_fe_invert(uint32_t* h, const uint32_t* f, int n) { return run_1(k_fe_invert, h, 10, f, 10, n); }
int dc_fe_pow22523(uint32_t* h, const uint32_t* f, int n) { return run_1(k_fe_pow22523, h, 10, f, 10, n); }
int dc_sc_reduce64(uint32_t* r, const uint32_t* x, int n) { return run_1(k_sc_reduce64, r, 8, x, 16, n); }
int dc_sc_is_canonical(int* out, const uint32_t* s, int n) { return run_1(k_sc_is_canonical, out, 1, s, 8, n); }
// na = 8 (sc_mul) or 5 (sc_mul<5>: a < 2^160)
int dc_sc_mul(uint32_t* res, const uint32_t* a, const uint32_t* b, int na, int n) {
    if (n <= 0) return 0;
    if (na != 8 && na != 5) return -1;
    DcRun r;
    const uint32_t* da = r.in(a, (size_t)8 * n);
    const uint32_t* db = r.in(b, (size_t)8 * n);
    uint32_t* d = r.out(res, (size_t)8 * n);
    if (r.ok()) {
        if (na == 8) k_sc_mul<8><<<blocks64(n), 64>>>(d, da, db, n);
        else k_sc_mul<5><<<blocks64(n), 64>>>(d, da, db, n);
    }
    return r.finish();
}
int dc_sc_recode(uint32_t* out, const uint32_t* a, int radix, int n) {
    if (n <= 0) return 0;
    if (radix != 16 && radix != 256 && radix != 65536) return -1;
    DcRun r;
    const uint32_t* da = r.in(a, (size_t)8 * n);
    uint32_t* d = r.out(out, (size_t)8 * n);
    if (r.ok()) k_sc_recode<<<blocks64(n), 64>>>(d, da, radix, n);
    return r.finish();
}
// w = 16 (16 digits) or 24 (11 digits); out: 16 int32 per scalar, unused ones 0
int dc_sc_recode_w(int32_t* out, const uint32_t* a, int w, int n) {
    if (w == 16) return run_1(k_sc_recode_w<16, 16>, out, 16, a, 8, n);
    if (w == 24) return run_1(k_sc_recode_w<24, 11>, out, 16, a, 8, n);
    return -1;
}
int dc_sc_nwin16(int* out, const uint32_t* a, int n) { return run_1(k_sc_nwin16, out, 1, a, 8, n); }
int dc_sc_halfsize(uint32_t* k1, uint32_t* k2, int* flags, const uint32_t* k, int n) {
    if (n <= 0) return 0;
    DcRun r;
    const uint32_t* dk = r.in(k, (size_t)8 * n);
    uint32_t* d1 = r.out(k1, (size_t)8 * n);
    uint32_t* d2 = r.out(k2, (size_t)8 * n);
    int* df = r.out(flags, (size_t)2 * n);
    if (r.ok()) k_sc_halfsize<<<blocks64(n), 64>>>(d1, d2, df, dk, n);
    return r.finish();
}
int dc_enc_rules(int* out, const uint32_t* s, int n) { return run_1(k_enc_rules, out, 2, s, 8, n); }
int dc_ge_frombytes_negate(int* ok, uint32_t* out, const uint32_t* s, int n) {
    if (n <= 0) return 0;
    DcRun r;
    const uint32_t* ds = r.in(s, (size_t)8 * n);
    int* dok = r.out(ok, (size_t)n);
    uint32_t* d = r.out(out, (size_t)40 * n);
    if (r.ok()) k_ge_frombytes_negate<<<blocks64(n), 64>>>(dok, d, ds, n);
    return r.finish();
}
int dc_ge_p2_tobytes(uint32_t* s, const uint32_t* xyz, int n) { return run_1(k_ge_p2_tobytes, s, 8, xyz, 30, n); }
// sm: n records of `stride` bytes each (record i = R || S || M, smlen[i] bytes, zero slack after it)
int dc_hash_k(uint32_t* kout, const uint8_t* sm, uint64_t stride, const uint64_t* smlen, const uint32_t* pk, int n) {
    if (n <= 0) return 0;
    for (int i = 0; i < n; i++)
        if (smlen[i] < 64 || smlen[i] + 256 > stride) return -1;
    DcRun r;
    const uint8_t* dsm = r.in(sm, (size_t)stride * n);
    const uint64_t* dl = r.in(smlen, (size_t)n);
    const uint32_t* dpk = r.in(pk, (size_t)8 * n);
    uint32_t* d = r.out(kout, (size_t)8 * n);
    if (r.ok()) k_hash_k<<<blocks64(n), 64>>>(d, dsm, stride, dl, dpk, n);
    return r.finish();
}

// per-wave entries: n operand sets, one 64-lane block each; 40 words (4 rows x 10 limbs) per operand
int dc_lp_binary(uint32_t* h, const uint32_t* f, const uint32_t* g, int op, int n) {
    if (n <= 0) return 0;
    if (op < 0 || op > 3) return -1;
    DcRun r;
    const uint32_t* df = r.in(f, (size_t)40 * n);
    const uint32_t* dg = r.in(g, (size_t)40 * n);
    uint32_t* dh = r.out(h, (size_t)40 * n);
    if (r.ok()) k_lp_binary<<<(unsigned)n, 64>>>(dh, df, dg, op);
    return r.finish();
}
int dc_lp_unary(uint32_t* h, const uint32_t* f, int op, int n) {
    if (n <= 0) return 0;
    if (op < 0 || op > 4) return -1;
    DcRun r;
    const uint32_t* df = r.in(f, (size_t)40 * n);
    uint32_t* dh = r.out(h, (size_t)40 * n);
    if (r.ok()) k_lp_unary<<<(unsigned)n, 64>>>(dh, df, op);
    return r.finish();
}
int dc_lp_halfsize(uint32_t* k1, uint32_t* k2, int* flags, const uint32_t* k, int n) {
    if (n <= 0) return 0;
    DcRun r;
    const uint32_t* dk = r.in(k, (size_t)8 * n);
    uint32_t* d1 = r.out(k1, (size_t)8 * n);
    uint32_t* d2 = r.out(k2, (size_t)8 * n);
    int* df = r.out(flags, (size_t)2 * n);
    if (r.ok()) k_lp_halfsize<<<(unsigned)n, 64>>>(d1, d2, df, dk);
    return r.finish();
}
int dc_lp_decompress_ar(int* flags, uint32_t* xy, const uint32_t* a_enc, const uint32_t* r_enc, int n) {
    if (n <= 0) return 0;
    DcRun r;
    const uint32_t* da = r.in(a_enc, (size_t)8 * n);
    const uint32_t* dr = r.in(r_enc, (size_t)8 * n);
    int* df = r.out(flags, (size_t)3 * n);
    uint32_t* dxy = r.out(xy, (size_t)80 * n);
    if (r.ok()) k_lp_decompress_ar<<<(unsigned)n, 64>>>(df, dxy, da, dr);
    return r.finish();
}
int dc_lp_ydbl_check(int* out, const uint32_t* a_enc, const uint32_t* r_enc, const int* nd, int n) {
    if (n <= 0) return 0;
    for (int i = 0; i < n; i++)
        if (nd[i] < 0 || nd[i] > 256) return -1;
    DcRun r;
    const uint32_t* da = r.in(a_enc, (size_t)8 * n);
    const uint32_t* dr = r.in(r_enc, (size_t)8 * n);
    const int* dn = r.in(nd, (size_t)n);
    int* d = r.out(out, (size_t)n);
    if (r.ok()) k_lp_ydbl_check<<<(unsigned)n, 64>>>(d, da, dr, dn);
    return r.finish();
}
int dc_lp_table_parts_check(int* out, const uint32_t* enc, int n) {
    if (n <= 0) return 0;
    DcRun r;
    const uint32_t* de = r.in(enc, (size_t)8 * n);
    int* d = r.out(out, (size_t)n);
    if (r.ok()) k_lp_table_parts_check<<<(unsigned)n, 64>>>(d, de);
    return r.finish();
}

}  // extern "C"
