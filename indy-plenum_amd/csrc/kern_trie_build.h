// The kernels of the device trie builder (pv_trie_root, DESIGN 7d "Device builder"): one lane per item of a
// pass of trie_build.h, included by pv_trie.hip inside its unnamed namespace. No kernel reads what another
// workgroup writes in the same launch: a pass reads what earlier launches wrote, and the stream orders them.
// The only atomics add to or OR into header words that later launches and the host read. Every kernel but the
// first returns at once when the error word is set, so a value offset that the checks refused is never used.
#ifndef PV_KERN_TRIE_BUILD_H
#define PV_KERN_TRIE_BUILD_H

#include "trie_build.h"

#define TB_LANE()                                              \
    const uint32_t i = blockIdx.x * TR_BLOCK + threadIdx.x;    \
    if (i >= count || c.hdr->err) return

__global__ __launch_bounds__(TR_BLOCK) void pv_tb_init_kernel(const TbCtx c, uint32_t count) {
    const uint32_t i = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (i < count) tb_init(c, i);
}
__global__ __launch_bounds__(TR_BLOCK) void pv_tb_word_kernel(const TbCtx c, uint32_t count, uint32_t w, uint64_t* __restrict__ out) {
    TB_LANE();
    out[i] = tb_sort_word(c, i, w);
}
__global__ __launch_bounds__(TR_BLOCK) void pv_tb_gather_kernel(const TbCtx c, uint32_t count, const uint64_t* __restrict__ sorted,
                                                                uint32_t* __restrict__ out) {
    TB_LANE();
    out[i] = tb_gather(c, i, sorted);
}
__global__ __launch_bounds__(TR_BLOCK) void pv_tb_keep_kernel(const TbCtx c, uint32_t count) {
    TB_LANE();
    tb_keep(c, i);
}
__global__ __launch_bounds__(TR_BLOCK) void pv_tb_compact_kernel(const TbCtx c, uint32_t count) {
    TB_LANE();
    tb_compact(c, i);
}
__global__ __launch_bounds__(TR_BLOCK) void pv_tb_lcp_kernel(const TbCtx c, uint32_t count) {
    TB_LANE();
    tb_lcp(c, i);
}
__global__ __launch_bounds__(TR_BLOCK) void pv_tb_branch_kernel(const TbCtx c, uint32_t count) {
    TB_LANE();
    tb_branch(c, i);
}
__global__ __launch_bounds__(TR_BLOCK) void pv_tb_leaf_size_kernel(const TbCtx c, uint32_t count) {
    TB_LANE();
    tb_leaf_size(c, i);
}
__global__ __launch_bounds__(TR_BLOCK) void pv_tb_small_kernel(const TbCtx c, uint32_t count) {
    TB_LANE();
    tb_small(c, i);
}
__global__ __launch_bounds__(TR_BLOCK) void pv_tb_size_kernel(const TbCtx c, uint32_t count) {
    TB_LANE();
    tb_size(c, i);
}
// the counts go through the workgroup's LDS: one atomic per workgroup and word on the header
__global__ __launch_bounds__(TR_BLOCK) void pv_tb_mark_kernel(const TbCtx c, uint32_t count) {
    __shared__ uint32_t s[3];
    if (threadIdx.x < 3) s[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * TR_BLOCK + threadIdx.x;
    const uint32_t f = i < count && !c.hdr->err ? tb_mark(c, i) : 0;
    if (f & 1) atomicAdd(&s[0], 1u);
    if (f & 2) atomicAdd(&s[1], 1u);
    if (f >> 8) atomicMax(&s[2], f >> 8);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s[0]) atomicAdd(&c.hdr->n_branch, s[0]);
        if (s[1]) atomicAdd(&c.hdr->n_ext, s[1]);
        if (s[2]) atomicMax(&c.hdr->max_depth, s[2]);
    }
}
__global__ __launch_bounds__(TR_BLOCK) void pv_tb_bounds_kernel(const TbCtx c, uint32_t count) {
    TB_LANE();
    tb_bounds(c, i);
}
__global__ __launch_bounds__(TR_BLOCK) void pv_tb_emit_kernel(const TbCtx c, uint32_t count) {
    TB_LANE();
    tb_emit(c, i);
}

#undef TB_LANE

#endif  // PV_KERN_TRIE_BUILD_H
