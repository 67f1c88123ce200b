// Order keys, the LDS radix select and the counting sort shared by the two NMS families (decode_nms.hip: Matrix-NMS;
// multiclass_nms.hip: greedy per-class NMS).  Every helper here is called by ALL NT threads of a workgroup.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ uint32_t score_to_key(float s) {
    const uint32_t b = __float_as_uint(s);
    return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}
__device__ __forceinline__ float key_to_score(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

constexpr int NT = 1024;      // threads
constexpr int KMAX = 1024;    // max nms_top_k
constexpr int RBITS = 11;     // radix-select digit
constexpr int CCAP = 8192;    // candidates staged in LDS (64 KB of dynamic shared memory)

// inclusive suffix sum over the workgroup (threads >= tid)
__device__ __forceinline__ int block_suffix_sum(int v, int *scratch /*[16+1]*/) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int s = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_down(s, d);
        if (lane + d < 64) s += o;
    }
    if (lane == 0) scratch[wv] = s;
    __syncthreads();
    int add = 0;
    for (int k = wv + 1; k < NT / 64; ++k) add += scratch[k];
    __syncthreads();
    return s + add;
}

// Descending sort of n <= KMAX DISTINCT non-zero keys (zeros = padding, they all land behind the real keys)
// by counting: rank(e) = #{i : key[i] > key[e]}.  Every thread of a wave reads the same key[i] (LDS
// broadcast), P2/NT threads share an element, and the whole sort costs two barriers instead of the
// log^2 barrier-separated stages of a bitonic network (1024-thread barriers are what this kernel waits on).
__device__ __forceinline__ void rank_sort_desc(const unsigned long long *in, unsigned long long *out, int n, int P2,
                                               int *rank /*[KMAX]*/) {
    const int tid = threadIdx.x;
    const int parts = NT / P2;                 // threads per element (P2 = power of two >= n, >= 64)
    const int e = tid & (P2 - 1), part = tid / P2;
    if (tid < KMAX) rank[tid] = 0;
    if (tid < KMAX) out[tid] = 0ull;
    __syncthreads();
    if (e < n) {
        const unsigned long long mine = in[e];
        const int len = (n + parts - 1) / parts, lo = part * len, hi = min(lo + len, n);
        int r = 0, i = lo;
        for (; i + 8 <= hi; i += 8) {          // 8 independent LDS reads in flight (the loop is latency-bound otherwise)
            unsigned long long v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = in[i + u];
#pragma unroll
            for (int u = 0; u < 8; ++u) r += v[u] > mine ? 1 : 0;
        }
        for (; i < hi; ++i) r += in[i] > mine ? 1 : 0;
        if (parts == 1) rank[e] = r; else atomicAdd(&rank[e], r);
    }
    __syncthreads();
    if (tid < n && in[tid] != 0ull) out[rank[tid]] = in[tid];
    __syncthreads();
}

// MSB-first radix select over `count` keys of `total_bits` bits (key_of(c), c < count): the largest T such that at least `need`
// keys are >= T, exact unless a digit's bin holds exactly the keys still needed (then the whole bin is taken: T = the bin's
// lower edge, same set).  All NT threads of the workgroup call it; hist = [1 << RBITS], scratch = [32], sel = [3] in LDS.
template <typename KeyFn>
__device__ __forceinline__ unsigned long long radix_select_threshold(KeyFn key_of, int count, int need, int total_bits,
                                                                       unsigned int *hist, int *scratch, int *sel) {
    const int tid = threadIdx.x;
    unsigned long long prefix = 0ull;
    int shift = total_bits;
    while (shift > 0) {
        const int bits = shift < RBITS ? shift : RBITS;
        const int hi_shift = shift;
        shift -= bits;
        for (int i = tid; i < (1 << RBITS); i += NT) hist[i] = 0u;
        __syncthreads();
        for (int c = tid; c < count; c += NT) {
            const unsigned long long k = key_of(c);
            if ((hi_shift >= 64 ? 0ull : (k >> hi_shift)) == prefix)
                atomicAdd(&hist[(unsigned)((k >> shift) & ((1ull << bits) - 1ull))], 1u);
        }
        __syncthreads();
        const int h0 = (int)hist[2 * tid], h1 = (int)hist[2 * tid + 1];
        const int incl = block_suffix_sum(h0 + h1, scratch);
        const int after = incl - (h0 + h1);   // candidates in bins above this thread's pair
        if (after < need && need <= after + h1) {
            sel[0] = 2 * tid + 1; sel[1] = after; sel[2] = h1;
        } else if (after + h1 < need && need <= after + h1 + h0) {
            sel[0] = 2 * tid; sel[1] = after + h1; sel[2] = h0;
        }
        __syncthreads();
        prefix = (prefix << bits) | (unsigned long long)sel[0];
        need -= sel[1];
        const bool whole_bin = (sel[2] == need);
        __syncthreads();
        if (whole_bin) break;
    }
    return prefix << shift;
}

}  // namespace
