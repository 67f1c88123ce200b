// Greedy per-class hard NMS (PaddleDetection's multiclass_nms operator) for gfx950, beside Matrix-NMS (decode_nms.hip).
//
// It starts from the same per-image candidate list (score key, box * C + class) that the decode kernels or
// ppy_nms_candidates_f32 append with atomics, i.e. in no particular order.  EVERY ordering decision below is taken on a key
// made of (score, class, box index), never on a list position, so the result is bit-identical from run to run and for any
// permutation of the list.  Three launches, kernel boundaries as the only synchronisation:
//   Z  mc_zero_kernel    (1 workgroup)               the per-image counters of the merged list
//   B  mc_class_kernel   (C x N workgroups)          one (image, class): filter the image's list by class, top nms_top_k by
//                                                    (score desc, box asc) with the LDS radix select, counting sort, the sorted
//                                                    boxes in LDS, greedy scan 64 candidates at a time; the selections are
//                                                    appended to the image's merged list
//   M  mc_merge_kernel   (N workgroups)              keep_top_k by (score desc, class asc, box asc), ordered store as
//                                                    (class asc, score desc, box asc)
// The IoU is PaddleDetection's JaccardOverlap in fp32, one rounding per operation: this file is compiled without contraction.
#include "common.h"
#include "nms_select.h"
#pragma clang fp contract(off)

namespace {

constexpr int MC_STAGE = 4096;      // composite keys of ONE class staged in LDS (32 KB); a larger class walks the global list

struct McArgs {
    const float *boxes;
    const uint32_t *cand_key, *cand_idx;
    const int *cand_count;
    float *out_dets;
    int *out_count, *out_keep;
    int M_total, C, cand_cap, top_k, keep_k, N, box_bits, cls_bits, background;
    float thr, norm;
    int *merged_count;                  // [N]
    unsigned long long *merged;         // [N][C * top_k]: (score key, C - 1 - class, box_mask - box), most significant first
};

__device__ __forceinline__ float mc_min(float a, float b) { return b < a ? b : a; }      // std::min / std::max
__device__ __forceinline__ float mc_max(float a, float b) { return a < b ? b : a; }

__device__ __forceinline__ float mc_area(const floatx4 b, float norm) {
    if (b[2] < b[0] || b[3] < b[1]) return 0.0f;
    return ((b[2] - b[0]) + norm) * ((b[3] - b[1]) + norm);
}

__device__ __forceinline__ float mc_iou(const floatx4 a, const floatx4 b, float norm) {
    if (b[0] > a[2] || b[2] < a[0] || b[1] > a[3] || b[3] < a[1]) return 0.0f;
    const float iw = (mc_min(a[2], b[2]) - mc_max(a[0], b[0])) + norm;
    const float ih = (mc_min(a[3], b[3]) - mc_max(a[1], b[1])) + norm;
    const float inter = iw * ih;
    return inter / ((mc_area(a, norm) + mc_area(b, norm)) - inter);
}

__global__ void __launch_bounds__(256) mc_zero_kernel(int *counts, int n) {
    for (int i = threadIdx.x; i < n; i += 256) counts[i] = 0;
}

__global__ void __launch_bounds__(NT) mc_class_kernel(const McArgs p) {
    __shared__ __attribute__((aligned(16))) unsigned long long stage[MC_STAGE];      // the class's keys; later the sorted boxes + the kept list
    __shared__ unsigned long long skey[KMAX], skey2[KMAX];
    __shared__ unsigned int hist[1 << RBITS];
    int *srank = reinterpret_cast<int *>(hist);                 // the histogram is dead once the threshold is known
    __shared__ int scratch[32];
    __shared__ int s_sel[3], s_cnt, s_cnt2, s_nkept, s_base;
    __shared__ unsigned long long s_col[64];
    __shared__ unsigned int s_supp[64];

    const int c = blockIdx.x, n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (c == p.background) return;
    const uint32_t *ckey = p.cand_key + (long long)n * p.cand_cap;
    const uint32_t *cidx = p.cand_idx + (long long)n * p.cand_cap;
    const int count = min(p.cand_count[n], p.cand_cap);
    const int bb = p.box_bits;
    const unsigned long long box_mask = (1ull << bb) - 1ull;
    // composite key of list entry i: larger == earlier in (score desc, box asc); 0 = the entry belongs to another class
    // (a real key is never 0: its score half would be the key of a negative NaN, which passes no threshold)
    auto comp_global = [&](int i) -> unsigned long long {
        const uint32_t flat = cidx[i];
        const uint32_t box = flat / (uint32_t)p.C;
        if (flat - box * (uint32_t)p.C != (uint32_t)c) return 0ull;
        return ((unsigned long long)ckey[i] << bb) | (box_mask - (unsigned long long)box);
    };

    // ---- 1. this class's entries: count them, stage the first MC_STAGE ----
    if (tid == 0) { s_cnt = 0; s_cnt2 = 0; s_nkept = 0; }
    skey[tid] = 0ull;
    if (tid < 64) s_supp[tid] = 0u;
    __syncthreads();
    for (int i = tid; i < count; i += NT) {
        const unsigned long long k = comp_global(i);
        if (k != 0ull) {
            const int pos = atomicAdd(&s_cnt, 1);
            if (pos < MC_STAGE) stage[pos] = k;
        }
    }
    __syncthreads();
    const int cnt = s_cnt;
    if (cnt == 0) return;
    const bool staged = cnt <= MC_STAGE;
    const int niter = staged ? cnt : count;
    auto key_of = [&](int i) -> unsigned long long { return staged ? stage[i] : comp_global(i); };

    // ---- 2. the top nms_top_k of them, sorted (score desc, box asc) ----
    const int K = min(p.top_k, cnt);
    unsigned long long T = 0ull;
    if (cnt > p.top_k) T = radix_select_threshold(key_of, niter, K, 32 + bb, hist, scratch, s_sel);
    for (int i = tid; i < niter; i += NT) {
        const unsigned long long k = key_of(i);
        if (k != 0ull && k >= T) {
            const int pos = atomicAdd(&s_cnt2, 1);
            if (pos < KMAX) skey[pos] = k;
        }
    }
    __syncthreads();
    int P = 64;
    while (P < K) P <<= 1;
    rank_sort_desc(skey, skey2, K, P, srank);

    // ---- 3. the sorted boxes in LDS (the staged keys are dead) ----
    floatx4 *sbox = reinterpret_cast<floatx4 *>(stage);                 // [KMAX]
    int *skept = reinterpret_cast<int *>(stage + 2 * KMAX);             // [KMAX] sorted positions of the selected, in selection order
    static_assert(MC_STAGE >= 2 * KMAX + KMAX / 2, "boxes and kept list alias the stage");
    if (tid < K) {
        const long long box = (long long)(box_mask - (skey2[tid] & box_mask));
        sbox[tid] = *reinterpret_cast<const floatx4 *>(p.boxes + ((long long)n * p.M_total + box) * 4);
    }
    __syncthreads();

    // ---- 4. greedy scan, 64 candidates (one ballot word) at a time ----
    // Candidate j is selected iff iou(j, k) <= thr for EVERY already selected k; `!(iou <= thr)` suppresses, so a NaN IoU does.
    //   (a) lane = candidate of the chunk, waves stride over the selected of earlier chunks (their box is an LDS broadcast)
    //   (b) wave wv, q = 0..3: column i = 4 wv + q of the chunk's own 64 x 64 matrix, as a ballot over the later candidates
    //   (c) wave 0 walks the chunk in order: an alive candidate is selected and kills its column
    int nkept = 0;
    for (int c0 = 0; c0 < K; c0 += 64) {
        const int nc = min(64, K - c0);
        const bool valid = lane < nc;
        const floatx4 bj = sbox[valid ? c0 + lane : c0];
        bool bad = false;
        for (int k = wv; k < nkept; k += NT / 64) bad |= !(mc_iou(bj, sbox[skept[k]], p.norm) <= p.thr);
        if (bad && valid) atomicOr(&s_supp[lane], 1u);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = 4 * wv + q;
            const floatx4 bi = sbox[i < nc ? c0 + i : c0];
            const bool hit = valid && lane > i && i < nc && !(mc_iou(bj, bi, p.norm) <= p.thr);
            const unsigned long long col = __ballot(hit);
            if (lane == 0) s_col[i] = col;
        }
        __syncthreads();
        if (wv == 0) {
            unsigned long long alive = __ballot(valid && s_supp[lane] == 0u);
            const unsigned long long mycol = s_col[lane];
            const unsigned int clo = (unsigned int)mycol, chi = (unsigned int)(mycol >> 32);
            unsigned long long kept = 0ull;
            for (int i = 0; i < nc; ++i) {
                const unsigned long long coli = ((unsigned long long)(unsigned int)__builtin_amdgcn_readlane((int)chi, i) << 32) |
                                                (unsigned long long)(unsigned int)__builtin_amdgcn_readlane((int)clo, i);
                if ((alive >> i) & 1ull) {
                    kept |= 1ull << i;
                    alive &= ~coli;
                }
            }
            if ((kept >> lane) & 1ull) skept[nkept + __popcll(kept & ((1ull << lane) - 1ull))] = c0 + lane;
            s_supp[lane] = 0u;
            if (lane == 0) s_nkept = nkept + __popcll(kept);
        }
        __syncthreads();
        nkept = s_nkept;
    }

    // ---- 5. append the selections to the image's merged list (its order is irrelevant: the merge orders by key) ----
    if (tid == 0) s_base = atomicAdd(p.merged_count + n, nkept);
    __syncthreads();
    unsigned long long *mg = p.merged + (long long)n * p.C * p.top_k + s_base;
    if (tid < nkept) {
        const unsigned long long k = skey2[skept[tid]];
        mg[tid] = ((k >> bb) << (bb + p.cls_bits)) | ((unsigned long long)(p.C - 1 - c) << bb) | (k & box_mask);
    }
}

__global__ void __launch_bounds__(NT) mc_merge_kernel(const McArgs p) {
    __shared__ unsigned long long skey[KMAX], skey2[KMAX];
    __shared__ unsigned int hist[1 << RBITS];
    int *srank = reinterpret_cast<int *>(hist);
    __shared__ int scratch[32];
    __shared__ int s_sel[3], s_cnt;
    extern __shared__ unsigned long long scache[];      // [CCAP] (dynamic)

    const int n = blockIdx.x, tid = threadIdx.x;
    float *dets = p.out_dets + (long long)n * p.keep_k * 6;
    int *keep = p.out_keep + (long long)n * p.keep_k;
    for (int i = tid; i < p.keep_k * 6; i += NT) dets[i] = -1.0f;
    for (int i = tid; i < p.keep_k; i += NT) keep[i] = -1;
    const int total = p.merged_count[n];
    if (total == 0) {
        if (tid == 0) p.out_count[n] = 0;
        return;
    }
    const unsigned long long *mg = p.merged + (long long)n * p.C * p.top_k;
    const bool cached = total <= CCAP;
    if (cached) {
        for (int i = tid; i < total; i += NT) scache[i] = mg[i];
    }
    if (tid == 0) s_cnt = 0;
    skey[tid] = 0ull;
    __syncthreads();
    auto key_of = [&](int i) -> unsigned long long { return cached ? scache[i] : mg[i]; };
    const int bb = p.box_bits, cb = p.cls_bits;
    const unsigned long long box_mask = (1ull << bb) - 1ull, cls_mask = (1ull << cb) - 1ull;

    // keep_top_k highest scores, ties to the earlier position of the class-by-class concatenation: (score desc, class asc, box asc)
    const int K = min(p.keep_k, total);
    unsigned long long T = 0ull;
    if (total > p.keep_k) T = radix_select_threshold(key_of, total, K, 32 + bb + cb, hist, scratch, s_sel);
    for (int i = tid; i < total; i += NT) {
        const unsigned long long k = key_of(i);
        if (k >= T) {
            const int pos = atomicAdd(&s_cnt, 1);
            // output order (class asc, score desc, box asc): the class field moves to the top (still never 0: the score field is not)
            if (pos < KMAX)
                skey[pos] = (((k >> bb) & cls_mask) << (32 + bb)) | ((k >> (bb + cb)) << bb) | (k & box_mask);
        }
    }
    __syncthreads();
    int P = 64;
    while (P < K) P <<= 1;
    rank_sort_desc(skey, skey2, K, P, srank);
    if (tid < K) {
        const unsigned long long k = skey2[tid];
        const int cls = p.C - 1 - (int)(k >> (32 + bb));
        const long long box = (long long)(box_mask - (k & box_mask));
        const floatx4 b = *reinterpret_cast<const floatx4 *>(p.boxes + ((long long)n * p.M_total + box) * 4);
        float *o = dets + tid * 6;
        o[0] = (float)cls;
        o[1] = key_to_score((uint32_t)((k >> bb) & 0xffffffffull));
        o[2] = b[0]; o[3] = b[1]; o[4] = b[2]; o[5] = b[3];
        keep[tid] = (int)(box * p.C + cls);
    }
    if (tid == 0) p.out_count[n] = K;
}

size_t mc_counts_bytes(int N) { return ((size_t)N * sizeof(int) + 15) / 16 * 16; }

}  // namespace

extern "C" size_t ppy_multiclass_nms_workspace_bytes(int N, int num_classes, int nms_top_k, int cand_cap) {
    (void)cand_cap;      // the candidate list is filtered in place, never copied: the bound does not grow with it
    if (N <= 0 || num_classes <= 0 || nms_top_k < 1 || nms_top_k > KMAX) return 0;
    return mc_counts_bytes(N) + (size_t)N * num_classes * nms_top_k * sizeof(unsigned long long);
}

extern "C" int ppy_multiclass_nms_f32(const float *boxes, int M_total, int num_classes, const uint32_t *cand_key,
                                      const uint32_t *cand_idx, const int *cand_count, int cand_cap, int N,
                                      int nms_top_k, int keep_top_k, float nms_threshold, int normalized, float nms_eta,
                                      int background_label, float *out_dets, int *out_count, int *out_keep_idx,
                                      void *ws, size_t ws_bytes, void *stream) {
    ppy_drop_stale_error();
    PPY_CHECK_ARG(boxes && cand_key && cand_idx && cand_count && out_dets && out_count && out_keep_idx);
    PPY_CHECK_ARG(N > 0 && N <= 65535 && M_total > 0 && num_classes > 0 && cand_cap > 0);
    PPY_CHECK_ARG(((uintptr_t)boxes & 15) == 0);
    const long long span = (long long)M_total * num_classes;
    PPY_CHECK_ARG(span < (1ll << 31));
    if (nms_top_k < 1 || nms_top_k > KMAX || keep_top_k < 1 || keep_top_k > KMAX || nms_eta != 1.0f) return PPY_ERR_UNSUPPORTED;
    if (!ws || ((uintptr_t)ws & 15) != 0 || ws_bytes < ppy_multiclass_nms_workspace_bytes(N, num_classes, nms_top_k, cand_cap))
        return PPY_ERR_WORKSPACE;
    McArgs p;
    p.boxes = boxes; p.cand_key = cand_key; p.cand_idx = cand_idx; p.cand_count = cand_count;
    p.out_dets = out_dets; p.out_count = out_count; p.out_keep = out_keep_idx;
    p.M_total = M_total; p.C = num_classes; p.cand_cap = cand_cap; p.top_k = nms_top_k; p.keep_k = keep_top_k; p.N = N;
    // (M_total * C < 2^31, so box_bits + cls_bits <= 32 and every composite key fits 64 bits)
    p.box_bits = 1;
    while ((1ll << p.box_bits) < M_total) ++p.box_bits;
    p.cls_bits = 1;
    while ((1ll << p.cls_bits) < num_classes) ++p.cls_bits;
    p.background = background_label;
    p.thr = nms_threshold;
    p.norm = normalized ? 0.0f : 1.0f;
    p.merged_count = reinterpret_cast<int *>(ws);
    p.merged = reinterpret_cast<unsigned long long *>((char *)ws + mc_counts_bytes(N));
    static PpyLdsAttr attr;
    if (ppy_lds_attr(attr, reinterpret_cast<const void *>(mc_merge_kernel), CCAP * 8) != PPY_OK) return PPY_ERR_LAUNCH;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mc_zero_kernel, dim3(1), dim3(256), 0, st, p.merged_count, N);
    hipLaunchKernelGGL(mc_class_kernel, dim3(num_classes, N), dim3(NT), 0, st, p);
    hipLaunchKernelGGL(mc_merge_kernel, dim3(N), dim3(NT), CCAP * 8, st, p);
    return ppy_launch_status();
}
