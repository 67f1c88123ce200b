// Cross-view greedy suppression for tiled (sliced) inference on gfx950: the rows that forward_padded wrote for a batch of
// VIEWS (tiles of large images plus, usually, the whole image squashed) are translated to image coordinates and merged per
// image, on the device, into one list in the forward_padded row format.  DESIGN.md section 10h has the contract;
// tests/tile_merge_ref.py restates it in numpy and the kernel agrees with it bit for bit.
//
// One launch, one workgroup of 1024 threads per image, kernel-internal barriers as the only synchronisation:
//   1  admit     the view table is read 64 entries at a time; a padding view, a view of another image and a view whose count
//                is 0 cost that entry and nothing else; the others are dealt to the 16 waves in turn, a lane per row.  An
//                admitted row becomes a 64-bit key in LDS:
//                (score key, ~(view * K + row)), so "larger key" == "earlier in (score desc, view asc, row asc)".  The keys
//                are distinct, so the position an LDS integer atomic hands out does not reach the result.
//   2  order     up to MV_RANK_MAX keys: the counting sort of nms_select.h (two barriers); more: a bitonic network over the
//                next power of two, zero keys (no real key is zero) as padding behind the real ones.
//   3  gather    the sorted candidates' translated box, class id and (view * K + row) go to the workspace, 32 bytes each,
//                once and by all threads, so that the scan reads them coalesced instead of chasing key -> table -> row.
//   4  scan      MV_CHUNK = 64 candidates (one ballot word) at a time, as mc_class_kernel does: (a) against the selected of
//                earlier chunks, whose boxes sit in LDS, (b) the chunk's own 64 x 64 matrix by ballots, (c) wave 0 walks the
//                chunk in order.  The scan ends with the chunk in which the keep_top_k-th selection falls.
//   5  store     the first keep_top_k selections: original class and score, translated box, (view, row); -1 behind them.
// fp32, one rounding per operation: this file is compiled without contraction.  No floating-point atomics anywhere.
#include <cstdio>
#include <vector>

#include "common.h"
#include "nms_select.h"
#pragma clang fp contract(off)

namespace {

constexpr int MV_MAX_ROWS = PPY_MERGE_MAX_ROWS;      // rows of one image (its views x K): the keys' LDS stage, 64 KB
constexpr int MV_RANK_MAX = PPY_MERGE_RANK_MAX;      // up to here the counting sort, beyond it the bitonic network
constexpr int MV_CHUNK = PPY_MERGE_CHUNK;            // candidates per scan step: one ballot word
static_assert(MV_RANK_MAX == KMAX && MV_CHUNK == 64 && PPY_MERGE_MAX_KEEP == KMAX, "the header's constants are the kernel's");
constexpr int MV_KEEP_CAP = KMAX + MV_CHUNK;   // selections held in LDS: the scan stops once keep_top_k <= KMAX are reached
constexpr int MV_REC_BYTES = 32;               // one gathered candidate in the workspace

struct MvRec {                                 // 32 bytes, 16-byte aligned
    floatx4 box;
    int cls;
    unsigned int idx;                          // view * K + row
    int pad[2];
};
static_assert(sizeof(MvRec) == MV_REC_BYTES, "record layout");

struct MvArgs {
    const float *dets;
    const int *count, *views;
    float *out_dets;
    int *out_count, *out_src;
    MvRec *recs;                               // [n][rec_cap]
    int V, K, n, keep_k, rec_cap, ios, agnostic;
    float thr, score_thr, norm;                // norm = 0 (pixel boxes are "normalized" in PaddleDetection's sense), kept as an
};                                             // operand so that the arithmetic is the restatement's, operation for operation

__device__ __forceinline__ float mv_min(float a, float b) { return b < a ? b : a; }      // std::min / std::max
__device__ __forceinline__ float mv_max(float a, float b) { return a < b ? b : a; }
__device__ __forceinline__ bool mv_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }      // false for NaN and inf

__device__ __forceinline__ float mv_area(const floatx4 b, float norm) {
    if (b[2] < b[0] || b[3] < b[1]) return 0.0f;
    return ((b[2] - b[0]) + norm) * ((b[3] - b[1]) + norm);
}

// a = the candidate, b = an already selected box.  IoU: PaddleDetection's JaccardOverlap; IoS: the same intersection over the
// smaller of the two areas.
__device__ __forceinline__ float mv_metric(const floatx4 a, const floatx4 b, float norm, int ios) {
    if (b[0] > a[2] || b[2] < a[0] || b[1] > a[3] || b[3] < a[1]) return 0.0f;
    const float iw = (mv_min(a[2], b[2]) - mv_max(a[0], b[0])) + norm;
    const float ih = (mv_min(a[3], b[3]) - mv_max(a[1], b[1])) + norm;
    const float inter = iw * ih;
    const float aa = mv_area(a, norm), ab = mv_area(b, norm);
    if (ios) return inter / (ab < aa ? ab : aa);
    return inter / ((aa + ab) - inter);
}

__device__ __forceinline__ float mv_lane_f(float v, int src) {      // v of lane `src` (wave-uniform)
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

__global__ void __launch_bounds__(NT) mv_merge_kernel(const MvArgs p) {
    extern __shared__ unsigned long long skeys[];                       // [MV_MAX_ROWS] (dynamic, 64 KB)
    __shared__ unsigned long long ssort[KMAX];                          // the counting sort's output
    __shared__ int srank[KMAX];
    __shared__ __attribute__((aligned(16))) floatx4 s_kbox[MV_KEEP_CAP];
    __shared__ int s_kcls[MV_KEEP_CAP];
    __shared__ unsigned int s_kidx[MV_KEEP_CAP];
    __shared__ unsigned long long s_col[MV_CHUNK];
    __shared__ unsigned int s_supp[MV_CHUNK];
    __shared__ int s_cnt, s_nkept;

    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int K = p.K;
    float *odets = p.out_dets + (long long)n * p.keep_k * 6;
    int *osrc = p.out_src + (long long)n * p.keep_k * 2;

    // ---- 1. admit ----
    if (tid == 0) { s_cnt = 0; s_nkept = 0; }
    if (tid < MV_CHUNK) s_supp[tid] = 0u;
    __syncthreads();
    int turn = 0;      // the image's views with rows, in table order, are dealt to the waves in turn
    for (int base = 0; base < p.V; base += 64) {
        const int v = base + lane;
        int c = 0;
        if (v < p.V && p.views[3 * v] == n) c = min(p.count[v], K);
        unsigned long long todo = __ballot(c > 0);
        while (todo) {
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            if ((turn++ & (NT / 64 - 1)) != wv) continue;
            const int cv = __builtin_amdgcn_readlane(c, l), vv = base + l;
            const float *rows = p.dets + (long long)vv * K * 6;
            for (int r = lane; r < cv; r += 64) {
                const float *d = rows + r * 6;
                const float cls = d[0], score = d[1];
                const bool ok = mv_finite(cls) && mv_finite(score) && mv_finite(d[2]) && mv_finite(d[3]) && mv_finite(d[4]) &&
                                mv_finite(d[5]) && cls >= 0.0f && cls < 16777216.0f && score >= p.score_thr;
                if (ok) {
                    const float s = score == 0.0f ? 0.0f : score;      // -0.0 ties with +0.0
                    const unsigned int idx = (unsigned int)vv * (unsigned int)K + (unsigned int)r;
                    const int pos = atomicAdd(&s_cnt, 1);
                    if (pos < MV_MAX_ROWS)      // (always: the host refuses an image with more rows)
                        skeys[pos] = ((unsigned long long)score_to_key(s) << 32) | (unsigned long long)(0xffffffffu - idx);
                }
            }
        }
    }
    __syncthreads();
    const int cnt = min(s_cnt, MV_MAX_ROWS);

    // ---- 2. order: sorted[i], i < cnt, descending ----
    const unsigned long long *sorted = skeys;
    if (cnt > 0 && cnt <= MV_RANK_MAX) {
        int P = 64;
        while (P < cnt) P <<= 1;
        rank_sort_desc(skeys, ssort, cnt, P, srank);
        sorted = ssort;
    } else if (cnt > MV_RANK_MAX) {
        int P = 2 * MV_RANK_MAX;
        while (P < cnt) P <<= 1;
        for (int i = cnt + tid; i < P; i += NT) skeys[i] = 0ull;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (P >> 1); t += NT) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), q = i | j;
                    const unsigned long long a = skeys[i], b = skeys[q];
                    const bool desc = (i & k) == 0;
                    if ((a < b) == desc) {
                        skeys[i] = b;
                        skeys[q] = a;
                    }
                }
                __syncthreads();
            }
        }
    }

    // ---- 3. gather the sorted candidates into the workspace ----
    MvRec *recs = p.recs + (long long)n * p.rec_cap;
    for (int i = tid; i < cnt; i += NT) {
        const unsigned int idx = 0xffffffffu - (unsigned int)sorted[i];
        const unsigned int v = idx / (unsigned int)K;
        const float *d = p.dets + (long long)idx * 6;
        const float ox = (float)p.views[3 * v + 1], oy = (float)p.views[3 * v + 2];
        MvRec rec;
        rec.box[0] = d[2] + ox;
        rec.box[1] = d[3] + oy;
        rec.box[2] = d[4] + ox;
        rec.box[3] = d[5] + oy;
        rec.cls = (int)d[0];
        rec.idx = idx;
        rec.pad[0] = rec.pad[1] = 0;
        recs[i] = rec;
    }
    __syncthreads();      // this workgroup's own global stores, read back below

    // ---- 4. greedy scan ----
    // Candidate j is selected iff metric(j, k) <= thr for EVERY already selected k (of its class, unless class-agnostic);
    // `!(metric <= thr)` suppresses, so a NaN metric does.
    int nkept = 0;
    for (int c0 = 0; c0 < cnt && nkept < p.keep_k; c0 += MV_CHUNK) {
        const int nc = min(MV_CHUNK, cnt - c0);
        const bool valid = lane < nc;
        const MvRec me = recs[valid ? c0 + lane : c0];
        const floatx4 bj = me.box;
        const int cj = me.cls;
        bool bad = false;
        for (int k = wv; k < nkept; k += NT / 64)
            bad |= (p.agnostic || s_kcls[k] == cj) && !(mv_metric(bj, s_kbox[k], p.norm, p.ios) <= p.thr);
        if (bad && valid) atomicOr(&s_supp[lane], 1u);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = 4 * wv + q;      // column i of the chunk's own matrix: every wave holds the whole chunk in its lanes
            floatx4 bi;
            bi[0] = mv_lane_f(bj[0], i);
            bi[1] = mv_lane_f(bj[1], i);
            bi[2] = mv_lane_f(bj[2], i);
            bi[3] = mv_lane_f(bj[3], i);
            const int ci = __builtin_amdgcn_readlane(cj, i);
            const bool hit = valid && lane > i && i < nc && (p.agnostic || ci == cj) && !(mv_metric(bj, bi, p.norm, p.ios) <= p.thr);
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
            if ((kept >> lane) & 1ull) {      // nkept < keep_k <= KMAX at the top of the loop: the position is < MV_KEEP_CAP
                const int pos = nkept + __popcll(kept & ((1ull << lane) - 1ull));
                s_kbox[pos] = bj;
                s_kcls[pos] = cj;
                s_kidx[pos] = me.idx;
            }
            s_supp[lane] = 0u;
            if (lane == 0) s_nkept = nkept + __popcll(kept);
        }
        __syncthreads();
        nkept = s_nkept;
    }

    // ---- 5. store ----
    const int nout = min(nkept, p.keep_k);
    for (int i = tid; i < p.keep_k; i += NT) {
        float *o = odets + i * 6;
        if (i < nout) {
            const unsigned int idx = s_kidx[i];
            const unsigned int v = idx / (unsigned int)K;
            const float *d = p.dets + (long long)idx * 6;
            const floatx4 b = s_kbox[i];
            o[0] = d[0];
            o[1] = d[1];
            o[2] = b[0]; o[3] = b[1]; o[4] = b[2]; o[5] = b[3];
            osrc[2 * i] = (int)v;
            osrc[2 * i + 1] = (int)(idx - v * (unsigned int)K);
        } else {
            o[0] = o[1] = o[2] = o[3] = o[4] = o[5] = -1.0f;
            osrc[2 * i] = osrc[2 * i + 1] = -1;
        }
    }
    if (tid == 0) p.out_count[n] = nout;
}

int mv_rec_cap(int V, int K) {
    const long long rows = (long long)V * K;
    return (int)(rows < MV_MAX_ROWS ? rows : MV_MAX_ROWS);
}

}  // namespace

extern "C" size_t ppy_merge_views_workspace_bytes(int n, int V, int K) {
    if (n < 1 || V < 1 || K < 1) return 0;
    return (size_t)n * mv_rec_cap(V, K) * MV_REC_BYTES;
}

extern "C" int ppy_merge_views_f32(const float *dets, const int *count, int V, int K, const int *h_views, const int *views, int n,
                                   int metric, float thresh, float score_thresh, int class_agnostic, int keep_top_k,
                                   float *out_dets, int *out_count, int *out_src, void *ws, size_t ws_bytes, char *h_reason,
                                   void *stream) {
    ppy_drop_stale_error();
    char local[96];
    char *r = h_reason ? h_reason : local;
    r[0] = 0;
    if (K < 1) {
        snprintf(r, 96, "K = %d rows per view, must be at least 1", K);
        return PPY_ERR_UNSUPPORTED;
    }
    if (keep_top_k < 1 || keep_top_k > KMAX) {
        snprintf(r, 96, "keep_top_k = %d, supported: 1..%d", keep_top_k, KMAX);
        return PPY_ERR_UNSUPPORTED;
    }
    if (metric != PPY_MERGE_IOU && metric != PPY_MERGE_IOS) {
        snprintf(r, 96, "metric code %d, known: %d (iou), %d (ios)", metric, PPY_MERGE_IOU, PPY_MERGE_IOS);
        return PPY_ERR_UNSUPPORTED;
    }
    if (thresh != thresh) {
        snprintf(r, 96, "thresh is NaN");
        return PPY_ERR_UNSUPPORTED;
    }
    if (score_thresh != score_thresh) {
        snprintf(r, 96, "score_thresh is NaN");
        return PPY_ERR_UNSUPPORTED;
    }
    // (the limits above come first: with K = 0 there are no rows, and a caller's empty tensor has no address)
    PPY_CHECK_ARG(dets && count && h_views && views && out_dets && out_count && out_src);
    PPY_CHECK_ARG(n >= 1 && n <= 65535 && V >= 1);
    PPY_CHECK_ARG((long long)V * K < (1ll << 31));      // view * K + row is a 32-bit field of the key
    // rows per image: every image's key stage is MV_MAX_ROWS.  Counted per image in one pass over the table; n <= 65535.
    {
        std::vector<int> per_image(n, 0);
        for (int v = 0; v < V; ++v) {
            const int im = h_views[3 * v];
            if (im == -1) continue;
            PPY_CHECK_ARG(im >= 0 && im < n);
            ++per_image[im];
        }
        for (int i = 0; i < n; ++i) {
            if ((long long)per_image[i] * K > MV_MAX_ROWS) {
                snprintf(r, 96, "image %d: %d views x %d rows = %lld rows, at most %d", i, per_image[i], K,
                         (long long)per_image[i] * K, MV_MAX_ROWS);
                return PPY_ERR_UNSUPPORTED;
            }
        }
    }
    if (!ws || ((uintptr_t)ws & 15) != 0 || ws_bytes < ppy_merge_views_workspace_bytes(n, V, K)) return PPY_ERR_WORKSPACE;
    MvArgs p;
    p.dets = dets; p.count = count; p.views = views;
    p.out_dets = out_dets; p.out_count = out_count; p.out_src = out_src;
    p.recs = reinterpret_cast<MvRec *>(ws);
    p.V = V; p.K = K; p.n = n; p.keep_k = keep_top_k; p.rec_cap = mv_rec_cap(V, K);
    p.ios = metric == PPY_MERGE_IOS ? 1 : 0;
    p.agnostic = class_agnostic ? 1 : 0;
    p.thr = thresh; p.score_thr = score_thresh; p.norm = 0.0f;
    static PpyLdsAttr attr;
    if (ppy_lds_attr(attr, reinterpret_cast<const void *>(mv_merge_kernel), MV_MAX_ROWS * 8) != PPY_OK) return PPY_ERR_LAUNCH;
    hipLaunchKernelGGL(mv_merge_kernel, dim3(n), dim3(NT), MV_MAX_ROWS * 8, (hipStream_t)stream, p);
    return ppy_launch_status();
}
