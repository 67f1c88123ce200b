// Weighted boxes fusion across views for test-time augmentation on gfx950: the rows that forward_padded wrote for a batch of
// VIEWS (the whole image at several input sides, plain and mirrored) are brought to image coordinates and FUSED per image, on the
// device: clusters grow in score order, each row is matched against the clusters' CURRENT fused boxes, a cluster's box is the
// score-weighted mean of its members and its confidence falls where only some views saw the object.  DESIGN.md section 10i has
// the contract; tests/fuse_views_ref.py restates it in numpy and the kernel agrees with it bit for bit.
//
// One launch, one workgroup of 1024 threads per image.  The admit, order and gather stages are those of merge_views.hip,
// restated here with the weighted score as the key (merge_views.hip itself is untouched):
//   1  admit     as merge_views, plus: score > 0 and a transformed box with x1 > x0 and y1 > y0.  Key: (key of s = score *
//                view_weight, ~(view * K + row)).  Every wave also sums the image's view weights in table order (wsum).
//   2  order     by that key, descending (counting sort up to FV_RANK_MAX keys, bitonic network beyond).
//   3  partition a second sort by (class ascending, position of step 2 ascending): a stable partition by class.  Classes are
//                independent, and within a class the rows keep the order of step 2.
//   4  gather    the partitioned rows' transformed box, class, s and (view * K + row) go to the workspace, 32 bytes each.
//   5  cluster   a class segment is walked by ONE wave, row after row (the contract is sequential in a class); waves take the
//                segments from an LDS counter, so there is no workgroup barrier per row.  The fused boxes of the clusters live in
//                LDS (the 128 KB the sorts used): lanes stride over the segment's clusters, the best match (largest IoU strictly
//                above thresh, earliest cluster on a tie) comes from a cross-lane reduction, lane 0 updates the sums (workspace)
//                and the fused box (LDS).  Cluster c of the segment that starts at partitioned position j0 owns slot j0 + c: a
//                segment has no more clusters than rows, so no allocation and no dependence on which wave ran it.
//   6  output    the clusters' (confidence key, ~slot) are sorted once more: confidence descending, then class ascending, then
//                creation order (slots ascend in both); the first keep_top_k are stored.
// fp32, one rounding per operation: this file is compiled without contraction.  No floating-point atomics anywhere.
#include <cstdio>
#include <vector>

#include "common.h"
#include "nms_select.h"
#pragma clang fp contract(off)

namespace {

constexpr int FV_MAX_ROWS = PPY_MERGE_MAX_ROWS;      // rows of one image (its views x K)
constexpr int FV_RANK_MAX = PPY_MERGE_RANK_MAX;      // up to here the counting sort, beyond it the bitonic network
static_assert(FV_RANK_MAX == KMAX && PPY_MERGE_MAX_KEEP == KMAX && FV_MAX_ROWS == 8192, "the header's constants are the kernel's");
constexpr int FV_POS_BITS = 13;                      // a position < FV_MAX_ROWS
constexpr int FV_LDS_BYTES = 2 * FV_MAX_ROWS * 8;    // two key stages of 64 KB; afterwards FV_MAX_ROWS fused boxes of 16 bytes
constexpr int FV_NONE = 0x7fffffff;

struct FvRec {                                 // a gathered row, 32 bytes
    floatx4 box;
    int cls;
    unsigned int idx;                          // view * K + row
    float s;                                   // score * view_weight
    int pad;
};
struct FvClus {                                // a cluster slot, 32 bytes.  While it grows: a = S, b = X; stored: a = conf, b = fused
    float a;
    float b[4];
    int members;                               // T; 0 = the slot holds no cluster
    unsigned int first;                        // view * K + row of the first member
    int pad;
};
static_assert(sizeof(FvRec) == 32 && sizeof(FvClus) == 32, "record layout");

struct FvArgs {
    const float *dets, *weight;
    const int *count, *views;
    float *out_dets;
    int *out_count, *out_src, *out_members;
    FvRec *recs;                               // [n][rec_cap]
    FvClus *clus;                              // [n][rec_cap]
    int V, K, n, keep_k, rec_cap;
    float thr, score_thr, norm;                // norm = 0, kept as an operand as in merge_views.hip
};

__device__ __forceinline__ float fv_min(float a, float b) { return b < a ? b : a; }      // std::min / std::max
__device__ __forceinline__ float fv_max(float a, float b) { return a < b ? b : a; }
__device__ __forceinline__ bool fv_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }

__device__ __forceinline__ float fv_area(const floatx4 b, float norm) {
    if (b[2] < b[0] || b[3] < b[1]) return 0.0f;
    return ((b[2] - b[0]) + norm) * ((b[3] - b[1]) + norm);
}

// a = the row, b = a cluster's fused box: PaddleDetection's JaccardOverlap, as merge_views.hip's 'iou'
__device__ __forceinline__ float fv_iou(const floatx4 a, const floatx4 b, float norm) {
    if (b[0] > a[2] || b[2] < a[0] || b[1] > a[3] || b[3] < a[1]) return 0.0f;
    const float iw = (fv_min(a[2], b[2]) - fv_max(a[0], b[0])) + norm;
    const float ih = (fv_min(a[3], b[3]) - fv_max(a[1], b[1])) + norm;
    const float inter = iw * ih;
    return inter / ((fv_area(a, norm) + fv_area(b, norm)) - inter);
}

__device__ __forceinline__ float fv_lane_f(float v, int src) {      // v of lane `src` (wave-uniform)
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// The row's box in image coordinates: mirrored in the view if mirror_w > 0, then moved to the view's origin.
__device__ __forceinline__ floatx4 fv_transform(const float *d, const int *view) {
    float x0 = d[2], x1 = d[4];
    const int mw = view[3];
    if (mw > 0) {
        const float w = (float)mw, nx0 = w - x1, nx1 = w - x0;
        x0 = nx0;
        x1 = nx1;
    }
    const float ox = (float)view[1], oy = (float)view[2];
    floatx4 b;
    b[0] = x0 + ox;
    b[1] = d[3] + oy;
    b[2] = x1 + ox;
    b[3] = d[5] + oy;
    return b;
}

// cnt distinct non-zero keys in keys[] ([FV_MAX_ROWS]), sorted in place, descending.  Called by all NT threads.
__device__ __forceinline__ void fv_sort_desc(unsigned long long *keys, int cnt, unsigned long long *ssort, int *srank) {
    const int tid = threadIdx.x;
    if (cnt > 0 && cnt <= FV_RANK_MAX) {
        int P = 64;
        while (P < cnt) P <<= 1;
        rank_sort_desc(keys, ssort, cnt, P, srank);
        for (int i = tid; i < cnt; i += NT) keys[i] = ssort[i];
        __syncthreads();
    } else if (cnt > FV_RANK_MAX) {
        int P = 2 * FV_RANK_MAX;
        while (P < cnt) P <<= 1;
        for (int i = cnt + tid; i < P; i += NT) keys[i] = 0ull;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (P >> 1); t += NT) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), q = i | j;
                    const unsigned long long a = keys[i], b = keys[q];
                    const bool desc = (i & k) == 0;
                    if ((a < b) == desc) {
                        keys[i] = b;
                        keys[q] = a;
                    }
                }
                __syncthreads();
            }
        }
    }
}

// One class segment, by one wave: the rows at partitioned positions j0, j0 + 1, ... while the class stays, in that order.
__device__ __forceinline__ void fv_segment(const FvArgs &p, const FvRec *recs, FvClus *clus, floatx4 *fused, int j0, int cnt,
                                           float wsum) {
    const int lane = threadIdx.x & 63;
    const int segcls = recs[j0].cls;
    floatx4 *fz = fused + j0;
    FvClus *cl = clus + j0;
    int nc = 0, len = 0;
    for (int c0 = j0;; c0 += 64) {
        const int jj = c0 + lane;
        const FvRec me = recs[jj < cnt ? jj : j0];
        const unsigned long long other = __ballot(!(jj < cnt && me.cls == segcls));
        const int nrows = other ? __ffsll((long long)other) - 1 : 64;
        for (int i = 0; i < nrows; ++i) {
            floatx4 b;
            b[0] = fv_lane_f(me.box[0], i);
            b[1] = fv_lane_f(me.box[1], i);
            b[2] = fv_lane_f(me.box[2], i);
            b[3] = fv_lane_f(me.box[3], i);
            float best = 0.0f;
            int bc = FV_NONE;
            for (int c = lane; c < nc; c += 64) {          // ascending in a lane: `>` keeps the earliest of equals
                const float m = fv_iou(b, fz[c], p.norm);
                if (m > p.thr && (bc == FV_NONE || m > best)) {      // a NaN IoU fails `m > thr`
                    best = m;
                    bc = c;
                }
            }
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const float om = __shfl_xor(best, d);
                const int oc = __shfl_xor(bc, d);
                if (oc != FV_NONE && (bc == FV_NONE || om > best || (om == best && oc < bc))) {
                    best = om;
                    bc = oc;
                }
            }
            const float s = fv_lane_f(me.s, i);
            const unsigned int first = (unsigned int)__builtin_amdgcn_readlane((int)me.idx, i);
            if (lane == 0) {
                if (bc != FV_NONE) {
                    FvClus c = cl[bc];
                    c.a = c.a + s;
                    floatx4 f;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float t = s * b[k];
                        c.b[k] = c.b[k] + t;
                        f[k] = c.b[k] / c.a;
                    }
                    c.members += 1;
                    cl[bc] = c;
                    fz[bc] = f;
                } else {
                    FvClus c;
                    c.a = s;
#pragma unroll
                    for (int k = 0; k < 4; ++k) c.b[k] = s * b[k];
                    c.members = 1;
                    c.first = first;
                    c.pad = 0;
                    cl[nc] = c;
                    fz[nc] = b;                             // the row's box, bit for bit
                }
            }
            nc += bc == FV_NONE ? 1 : 0;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");      // lane 0's LDS store, read by every lane for the next row
        }
        len += nrows;
        if (nrows < 64) break;
    }
    __threadfence_block();      // lane 0's stores to the workspace, read by the other lanes below
    // every slot of the segment: a cluster's confidence and final box, or "no cluster"
    for (int c = lane; c < len; c += 64) {
        FvClus o;
        if (c < nc) {
            const FvClus g = cl[c];
            const float tf = (float)g.members;
            const float q = g.a / tf;
            const float m = wsum < tf ? wsum : tf;          // std::min(T, wsum)
            o.a = (q * m) / wsum;
            const floatx4 f = fz[c];
            o.b[0] = f[0]; o.b[1] = f[1]; o.b[2] = f[2]; o.b[3] = f[3];
            o.members = g.members;
            o.first = g.first;
        } else {
            o.a = 0.0f;
            o.b[0] = o.b[1] = o.b[2] = o.b[3] = 0.0f;
            o.members = 0;
            o.first = 0u;
        }
        o.pad = 0;
        cl[c] = o;
    }
}

__global__ void __launch_bounds__(NT) fv_fuse_kernel(const FvArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sdyn[];                       // [2][FV_MAX_ROWS] keys; later [FV_MAX_ROWS] floatx4
    __shared__ unsigned long long ssort[KMAX];                          // the counting sort's output
    __shared__ int srank[KMAX];
    __shared__ int s_cnt, s_next, s_ncl;

    unsigned long long *keyA = sdyn, *keyB = sdyn + FV_MAX_ROWS;
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int K = p.K;

    // ---- 1. admit; wsum ----
    if (tid == 0) { s_cnt = 0; s_next = 0; s_ncl = 0; }
    __syncthreads();
    float wsum = 0.0f;
    int turn = 0;      // the image's views with rows, in table order, are dealt to the waves in turn
    for (int base = 0; base < p.V; base += 64) {
        const int v = base + lane;
        const bool mine = v < p.V && p.views[4 * v] == n;
        const float w = mine ? p.weight[v] : 0.0f;
        int c = 0;
        if (mine) c = min(p.count[v], K);
        unsigned long long all = __ballot(mine);
        while (all) {                                   // fp32, in table order, the same in every wave
            const int l = __ffsll((long long)all) - 1;
            all &= all - 1ull;
            wsum = wsum + fv_lane_f(w, l);
        }
        unsigned long long todo = __ballot(c > 0);
        while (todo) {
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            if ((turn++ & (NT / 64 - 1)) != wv) continue;
            const int cv = __builtin_amdgcn_readlane(c, l), vv = base + l;
            const float wv_ = fv_lane_f(w, l);
            const float *rows = p.dets + (long long)vv * K * 6;
            const int *view = p.views + 4 * vv;
            for (int r = lane; r < cv; r += 64) {
                const float *d = rows + r * 6;
                const float cls = d[0], score = d[1];
                bool ok = fv_finite(cls) && fv_finite(score) && fv_finite(d[2]) && fv_finite(d[3]) && fv_finite(d[4]) &&
                          fv_finite(d[5]) && cls >= 0.0f && cls < 16777216.0f && score >= p.score_thr && score > 0.0f;
                if (ok) {
                    const floatx4 b = fv_transform(d, view);
                    ok = b[2] > b[0] && b[3] > b[1];
                }
                if (ok) {
                    const float s = score * wv_;
                    const unsigned int idx = (unsigned int)vv * (unsigned int)K + (unsigned int)r;
                    const int pos = atomicAdd(&s_cnt, 1);
                    if (pos < FV_MAX_ROWS)      // (always: the host refuses an image with more rows)
                        keyA[pos] = ((unsigned long long)score_to_key(s) << 32) | (unsigned long long)(0xffffffffu - idx);
                }
            }
        }
    }
    __syncthreads();
    const int cnt = min(s_cnt, FV_MAX_ROWS);

    // ---- 2. order ----
    fv_sort_desc(keyA, cnt, ssort, srank);

    // ---- 3. stable partition by class: (class ascending, position ascending) as a descending key ----
    for (int i = tid; i < cnt; i += NT) {
        const unsigned int idx = 0xffffffffu - (unsigned int)keyA[i];
        const unsigned int cls = (unsigned int)(int)p.dets[(long long)idx * 6];      // < 2^24
        keyB[i] = (1ull << 40) | ((unsigned long long)(0xffffffu - cls) << FV_POS_BITS) | (unsigned long long)(FV_MAX_ROWS - 1 - i);
    }
    __syncthreads();
    fv_sort_desc(keyB, cnt, ssort, srank);

    // ---- 4. gather ----
    FvRec *recs = p.recs + (long long)n * p.rec_cap;
    FvClus *clus = p.clus + (long long)n * p.rec_cap;
    for (int j = tid; j < cnt; j += NT) {
        const int pos = FV_MAX_ROWS - 1 - (int)(keyB[j] & (unsigned long long)(FV_MAX_ROWS - 1));
        const unsigned int idx = 0xffffffffu - (unsigned int)keyA[pos];
        const unsigned int v = idx / (unsigned int)K;
        const float *d = p.dets + (long long)idx * 6;
        FvRec rec;
        rec.box = fv_transform(d, p.views + 4 * v);
        rec.cls = (int)d[0];
        rec.idx = idx;
        rec.s = d[1] * p.weight[v];
        rec.pad = 0;
        recs[j] = rec;
    }
    __syncthreads();      // this workgroup's own global stores, read back below; and the key stages are free from here

    // ---- 5. clusters: a wave per class segment ----
    floatx4 *fused = reinterpret_cast<floatx4 *>(sdyn);
    for (;;) {
        int blk = 0;
        if (lane == 0) blk = atomicAdd(&s_next, 64);
        blk = __builtin_amdgcn_readfirstlane(blk);
        if (blk >= cnt) break;
        const int j = blk + lane;
        bool head = false;
        if (j < cnt) head = j == 0 || recs[j].cls != recs[j - 1].cls;
        unsigned long long heads = __ballot(head);
        while (heads) {
            const int l = __ffsll((long long)heads) - 1;
            heads &= heads - 1ull;
            fv_segment(p, recs, clus, fused, blk + l, cnt, wsum);
        }
    }
    __threadfence_block();
    __syncthreads();

    // ---- 6. output: confidence descending, then slot ascending (= class ascending, then creation order) ----
    for (int j = tid; j < cnt; j += NT) {
        const FvClus c = clus[j];
        if (c.members > 0) {
            const int pos = atomicAdd(&s_ncl, 1);
            keyA[pos] = ((unsigned long long)score_to_key(c.a) << 32) | (unsigned long long)(0xffffffffu - (unsigned int)j);
        }
    }
    __syncthreads();
    const int ncl = s_ncl;
    fv_sort_desc(keyA, ncl, ssort, srank);
    const int nout = min(ncl, p.keep_k);
    float *odets = p.out_dets + (long long)n * p.keep_k * 6;
    int *osrc = p.out_src + (long long)n * p.keep_k * 2;
    int *omem = p.out_members + (long long)n * p.keep_k;
    for (int i = tid; i < p.keep_k; i += NT) {
        float *o = odets + i * 6;
        if (i < nout) {
            const unsigned int slot = 0xffffffffu - (unsigned int)keyA[i];
            const FvClus c = clus[slot];
            const unsigned int v = c.first / (unsigned int)K;
            o[0] = (float)recs[slot].cls;      // a slot's row is of the slot's segment
            o[1] = c.a;
            o[2] = c.b[0]; o[3] = c.b[1]; o[4] = c.b[2]; o[5] = c.b[3];
            osrc[2 * i] = (int)v;
            osrc[2 * i + 1] = (int)(c.first - v * (unsigned int)K);
            omem[i] = c.members;
        } else {
            o[0] = o[1] = o[2] = o[3] = o[4] = o[5] = -1.0f;
            osrc[2 * i] = osrc[2 * i + 1] = -1;
            omem[i] = -1;
        }
    }
    if (tid == 0) p.out_count[n] = nout;
}

int fv_rec_cap(int V, int K) {
    const long long rows = (long long)V * K;
    return (int)(rows < FV_MAX_ROWS ? rows : FV_MAX_ROWS);
}

}  // namespace

extern "C" size_t ppy_fuse_views_workspace_bytes(int n, int V, int K) {
    if (n < 1 || V < 1 || K < 1) return 0;
    return (size_t)n * fv_rec_cap(V, K) * (sizeof(FvRec) + sizeof(FvClus));
}

extern "C" int ppy_fuse_views_f32(const float *dets, const int *count, int V, int K, const int *h_views, const int *views,
                                  const float *h_view_weight, const float *view_weight, int n, float thresh, float score_thresh,
                                  int keep_top_k, float *out_dets, int *out_count, int *out_src, int *out_members, void *ws,
                                  size_t ws_bytes, char *h_reason, void *stream) {
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
    if (thresh != thresh) {
        snprintf(r, 96, "thresh is NaN");
        return PPY_ERR_UNSUPPORTED;
    }
    if (score_thresh != score_thresh) {
        snprintf(r, 96, "score_thresh is NaN");
        return PPY_ERR_UNSUPPORTED;
    }
    PPY_CHECK_ARG(dets && count && h_views && views && h_view_weight && view_weight && out_dets && out_count && out_src && out_members);
    PPY_CHECK_ARG(n >= 1 && n <= 65535 && V >= 1);
    PPY_CHECK_ARG((long long)V * K < (1ll << 31));      // view * K + row is a 32-bit field of the key
    {
        std::vector<int> per_image(n, 0);
        for (int v = 0; v < V; ++v) {
            const int im = h_views[4 * v];
            if (im == -1) continue;                    // a padding view: nothing of it is read
            PPY_CHECK_ARG(im >= 0 && im < n);
            if (h_views[4 * v + 3] < 0) {
                snprintf(r, 96, "view %d: mirror_w = %d, must be 0 (plain) or the mirrored width", v, h_views[4 * v + 3]);
                return PPY_ERR_UNSUPPORTED;
            }
            const float w = h_view_weight[v];
            if (!(w > 0.0f && w <= 3.402823466e+38f)) {
                snprintf(r, 96, "view %d: weight %g, must be finite and positive", v, (double)w);
                return PPY_ERR_UNSUPPORTED;
            }
            ++per_image[im];
        }
        for (int i = 0; i < n; ++i) {
            if ((long long)per_image[i] * K > FV_MAX_ROWS) {
                snprintf(r, 96, "image %d: %d views x %d rows = %lld rows, at most %d", i, per_image[i], K,
                         (long long)per_image[i] * K, FV_MAX_ROWS);
                return PPY_ERR_UNSUPPORTED;
            }
        }
    }
    if (!ws || ((uintptr_t)ws & 15) != 0 || ws_bytes < ppy_fuse_views_workspace_bytes(n, V, K)) return PPY_ERR_WORKSPACE;
    FvArgs p;
    p.dets = dets; p.weight = view_weight; p.count = count; p.views = views;
    p.out_dets = out_dets; p.out_count = out_count; p.out_src = out_src; p.out_members = out_members;
    p.rec_cap = fv_rec_cap(V, K);
    p.recs = reinterpret_cast<FvRec *>(ws);
    p.clus = reinterpret_cast<FvClus *>(static_cast<char *>(ws) + (size_t)n * p.rec_cap * sizeof(FvRec));
    p.V = V; p.K = K; p.n = n; p.keep_k = keep_top_k;
    p.thr = thresh; p.score_thr = score_thresh; p.norm = 0.0f;
    static PpyLdsAttr attr;
    if (ppy_lds_attr(attr, reinterpret_cast<const void *>(fv_fuse_kernel), FV_LDS_BYTES) != PPY_OK) return PPY_ERR_LAUNCH;
    hipLaunchKernelGGL(fv_fuse_kernel, dim3(n), dim3(NT), FV_LDS_BYTES, (hipStream_t)stream, p);
    return ppy_launch_status();
}
