// COCO bbox evaluation on the device (ppyolo_hip/cocoeval.py): pycocotools COCOeval(cocoGt, cocoDt, 'bbox') evaluate() +
// accumulate() with its default Params, bit for bit in float64 (tests/cocoeval_ref.py restates it).
//
// records kernel  forward_padded rows -> detection records: the reference writer's arithmetic (tools/cocotools.py):
//                 w = xmax - xmin + 1 in float32, every bbox entry round(double(v) * 10) / 10, score double(float32),
//                 area = w * h of the rounded entries (COCO.loadRes), pair = image index * K + category index.
// group           bitonic sort of (pair, score desc, record index): one key per record, unique, so the sorted order is
//                 the stable order pycocotools' mergesort gives; segment bounds per pair from neighbour compares.
// match           one wave per (image, category) pair: 40 greedy chains (area range x threshold) in 40 lanes walk the
//                 first maxDet detections; the wave computes each detection's IoU row with the pair's GTs into dynamic
//                 LDS sized to the caller's largest pair (pairs beyond it recompute: same double ops either way).  Per
//                 detection and chain one status byte: 0 ignored, 1 TP, 2 FP.
// accumulate      second bitonic sort of the truncated lists by (category, score desc, position in the pair order), i.e.
//                 (score desc, image, rank); one wave per (category, area, maxDet, threshold) scans it with ballots and
//                 records p_v = v / ((f_v + v) + eps) at the v-th TP (f_v: FPs ahead of it), then takes the suffix max
//                 and picks recall threshold r at v_r = min{v : v / npig >= recThrs[r]} -- the envelope of pr sampled by
//                 searchsorted, without an array per detection.
// Phases meet only across launches; no float atomics, no integer atomics.
#include "common.h"

namespace {

#pragma clang fp contract(off)

struct SortElem {
    unsigned long long key;         // score, order-preserving and inverted: ascending key = descending score
    unsigned int grp;               // pair (group sort) or category (accumulate sort); 0xffffffff = not an element
    unsigned int idx;               // record index (group sort) or position in the group order (accumulate sort)
};

constexpr int TILE = 2048;          // elements one workgroup sorts / merges in LDS (2048 x 16 B = 32 KB)
constexpr int MAX_CHAINS = 64;      // area ranges x IoU thresholds, one lane each
constexpr int ROW_GTS_MAX = 4096;   // IoUs of one detection row kept in LDS (32 KB of dynamic LDS at most)
constexpr unsigned NONE = 0xffffffffu;

__device__ __forceinline__ bool elem_less(const SortElem &a, const SortElem &b) {
    if (a.grp != b.grp) return a.grp < b.grp;
    if (a.key != b.key) return a.key < b.key;
    return a.idx < b.idx;
}

__device__ __forceinline__ unsigned long long score_key(double s) {
    if (s == 0.0) s = 0.0;          // -0.0 and 0.0 compare equal in numpy's sort: one key
    const unsigned long long b = (unsigned long long)__double_as_longlong(s);
    const unsigned long long asc = (b >> 63) ? ~b : (b | (1ull << 63));
    return ~asc;
}

__device__ __forceinline__ void cmp_swap(SortElem &a, SortElem &b, bool asc) {
    if (elem_less(b, a) == asc) {
        const SortElem t = a;
        a = b;
        b = t;
    }
}

// compare-exchange of s[lo] and s[lo + j] in LDS through registers
__device__ __forceinline__ void exchange(SortElem *s, int lo, int j, bool asc) {
    const SortElem a = s[lo], b = s[lo + j];
    if (elem_less(b, a) == asc) {
        s[lo] = b;
        s[lo + j] = a;
    }
}

// t-th compare pair of a bitonic step with distance j: lo has bit j clear
__device__ __forceinline__ long long pair_lo(long long t, long long j) { return ((t & ~(j - 1)) << 1) | (t & (j - 1)); }

// every tile sorted by the global bitonic pattern for k = 2 .. TILE
__global__ __launch_bounds__(1024) void bitonic_tile_kernel(SortElem *e) {
    __shared__ SortElem s[TILE];
    const long long base = (long long)blockIdx.x * TILE;
    for (int i = threadIdx.x; i < TILE; i += 1024) s[i] = e[base + i];
    __syncthreads();
    for (int k = 2; k <= TILE; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int lo = (int)pair_lo(threadIdx.x, j);
            exchange(s, lo, j, ((base + lo) & k) == 0);
            __syncthreads();
        }
    for (int i = threadIdx.x; i < TILE; i += 1024) e[base + i] = s[i];
}

// one step k, j >= TILE over the whole array
__global__ __launch_bounds__(256) void bitonic_step_kernel(SortElem *e, long long half, long long k, long long j) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= half) return;
    const long long lo = pair_lo(t, j);
    SortElem a = e[lo], b = e[lo + j];
    cmp_swap(a, b, (lo & k) == 0);
    e[lo] = a;
    e[lo + j] = b;
}

// the steps j = TILE / 2 .. 1 of stage k inside each tile
__global__ __launch_bounds__(1024) void bitonic_merge_kernel(SortElem *e, long long k) {
    __shared__ SortElem s[TILE];
    const long long base = (long long)blockIdx.x * TILE;
    for (int i = threadIdx.x; i < TILE; i += 1024) s[i] = e[base + i];
    __syncthreads();
    for (int j = TILE >> 1; j > 0; j >>= 1) {
        const int lo = (int)pair_lo(threadIdx.x, j);
        exchange(s, lo, j, ((base + lo) & k) == 0);
        __syncthreads();
    }
    for (int i = threadIdx.x; i < TILE; i += 1024) e[base + i] = s[i];
}

int bitonic_sort(SortElem *e, long long n_pad, hipStream_t st) {
    hipLaunchKernelGGL(bitonic_tile_kernel, dim3((unsigned)(n_pad / TILE)), dim3(1024), 0, st, e);
    const long long half = n_pad / 2;
    for (long long k = 2 * TILE; k <= n_pad; k <<= 1) {
        for (long long j = k >> 1; j >= TILE; j >>= 1)
            hipLaunchKernelGGL(bitonic_step_kernel, dim3((unsigned)((half + 255) / 256)), dim3(256), 0, st, e, half, k, j);
        hipLaunchKernelGGL(bitonic_merge_kernel, dim3((unsigned)(n_pad / TILE)), dim3(1024), 0, st, e, k);
    }
    return ppy_launch_status();
}

__device__ __forceinline__ double round_tenth(float v) {
    double r = rint((double)v * 10.0) / 10.0;           // Python round(): half to even; int / 10 is correctly rounded
    if (r == 0.0) r = 0.0;                              // round() returns the int 0, never -0.0
    return r;
}

__global__ __launch_bounds__(256) void records_kernel(const float *dets, int n, int keep_k, const int *count,
                                                      const int *img_index, const int *cls2cat, int num_classes, int K,
                                                      double *rec, int *pair, int *bad) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)n * keep_k) return;
    const int i = (int)(t / keep_k), row = (int)(t % keep_k);
    const float *d = dets + t * 6;
    double *o = rec + t * 6;
    int p = -1;
    const int img = img_index[i];
    if (row < count[i] && img >= 0) {
        const float lab = d[0], sc = d[1];
        const float x0 = d[2], y0 = d[3], x1 = d[4], y1 = d[5];
        if (lab != lab || sc != sc || x0 != x0 || y0 != y0 || x1 != x1 || y1 != y1) {
            bad[0] = 1;                                 // the host raises at evaluate(), like a NaN result record
        } else {
            const float w = x1 - x0 + 1.0f, h = y1 - y0 + 1.0f;
            o[0] = round_tenth(x0);
            o[1] = round_tenth(y0);
            o[2] = round_tenth(w);
            o[3] = round_tenth(h);
            o[4] = o[2] * o[3];
            o[5] = (double)sc;
            const int c = (int)lab;
            const int k = (c >= 0 && c < num_classes) ? cls2cat[c] : -1;
            if (k >= 0 && k < K) p = img * K + k;
        }
    }
    pair[t] = p;
}

__global__ __launch_bounds__(256) void group_keys_kernel(const double *rec, const int *pair, long long n, long long n_pad,
                                                         SortElem *e) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_pad) return;
    SortElem s;
    s.key = ~0ull;
    s.grp = NONE;
    s.idx = NONE;
    if (t < n && pair[t] >= 0) {
        s.key = score_key(rec[t * 6 + 5]);
        s.grp = (unsigned)pair[t];
        s.idx = (unsigned)t;
    }
    e[t] = s;
}

// first / one-past-last sorted position of every group present (the caller zeroes both arrays)
__global__ __launch_bounds__(256) void segments_kernel(const SortElem *e, long long n_pad, int *start, int *end) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_pad) return;
    const unsigned g = e[t].grp;
    if (g == NONE) return;
    if (t == 0 || e[t - 1].grp != g) start[g] = (int)t;
    if (t == n_pad - 1 || e[t + 1].grp != g) end[g] = (int)(t + 1);
}

__device__ __forceinline__ double bb_iou(const double *d, const double *g, bool crowd) {       // maskApi.c bbIou
    const double ga = g[2] * g[3], da = d[2] * d[3];
    const double w = fmin(d[2] + d[0], g[2] + g[0]) - fmax(d[0], g[0]);
    if (w <= 0) return 0.0;
    const double h = fmin(d[3] + d[1], g[3] + g[1]) - fmax(d[1], g[1]);
    if (h <= 0) return 0.0;
    const double i = w * h;
    const double u = crowd ? da : da + ga - i;
    return i / u;
}

struct MatchArgs {
    const double *rec;
    const SortElem *s1;
    const int *seg_start, *seg_end;
    const int *gt_off;
    const double *gt_box, *gt_area;
    const int *gt_crowd, *gt_idnz;
    const double *iou_thrs, *area_rng;
    int T, A, max_det;
    int row_gts;                    // GTs per pair whose IoU row fits the dynamic LDS
    unsigned char *status;          // [sorted position][A * T]
    unsigned short *rank;           // [sorted position]: rank in its pair, 0xffff past max_det
    unsigned char *gtm;             // [gt][MAX_CHAINS] scratch
    int *npig_pair;                 // [P][A]
    unsigned char *active;          // [P]: the pair has a GT or a detection (evaluateImg does not return None)
};

__global__ __launch_bounds__(64) void match_kernel(MatchArgs m) {
    extern __shared__ double iou_row[];     // [row_gts]: IoUs of the current detection with the pair's GTs
    const int p = blockIdx.x;
    const int lane = threadIdx.x;
    const int s0 = m.seg_start[p];
    const int cnt = m.seg_end[p] - s0;
    const int nd = cnt < m.max_det ? cnt : m.max_det;
    const int g0 = m.gt_off[p], ng = m.gt_off[p + 1] - g0;
    if (lane == 0) m.active[p] = (nd > 0 || ng > 0) ? 1 : 0;
    if (lane < m.A) {
        const double lo = m.area_rng[2 * lane], hi = m.area_rng[2 * lane + 1];
        int c = 0;
        for (int g = 0; g < ng; ++g) {
            const double ar = m.gt_area[g0 + g];
            c += (!m.gt_crowd[g0 + g] && !(ar < lo || ar > hi)) ? 1 : 0;
        }
        m.npig_pair[(long long)p * m.A + lane] = c;
    }
    for (int d = lane; d < cnt; d += 64) m.rank[s0 + d] = d < m.max_det ? (unsigned short)d : (unsigned short)0xffff;
    if (nd == 0) return;
    // one row of the IoU matrix at a time, shared by the chains; a pair with more GTs than the row holds has every chain
    // compute its IoUs itself (the same double operations, so the same bits)
    const bool cached = ng <= m.row_gts;
    const bool chain = lane < m.A * m.T;
    const int a = chain ? lane / m.T : 0, ti = chain ? lane - a * m.T : 0;
    const double lo = m.area_rng[2 * a], hi = m.area_rng[2 * a + 1];
    const double thr0 = m.iou_thrs[ti] < 1 - 1e-10 ? m.iou_thrs[ti] : 1 - 1e-10;      // min([t, 1 - 1e-10])
    unsigned char *gtm = m.gtm + (long long)g0 * MAX_CHAINS + lane;
    if (chain)
        for (int g = 0; g < ng; ++g) gtm[(long long)g * MAX_CHAINS] = 0;
    for (int d = 0; d < nd; ++d) {
        const double *db = m.rec + (long long)m.s1[s0 + d].idx * 6;
        if (cached) {
            __syncthreads();                // every chain is done with the previous row
            for (int g = lane; g < ng; g += 64)
                iou_row[g] = bb_iou(db, m.gt_box + (long long)(g0 + g) * 4, m.gt_crowd[g0 + g] != 0);
            __syncthreads();
        }
        if (!chain) continue;
        double best = thr0;
        int mg = -1, mig = 0;
        bool stop = false;
        // the GTs stably sorted by ignore flag: the kept ones in order, then the ignored ones in order
        for (int pass = 0; pass < 2 && !stop; ++pass)
            for (int g = 0; g < ng; ++g) {
                const double ar = m.gt_area[g0 + g];
                const bool crowd = m.gt_crowd[g0 + g] != 0;
                const int ig = (crowd || ar < lo || ar > hi) ? 1 : 0;
                if (ig != pass) continue;
                if (gtm[(long long)g * MAX_CHAINS] && !crowd) continue;
                if (mg > -1 && mig == 0 && ig == 1) {
                    stop = true;
                    break;
                }
                const double v = cached ? iou_row[g] : bb_iou(db, m.gt_box + (long long)(g0 + g) * 4, crowd);
                if (v < best) continue;
                best = v;
                mg = g;
                mig = ig;
            }
        const bool outside = db[4] < lo || db[4] > hi;
        unsigned char st;
        if (mg == -1) {
            st = outside ? 0 : 2;
        } else {
            gtm[(long long)mg * MAX_CHAINS] = 1;
            if (m.gt_idnz[g0 + mg]) st = mig ? 0 : 1;           // dtm = the GT's id; an id of 0 reads as unmatched
            else st = (mig || outside) ? 0 : 2;
        }
        m.status[(long long)(s0 + d) * (m.A * m.T) + lane] = st;
    }
}

__global__ __launch_bounds__(256) void acc_keys_kernel(const SortElem *s1, const unsigned short *rank, long long n_pad, int K,
                                                       SortElem *s2) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_pad) return;
    const SortElem a = s1[t];
    SortElem s;
    s.key = ~0ull;
    s.grp = NONE;
    s.idx = NONE;
    if (a.grp != NONE && rank[t] != 0xffff) {
        s.key = a.key;
        s.grp = a.grp % (unsigned)K;
        s.idx = (unsigned)t;
    }
    s2[t] = s;
}

// npig and "some image has a GT or detection of the category" per (category, area): one wave each, integer sums
__global__ __launch_bounds__(64) void npig_kernel(const int *npig_pair, const unsigned char *active, int I, int K, int A,
                                                  int *npig_cat, int *active_cat) {
    const int k = blockIdx.x / A, a = blockIdx.x - k * A;
    int c = 0, act = 0;
    for (int i = threadIdx.x; i < I; i += 64) {
        const long long p = (long long)i * K + k;
        c += npig_pair[p * A + a];
        act |= active[p];
    }
    for (int o = 32; o > 0; o >>= 1) {
        c += __shfl_xor(c, o);
        act |= __shfl_xor(act, o);
    }
    if (threadIdx.x == 0) {
        npig_cat[blockIdx.x] = c;
        if (a == 0) active_cat[k] = act;
    }
}

struct AccArgs {
    const double *rec;
    const SortElem *s1, *s2;
    const unsigned short *rank;
    const unsigned char *status;
    const int *cat_start, *cat_end;
    const int *npig_cat, *active_cat;
    const int *gt_cat_off;          // [K + 1]: GTs per category, prefix (bounds the TP count)
    const double *rec_thrs;
    const int *max_dets;            // [M] (device)
    int T, R, K, A, M, G;
    double *pv, *sv;                // [A * M * T][G]: p_v and the score at the v-th TP
    double *precision, *recall, *scores;
};

__global__ __launch_bounds__(64) void accumulate_kernel(AccArgs g) {
    int b = blockIdx.x;
    const int ti = b % g.T;
    b /= g.T;
    const int mi = b % g.M;
    b /= g.M;
    const int a = b % g.A;
    const int k = b / g.A;
    const int lane = threadIdx.x;
    const long long TK = g.K, AM = (long long)g.A * g.M;
    const long long o_rec = ((long long)ti * TK + k) * AM + (long long)a * g.M + mi;            // recall[t][k][a][m]
    auto o_pr = [&](int r) { return (((long long)ti * g.R + r) * TK + k) * AM + (long long)a * g.M + mi; };
    const int npig = g.npig_cat[k * g.A + a];
    if (!g.active_cat[k] || npig == 0) {
        if (lane == 0) g.recall[o_rec] = -1.0;
        for (int r = lane; r < g.R; r += 64) {
            g.precision[o_pr(r)] = -1.0;
            g.scores[o_pr(r)] = -1.0;
        }
        return;
    }
    const int mdet = g.max_dets[mi];
    const int AT = g.A * g.T, ch = a * g.T + ti;
    const long long wbase = ((long long)(a * g.M + mi) * g.T + ti) * g.G + g.gt_cat_off[k];
    double *pv = g.pv + wbase, *sv = g.sv + wbase;                // [v - 1] for v = 1 .. npig
    const int vcap = g.gt_cat_off[k + 1] - g.gt_cat_off[k];       // TPs <= npig <= the category's GTs: the row's length
    const int c0 = g.cat_start[k], c1 = g.cat_end[k];
    int tp = 0, fp = 0, nd = 0;
    double first_score = 0.0;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int base = c0; base < c1; base += 64) {
        const int e = base + lane;
        bool present = false;
        unsigned char st = 0;
        double sc = 0.0;
        if (e < c1) {
            const unsigned i = g.s2[e].idx;
            if (g.rank[i] < mdet) {
                present = true;
                st = g.status[(long long)i * AT + ch];
                sc = g.rec[(long long)g.s1[i].idx * 6 + 5];
            }
        }
        const unsigned long long pm = __ballot(present), tm = __ballot(present && st == 1), fm = __ballot(present && st == 2);
        if (nd == 0 && pm) {
            const int first = __ffsll((long long)pm) - 1;
            first_score = __shfl(sc, first);
        }
        const int v = tp + __popcll(tm & below) + 1;
        if (present && st == 1 && v <= vcap) {
            const int f = fp + __popcll(fm & below);
            pv[v - 1] = (double)v / (((double)f + (double)v) + 2.220446049250313e-16);
            sv[v - 1] = sc;
        }
        tp += __popcll(tm);
        fp += __popcll(fm);
        nd += __popcll(pm);
    }
    __syncthreads();
    // suffix max of p_v over v = tp .. 1, in place
    double run = 0.0;
    for (int top = tp; top >= 1; top -= 64) {
        const int v = top - lane;
        double x = v >= 1 ? pv[v - 1] : 0.0;
        for (int o = 1; o < 64; o <<= 1) {             // inclusive max over lanes <= this one (higher v)
            const double y = __shfl_up(x, o);
            if (lane >= o) x = fmax(x, y);
        }
        x = fmax(x, run);
        if (v >= 1) pv[v - 1] = x;
        run = __shfl(x, 63);
    }
    __syncthreads();
    if (lane == 0) g.recall[o_rec] = nd ? (double)tp / (double)npig : 0.0;
    for (int r = lane; r < g.R; r += 64) {
        const double thr = g.rec_thrs[r];
        double q = 0.0, s = 0.0;
        if (nd > 0) {
            // v_r = min{v : v / npig >= thr} (the division numpy does on tp / npig); searchsorted lands on the v_r-th TP
            long long v = (long long)ceil(thr * (double)npig);
            if (v < 0) v = 0;
            while (v > 0 && (double)(v - 1) / (double)npig >= thr) --v;
            while (v <= (long long)npig && (double)v / (double)npig < thr) ++v;
            if (v == 0) {                               // position 0: the whole envelope, the first detection's score
                q = tp >= 1 ? pv[0] : 0.0;
                s = first_score;
            } else if (v <= tp) {
                q = pv[v - 1];
                s = sv[v - 1];
            }
        }
        g.precision[o_pr(r)] = q;
        g.scores[o_pr(r)] = s;
    }
}

constexpr size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

struct Layout {
    size_t s1, s2, seg_start, seg_end, rank, status, gtm, npig_pair, active, cat_start, cat_end, npig_cat, active_cat, pv, sv,
        total;
};

Layout layout(long long n_pad, long long P, int K, int G, int A, int T, int M) {
    Layout l;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += align_up(bytes);
        return at;
    };
    l.s1 = take(n_pad * sizeof(SortElem));
    l.s2 = take(n_pad * sizeof(SortElem));
    l.seg_start = take(P * sizeof(int));
    l.seg_end = take(P * sizeof(int));
    l.rank = take(n_pad * sizeof(unsigned short));
    l.status = take(n_pad * (size_t)(A * T));
    l.gtm = take((size_t)(G > 0 ? G : 1) * MAX_CHAINS);
    l.npig_pair = take(P * A * sizeof(int));
    l.active = take(P);
    l.cat_start = take(K * sizeof(int));
    l.cat_end = take(K * sizeof(int));
    l.npig_cat = take((size_t)K * A * sizeof(int));
    l.active_cat = take(K * sizeof(int));
    l.pv = take((size_t)A * M * T * (G > 0 ? G : 1) * sizeof(double));
    l.sv = take((size_t)A * M * T * (G > 0 ? G : 1) * sizeof(double));
    l.total = o;
    return l;
}

long long pad_pow2(long long n) {
    long long p = TILE;
    while (p < n) p <<= 1;
    return p;
}

}  // namespace

extern "C" size_t ppy_cocoeval_workspace_bytes(long long num_records, int num_images, int num_cats, int num_gts,
                                               int num_iou_thrs, int num_areas, int num_max_dets) {
    if (num_records < 0 || num_images <= 0 || num_cats <= 0 || num_gts < 0 || num_iou_thrs <= 0 || num_areas <= 0 ||
        num_max_dets <= 0)
        return 0;
    return layout(pad_pow2(num_records), (long long)num_images * num_cats, num_cats, num_gts, num_areas, num_iou_thrs,
                  num_max_dets).total;
}

extern "C" int ppy_cocoeval_records_f32(const float *dets, int n, int keep_k, const int *count, const int *img_index,
                                        const int *cls2cat, int num_classes, int num_cats, double *records, int *pair,
                                        int *bad, void *stream) {
    ppy_drop_stale_error();
    PPY_CHECK_ARG(dets && count && img_index && cls2cat && records && pair && bad && n > 0 && keep_k > 0 && num_classes > 0 &&
                  num_cats > 0);
    const long long total = (long long)n * keep_k;
    PPY_CHECK_ARG(total < (1ll << 31));
    hipLaunchKernelGGL(records_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dets, n,
                       keep_k, count, img_index, cls2cat, num_classes, num_cats, records, pair, bad);
    return ppy_launch_status();
}

extern "C" int ppy_cocoeval_bbox(const double *records, const int *pair, long long num_records, int num_images, int num_cats,
                                 const int *gt_off, const double *gt_box, const double *gt_area, const int *gt_crowd,
                                 const int *gt_idnz, const int *gt_cat_off, int num_gts, int iou_row_gts,
                                 const double *iou_thrs, int T,
                                 const double *rec_thrs, int R, const double *area_rng, int A, const int *max_dets,
                                 const int *h_max_dets, int M, double *precision, double *recall, double *scores,
                                 void *workspace, size_t workspace_bytes, void *stream) {
    ppy_drop_stale_error();
    PPY_CHECK_ARG(num_records >= 0 && (num_records == 0 || (records && pair)) && num_images > 0 && num_cats > 0 &&
                  gt_off && gt_cat_off && num_gts >= 0 && iou_row_gts >= 0 && (num_gts == 0 || (gt_box && gt_area && gt_crowd && gt_idnz)) &&
                  iou_thrs && rec_thrs && area_rng && max_dets && h_max_dets && T > 0 && R > 0 && A > 0 && M > 0 &&
                  A * T <= MAX_CHAINS && precision && recall && scores);
    const long long P = (long long)num_images * num_cats;
    const long long n_pad = pad_pow2(num_records);
    PPY_CHECK_ARG(P < (1ll << 31) - 1 && n_pad <= (1ll << 31));
    int max_det = 0;
    for (int i = 0; i < M; ++i) {
        PPY_CHECK_ARG(h_max_dets[i] > 0 && h_max_dets[i] < 0xffff);
        max_det = h_max_dets[i] > max_det ? h_max_dets[i] : max_det;
    }
    const Layout l = layout(n_pad, P, num_cats, num_gts, A, T, M);
    if (!workspace || workspace_bytes < l.total) return PPY_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    SortElem *s1 = (SortElem *)(ws + l.s1), *s2 = (SortElem *)(ws + l.s2);
    int *seg_start = (int *)(ws + l.seg_start), *seg_end = (int *)(ws + l.seg_end);
    int *cat_start = (int *)(ws + l.cat_start), *cat_end = (int *)(ws + l.cat_end);
    unsigned short *rank = (unsigned short *)(ws + l.rank);
    const unsigned nb = (unsigned)((n_pad + 255) / 256);
    // group: (pair, score desc, record index)
    hipLaunchKernelGGL(group_keys_kernel, dim3(nb), dim3(256), 0, st, records, pair, num_records, n_pad, s1);
    int rc = bitonic_sort(s1, n_pad, st);
    if (rc != PPY_OK) return rc;
    if (hipMemsetAsync(seg_start, 0, (size_t)(l.rank - l.seg_start), st) != hipSuccess) return PPY_ERR_LAUNCH;
    hipLaunchKernelGGL(segments_kernel, dim3(nb), dim3(256), 0, st, s1, n_pad, seg_start, seg_end);
    // match
    MatchArgs m;
    m.rec = records;
    m.s1 = s1;
    m.seg_start = seg_start;
    m.seg_end = seg_end;
    m.gt_off = gt_off;
    m.gt_box = gt_box;
    m.gt_area = gt_area;
    m.gt_crowd = gt_crowd;
    m.gt_idnz = gt_idnz;
    m.iou_thrs = iou_thrs;
    m.area_rng = area_rng;
    m.T = T;
    m.A = A;
    m.max_det = max_det;
    m.row_gts = iou_row_gts < ROW_GTS_MAX ? iou_row_gts : ROW_GTS_MAX;
    m.status = (unsigned char *)(ws + l.status);
    m.rank = rank;
    m.gtm = (unsigned char *)(ws + l.gtm);
    m.npig_pair = (int *)(ws + l.npig_pair);
    m.active = (unsigned char *)(ws + l.active);
    if (hipMemsetAsync(rank, 0xff, n_pad * sizeof(unsigned short), st) != hipSuccess) return PPY_ERR_LAUNCH;
    hipLaunchKernelGGL(match_kernel, dim3((unsigned)P), dim3(64), (size_t)(m.row_gts > 0 ? m.row_gts : 1) * sizeof(double), st, m);
    // accumulate: (category, score desc, position in the pair order) over the truncated lists
    hipLaunchKernelGGL(acc_keys_kernel, dim3(nb), dim3(256), 0, st, s1, rank, n_pad, num_cats, s2);
    rc = bitonic_sort(s2, n_pad, st);
    if (rc != PPY_OK) return rc;
    if (hipMemsetAsync(cat_start, 0, (size_t)(l.npig_cat - l.cat_start), st) != hipSuccess) return PPY_ERR_LAUNCH;
    hipLaunchKernelGGL(segments_kernel, dim3(nb), dim3(256), 0, st, s2, n_pad, cat_start, cat_end);
    hipLaunchKernelGGL(npig_kernel, dim3((unsigned)(num_cats * A)), dim3(64), 0, st, (const int *)m.npig_pair, m.active,
                       num_images, num_cats, A, (int *)(ws + l.npig_cat), (int *)(ws + l.active_cat));
    AccArgs g;
    g.rec = records;
    g.s1 = s1;
    g.s2 = s2;
    g.rank = rank;
    g.status = m.status;
    g.cat_start = cat_start;
    g.cat_end = cat_end;
    g.npig_cat = (const int *)(ws + l.npig_cat);
    g.active_cat = (const int *)(ws + l.active_cat);
    g.gt_cat_off = gt_cat_off;
    g.rec_thrs = rec_thrs;
    g.max_dets = max_dets;
    g.T = T;
    g.R = R;
    g.K = num_cats;
    g.A = A;
    g.M = M;
    g.G = num_gts > 0 ? num_gts : 1;
    g.pv = (double *)(ws + l.pv);
    g.sv = (double *)(ws + l.sv);
    g.precision = precision;
    g.recall = recall;
    g.scores = scores;
    hipLaunchKernelGGL(accumulate_kernel, dim3((unsigned)(num_cats * A * M * T)), dim3(64), 0, st, g);
    return ppy_launch_status();
}
