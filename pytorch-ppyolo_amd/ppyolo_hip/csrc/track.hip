// Tracking across frames on gfx950: the rows forward_padded wrote for the current frame of each of n STREAMS are associated with
// the stream's tracks, whose state lives in a caller-owned device buffer that this kernel reads and rewrites.  ByteTrack-shaped and
// deterministic: a constant-velocity Kalman filter per track (four independent two-state filters: cx, cy, a = w / h, h), greedy
// IoU association in three stages (high rows x tracked and lost tracks, low rows x the tracked tracks left, high rows left x new
// tracks), new tracks confirmed on their second frame, lost tracks kept for max_lost frames.  include/ppyolo_hip.h has the
// contract, DESIGN.md section 10j the reasons; tests/track_ref.py restates it in numpy and the kernel agrees with it bit for bit.
//
// One launch, one workgroup of 1024 threads per stream.  Thread t OWNS slot t (max_tracks <= 1024) and keeps it in registers from
// the load to the store; thread r owns row r (K <= 1024).  What the association reads of both lies in LDS:
//   1  predict   the thread's slot; the predicted box, class, state and id go to LDS
//   2  admit     the thread's row; its box, class, score and level (not admitted, low, high) go to LDS
//   3  associate per stage, ROUNDS of mutual best: every free row of the stage names its best free track (IoU descending, then id
//                ascending), every free track its best free row (IoU descending, then row ascending); a pair that names each
//                other is taken.  The contract's sequential rule takes the pairs in the strict order (IoU descending, id ascending,
//                row ascending) while both ends are free: the first pair of that order among the free ones is the best of its row
//                and of its track, so every round takes at least that pair, and a pair that is the best of both its ends has no
//                earlier pair that could take either end: the rounds end with the sequential result.  Items (rows, then tracks)
//                are dealt to groups of G lanes (the largest power of two with items x G <= 1024) that share the inner loop and
//                reduce across lanes: a frame of 100 rows keeps 800 threads busy, not 100.
//   4  update    matched slots, in registers; demote, free; open new tracks (two workgroup prefix sums pair the j-th opening row
//                with the j-th free slot)
//   5  output    the slots to report are ranked by id (ids are distinct: rank = the number of smaller ids)
// fp32, one rounding per operation: this file is compiled without contraction.  No floating-point atomics, no atomics at all.
#include <cstdio>

#include "common.h"
#pragma clang fp contract(off)

namespace {

constexpr int TK_NT = 1024;
static_assert(PPY_TRACK_MAX_TRACKS == TK_NT && PPY_TRACK_MAX_ROWS == TK_NT, "a thread owns a slot and a row");
constexpr int TK_FREE = 0, TK_NEW = 1, TK_TRACKED = 2, TK_LOST = 3;
constexpr int TK_CX = 0, TK_CY = 1, TK_A = 2, TK_H = 3;
constexpr int TK_SLOT_LDS = 32, TK_ROW_LDS = 36;      // bytes of LDS per slot and per row (below)

struct TkFilter {
    float x, v, ppp, ppv, pvv;
};
struct TkSlot {                                // 112 bytes; a FREE slot is all zero
    int state, id, cls;
    float score;
    int hits, last;
    TkFilter f[4];
    int pad[2];
};
struct TkHead {                                // 16 bytes in front of a stream's slots
    int frame, issued, dropped, pad;
};
static_assert(sizeof(TkSlot) == 112 && sizeof(TkHead) == 16, "state layout");

struct TkArgs {
    const float *dets;
    const int *count;
    char *state;
    float *out_dets;
    int *out_count, *out_ids, *out_src, *out_hits;
    int K, T;
    ppy_track_params_t prm;
};

__device__ __forceinline__ float tk_min(float a, float b) { return b < a ? b : a; }      // std::min / std::max
__device__ __forceinline__ float tk_max(float a, float b) { return a < b ? b : a; }
__device__ __forceinline__ bool tk_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }
__device__ __forceinline__ float tk_area(const floatx4 b) {
    if (b[2] < b[0] || b[3] < b[1]) return 0.0f;
    return (b[2] - b[0]) * (b[3] - b[1]);
}
// a = the row, b = the track's predicted box: JaccardOverlap with norm = 0 (PPY_MERGE_IOU)
__device__ __forceinline__ float tk_iou(const floatx4 a, const floatx4 b) {
    if (b[0] > a[2] || b[2] < a[0] || b[1] > a[3] || b[3] < a[1]) return 0.0f;
    const float iw = tk_min(a[2], b[2]) - tk_max(a[0], b[0]);
    const float ih = tk_min(a[3], b[3]) - tk_max(a[1], b[1]);
    const float inter = iw * ih;
    return inter / ((tk_area(a) + tk_area(b)) - inter);
}

__device__ __forceinline__ floatx4 tk_box(const TkSlot &s) {
    const float w = s.f[TK_A].x * s.f[TK_H].x;
    const float hw = w * 0.5f, hh = s.f[TK_H].x * 0.5f;
    floatx4 b;
    b[0] = s.f[TK_CX].x - hw;
    b[1] = s.f[TK_CY].x - hh;
    b[2] = s.f[TK_CX].x + hw;
    b[3] = s.f[TK_CY].x + hh;
    return b;
}

__device__ __forceinline__ void tk_predict(TkSlot &s) {
    if (s.state != TK_TRACKED) s.f[TK_H].v = 0.0f;
    const float h = s.f[TK_H].x;
    const float tp = h / 20.0f, tv = h / 160.0f;
    const float qp = tp * tp, qv = tv * tv;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        TkFilter f = s.f[k];
        const float p = k == TK_A ? 1e-4f : qp, q = k == TK_A ? 1e-10f : qv;
        s.f[k].x = f.x + f.v;
        s.f[k].ppp = ((f.ppp + f.ppv) + (f.ppv + f.pvv)) + p;
        s.f[k].ppv = f.ppv + f.pvv;
        s.f[k].pvv = f.pvv + q;
    }
}

// z = (cx, cy, w / h, h) of a row's box
__device__ __forceinline__ void tk_measure(const floatx4 b, float (&z)[4]) {
    const float w = b[2] - b[0], h = b[3] - b[1];
    z[TK_CX] = b[0] + w * 0.5f;
    z[TK_CY] = b[1] + h * 0.5f;
    z[TK_A] = w / h;
    z[TK_H] = h;
}

__device__ __forceinline__ void tk_update(TkSlot &s, const float (&z)[4]) {
    const float tr = s.f[TK_H].x / 20.0f;
    const float rp = tr * tr;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const TkFilter f = s.f[k];
        const float sum = f.ppp + (k == TK_A ? 1e-2f : rp);
        const float kp = f.ppp / sum, kv = f.ppv / sum;
        const float y = z[k] - f.x;
        s.f[k].x = f.x + kp * y;
        s.f[k].v = f.v + kv * y;
        s.f[k].ppp = f.ppp - kp * f.ppp;
        s.f[k].ppv = f.ppv - kp * f.ppv;
        s.f[k].pvv = f.pvv - kv * f.ppv;
    }
}

__device__ __forceinline__ void tk_open(TkSlot &s, const float (&z)[4]) {
    const float h = z[TK_H];
    const float tp = (2.0f * h) / 20.0f, tv = (10.0f * h) / 160.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        s.f[k].x = z[k];
        s.f[k].v = 0.0f;
        s.f[k].ppp = k == TK_A ? 1e-4f : tp * tp;
        s.f[k].ppv = 0.0f;
        s.f[k].pvv = k == TK_A ? 1e-10f : tv * tv;
    }
}

// exclusive prefix sum of v over the workgroup's threads, and the total; called by all threads
__device__ __forceinline__ int tk_prefix(int v, int *scratch /*[16]*/, int &total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int s = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(s, d);
        if (lane >= d) s += o;
    }
    if (lane == 63) scratch[wv] = s;
    __syncthreads();
    int add = 0, all = 0;
    for (int k = 0; k < TK_NT / 64; ++k) {
        const int c = scratch[k];
        if (k < wv) add += c;
        all += c;
    }
    __syncthreads();
    total = all;
    return s - v + add;
}

struct TkLds {
    floatx4 *tbox, *rbox;          // [T] predicted boxes, [K] row boxes
    int *tcls, *tstate, *tid_, *tmatch;      // [T]; tmatch = the row a slot took, -1
    int *rcls, *rlevel, *rmatch, *rbest;     // [K]; rlevel 0 = not admitted, 1 = low, 2 = high; rmatch = the slot, -1
    float *rscore;                 // [K]
};

// One side of a round.  ROWS: every free row of the stage -> its best free track into rbest[]; else every free track -> its best
// free row, returned to the lanes of its group (lane `sub` == 0 keeps it).  Called by all threads.
template <bool ROWS>
__device__ __forceinline__ int tk_best(const TkLds &L, int items, int inner, int G, int tstate_a, int tstate_b, int level, float thr,
                                       bool agnostic) {
    const int item = (int)threadIdx.x / G, sub = (int)threadIdx.x & (G - 1);      // items x G <= 1024 or G == 1: at most one item each
    float best = 0.0f;
    int bi = -1, bo = 0;      // the best partner, and what orders equal IoUs (the track's id / the row)
    bool act = item < items;
    if (act) {
        if (ROWS) act = L.rlevel[item] == level && L.rmatch[item] < 0;
        else act = (L.tstate[item] == tstate_a || L.tstate[item] == tstate_b) && L.tmatch[item] < 0;
    }
    if (act) {
        const floatx4 mine = ROWS ? L.rbox[item] : L.tbox[item];
        const int mcls = ROWS ? L.rcls[item] : L.tcls[item];
        for (int j = sub; j < inner; j += G) {
            bool ok;
            if (ROWS) ok = (L.tstate[j] == tstate_a || L.tstate[j] == tstate_b) && L.tmatch[j] < 0;
            else ok = L.rlevel[j] == level && L.rmatch[j] < 0;
            if (!ok || !(agnostic || (ROWS ? L.tcls[j] : L.rcls[j]) == mcls)) continue;
            const float m = ROWS ? tk_iou(mine, L.tbox[j]) : tk_iou(L.rbox[j], mine);
            const int o = ROWS ? L.tid_[j] : j;
            if (m > thr && (bi < 0 || m > best || (m == best && o < bo))) {      // a NaN IoU fails `m > thr`
                best = m;
                bi = j;
                bo = o;
            }
        }
    }
    for (int d = 1; d < G; d <<= 1) {
        const float om = __shfl_xor(best, d);
        const int oi = __shfl_xor(bi, d), oo = __shfl_xor(bo, d);
        if (oi >= 0 && (bi < 0 || om > best || (om == best && oo < bo))) {
            best = om;
            bi = oi;
            bo = oo;
        }
    }
    return bi;
}

__device__ __forceinline__ int tk_group(int items) {      // lanes per item
    int G = 64;
    while (G > 1 && items * G > TK_NT) G >>= 1;
    return G;
}

__global__ void __launch_bounds__(TK_NT) tk_update_kernel(const TkArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sdyn[];
    __shared__ int s_scan[TK_NT / 64];
    __shared__ int s_any;

    const int n = blockIdx.x, tid = threadIdx.x, T = p.T, K = p.K;
    float *odets = p.out_dets + (long long)n * T * 6;
    int *oids = p.out_ids + (long long)n * T, *osrc = p.out_src + (long long)n * T, *ohits = p.out_hits + (long long)n * T;
    const int cnt = p.count[n];
    if (cnt < 0) {      // no frame for this stream: the state stays as it is
        if (tid < T) {
            float *o = odets + tid * 6;
            o[0] = o[1] = o[2] = o[3] = o[4] = o[5] = -1.0f;
            oids[tid] = osrc[tid] = ohits[tid] = -1;
        }
        if (tid == 0) p.out_count[n] = 0;
        return;
    }
    TkLds L;
    L.tbox = reinterpret_cast<floatx4 *>(sdyn);
    L.rbox = L.tbox + T;
    L.tcls = reinterpret_cast<int *>(L.rbox + K);
    L.tstate = L.tcls + T;
    L.tid_ = L.tstate + T;
    L.tmatch = L.tid_ + T;
    L.rcls = L.tmatch + T;
    L.rlevel = L.rcls + K;
    L.rmatch = L.rlevel + K;
    L.rbest = L.rmatch + K;
    L.rscore = reinterpret_cast<float *>(L.rbest + K);

    char *sbase = p.state + (size_t)n * (sizeof(TkHead) + (size_t)T * sizeof(TkSlot));
    TkHead head = *reinterpret_cast<const TkHead *>(sbase);
    TkSlot *slots = reinterpret_cast<TkSlot *>(sbase + sizeof(TkHead));
    const int frame = head.frame + 1;

    // ---- 1. predict ----
    const bool own = tid < T;
    TkSlot s;
    if (own) {
        s = slots[tid];
        if (s.state != TK_FREE) tk_predict(s);
        L.tbox[tid] = tk_box(s);
        L.tcls[tid] = s.cls;
        L.tstate[tid] = s.state;
        L.tid_[tid] = s.id;
        L.tmatch[tid] = -1;
    }
    // ---- 2. admit ----
    if (tid < K) {
        int level = 0, cls = 0;
        floatx4 b = {0.0f, 0.0f, 0.0f, 0.0f};
        float score = 0.0f;
        if (tid < cnt) {
            const float *d = p.dets + ((long long)n * K + tid) * 6;
            const float c = d[0];
            score = d[1];
            b[0] = d[2]; b[1] = d[3]; b[2] = d[4]; b[3] = d[5];
            const bool ok = tk_finite(c) && tk_finite(score) && tk_finite(b[0]) && tk_finite(b[1]) && tk_finite(b[2]) && tk_finite(b[3]) &&
                            c >= 0.0f && c < 16777216.0f && b[2] > b[0] && b[3] > b[1] && score >= p.prm.low_thresh;
            if (ok) {
                level = score >= p.prm.high_thresh ? 2 : 1;
                cls = (int)c;
            }
        }
        L.rbox[tid] = b;
        L.rcls[tid] = cls;
        L.rscore[tid] = score;
        L.rlevel[tid] = level;
        L.rmatch[tid] = -1;
    }
    __syncthreads();

    // ---- 3. associate ----
    const int GR = tk_group(K), GT = tk_group(T);
    const bool agnostic = p.prm.class_agnostic != 0;
    for (int stage = 0; stage < 3; ++stage) {
        const int sa = stage == 2 ? TK_NEW : TK_TRACKED, sb = stage == 0 ? TK_LOST : sa;
        const int level = stage == 1 ? 1 : 2;
        const float thr = p.prm.match_thresh[stage];
        for (;;) {
            if (tid == 0) s_any = 0;
            const int bt = tk_best<true>(L, K, T, GR, sa, sb, level, thr, agnostic);
            if ((tid & (GR - 1)) == 0 && tid / GR < K) L.rbest[tid / GR] = bt;
            __syncthreads();
            const int br = tk_best<false>(L, T, K, GT, sa, sb, level, thr, agnostic);
            const int t = tid / GT;
            const bool take = (tid & (GT - 1)) == 0 && t < T && br >= 0 && L.rbest[br] == t;
            __syncthreads();      // every group has read tmatch / rmatch of this round
            if (take) {
                L.tmatch[t] = br;
                L.rmatch[br] = t;
                s_any = 1;
            }
            __syncthreads();
            const int any = s_any;
            __syncthreads();
            if (!any) break;
        }
    }

    // ---- 4. update; demote and free; open ----
    int src = -1;
    if (own) {
        src = L.tmatch[tid];
        if (src >= 0) {
            float z[4];
            tk_measure(L.rbox[src], z);
            tk_update(s, z);
            s.score = L.rscore[src];
            s.cls = L.rcls[src];
            s.hits += 1;
            s.last = frame;
            s.state = TK_TRACKED;
        } else if (s.state == TK_TRACKED) {
            s.state = TK_LOST;
        } else if (s.state == TK_NEW) {
            s.state = TK_FREE;
        }
        if (s.state == TK_LOST && frame - s.last > p.prm.max_lost) s.state = TK_FREE;
    }
    const bool wants = tid < K && L.rlevel[tid] == 2 && L.rmatch[tid] < 0 && L.rscore[tid] >= p.prm.new_thresh;
    const bool isfree = own && s.state == TK_FREE;
    int nwant, nfree;
    const int wrank = tk_prefix(wants ? 1 : 0, s_scan, nwant);
    const int frank = tk_prefix(isfree ? 1 : 0, s_scan, nfree);
    if (wants) L.rbest[wrank] = tid;      // the opening rows in row order (rbest is free from here)
    __syncthreads();
    const int nopen = nwant < nfree ? nwant : nfree;
    if (isfree) {
        if (frank < nopen) {
            src = L.rbest[frank];
            float z[4];
            tk_measure(L.rbox[src], z);
            tk_open(s, z);
            s.state = frame == 1 ? TK_TRACKED : TK_NEW;
            s.id = head.issued + 1 + frank;
            s.cls = L.rcls[src];
            s.score = L.rscore[src];
            s.hits = 1;
            s.last = frame;
            s.pad[0] = s.pad[1] = 0;
        } else {
            s = TkSlot{};      // a FREE slot is all zero
        }
    }
    if (own) slots[tid] = s;
    if (tid == 0) {
        head.frame = frame;
        head.issued += nopen;
        head.dropped += nwant - nopen;
        *reinterpret_cast<TkHead *>(sbase) = head;
    }

    // ---- 5. output: the TRACKED slots matched or opened in this call, by id ----
    const bool rep = own && s.state == TK_TRACKED && src >= 0;
    if (own) L.tid_[tid] = rep ? s.id : 0;      // (ids start at 1; every thread wrote its own entry before: no barrier needed above)
    int nout;
    tk_prefix(rep ? 1 : 0, s_scan, nout);       // (its barriers also publish tid_)
    if (rep) {
        int rank = 0, j = 0;
        for (; j + 8 <= T; j += 8) {            // 8 independent LDS reads in flight
            int v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = L.tid_[j + u];
#pragma unroll
            for (int u = 0; u < 8; ++u) rank += (v[u] != 0 && v[u] < s.id) ? 1 : 0;
        }
        for (; j < T; ++j) {
            const int v = L.tid_[j];
            rank += (v != 0 && v < s.id) ? 1 : 0;
        }
        const floatx4 b = tk_box(s);
        float *o = odets + rank * 6;
        o[0] = (float)s.cls;
        o[1] = s.score;
        o[2] = b[0]; o[3] = b[1]; o[4] = b[2]; o[5] = b[3];
        oids[rank] = s.id;
        osrc[rank] = src;
        ohits[rank] = s.hits;
    }
    if (own && tid >= nout) {
        float *o = odets + tid * 6;
        o[0] = o[1] = o[2] = o[3] = o[4] = o[5] = -1.0f;
        oids[tid] = osrc[tid] = ohits[tid] = -1;
    }
    if (tid == 0) p.out_count[n] = nout;
}

size_t tk_lds_bytes(int T, int K) { return (size_t)T * TK_SLOT_LDS + (size_t)K * TK_ROW_LDS; }

}  // namespace

extern "C" size_t ppy_track_state_bytes(int n, int max_tracks) {
    if (n < 1 || max_tracks < 1 || max_tracks > PPY_TRACK_MAX_TRACKS) return 0;
    return (size_t)n * (sizeof(TkHead) + (size_t)max_tracks * sizeof(TkSlot));
}

extern "C" size_t ppy_track_workspace_bytes(int n, int max_tracks, int K) {
    (void)n; (void)max_tracks; (void)K;
    return 0;      // everything between the load and the store of the state lives in registers and LDS
}

extern "C" int ppy_track_update_f32(const float *dets, const int *count, int n, int K, int max_tracks, const ppy_track_params_t *h_params,
                                    void *state, size_t state_bytes, float *out_dets, int *out_count, int *out_ids, int *out_src,
                                    int *out_hits, void *ws, size_t ws_bytes, char *h_reason, void *stream) {
    ppy_drop_stale_error();
    (void)ws; (void)ws_bytes;
    char local[96];
    char *r = h_reason ? h_reason : local;
    r[0] = 0;
    if (max_tracks < 1 || max_tracks > PPY_TRACK_MAX_TRACKS) {
        snprintf(r, 96, "max_tracks = %d, supported: 1..%d", max_tracks, PPY_TRACK_MAX_TRACKS);
        return PPY_ERR_UNSUPPORTED;
    }
    if (K < 1 || K > PPY_TRACK_MAX_ROWS) {
        snprintf(r, 96, "K = %d rows per frame, supported: 1..%d", K, PPY_TRACK_MAX_ROWS);
        return PPY_ERR_UNSUPPORTED;
    }
    PPY_CHECK_ARG(h_params);
    const struct { const char *name; float v; } thr[6] = {
        {"high_thresh", h_params->high_thresh}, {"low_thresh", h_params->low_thresh}, {"new_thresh", h_params->new_thresh},
        {"match_thresh[0]", h_params->match_thresh[0]}, {"match_thresh[1]", h_params->match_thresh[1]},
        {"match_thresh[2]", h_params->match_thresh[2]}};
    for (int i = 0; i < 6; ++i) {
        if (thr[i].v != thr[i].v) {
            snprintf(r, 96, "%s is NaN", thr[i].name);
            return PPY_ERR_UNSUPPORTED;
        }
    }
    if (h_params->max_lost < 0) {
        snprintf(r, 96, "max_lost = %d, must be at least 0", h_params->max_lost);
        return PPY_ERR_UNSUPPORTED;
    }
    PPY_CHECK_ARG(dets && count && state && out_dets && out_count && out_ids && out_src && out_hits);
    PPY_CHECK_ARG(n >= 1 && n <= 65535);
    PPY_CHECK_ARG(((uintptr_t)state & 15) == 0 && state_bytes >= ppy_track_state_bytes(n, max_tracks));
    TkArgs p;
    p.dets = dets; p.count = count; p.state = static_cast<char *>(state);
    p.out_dets = out_dets; p.out_count = out_count; p.out_ids = out_ids; p.out_src = out_src; p.out_hits = out_hits;
    p.K = K; p.T = max_tracks;
    p.prm = *h_params;
    const int lds = (int)tk_lds_bytes(max_tracks, K);
    static PpyLdsAttr attr;
    if (ppy_lds_attr(attr, reinterpret_cast<const void *>(tk_update_kernel), lds) != PPY_OK) return PPY_ERR_LAUNCH;
    hipLaunchKernelGGL(tk_update_kernel, dim3(n), dim3(TK_NT), lds, (hipStream_t)stream, p);
    return ppy_launch_status();
}
