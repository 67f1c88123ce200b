// Pillow's Image.resize(size, filter, box=(x0, y0, x1, y1)) for 3-channel uint8 images on the device, bit for bit, with the boxes
// read ON THE DEVICE: the rows of forward_padded (or a caller's list of boxes) are selected, planned and resized without the
// host ever seeing a coordinate.  Pillow 12.2.0: libImaging Resample.c (precompute_coeffs with a box, ImagingResample's two
// passes) for filters 1..5, the affine scaler of Geometry.c for NEAREST.  DESIGN.md section 10g has the rules.
//
// One call resizes up to `cap` crops of a batch of n images to one (ow, oh) with one filter; every grid is sized from what the
// host knows (n, K or M, ow, oh, the image sizes), and no launch waits for the host:
//   launch 1  crop_select_kernel<ROWS>: ONE workgroup.  Validity of every candidate, an ordered block scan (no atomics: the
//             result cannot depend on scheduling) -> src[cap][2] = (image, row or list index), -1 past the end; total[1];
//             boxes[cap][4] = the (padded) float32 boxes, 0 past the end.
//   launch 2  crop_plan_kernel: one thread per (crop, axis, output sample) writes bounds (first tap, taps) and the 2^22
//             fixed-point weights -- precompute_coeffs in double, operation for operation, compiled WITHOUT contraction --
//             or the index map of NEAREST / of an axis Pillow skips; one thread per crop writes first / rows of the
//             horizontal pass and the skip flag.  The double weights wait for their sum in the crop's intermediate, which
//             launch 3 has not written yet.
//   launch 3  crop_horizontal_kernel: source rows [first, first + rows) -> the crop's uint8 intermediate of ow columns.
//   launch 4  crop_vertical_kernel: intermediate (or the source, where Pillow skips the horizontal pass) -> out[cap][oh][ow][3];
//             crops past `total` are written as zero.
// Workgroups of crops past `total` leave at once in launches 2 and 3.  Unlike ppy_pil_resize_* (one table per distinct axis of
// the batch, planned on the host) every crop owns its tables: every box is its own fractional axis.
#include <cmath>
#include <cstdio>
#include <cstring>

#ifndef PPY_PIL_HOST_ONLY
#include "common.h"
#define PPY_HD __host__ __device__
#else      // the validation alone as plain C++ (tools/pil_crop_asan.cpp: AddressSanitizer build, no HIP headers)
#include <stddef.h>
#include <stdint.h>

#include "../../../include/ppyolo_hip.h"
#define PPY_CHECK_ARG(cond) \
    do {                    \
        if (!(cond)) return PPY_ERR_BAD_ARG; \
    } while (0)
#define PPY_HD
#endif

#pragma clang fp contract(off)      // the select rule's float32 padding and the planner's doubles: one rounding per operation

namespace {

constexpr int CROP_MAX_IMAGES = 1024, CROP_MAX_IN = 65535, CROP_MAX_OUT = 8192, CROP_MAX_KSIZE = 1024, CROP_MAX_CROPS = 65536;
constexpr int CROP_BITS = 22;
constexpr int CROP_SELECT_THREADS = 1024;

struct CropLayout {            // what the host derives from the request; passed to the kernels by value
    int n, cap, ow, oh, filter;
    int kx, ky;                // taps reserved per output sample of each axis (0: NEAREST); >= any crop's ksize
    int max_h, mid_pitch;      // rows and bytes per row reserved for one crop's intermediate
    long long off_meta, off_scan, off_xtab, off_ytab, off_mid;      // byte offsets in the workspace
    long long xtab_ints, ytab_ints, mid_bytes;                      // per crop
    long long ws_bytes;
    int wtmp;                  // the planner may park its double weights in the crop's (not yet written) intermediate
};
// per crop, at off_meta: 8 ints
enum { CM_FIRST = 0, CM_ROWS = 1, CM_SKIP_H = 2, CM_XMAP = 3, CM_YMAP = 4 };

PPY_HD inline double crop_support(int f) { return f == 4 ? 0.5 : (f == 2 || f == 5) ? 1.0 : f == 3 ? 2.0 : 3.0; }

PPY_HD inline double crop_filter(int f, double x) {      // Resample.c's filters, operation for operation
    switch (f) {
    case 4: return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
    case 2:
        if (x < 0.0) x = -x;
        return x < 1.0 ? 1.0 - x : 0.0;
    case 5:
        if (x < 0.0) x = -x;
        if (x == 0.0) return 1.0;
        if (x >= 1.0) return 0.0;
        x = x * M_PI;
        return sin(x) / x * (0.54f + 0.46f * cos(x));      // (float literals, as in Pillow)
    case 3: {
        const double a = -0.5;
        if (x < 0.0) x = -x;
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
        if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
        return 0.0;
    }
    default: {                                   // 1: lanczos
        if (!(-3.0 <= x && x < 3.0)) return 0.0;
        double s1 = 1.0, s3 = 1.0;
        if (x != 0.0) {
            const double p = x * M_PI;
            s1 = sin(p) / p;
        }
        const double y = x / 3;
        if (y != 0.0) {
            const double p = y * M_PI;
            s3 = sin(p) / p;
        }
        return s1 * s3;
    }
    }
}

// the most taps any box inside an axis of `in` pixels can need for `out` samples: the box is at most the axis
long long crop_ksize_cap(int in, int out, int filter) {
    if (filter == 0) return 0;
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    return (long long)std::ceil(crop_support(filter) * fs) * 2 + 1;
}

inline long long crop_align(long long v) { return (v + 255) & ~255LL; }

// Validates the request and lays the workspace out.  form: 0 rows (rows_or_m = K), 1 list (rows_or_m = M).  reason: NULL or 96.
int crop_layout(int n, const ppy_pil_image_t *im, int form, int rows_or_m, int ow, int oh, int filter, float pad, int top_k,
                CropLayout &L, char *reason) {
    char local[96];
    char *r = reason ? reason : local;
    r[0] = 0;
    if (!(n >= 1 && n <= CROP_MAX_IMAGES) || !im) {
        snprintf(r, 96, "batch of %d images, supported: 1..%d", n, CROP_MAX_IMAGES);
        return PPY_ERR_BAD_ARG;
    }
    PPY_CHECK_ARG(form == 0 || form == 1);
    if (filter < 0 || filter > 5) {
        snprintf(r, 96, "filter code %d, Pillow's codes are 0..5", filter);
        return PPY_ERR_UNSUPPORTED;
    }
    if (ow < 1 || ow > CROP_MAX_OUT || oh < 1 || oh > CROP_MAX_OUT) {
        snprintf(r, 96, "output size %d x %d, each side must be in 1..%d", ow, oh, CROP_MAX_OUT);
        return PPY_ERR_UNSUPPORTED;
    }
    const long long cap = form == 0 ? (long long)n * rows_or_m : (long long)rows_or_m;
    if (rows_or_m < 1 || cap > CROP_MAX_CROPS) {
        if (form == 0)
            snprintf(r, 96, "%d images x %d rows = %lld candidates, supported: 1..%d", n, rows_or_m, cap, CROP_MAX_CROPS);
        else
            snprintf(r, 96, "a list of %d boxes, supported: 1..%d", rows_or_m, CROP_MAX_CROPS);
        return PPY_ERR_UNSUPPORTED;
    }
    if (form == 0) {
        if (!(pad >= 0.0f && pad <= 4.0f)) {      // (false for NaN too)
            snprintf(r, 96, "pad %g, must be a finite value in [0, 4]", (double)pad);
            return PPY_ERR_UNSUPPORTED;
        }
        if (top_k < 1) {
            snprintf(r, 96, "top_k %d, must be at least 1", top_k);
            return PPY_ERR_UNSUPPORTED;
        }
    }
    int max_w = 0, max_h = 0;
    for (int i = 0; i < n; ++i) {
        if (im[i].h < 1 || im[i].h > CROP_MAX_IN || im[i].w < 1 || im[i].w > CROP_MAX_IN) {
            snprintf(r, 96, "image %d: input size %d x %d, each side must be in 1..%d", i, im[i].w, im[i].h, CROP_MAX_IN);
            return PPY_ERR_UNSUPPORTED;
        }
        if ((long long)im[i].h > 100LL * im[i].w) {
            snprintf(r, 96, "image %d: %d x %d is taller than 100 x its width (Pillow resizes such sources vertically first)", i,
                     im[i].w, im[i].h);
            return PPY_ERR_UNSUPPORTED;
        }
        if (im[i].w > max_w) max_w = im[i].w;
        if (im[i].h > max_h) max_h = im[i].h;
    }
    const long long kx = crop_ksize_cap(max_w, ow, filter), ky = crop_ksize_cap(max_h, oh, filter);
    if (kx > CROP_MAX_KSIZE || ky > CROP_MAX_KSIZE) {
        snprintf(r, 96, "largest side %d to %d needs ksize %lld, at most %d", kx > ky ? max_w : max_h, kx > ky ? ow : oh,
                 kx > ky ? kx : ky, CROP_MAX_KSIZE);
        return PPY_ERR_UNSUPPORTED;
    }
    L.n = n;
    L.cap = (int)cap;
    L.ow = ow;
    L.oh = oh;
    L.filter = filter;
    L.kx = (int)kx;
    L.ky = (int)ky;
    L.max_h = max_h;
    L.mid_pitch = (3 * ow + 15) & ~15;
    L.xtab_ints = (long long)ow * (2 + kx);
    L.ytab_ints = (long long)oh * (2 + ky);
    L.mid_bytes = crop_align((long long)max_h * L.mid_pitch);
    L.off_meta = 0;
    L.off_scan = crop_align(cap * 32);
    L.off_xtab = L.off_scan + crop_align(cap * 4);
    L.off_ytab = L.off_xtab + crop_align(cap * L.xtab_ints * 4);
    L.off_mid = L.off_ytab + crop_align(cap * L.ytab_ints * 4);
    L.ws_bytes = L.off_mid + cap * L.mid_bytes;
    L.wtmp = (long long)(ow + oh) * (kx > ky ? kx : ky) * 8 <= L.mid_bytes ? 1 : 0;
    return PPY_OK;
}

int crop_check_pitches(int n, const ppy_pil_image_t *im) {
    for (int i = 0; i < n; ++i) PPY_CHECK_ARG(im[i].base && (im[i].h == 1 || im[i].pitch >= 3LL * im[i].w));
    return PPY_OK;
}

#ifndef PPY_PIL_HOST_ONLY
// ---- launch 1: select ---------------------------------------------------------------------------------------------------------
// Exclusive prefix of v over the workgroup's 1024 threads, in thread order; sum = the workgroup's total.  Every thread calls it.
__device__ __forceinline__ int crop_block_scan(int v, int *s_wave, int &sum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    __syncthreads();          // (the previous call's readers are done with s_wave)
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int base = 0;
    sum = 0;
#pragma unroll
    for (int w = 0; w < CROP_SELECT_THREADS / 64; ++w) {
        const int t = s_wave[w];
        if (w < wave) base += t;
        sum += t;
    }
    return base + inc - v;
}

__device__ __forceinline__ bool crop_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }      // false for NaN and inf

// Pillow's own test of a box (it refuses x0 < 0, y0 < 0, x1 > w, y1 > h) plus a non-empty one.
__device__ __forceinline__ bool crop_box_ok(float x0, float y0, float x1, float y1, int w, int h) {
    return crop_finite(x0) && crop_finite(y0) && crop_finite(x1) && crop_finite(y1) && 0.0f <= x0 && x0 < x1 && x1 <= (float)w &&
           0.0f <= y0 && y0 < y1 && y1 <= (float)h;
}

// Candidate e of the rows form: is it valid, and its padded box.  A row whose own box leaves the image is skipped (Pillow
// would refuse it); the padding is clipped to the image.
__device__ __forceinline__ bool crop_row_box(const CropLayout &L, const ppy_pil_image_t *images, const float *dets, const int *count,
                                             int K, float thresh, float pad, int e, float (&b)[4]) {
    const int i = e / K, r = e - i * K;
    if (r >= count[i]) return false;
    const float *d = dets + (long long)e * 6;
    const float cls = d[0], score = d[1], x0 = d[2], y0 = d[3], x1 = d[4], y1 = d[5];
    const int w = images[i].w, h = images[i].h;
    if (!(crop_finite(cls) && crop_finite(score) && cls >= 0.0f && score >= thresh)) return false;
    if (!crop_box_ok(x0, y0, x1, y1, w, h)) return false;
    const float bw = x1 - x0, bh = y1 - y0;
    b[0] = fmaxf(x0 - pad * bw, 0.0f);
    b[1] = fmaxf(y0 - pad * bh, 0.0f);
    b[2] = fminf(x1 + pad * bw, (float)w);
    b[3] = fminf(y1 + pad * bh, (float)h);
    return crop_box_ok(b[0], b[1], b[2], b[3], w, h);
}

// ROWS: in_a = dets [n][K][6], in_b = count [n].  List: in_a = boxes [M][4], in_b = image [M]; the list's order is kept.
template <bool ROWS>
__global__ __launch_bounds__(CROP_SELECT_THREADS) void crop_select_kernel(CropLayout L, const ppy_pil_image_t *__restrict__ images,
                                                                          const float *__restrict__ in_a, const int *__restrict__ in_b,
                                                                          int K, float thresh, float pad, int top_k,
                                                                          unsigned char *__restrict__ ws, int *__restrict__ src,
                                                                          int *__restrict__ total, float *__restrict__ boxes) {
    __shared__ int s_wave[CROP_SELECT_THREADS / 64];
    int *scan = reinterpret_cast<int *>(ws + L.off_scan);      // rows form: 2 * (valid rows in front of e) + (e is valid)
    const int cap = L.cap;
    int carry = 0, sum;
    if (ROWS) {
        for (int e0 = 0; e0 < cap; e0 += CROP_SELECT_THREADS) {
            const int e = e0 + (int)threadIdx.x;
            float b[4];
            const int valid = e < cap && crop_row_box(L, images, in_a, in_b, K, thresh, pad, e, b) ? 1 : 0;
            const int pre = carry + crop_block_scan(valid, s_wave, sum);
            if (e < cap) scan[e] = 2 * pre + valid;
            carry += sum;
        }
        __syncthreads();      // scan[] of this workgroup's own stores
        carry = 0;
    }
    for (int e0 = 0; e0 < cap; e0 += CROP_SELECT_THREADS) {
        const int e = e0 + (int)threadIdx.x;
        float b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        int taken = 0, img = 0, row = e;
        if (e < cap) {
            if (ROWS) {
                img = e / K;
                row = e - img * K;
                const int me = scan[e];
                taken = (me & 1) && (me >> 1) - (scan[img * K] >> 1) < top_k ? 1 : 0;
                if (taken) crop_row_box(L, images, in_a, in_b, K, thresh, pad, e, b);
            } else {
                img = in_b[e];
                if (img >= 0 && img < L.n) {
                    b[0] = in_a[4 * (long long)e];
                    b[1] = in_a[4 * (long long)e + 1];
                    b[2] = in_a[4 * (long long)e + 2];
                    b[3] = in_a[4 * (long long)e + 3];
                    taken = crop_box_ok(b[0], b[1], b[2], b[3], images[img].w, images[img].h) ? 1 : 0;
                }
            }
        }
        const int pos = carry + crop_block_scan(taken, s_wave, sum);
        if (taken) {
            src[2 * pos] = img;
            src[2 * pos + 1] = row;
#pragma unroll
            for (int j = 0; j < 4; ++j) boxes[4 * (long long)pos + j] = b[j];
        }
        carry += sum;
    }
    if (threadIdx.x == 0) total[0] = carry;
    for (int e = carry + (int)threadIdx.x; e < cap; e += CROP_SELECT_THREADS) {
        src[2 * e] = src[2 * e + 1] = -1;
#pragma unroll
        for (int j = 0; j < 4; ++j) boxes[4 * (long long)e + j] = 0.0f;
    }
}

// ---- launch 2: plan -----------------------------------------------------------------------------------------------------------
// bounds of output sample xx of one axis: precompute_coeffs' xmin and xmax - xmin
__device__ __forceinline__ void crop_bounds(double in0, double scale, double support, int insz, int xx, double &center, int &xmin, int &cnt) {
    center = in0 + (xx + 0.5) * scale;
    xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > insz) xmax = insz;
    cnt = xmax - xmin;
}

__global__ __launch_bounds__(256) void crop_plan_kernel(CropLayout L, const ppy_pil_image_t *__restrict__ images, const int *__restrict__ src,
                                                        const int *__restrict__ total, const float *__restrict__ boxes,
                                                        unsigned char *__restrict__ ws) {
    const int c = blockIdx.x;
    if (c >= total[0]) return;
    const int s = blockIdx.y * 256 + threadIdx.x;
    if (s >= L.ow + L.oh) return;
    const bool yaxis = s >= L.ow;
    const int xx = yaxis ? s - L.ow : s, out = yaxis ? L.oh : L.ow, kcap = yaxis ? L.ky : L.kx;
    const ppy_pil_image_t im = images[src[2 * c]];
    const int insz = yaxis ? im.h : im.w;
    const float in0 = boxes[4 * (long long)c + (yaxis ? 1 : 0)], in1 = boxes[4 * (long long)c + (yaxis ? 3 : 2)];
    int *meta = reinterpret_cast<int *>(ws + L.off_meta) + 8 * (long long)c;
    int *bounds = reinterpret_cast<int *>(ws + (yaxis ? L.off_ytab : L.off_xtab)) + (long long)c * (yaxis ? L.ytab_ints : L.xtab_ints);
    int *kk = bounds + 2 * (long long)out;
    // Pillow runs a pass unless the axis keeps its size AND the box is the whole axis
    const bool skip = out == insz && in0 == 0.0f && in1 == (float)out;
    const bool skip_h = L.ow == im.w && boxes[4 * (long long)c] == 0.0f && boxes[4 * (long long)c + 2] == (float)L.ow;
    const double scale = (double)(in1 - in0) / out;      // (the subtraction in float32, as Pillow's C does it)
    if (skip || L.filter == 0) {                         // an index map
        if (xx != 0) {
            if (skip) bounds[2 * xx] = xx, bounds[2 * xx + 1] = 1;
            return;
        }
        int first = 0, last = insz;
        if (skip) {
            bounds[0] = 0, bounds[1] = 1;
        } else {              // the affine scaler: the coordinate is accumulated, not recomputed -- one thread walks the axis
            double xo = in0 + scale * 0.5;
            for (int x = 0; x < out; ++x) {
                int v = (int)floor(xo);
                v = v < 0 ? 0 : (v > insz - 1 ? insz - 1 : v);      // (keeps the kernels in bounds; not taken for a box inside the image)
                if (x == 0) first = v;
                last = v + 1;
                bounds[2 * x] = v;
                bounds[2 * x + 1] = 1;
                xo += scale;
            }
        }
        if (yaxis) {
            meta[CM_FIRST] = skip_h ? 0 : first;
            meta[CM_ROWS] = skip_h ? 0 : last - first;
            meta[CM_YMAP] = 1;
        } else {
            meta[CM_SKIP_H] = skip_h ? 1 : 0;
            meta[CM_XMAP] = 1;
        }
        return;
    }
    const double fs = scale < 1.0 ? 1.0 : scale, support = crop_support(L.filter) * fs, ss = 1.0 / fs;
    double center;
    int xmin, cnt;
    crop_bounds((double)in0, scale, support, insz, xx, center, xmin, cnt);
    if (xx == 0) {
        if (yaxis) {
            double c1;
            int lmin, lcnt;
            crop_bounds((double)in0, scale, support, insz, out - 1, c1, lmin, lcnt);
            lcnt = lcnt < 0 ? 0 : lcnt;
            meta[CM_FIRST] = skip_h ? 0 : xmin;
            meta[CM_ROWS] = skip_h ? 0 : lmin + lcnt - xmin;
            meta[CM_YMAP] = 0;
        } else {
            meta[CM_SKIP_H] = 0;
            meta[CM_XMAP] = 0;
        }
    }
    if (cnt > kcap) cnt = kcap;                           // (never taken: kcap bounds every box inside the image)
    if (cnt < 0) cnt = 0;
    // The weights are needed twice, for their sum and then divided by it.  Where the crop's intermediate (written by launch 3,
    // not before) has the room, the doubles wait there, tap-major so that a wave's stores are contiguous; otherwise they are
    // computed again: the same operations on the same operands, the same doubles.  Either way the bits are the same.
    double *wtmp = L.wtmp ? reinterpret_cast<double *>(ws + L.off_mid + (long long)c * L.mid_bytes) + s : nullptr;
    const long long wstride = L.ow + L.oh;
    double ww = 0.0;
    for (int x = 0; x < cnt; ++x) {
        const double v = crop_filter(L.filter, (x + xmin - center + 0.5) * ss);
        if (wtmp) wtmp[x * wstride] = v;
        ww += v;
    }
    int *k = kk + (long long)xx * kcap;
    for (int x = 0; x < cnt; ++x) {
        double v = wtmp ? wtmp[x * wstride] : crop_filter(L.filter, (x + xmin - center + 0.5) * ss);
        if (ww != 0.0) v /= ww;
        k[x] = v < 0 ? (int)(-0.5 + v * (1 << CROP_BITS)) : (int)(0.5 + v * (1 << CROP_BITS));
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = cnt;
}

// ---- launches 3 and 4 ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int crop_clip8(int acc) { return min(max(acc >> CROP_BITS, 0), 255); }

// One thread = one pixel of the intermediate (3 channels); a workgroup = 64 columns x 4 rows, striding over the crop's rows.
// grid: x = cap * ceil(ow / 64), y = row groups.
__global__ __launch_bounds__(256) void crop_horizontal_kernel(CropLayout L, const ppy_pil_image_t *__restrict__ images,
                                                              const int *__restrict__ src, const int *__restrict__ total,
                                                              unsigned char *__restrict__ ws) {
    const int bx = (L.ow + 63) >> 6;
    const int c = blockIdx.x / bx;
    if (c >= total[0]) return;
    const int *meta = reinterpret_cast<const int *>(ws + L.off_meta) + 8 * (long long)c;
    if (meta[CM_SKIP_H]) return;
    const ppy_pil_image_t im = images[src[2 * c]];
    const int first = max(meta[CM_FIRST], 0);
    const int rows = min(min(meta[CM_ROWS], L.max_h), im.h - first);
    const int x = (blockIdx.x - c * bx) * 64 + (threadIdx.x & 63);
    if (x >= L.ow) return;
    const int *bounds = reinterpret_cast<const int *>(ws + L.off_xtab) + (long long)c * L.xtab_ints;
    const int x0 = bounds[2 * x], cnt = bounds[2 * x + 1];
    const int *k = bounds + 2 * (long long)L.ow + (long long)x * L.kx;
    const bool map = meta[CM_XMAP] != 0;
    unsigned char *mid = ws + L.off_mid + (long long)c * L.mid_bytes;
    for (int r = blockIdx.y * 4 + (threadIdx.x >> 6); r < rows; r += gridDim.y * 4) {
        const unsigned char *p = im.base + (long long)(first + r) * im.pitch + (long long)x0 * 3;
        unsigned char *o = mid + (long long)r * L.mid_pitch + x * 3;
        if (map) {
            o[0] = p[0];
            o[1] = p[1];
            o[2] = p[2];
            continue;
        }
        int a0 = 1 << (CROP_BITS - 1), a1 = a0, a2 = a0;
        for (int j = 0; j < cnt; ++j) {
            const int kj = k[j];
            a0 += (int)p[3 * j] * kj;
            a1 += (int)p[3 * j + 1] * kj;
            a2 += (int)p[3 * j + 2] * kj;
        }
        o[0] = (unsigned char)crop_clip8(a0);
        o[1] = (unsigned char)crop_clip8(a1);
        o[2] = (unsigned char)crop_clip8(a2);
    }
}

// 12 bytes = 4 pixels of a row as three dwords; `cols` (1..4) of them exist.  Dword loads where the row allows it.
__device__ __forceinline__ void crop_load4(const unsigned char *p, bool dwords, int cols, unsigned (&d)[3]) {
    if (dwords && cols == 4) {
        const unsigned *q = reinterpret_cast<const unsigned *>(p);
        d[0] = q[0];
        d[1] = q[1];
        d[2] = q[2];
        return;
    }
    d[0] = d[1] = d[2] = 0;
#pragma unroll
    for (int b = 0; b < 12; ++b)
        if (b < 3 * cols) d[b >> 2] |= (unsigned)p[b] << (8 * (b & 3));
}

// One thread = 4 consecutive output columns of one output row; a workgroup = 128 columns x 8 rows.
// grid: x = cap * ceil(ceil(ow / 4) / 32), y = ceil(oh / 8).
__global__ __launch_bounds__(256) void crop_vertical_kernel(CropLayout L, const ppy_pil_image_t *__restrict__ images,
                                                            const int *__restrict__ src, const int *__restrict__ total,
                                                            const unsigned char *__restrict__ ws, unsigned char *__restrict__ out) {
    const int ow = L.ow, oh = L.oh;
    const int bx = (((ow + 3) >> 2) + 31) >> 5;
    const int c = blockIdx.x / bx;
    const int x = ((blockIdx.x - c * bx) * 32 + (threadIdx.x & 31)) * 4, y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= ow || y >= oh) return;
    const int cols = min(4, ow - x);
    unsigned char *o = out + ((long long)c * oh + y) * (long long)ow * 3 + (long long)x * 3;
    const bool wide = cols == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0;
    int v[12];
    if (c >= total[0]) {          // past the end: zero
#pragma unroll
        for (int b = 0; b < 12; ++b) v[b] = 0;
    } else {
        const int *meta = reinterpret_cast<const int *>(ws + L.off_meta) + 8 * (long long)c;
        const int *bounds = reinterpret_cast<const int *>(ws + L.off_ytab) + (long long)c * L.ytab_ints;
        int y0 = bounds[2 * y], cnt = bounds[2 * y + 1];
        const unsigned char *base;
        long long pitch;
        if (meta[CM_SKIP_H]) {    // ow == w: the vertical pass reads the source's own columns
            const ppy_pil_image_t im = images[src[2 * c]];
            base = im.base;
            pitch = im.pitch;
            cnt = min(cnt, im.h - y0);
        } else {
            const int rows = min(meta[CM_ROWS], L.max_h);
            base = ws + L.off_mid + (long long)c * L.mid_bytes;
            pitch = L.mid_pitch;
            y0 -= meta[CM_FIRST];
            y0 = min(max(y0, 0), max(rows - 1, 0));
            cnt = min(cnt, rows - y0);
        }
        const bool dwords = ((reinterpret_cast<uintptr_t>(base) | (unsigned long long)pitch) & 3) == 0;      // (x * 3 is a multiple of 12)
        const unsigned char *p = base + (long long)y0 * pitch + (long long)x * 3;
        if (meta[CM_YMAP]) {
            unsigned d[3];
            crop_load4(p, dwords, cols, d);
#pragma unroll
            for (int b = 0; b < 12; ++b) v[b] = (int)((d[b >> 2] >> (8 * (b & 3))) & 0xffu);
        } else {
            const int *k = bounds + 2 * (long long)oh + (long long)y * L.ky;
            int acc[12];
#pragma unroll
            for (int b = 0; b < 12; ++b) acc[b] = 1 << (CROP_BITS - 1);
            for (int j = 0; j < cnt; ++j) {
                const int kj = k[j];
                unsigned d[3];
                crop_load4(p + (long long)j * pitch, dwords, cols, d);
#pragma unroll
                for (int b = 0; b < 12; ++b) acc[b] += (int)((d[b >> 2] >> (8 * (b & 3))) & 0xffu) * kj;
            }
#pragma unroll
            for (int b = 0; b < 12; ++b) v[b] = crop_clip8(acc[b]);
        }
    }
    if (wide) {
        unsigned *q = reinterpret_cast<unsigned *>(o);
#pragma unroll
        for (int d = 0; d < 3; ++d)
            q[d] = (unsigned)v[4 * d] | ((unsigned)v[4 * d + 1] << 8) | ((unsigned)v[4 * d + 2] << 16) | ((unsigned)v[4 * d + 3] << 24);
    } else {
#pragma unroll
        for (int b = 0; b < 12; ++b)
            if (b < 3 * cols) o[b] = (unsigned char)v[b];
    }
}

template <bool ROWS>
int crop_launch(int n, const ppy_pil_image_t *h_images, const ppy_pil_image_t *d_images, const float *in_a, const int *in_b, int rows_or_m,
                float thresh, float pad, int top_k, int ow, int oh, int filter, void *ws, size_t ws_bytes, unsigned char *out, int *src,
                int *total, float *boxes, void *stream) {
    ppy_drop_stale_error();
    CropLayout L;
    const int rc = crop_layout(n, h_images, ROWS ? 0 : 1, rows_or_m, ow, oh, filter, pad, top_k, L, nullptr);
    if (rc != PPY_OK) return rc;
    PPY_CHECK_ARG(d_images && in_a && in_b && out && src && total && boxes);
    PPY_CHECK_ARG(!ROWS || thresh == thresh);
    if (crop_check_pitches(n, h_images) != PPY_OK) return PPY_ERR_BAD_ARG;
    if (!ws || (size_t)L.ws_bytes > ws_bytes) return PPY_ERR_WORKSPACE;
    PPY_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 15) == 0);
    hipStream_t st = (hipStream_t)stream;
    unsigned char *w8 = static_cast<unsigned char *>(ws);
    hipLaunchKernelGGL((crop_select_kernel<ROWS>), dim3(1), dim3(CROP_SELECT_THREADS), 0, st, L, d_images, in_a, in_b, ROWS ? rows_or_m : 1,
                       thresh, pad, top_k, w8, src, total, boxes);
    hipLaunchKernelGGL(crop_plan_kernel, dim3(L.cap, ceil_div(ow + oh, 256)), dim3(256), 0, st, L, d_images, src, total, boxes, w8);
    const int row_groups = ceil_div(L.max_h, 4);
    hipLaunchKernelGGL(crop_horizontal_kernel, dim3(L.cap * ceil_div(ow, 64), row_groups < 16 ? row_groups : 16), dim3(256), 0, st, L,
                       d_images, src, total, w8);
    hipLaunchKernelGGL(crop_vertical_kernel, dim3(L.cap * ceil_div(ceil_div(ow, 4), 32), ceil_div(oh, 8)), dim3(256), 0, st, L, d_images,
                       src, total, w8, out);
    return ppy_launch_status();
}
#endif  // PPY_PIL_HOST_ONLY

}  // namespace

extern "C" int ppy_pil_crop_plan_bytes(int n, const ppy_pil_image_t *h_images, int form, int rows_or_m, int ow, int oh, int filter, float pad,
                                       int top_k, size_t *ws_bytes, int *ksize_cap, char *h_reason) {
    CropLayout L;
    const int rc = crop_layout(n, h_images, form, rows_or_m, ow, oh, filter, pad, top_k, L, h_reason);
    if (rc != PPY_OK) return rc;
    if (crop_check_pitches(n, h_images) != PPY_OK) return PPY_ERR_BAD_ARG;
    if (ws_bytes) *ws_bytes = (size_t)L.ws_bytes;
    if (ksize_cap) ksize_cap[0] = L.kx, ksize_cap[1] = L.ky;
    return PPY_OK;
}

#ifndef PPY_PIL_HOST_ONLY
extern "C" int ppy_pil_crop_rows_u8(int n, const ppy_pil_image_t *h_images, const ppy_pil_image_t *images, const float *dets, const int *count,
                                    int K, float thresh, float pad, int top_k, int ow, int oh, int filter, void *ws, size_t ws_bytes,
                                    unsigned char *out, int *src, int *total, float *boxes, void *stream) {
    return crop_launch<true>(n, h_images, images, dets, count, K, thresh, pad, top_k, ow, oh, filter, ws, ws_bytes, out, src, total, boxes,
                             stream);
}

extern "C" int ppy_pil_crop_list_u8(int n, const ppy_pil_image_t *h_images, const ppy_pil_image_t *images, const float *boxes_in,
                                    const int *image, int M, int ow, int oh, int filter, void *ws, size_t ws_bytes, unsigned char *out,
                                    int *src, int *total, float *boxes, void *stream) {
    return crop_launch<false>(n, h_images, images, boxes_in, image, M, 0.0f, 0.0f, 1, ow, oh, filter, ws, ws_bytes, out, src, total, boxes,
                              stream);
}
#endif  // PPY_PIL_HOST_ONLY
