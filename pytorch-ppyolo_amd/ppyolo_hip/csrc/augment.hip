// Training batches on the device (ppyolo_hip/augment.py): the reference's training reader restated as a host planner
// plus these kernels.  The planner uploads ONE blob per batch: per-sample descriptors (struct AugSample, at offset 0),
// resize coefficient tables, the uint8 BGR source images, the target element offsets / values and the padded boxes.
//
// canvas_px      the pre-resize image of a sample at (y, x), all three channels, straight from the uint8 sources:
//                flip / crop index map -> RandomExpand fill or wrapped source value -> ColorDistort ops in the planned
//                order -> MixupImage blend (with DecodeImage's BGR->RGB swap).  Values are carried in double, which holds
//                every uint8 / float32 / float64 value of the chain exactly; each step rounds as numpy does (below).
// render kernel  cv2.resize over canvas_px (index tables from the planner), then NormalizeImage, NCHW float32.
// canvas kernel  canvas_px of one sample into a caller buffer in its natural dtype (pinning only).
// target kernels zero-fill of the dense targets, then the per-box elements the host computed (unique offsets).
//
// A source image lies either in the blob (src0 / src1 are byte offsets, rows packed) or OUTSIDE it (ext0 / ext1 set: src0 /
// src1 are indices into a table of device images that arrives in the kernel arguments, each with its own row pitch and any
// alignment -- a decoder's output or a cropped view of a larger tensor, read where it lies).  The table travels in windows of
// AUG_MAX_SOURCES entries, one launch per window, consecutive windows sharing one entry; a sample is rendered by the
// launch whose window starts at or below its lowest external index, so its two sources must lie in one window (adjacent
// entries always do; pack_batch emits them so).  Samples without external sources belong to the first launch.
//
// numpy >= 2 (NEP 50) dtype chain, restated:
//   mixup        f32(a) * f32(f), then + f32(b) * f32(1 - f) in float32 (0 where neither image lies), astype(uint8) truncates
//   brightness   astype(f32); + f32(delta)          contrast  astype(f32); * f32(delta)
//   saturation   gray = (a0*.299f + a1*.587f) + a2*.114f; gray *= f32(1 - delta); a *= f32(delta); a += gray
//   hue          np.dot(f32 image, float64 t) -> float64: the BLAS dgemm with k = 3 evaluates fma(a2, t2c, fma(a1, t1c, a0*t0c))
//   expand       astype(uint8) of float values WRAPS: truncate to an integer, keep the low 8 bits
//   resize       OpenCV 4.x scalar templates: 11-bit fixed point for 8U generic, float / double work types otherwise
//   normalise    uint8: the reference's numpy table; float: f32(x) / 255.f, then (double) - mean, (double) / std, each to f32
#include "common.h"

#include <type_traits>

namespace {

#pragma clang fp contract(off)

struct AugSample {
    long long src0, src1, xfirst, xw, yfirst, yw;                       // byte offsets into the blob
    long long ext0, ext1;                                               // 1: src0 / src1 is an index into the source table
    double hue[9];                                                      // t of np.dot(img, t), row-major
    double spare[4];                                                    // [0], [1]: f32(factor), f32(1 - factor) of mixup
    int h0, w0, h1, w1, mh, mw, nops, eh, ew, ey, ex, fill[3], cy, cx, ch, cw, flip, color_dtype, canvas_dtype, mode,
        fixpt, kx, ky, ix, iy, to_rgb, op[4];
    float oc[8];                                                        // per op: f32(delta), f32(1 - delta)
};
static_assert(sizeof(AugSample) == 328, "AugSample must match ppyolo_hip/augment.py DESC_BYTES");

enum { U8 = 0, F32 = 1, F64 = 2 };
enum { OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_SATURATION = 2, OP_HUE = 3 };
enum { MODE_NEAREST = 0, MODE_SEP = 1, MODE_AREA_FAST = 2 };

struct NormArgs {
    double mean[3], std[3];
    int is_scale;
};

constexpr int AUG_MAX_SOURCES = 16;                     // table entries per launch
constexpr int AUG_SRC_STEP = AUG_MAX_SOURCES - 1;       // distance of two windows' first entries
struct AugSource {
    const unsigned char *ptr;
    long long pitch;                                    // bytes per row, >= 3 * w
    int h, w;
};
struct AugSources {                                      // (the three ints first: a launch without external sources reads no further)
    int base, count, last;                              // first table index of the window, entries in it, the last window
    AugSource s[AUG_MAX_SOURCES];
};
// where a sample's two sources lie, resolved once per thread (source_px)
struct AugPix {
    const unsigned char *p0, *p1;
    int pitch0, pitch1;                                 // (the entry point refuses a pitch beyond int)
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the ColorDistort output (colour-stage dtype) at (y, x) of the mixup / source image
__device__ __forceinline__ void color_px(const AugPix &sp, const AugSample &d, int y, int x, double v[3]) {
    float f[3];
    if (d.h1 > 0) {         // MixupImage._mixup_img
        const bool in0 = y < d.h0 && x < d.w0, in1 = y < d.h1 && x < d.w1;
        const unsigned char *p0 = sp.p0 + (long long)clampi(y, 0, d.h0 - 1) * sp.pitch0 + (long long)clampi(x, 0, d.w0 - 1) * 3;
        const unsigned char *p1 = sp.p1 + (long long)clampi(y, 0, d.h1 - 1) * sp.pitch1 + (long long)clampi(x, 0, d.w1 - 1) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int cs = d.to_rgb ? 2 - c : c;
            float m = 0.0f;
            if (in0) m = (float)p0[cs] * (float)d.spare[0];
            if (in1) m = m + (float)p1[cs] * (float)d.spare[1];
            f[c] = (float)((int)m & 255);
        }
    } else {
        const unsigned char *p0 = sp.p0 + (long long)clampi(y, 0, d.h0 - 1) * sp.pitch0 + (long long)clampi(x, 0, d.w0 - 1) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) f[c] = (float)p0[d.to_rgb ? 2 - c : c];
    }
    bool is64 = false;
    double g[3];
    for (int k = 0; k < d.nops; ++k) {
        if (is64) {
#pragma unroll
            for (int c = 0; c < 3; ++c) f[c] = (float)g[c];         // astype(float32)
            is64 = false;
        }
        const float a = d.oc[2 * k], b = d.oc[2 * k + 1];
        switch (d.op[k]) {
        case OP_BRIGHTNESS:
#pragma unroll
            for (int c = 0; c < 3; ++c) f[c] = f[c] + a;
            break;
        case OP_CONTRAST:
#pragma unroll
            for (int c = 0; c < 3; ++c) f[c] = f[c] * a;
            break;
        case OP_SATURATION: {
            float gray = f[0] * (float)0.299 + f[1] * (float)0.587;
            gray = gray + f[2] * (float)0.114;
            gray = gray * b;
#pragma unroll
            for (int c = 0; c < 3; ++c) f[c] = f[c] * a + gray;
            break;
        }
        default: {          // OP_HUE
#pragma unroll
            for (int c = 0; c < 3; ++c)
                g[c] = __builtin_fma((double)f[2], d.hue[6 + c], __builtin_fma((double)f[1], d.hue[3 + c], (double)f[0] * d.hue[c]));
            is64 = true;
        }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = is64 ? g[c] : (double)f[c];
}

// the pre-resize canvas at (y, x): RandomFlipImage / RandomCrop index map, RandomExpand, colour stage
__device__ __forceinline__ void canvas_px(const AugPix &sp, const AugSample &d, int y, int x, double v[3]) {
    int X = (d.flip ? d.cw - 1 - x : x) + d.cx;
    int Y = y + d.cy;
    if (d.eh > 0) {
        const int yy = Y - d.ey, xx = X - d.ex;
        if (yy < 0 || yy >= d.mh || xx < 0 || xx >= d.mw) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = (double)d.fill[c];
            return;
        }
        color_px(sp, d, yy, xx, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (double)((long long)v[c] & 255);        // astype(uint8): truncate, wrap
        return;
    }
    color_px(sp, d, Y, X, v);
}

__device__ __forceinline__ bool desc_ok(const AugSample &d, long long nbytes, int S) {
    if (d.h0 <= 0 || d.w0 <= 0 || d.h1 < 0 || d.w1 < 0 || d.nops < 0 || d.nops > 4 || d.ch <= 0 || d.cw <= 0) return false;
    if (d.w0 > 0x7fffffff / 3 || d.w1 > 0x7fffffff / 3) return false;           // a row's bytes fit an int (AugPix)
    if (d.mh < d.h0 || d.mw < d.w0 || d.mh < d.h1 || d.mw < d.w1) return false;
    const int H = d.eh > 0 ? d.eh : d.mh, W = d.eh > 0 ? d.ew : d.mw;
    if (d.cy < 0 || d.cx < 0 || d.cy + d.ch > H || d.cx + d.cw > W) return false;
    if (S > 0) {
        if (d.kx <= 0 || d.ky <= 0 || d.kx > 64 || d.ky > 64) return false;
        if (d.xfirst < 0 || d.xfirst + 4LL * S > nbytes || d.yfirst < 0 || d.yfirst + 4LL * S > nbytes) return false;
        if (d.xw < 0 || d.xw + 4LL * S * d.kx > nbytes || d.yw < 0 || d.yw + 4LL * S * d.ky > nbytes) return false;
        if (d.mode == MODE_AREA_FAST && (d.ix <= 0 || d.iy <= 0 || d.ix * S > d.cw || d.iy * S > d.ch)) return false;
    }
    return true;
}

// One source of a sample: its first pixel and row pitch.  In the blob: the bytes must lie inside it.  External: the index must
// lie in this launch's window and the table entry must have the descriptor's extent.
__device__ __forceinline__ bool source_ok(const unsigned char *blob, long long nbytes, const AugSources &T, long long ext,
                                          long long src, int h, int w, const unsigned char *&p, int &pitch) {
    if (ext == 0) {
        if (src < 0 || src + (long long)h * w * 3 > nbytes) return false;
        p = blob + src;
        pitch = 3 * w;
        return true;
    }
    if (ext != 1 || src < T.base || src >= (long long)T.base + T.count) return false;
    const AugSource &s = T.s[(int)(src - T.base)];
    if (s.h != h || s.w != w) return false;
    p = s.ptr;
    pitch = (int)s.pitch;
    return true;
}

// desc_ok's half about the sources, and whether the sample is THIS launch's: the launch whose window starts at or below the
// sample's lowest external index (the first launch for a sample that has none) -> sp
__device__ __forceinline__ bool source_px(const unsigned char *blob, long long nbytes, const AugSources &T, const AugSample &d,
                                          AugPix &sp) {
    if ((d.ext0 | d.ext1) == 0) {           // every source in the blob: the first launch's
        if (T.base != 0 || d.src0 < 0 || d.src0 + (long long)d.h0 * d.w0 * 3 > nbytes) return false;
        if (d.h1 > 0 && (d.src1 < 0 || d.src1 + (long long)d.h1 * d.w1 * 3 > nbytes)) return false;
        sp.p0 = blob + d.src0;
        sp.pitch0 = 3 * d.w0;
        sp.p1 = blob + d.src1;
        sp.pitch1 = 3 * d.w1;
        return true;
    }
    const bool e0 = d.ext0 != 0, e1 = d.h1 > 0 && d.ext1 != 0;
    long long lo = e0 ? d.src0 : (e1 ? d.src1 : 0);
    if (e0 && e1 && d.src1 < lo) lo = d.src1;
    if (lo < T.base || (!T.last && lo >= (long long)T.base + AUG_SRC_STEP)) return false;
    if (!source_ok(blob, nbytes, T, d.ext0, d.src0, d.h0, d.w0, sp.p0, sp.pitch0)) return false;
    sp.p1 = sp.p0;
    sp.pitch1 = sp.pitch0;
    if (d.h1 > 0 && !source_ok(blob, nbytes, T, d.ext1, d.src1, d.h1, d.w1, sp.p1, sp.pitch1)) return false;
    return true;
}

__device__ __forceinline__ float normalise_f(float x, int c, const NormArgs &na) {
    if (na.is_scale) x = x / 255.0f;
    x = (float)((double)x - na.mean[c]);
    return (float)((double)x / na.std[c]);
}

// one output pixel, all three channels, canvas dtype CT (0 u8, 1 f32, 2 f64)
template <int CT>
__device__ __forceinline__ void render_px(const unsigned char *blob, const AugPix &sp, const AugSample &d, int dx, int dy,
                                          const float *lut, const NormArgs &na, float out[3]) {
    typedef typename std::conditional<CT == F64, double, float>::type WT;
    const int *xf = reinterpret_cast<const int *>(blob + d.xfirst), *yf = reinterpret_cast<const int *>(blob + d.yfirst);
    const float *xw = reinterpret_cast<const float *>(blob + d.xw), *yw = reinterpret_cast<const float *>(blob + d.yw);
    double r[3];
    bool u8 = CT == U8;         // the resized value is a uint8 (table) rather than a float of the canvas type
    if (d.mode == MODE_NEAREST) {
        canvas_px(sp, d, clampi(yf[dy], 0, d.ch - 1), clampi(xf[dx], 0, d.cw - 1), r);
    } else if (d.mode == MODE_AREA_FAST) {          // resizeAreaFast_: the block in row-major order
        const int x0 = xf[dx], y0 = yf[dy], area = d.ix * d.iy;
        if (CT == U8) {
            int s[3] = {0, 0, 0};
            for (int yy = 0; yy < d.iy; ++yy)
                for (int xx = 0; xx < d.ix; ++xx) {
                    double v[3];
                    canvas_px(sp, d, clampi(y0 + yy, 0, d.ch - 1), clampi(x0 + xx, 0, d.cw - 1), v);
#pragma unroll
                    for (int c = 0; c < 3; ++c) s[c] += (int)v[c];
                }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                int q;
                if (d.ix == 2 && d.iy == 2) q = (s[c] + 2) >> 2;               // ResizeAreaFastVec_SIMD_8u
                else q = (int)rintf((float)s[c] * (1.0f / (float)area));
                r[c] = (double)clampi(q, 0, 255);
            }
        } else {
            WT s[3] = {0, 0, 0};
            for (int yy = 0; yy < d.iy; ++yy)
                for (int xx = 0; xx < d.ix; ++xx) {
                    double v[3];
                    canvas_px(sp, d, clampi(y0 + yy, 0, d.ch - 1), clampi(x0 + xx, 0, d.cw - 1), v);
#pragma unroll
                    for (int c = 0; c < 3; ++c) s[c] = s[c] + (WT)v[c];
                }
            const float sc = 1.0f / (float)area;
#pragma unroll
            for (int c = 0; c < 3; ++c) r[c] = (double)(s[c] * (WT)sc);
        }
    } else if (CT == U8 && d.fixpt) {               // HResize*<uchar,int,short> + VResize*<..., FixedPtCast<int,uchar,22>>
        int acc[3] = {0, 0, 0};
        const int x0 = xf[dx], y0 = yf[dy];
        for (int k = 0; k < d.ky; ++k) {
            const int row = clampi(y0 + k, 0, d.ch - 1);
            int hs[3] = {0, 0, 0};
            for (int j = 0; j < d.kx; ++j) {
                double v[3];
                canvas_px(sp, d, row, clampi(x0 + j, 0, d.cw - 1), v);
                const int wj = (int)xw[dx * d.kx + j];
#pragma unroll
                for (int c = 0; c < 3; ++c) hs[c] += (int)v[c] * wj;
            }
            const int wk = (int)yw[dy * d.ky + k];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += hs[c] * wk;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] = (double)clampi((acc[c] + (1 << 21)) >> 22, 0, 255);
    } else {                                        // float work type: left to right, horizontal sums first
        WT acc[3] = {0, 0, 0};
        const int x0 = xf[dx], y0 = yf[dy];
        for (int k = 0; k < d.ky; ++k) {
            const int row = clampi(y0 + k, 0, d.ch - 1);
            WT hs[3] = {0, 0, 0};
            for (int j = 0; j < d.kx; ++j) {
                double v[3];
                canvas_px(sp, d, row, clampi(x0 + j, 0, d.cw - 1), v);
                const WT wj = (WT)xw[dx * d.kx + j];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const WT t = (WT)v[c] * wj;
                    hs[c] = j == 0 ? t : hs[c] + t;
                }
            }
            const WT wk = (WT)yw[dy * d.ky + k];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const WT t = hs[c] * wk;
                acc[c] = k == 0 ? t : acc[c] + t;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] = CT == U8 ? (double)clampi((int)rintf((float)acc[c]), 0, 255) : (double)acc[c];
    }
    if (u8) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = lut[c * 256 + (int)r[c]];
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = normalise_f((float)r[c], c, na);
    }
}

__global__ __launch_bounds__(256) void augment_render_kernel(const unsigned char *blob, long long nbytes, int S,
                                                             const float *lut, NormArgs na, float *out, AugSources T) {
    const AugSample &d = reinterpret_cast<const AugSample *>(blob)[blockIdx.z];
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    AugPix sp;
    if (dx >= S || dy >= S || !desc_ok(d, nbytes, S) || !source_px(blob, nbytes, T, d, sp)) return;
    float o[3];
    if (d.canvas_dtype == U8) render_px<U8>(blob, sp, d, dx, dy, lut, na, o);
    else if (d.canvas_dtype == F32) render_px<F32>(blob, sp, d, dx, dy, lut, na, o);
    else render_px<F64>(blob, sp, d, dx, dy, lut, na, o);
    const long long plane = (long long)S * S;
    float *p = out + (long long)blockIdx.z * 3 * plane + (long long)dy * S + dx;
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c * plane] = o[c];
}

__global__ __launch_bounds__(256) void augment_canvas_kernel(const unsigned char *blob, long long nbytes, int index, int h,
                                                             int w, int dtype, void *out, AugSources T) {
    const AugSample &d = reinterpret_cast<const AugSample *>(blob)[index];
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    AugPix sp;
    if (x >= w || y >= h || d.ch != h || d.cw != w || d.canvas_dtype != dtype || !desc_ok(d, nbytes, 0) ||
        !source_px(blob, nbytes, T, d, sp))
        return;
    double v[3];
    canvas_px(sp, d, y, x, v);
    const long long o = ((long long)y * w + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (dtype == U8) static_cast<unsigned char *>(out)[o + c] = (unsigned char)(int)v[c];
        else if (dtype == F32) static_cast<float *>(out)[o + c] = (float)v[c];
        else static_cast<double *>(out)[o + c] = v[c];
    }
}

__global__ __launch_bounds__(256) void augment_fill_kernel(float *out, long long total) {
    const long long n4 = total >> 2;
    const long long stride = (long long)gridDim.x * blockDim.x;
    floatx4 z = {0.f, 0.f, 0.f, 0.f};
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride)
        reinterpret_cast<floatx4 *>(out)[i] = z;
    const long long t = (n4 << 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < total) out[t] = 0.f;
}

__global__ __launch_bounds__(256) void augment_scatter_kernel(float *out, long long total, const long long *off,
                                                              const float *val, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long o = off[i];
    if (o >= 0 && o < total) out[o] = val[i];
}

}  // namespace

// the source table of one launch: window k of the host arrays (consecutive windows share one entry)
static int augment_window(int k, int windows, int n_src, const unsigned char *const *ptrs, const long long *pitch, const int *h,
                          const int *w, AugSources &T) {
    T.base = k * AUG_SRC_STEP;
    T.count = n_src - T.base < AUG_MAX_SOURCES ? n_src - T.base : AUG_MAX_SOURCES;
    T.last = k == windows - 1;
    for (int i = 0; i < AUG_MAX_SOURCES; ++i) {
        AugSource &s = T.s[i];
        s.ptr = nullptr;
        s.pitch = 0;
        s.h = s.w = 0;
        if (i >= T.count) continue;
        const int g = T.base + i;
        PPY_CHECK_ARG(ptrs[g] && h[g] > 0 && w[g] > 0 && pitch[g] >= 3LL * w[g] && pitch[g] <= 0x7fffffffLL);
        s.ptr = ptrs[g];
        s.pitch = pitch[g];
        s.h = h[g];
        s.w = w[g];
    }
    return PPY_OK;
}

static int augment_windows(int n_src) { return n_src <= AUG_MAX_SOURCES ? 1 : ceil_div(n_src - 1, AUG_SRC_STEP); }

extern "C" int ppy_augment_render_src_f32(const void *blob, long long blob_bytes, int n, int S, const float *lut,
                                          const double *mean_std, int is_scale, float *out, int n_src,
                                          const unsigned char *const *src_ptrs, const long long *src_pitch, const int *src_h,
                                          const int *src_w, void *stream) {
    ppy_drop_stale_error();
    PPY_CHECK_ARG(blob && lut && mean_std && out && n > 0 && n <= 65535 && S > 0 && S <= 8192 &&
                  blob_bytes >= (long long)n * (long long)sizeof(AugSample) && ((uintptr_t)blob & 7) == 0);
    PPY_CHECK_ARG(n_src >= 0 && (n_src == 0 || (src_ptrs && src_pitch && src_h && src_w)));
    NormArgs na;
    for (int c = 0; c < 3; ++c) {
        na.mean[c] = mean_std[c];
        na.std[c] = mean_std[3 + c];
        PPY_CHECK_ARG(na.std[c] != 0.0);
    }
    na.is_scale = is_scale ? 1 : 0;
    const int windows = augment_windows(n_src);
    AugSources T;
    for (int k = 0; k < windows; ++k) {         // every entry is checked before the first launch
        const int rc = augment_window(k, windows, n_src, src_ptrs, src_pitch, src_h, src_w, T);
        if (rc != PPY_OK) return rc;
    }
    for (int k = 0; k < windows; ++k) {
        augment_window(k, windows, n_src, src_ptrs, src_pitch, src_h, src_w, T);
        hipLaunchKernelGGL(augment_render_kernel, dim3(ceil_div(S, 64), ceil_div(S, 4), n), dim3(256), 0, (hipStream_t)stream,
                           (const unsigned char *)blob, blob_bytes, S, lut, na, out, T);
    }
    return ppy_launch_status();
}

extern "C" int ppy_augment_render_f32(const void *blob, long long blob_bytes, int n, int S, const float *lut,
                                      const double *mean_std, int is_scale, float *out, void *stream) {
    return ppy_augment_render_src_f32(blob, blob_bytes, n, S, lut, mean_std, is_scale, out, 0, nullptr, nullptr, nullptr, nullptr,
                                      stream);
}

extern "C" int ppy_augment_canvas_src(const void *blob, long long blob_bytes, int index, int h, int w, int dtype, void *out,
                                      int n_src, const unsigned char *const *src_ptrs, const long long *src_pitch,
                                      const int *src_h, const int *src_w, void *stream) {
    ppy_drop_stale_error();
    PPY_CHECK_ARG(blob && out && index >= 0 && h > 0 && w > 0 && h <= 65535 * 4 && dtype >= 0 && dtype <= 2 &&
                  blob_bytes >= (long long)(index + 1) * (long long)sizeof(AugSample) && ((uintptr_t)blob & 7) == 0);
    PPY_CHECK_ARG(n_src >= 0 && (n_src == 0 || (src_ptrs && src_pitch && src_h && src_w)));
    const int windows = augment_windows(n_src);
    AugSources T;
    for (int k = 0; k < windows; ++k) {
        const int rc = augment_window(k, windows, n_src, src_ptrs, src_pitch, src_h, src_w, T);
        if (rc != PPY_OK) return rc;
    }
    for (int k = 0; k < windows; ++k) {         // the sample is one window's: the other launches write nothing
        augment_window(k, windows, n_src, src_ptrs, src_pitch, src_h, src_w, T);
        hipLaunchKernelGGL(augment_canvas_kernel, dim3(ceil_div(w, 64), ceil_div(h, 4)), dim3(256), 0, (hipStream_t)stream,
                           (const unsigned char *)blob, blob_bytes, index, h, w, dtype, out, T);
    }
    return ppy_launch_status();
}

extern "C" int ppy_augment_canvas(const void *blob, long long blob_bytes, int index, int h, int w, int dtype, void *out,
                                  void *stream) {
    return ppy_augment_canvas_src(blob, blob_bytes, index, h, w, dtype, out, 0, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int ppy_augment_targets_f32(float *out, long long total, const long long *offsets, const float *values, int n,
                                       void *stream) {
    ppy_drop_stale_error();
    PPY_CHECK_ARG(out && total > 0 && n >= 0 && (n == 0 || (offsets && values)) && ((uintptr_t)out & 15) == 0);
    const long long n4 = total >> 2;
    const int blocks = (int)(n4 / 256 + 1 < 4096 ? n4 / 256 + 1 : 4096);
    hipLaunchKernelGGL(augment_fill_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, out, total);
    if (n > 0)
        hipLaunchKernelGGL(augment_scatter_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, out, total,
                           offsets, values, n);
    return ppy_launch_status();
}
