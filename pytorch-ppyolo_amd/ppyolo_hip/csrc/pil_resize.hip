// Pillow's Image.resize for 3-channel uint8 images on the device, bit for bit: the reference's ResizeImage(use_cv2=False)
// (tools/transform.py:1016-1024 = Image.fromarray(im).resize((S, S), interp)), as Pillow 12.2.0 computes it (libImaging
// Resample.c for filters 1..5, the affine scaler of Geometry.c for NEAREST).  DESIGN.md section 10d has the rules.
//
// Structure = Pillow's own: a HORIZONTAL pass into a uint8 image of h rows x ow columns, then a VERTICAL pass on that image,
// each `clip8((2^21 + sum pixel * k) >> 22)` in int32 with coefficients k = round(w * 2^22) from double weights.  Because the
// intermediate is rounded to uint8 exactly where Pillow rounds it, the result is Pillow's at any ratio by construction.
//   host   ppy_pil_resize_plan writes ONE blob: header, per-image descriptors, and one table per distinct axis (in, out):
//          bounds[out] = (first tap, taps), k[out][ksize].  No GPU call; tests/test_pil_resize_host.py reads the tables back.
//   launch 1  pil_horizontal_kernel: source (pixel stride 3, any pitch) -> intermediate in the caller's workspace (images whose
//          width does not change have no blocks to run).
//   launch 2  pil_vertical_kernel<STORE>: intermediate (or the source, where launch 1 was skipped) -> STORE 0: uint8 HWC;
//          STORE 1: R/B swap, lut[c][v], NCHW float32, one 16-byte store per channel (what preprocess_tile_kernel stores).
// An axis that keeps its size and both axes of NEAREST are INDEX MAPS: tables with ksize = 0 whose bound is the one source
// index; the kernels copy that pixel.  Images of different sizes share both launches (blockIdx.z = image).
// All device arithmetic is integer; the doubles live in the host planner.
#include <cmath>
#include <cstdio>
#include <cstring>

#ifndef PPY_PIL_HOST_ONLY
#include "common.h"
#else      // the planner alone as plain C++ (tools/pil_resize_asan.cpp: AddressSanitizer build, no HIP headers)
#include <stddef.h>
#include <stdint.h>

#include "../../../include/ppyolo_hip.h"
#define PPY_CHECK_ARG(cond) \
    do {                    \
        if (!(cond)) return PPY_ERR_BAD_ARG; \
    } while (0)
#endif

namespace {

constexpr unsigned PIL_MAGIC = 0x314c4950u;      // "PIL1"
constexpr int PIL_MAX_IMAGES = 1024, PIL_MAX_IN = 65535, PIL_MAX_OUT = 8192, PIL_MAX_KSIZE = 1024;
constexpr int PIL_BITS = 22;

struct PilHeader {            // 64 bytes at offset 0 of the blob
    unsigned magic;
    int n, ow, oh, filter, n_tables;
    int max_h_horizontal;     // tallest image that runs the horizontal pass (0: launch 1 is skipped)
    int mid_pitch;            // bytes per row of every intermediate image: 3 * ow rounded up to 16
    long long blob_bytes, ws_bytes;
    int desc_offset, table_offset;
    int reserved[2];
};
struct PilImage {             // 48 bytes each, at desc_offset
    const unsigned char *src;
    long long pitch;
    int h, w;
    int xtab, ytab;           // byte offsets of the axis tables in the blob; xtab < 0: the horizontal pass is skipped
    long long mid_offset;     // of the intermediate image in the workspace
    long long reserved;
};
struct PilTable {             // 16 bytes, then int bounds[out][2], then int k[out][ksize]
    int in, out, ksize, kind; // kind: the filter code, or -1 for the identity map of an axis that keeps its size
};
static_assert(sizeof(PilHeader) == 64 && sizeof(PilImage) == 48 && sizeof(PilTable) == 16, "blob layout");

// ---- host planner ----------------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)
inline double pil_filter(int f, double x) {      // Resample.c's filters, operation for operation
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
        return std::sin(x) / x * (0.54f + 0.46f * std::cos(x));      // (float literals, as in Pillow)
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
            s1 = std::sin(p) / p;
        }
        const double y = x / 3;
        if (y != 0.0) {
            const double p = y * M_PI;
            s3 = std::sin(p) / p;
        }
        return s1 * s3;
    }
    }
}
inline double pil_support(int f) { return f == 4 ? 0.5 : (f == 2 || f == 5) ? 1.0 : f == 3 ? 2.0 : 3.0; }

// taps per output sample of one axis; 0 for an index map (kind -1 or NEAREST)
long long pil_ksize(int in, int out, int kind) {
    if (kind <= 0) return 0;
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    return (long long)std::ceil(pil_support(kind) * fs) * 2 + 1;
}
size_t pil_table_bytes(int out, long long ksize) { return sizeof(PilTable) + (size_t)out * 8 + (size_t)out * (size_t)ksize * 4; }

void pil_fill_table(unsigned char *at, int in, int out, int kind) {
    const int ksize = (int)pil_ksize(in, out, kind);
    PilTable t = {in, out, ksize, kind};
    memcpy(at, &t, sizeof t);
    int *bounds = reinterpret_cast<int *>(at + sizeof t), *kk = bounds + 2 * (size_t)out;
    if (kind < 0) {
        for (int x = 0; x < out; ++x) bounds[2 * x] = x, bounds[2 * x + 1] = 1;
        return;
    }
    const double scale = (double)in / (double)out;
    if (kind == 0) {          // the affine scaler: the coordinate is accumulated, not recomputed
        double xo = scale * 0.5;
        for (int x = 0; x < out; ++x) {
            int s = (int)std::floor(xo);
            s = s < 0 ? 0 : (s > in - 1 ? in - 1 : s);      // (never taken for a whole-image resize; keeps the kernel in bounds)
            bounds[2 * x] = s;
            bounds[2 * x + 1] = 1;
            xo += scale;
        }
        return;
    }
    const double fs = scale < 1.0 ? 1.0 : scale, support = pil_support(kind) * fs, ss = 1.0 / fs;
    double w[PIL_MAX_KSIZE];
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            w[x] = pil_filter(kind, (x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        int *k = kk + (size_t)xx * ksize;
        for (int x = 0; x < xmax; ++x) {
            double v = w[x];
            if (ww != 0.0) v /= ww;
            k[x] = v < 0 ? (int)(-0.5 + v * (1 << PIL_BITS)) : (int)(0.5 + v * (1 << PIL_BITS));
        }
        for (int x = xmax; x < ksize; ++x) k[x] = 0;
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}

struct PilAxis {
    int in, out, kind;
    size_t offset;
};
struct PilLayout {
    PilAxis axes[2 * PIL_MAX_IMAGES];
    int n_axes;
    int xaxis[PIL_MAX_IMAGES], yaxis[PIL_MAX_IMAGES];      // index into axes; xaxis -1: skipped
    size_t blob_bytes, ws_bytes;
    int mid_pitch, max_h_horizontal;
};

int pil_axis(PilLayout &L, int in, int out, int kind, size_t &cursor) {
    for (int i = 0; i < L.n_axes; ++i)
        if (L.axes[i].in == in && L.axes[i].out == out && L.axes[i].kind == kind) return i;
    L.axes[L.n_axes] = {in, out, kind, cursor};
    cursor += (pil_table_bytes(out, pil_ksize(in, out, kind)) + 15) & ~(size_t)15;
    return L.n_axes++;
}

// Validates the request and lays the blob out.  reason: NULL or 96 characters.
int pil_layout(int n, const ppy_pil_image_t *im, int ow, int oh, int filter, PilLayout &L, char *reason) {
    char local[96];
    char *r = reason ? reason : local;
    r[0] = 0;
    if (!(n >= 1 && n <= PIL_MAX_IMAGES) || !im) {
        snprintf(r, 96, "batch of %d images, supported: 1..%d", n, PIL_MAX_IMAGES);
        return PPY_ERR_BAD_ARG;
    }
    if (filter < 0 || filter > 5) {
        snprintf(r, 96, "filter code %d, Pillow's codes are 0..5", filter);
        return PPY_ERR_UNSUPPORTED;
    }
    if (ow < 1 || ow > PIL_MAX_OUT || oh < 1 || oh > PIL_MAX_OUT) {
        snprintf(r, 96, "output size %d x %d, each side must be in 1..%d", ow, oh, PIL_MAX_OUT);
        return PPY_ERR_UNSUPPORTED;
    }
    for (int i = 0; i < n; ++i) {
        if (im[i].h < 1 || im[i].h > PIL_MAX_IN || im[i].w < 1 || im[i].w > PIL_MAX_IN) {
            snprintf(r, 96, "image %d: input size %d x %d, each side must be in 1..%d", i, im[i].w, im[i].h, PIL_MAX_IN);
            return PPY_ERR_UNSUPPORTED;
        }
        const long long kx = im[i].w == ow ? 0 : pil_ksize(im[i].w, ow, filter), ky = im[i].h == oh ? 0 : pil_ksize(im[i].h, oh, filter);
        if (kx > PIL_MAX_KSIZE || ky > PIL_MAX_KSIZE) {
            snprintf(r, 96, "image %d: %d x %d to %d x %d needs ksize %lld, at most %d", i, im[i].w, im[i].h, ow, oh, kx > ky ? kx : ky,
                     PIL_MAX_KSIZE);
            return PPY_ERR_UNSUPPORTED;
        }
    }
    L.n_axes = 0;
    L.mid_pitch = (3 * ow + 15) & ~15;
    L.max_h_horizontal = 0;
    size_t cursor = (sizeof(PilHeader) + (size_t)n * sizeof(PilImage) + 15) & ~(size_t)15, ws = 0;
    for (int i = 0; i < n; ++i) {
        L.xaxis[i] = im[i].w == ow ? -1 : pil_axis(L, im[i].w, ow, filter, cursor);
        L.yaxis[i] = pil_axis(L, im[i].h, oh, im[i].h == oh ? -1 : filter, cursor);
        if (L.xaxis[i] >= 0) {
            ws += ((size_t)im[i].h * (size_t)L.mid_pitch + 255) & ~(size_t)255;
            if (im[i].h > L.max_h_horizontal) L.max_h_horizontal = im[i].h;
        }
    }
    L.blob_bytes = cursor;
    L.ws_bytes = ws;
    if (cursor > ((size_t)1 << 31) - 1) {
        snprintf(r, 96, "the batch's tables need %zu bytes, at most 2^31 - 1", cursor);
        return PPY_ERR_UNSUPPORTED;
    }
    return PPY_OK;
}

#ifndef PPY_PIL_HOST_ONLY
// ---- kernels ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int pil_clip8(int acc) { return min(max(acc >> PIL_BITS, 0), 255); }

// One thread = one pixel of the intermediate image (3 channels); a workgroup = 64 columns x 4 source rows.
__global__ __launch_bounds__(256) void pil_horizontal_kernel(const unsigned char *__restrict__ blob, unsigned char *__restrict__ ws) {
    const PilHeader &hd = *reinterpret_cast<const PilHeader *>(blob);
    const PilImage &im = reinterpret_cast<const PilImage *>(blob + hd.desc_offset)[blockIdx.z];
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (im.xtab < 0 || y >= im.h || x >= hd.ow) return;
    const PilTable &t = *reinterpret_cast<const PilTable *>(blob + im.xtab);
    const int *bounds = reinterpret_cast<const int *>(blob + im.xtab + sizeof(PilTable));
    const int x0 = bounds[2 * x], cnt = bounds[2 * x + 1];
    const unsigned char *p = im.src + (long long)y * im.pitch + (long long)x0 * 3;
    unsigned char *o = ws + im.mid_offset + (long long)y * hd.mid_pitch + x * 3;
    if (t.ksize == 0) {       // index map (NEAREST)
        o[0] = p[0];
        o[1] = p[1];
        o[2] = p[2];
        return;
    }
    const int *k = bounds + 2 * (long long)t.out + (long long)x * t.ksize;
    int a0 = 1 << (PIL_BITS - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < cnt; ++j) {
        const int kj = k[j];
        a0 += (int)p[3 * j] * kj;
        a1 += (int)p[3 * j + 1] * kj;
        a2 += (int)p[3 * j + 2] * kj;
    }
    o[0] = (unsigned char)pil_clip8(a0);
    o[1] = (unsigned char)pil_clip8(a1);
    o[2] = (unsigned char)pil_clip8(a2);
}

// 12 bytes = 4 pixels of a row as three dwords; `cols` (1..4) of them exist.  Dword loads where the row allows it.
__device__ __forceinline__ void pil_load4(const unsigned char *p, bool dwords, int cols, unsigned (&d)[3]) {
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
// STORE 0: out = uint8 [n][oh][ow][3].  STORE 1: out = float [n][3][oh][ow] through lut[c][v], channels swapped if swap_rb.
template <int STORE>
__global__ __launch_bounds__(256) void pil_vertical_kernel(const unsigned char *__restrict__ blob, const unsigned char *__restrict__ ws,
                                                           void *__restrict__ out, const float *__restrict__ lut, int swap_rb) {
    __shared__ float s_lut[STORE ? 3 * 256 : 1];
    if (STORE) {
        s_lut[threadIdx.x] = lut[threadIdx.x];
        s_lut[256 + threadIdx.x] = lut[256 + threadIdx.x];
        s_lut[512 + threadIdx.x] = lut[512 + threadIdx.x];
        __syncthreads();
    }
    const PilHeader &hd = *reinterpret_cast<const PilHeader *>(blob);
    const PilImage &im = reinterpret_cast<const PilImage *>(blob + hd.desc_offset)[blockIdx.z];
    const int ow = hd.ow, oh = hd.oh;
    const int x = (blockIdx.x * 32 + (threadIdx.x & 31)) * 4, y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= ow || y >= oh) return;
    const int cols = min(4, ow - x);
    const unsigned char *src;
    long long pitch;
    if (im.xtab < 0) {
        src = im.src;
        pitch = im.pitch;
    } else {
        src = ws + im.mid_offset;
        pitch = hd.mid_pitch;
    }
    const bool dwords = ((reinterpret_cast<uintptr_t>(src) | (unsigned long long)pitch) & 3) == 0;      // (x * 3 is a multiple of 12)
    const PilTable &t = *reinterpret_cast<const PilTable *>(blob + im.ytab);
    const int *bounds = reinterpret_cast<const int *>(blob + im.ytab + sizeof(PilTable));
    const int y0 = bounds[2 * y], cnt = bounds[2 * y + 1];
    const unsigned char *p = src + (long long)y0 * pitch + (long long)x * 3;
    int v[12];
    if (t.ksize == 0) {       // index map: an axis that keeps its size, or NEAREST
        unsigned d[3];
        pil_load4(p, dwords, cols, d);
#pragma unroll
        for (int b = 0; b < 12; ++b) v[b] = (int)((d[b >> 2] >> (8 * (b & 3))) & 0xffu);
    } else {
        const int *k = bounds + 2 * (long long)t.out + (long long)y * t.ksize;
        int acc[12];
#pragma unroll
        for (int b = 0; b < 12; ++b) acc[b] = 1 << (PIL_BITS - 1);
        for (int j = 0; j < cnt; ++j) {
            const int kj = k[j];
            unsigned d[3];
            pil_load4(p + (long long)j * pitch, dwords, cols, d);
#pragma unroll
            for (int b = 0; b < 12; ++b) acc[b] += (int)((d[b >> 2] >> (8 * (b & 3))) & 0xffu) * kj;
        }
#pragma unroll
        for (int b = 0; b < 12; ++b) v[b] = pil_clip8(acc[b]);
    }
    if (STORE == 0) {
        unsigned char *o = static_cast<unsigned char *>(out) + ((long long)blockIdx.z * oh + y) * (long long)ow * 3 + (long long)x * 3;
        if (cols == 4 && ((reinterpret_cast<uintptr_t>(out) | (unsigned long long)((long long)ow * 3)) & 3) == 0) {
            unsigned *q = reinterpret_cast<unsigned *>(o);
#pragma unroll
            for (int d = 0; d < 3; ++d)
                q[d] = (unsigned)v[4 * d] | ((unsigned)v[4 * d + 1] << 8) | ((unsigned)v[4 * d + 2] << 16) | ((unsigned)v[4 * d + 3] << 24);
        } else {
#pragma unroll
            for (int b = 0; b < 12; ++b)
                if (b < 3 * cols) o[b] = (unsigned char)v[b];
        }
    } else {
        const long long plane = (long long)oh * ow;
        float *o = static_cast<float *>(out) + (long long)blockIdx.z * 3 * plane + (long long)y * ow + x;
        const bool vec = (ow & 3) == 0;          // (then cols == 4 and the row start is 16-byte aligned)
#pragma unroll
        for (int c = 0; c < 3; ++c) {            // c = OUTPUT channel
            const int cs = swap_rb ? 2 - c : c;
            float f[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) f[e] = s_lut[c * 256 + v[3 * e + cs]];
            if (vec) {
                floatx4 vv = {f[0], f[1], f[2], f[3]};
                *reinterpret_cast<floatx4 *>(o + c * plane) = vv;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < cols) o[c * plane + e] = f[e];
            }
        }
    }
}

// What the launches check of the HOST blob before they size a grid from it.
int pil_check_blob(int n, const void *h_blob, const void *d_blob, size_t blob_bytes, const void *ws, size_t ws_bytes, PilHeader &hd) {
    PPY_CHECK_ARG(h_blob && d_blob && blob_bytes >= sizeof(PilHeader));
    memcpy(&hd, h_blob, sizeof hd);
    PPY_CHECK_ARG(hd.magic == PIL_MAGIC && hd.n == n && n >= 1 && n <= PIL_MAX_IMAGES);
    PPY_CHECK_ARG(hd.blob_bytes > 0 && (size_t)hd.blob_bytes <= blob_bytes);
    PPY_CHECK_ARG(hd.ow >= 1 && hd.ow <= PIL_MAX_OUT && hd.oh >= 1 && hd.oh <= PIL_MAX_OUT);
    PPY_CHECK_ARG(hd.max_h_horizontal >= 0 && hd.max_h_horizontal <= PIL_MAX_IN);
    if ((size_t)hd.ws_bytes > ws_bytes || (hd.ws_bytes > 0 && !ws)) return PPY_ERR_WORKSPACE;
    const PilImage *im = reinterpret_cast<const PilImage *>(static_cast<const unsigned char *>(h_blob) + hd.desc_offset);
    for (int i = 0; i < n; ++i) {
        PPY_CHECK_ARG(im[i].src && im[i].h >= 1 && im[i].w >= 1 && (im[i].h == 1 || im[i].pitch >= 3LL * im[i].w));
        PPY_CHECK_ARG(im[i].ytab >= hd.table_offset && im[i].ytab < hd.blob_bytes && im[i].xtab < hd.blob_bytes);
    }
    return PPY_OK;
}

template <int STORE>
int pil_launch(int n, const void *h_blob, const void *d_blob, size_t blob_bytes, void *ws, size_t ws_bytes, void *out, const float *lut,
               int swap_rb, void *stream) {
    ppy_drop_stale_error();
    PilHeader hd;
    const int rc = pil_check_blob(n, h_blob, d_blob, blob_bytes, ws, ws_bytes, hd);
    if (rc != PPY_OK) return rc;
    PPY_CHECK_ARG(out && (STORE == 0 || lut));
    const unsigned char *blob = static_cast<const unsigned char *>(d_blob);
    if (hd.max_h_horizontal > 0)
        hipLaunchKernelGGL(pil_horizontal_kernel, dim3(ceil_div(hd.ow, 64), ceil_div(hd.max_h_horizontal, 4), n), dim3(256), 0,
                           (hipStream_t)stream, blob, static_cast<unsigned char *>(ws));
    hipLaunchKernelGGL((pil_vertical_kernel<STORE>), dim3(ceil_div(ceil_div(hd.ow, 4), 32), ceil_div(hd.oh, 8), n), dim3(256), 0,
                       (hipStream_t)stream, blob, static_cast<const unsigned char *>(ws), out, lut, swap_rb);
    return ppy_launch_status();
}
#endif  // PPY_PIL_HOST_ONLY

}  // namespace

extern "C" size_t ppy_pil_resize_plan_bytes(int n, const ppy_pil_image_t *h_images, int ow, int oh, int filter) {
    static thread_local PilLayout L;
    if (pil_layout(n, h_images, ow, oh, filter, L, nullptr) != PPY_OK) return 0;
    return L.blob_bytes;
}

extern "C" int ppy_pil_resize_plan(int n, const ppy_pil_image_t *h_images, int ow, int oh, int filter, void *h_blob, size_t blob_bytes,
                                   size_t *ws_bytes, char *h_reason) {
    static thread_local PilLayout L;
    const int rc = pil_layout(n, h_images, ow, oh, filter, L, h_reason);
    if (rc != PPY_OK) return rc;
    PPY_CHECK_ARG(h_blob && (reinterpret_cast<uintptr_t>(h_blob) & 7) == 0);
    if (blob_bytes < L.blob_bytes) return PPY_ERR_WORKSPACE;
    for (int i = 0; i < n; ++i)
        PPY_CHECK_ARG(h_images[i].base && (h_images[i].h == 1 || h_images[i].pitch >= 3LL * h_images[i].w));
    unsigned char *b = static_cast<unsigned char *>(h_blob);
    PilHeader hd;
    memset(&hd, 0, sizeof hd);
    hd.magic = PIL_MAGIC;
    hd.n = n;
    hd.ow = ow;
    hd.oh = oh;
    hd.filter = filter;
    hd.n_tables = L.n_axes;
    hd.max_h_horizontal = L.max_h_horizontal;
    hd.mid_pitch = L.mid_pitch;
    hd.blob_bytes = (long long)L.blob_bytes;
    hd.ws_bytes = (long long)L.ws_bytes;
    hd.desc_offset = (int)sizeof(PilHeader);
    hd.table_offset = L.n_axes ? (int)L.axes[0].offset : (int)L.blob_bytes;
    memcpy(b, &hd, sizeof hd);
    size_t mid = 0;
    for (int i = 0; i < n; ++i) {
        PilImage d;
        memset(&d, 0, sizeof d);
        d.src = h_images[i].base;
        d.pitch = h_images[i].h == 1 && h_images[i].pitch < 3LL * h_images[i].w ? 3LL * h_images[i].w : h_images[i].pitch;
        d.h = h_images[i].h;
        d.w = h_images[i].w;
        d.xtab = L.xaxis[i] < 0 ? -1 : (int)L.axes[L.xaxis[i]].offset;
        d.ytab = (int)L.axes[L.yaxis[i]].offset;
        d.mid_offset = (long long)mid;
        if (L.xaxis[i] >= 0) mid += ((size_t)d.h * (size_t)L.mid_pitch + 255) & ~(size_t)255;
        memcpy(b + sizeof(PilHeader) + (size_t)i * sizeof(PilImage), &d, sizeof d);
    }
    for (int a = 0; a < L.n_axes; ++a) pil_fill_table(b + L.axes[a].offset, L.axes[a].in, L.axes[a].out, L.axes[a].kind);
    if (ws_bytes) *ws_bytes = L.ws_bytes;
    return PPY_OK;
}

#ifndef PPY_PIL_HOST_ONLY
extern "C" int ppy_pil_resize_u8(int n, const void *h_blob, const void *blob, size_t blob_bytes, void *ws, size_t ws_bytes,
                                 unsigned char *out, void *stream) {
    return pil_launch<0>(n, h_blob, blob, blob_bytes, ws, ws_bytes, out, nullptr, 0, stream);
}

extern "C" int ppy_preprocess_pil_u8_f32(int n, const void *h_blob, const void *blob, size_t blob_bytes, void *ws, size_t ws_bytes,
                                         int swap_rb, const float *lut, float *out, void *stream) {
    PPY_CHECK_ARG(out && (reinterpret_cast<uintptr_t>(out) & 15) == 0);
    return pil_launch<1>(n, h_blob, blob, blob_bytes, ws, ws_bytes, out, lut, swap_rb ? 1 : 0, stream);
}
#endif  // PPY_PIL_HOST_ONLY
