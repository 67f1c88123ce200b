// GroupNorm and Mish of Conv2dUnit (reference model/custom_layers.py:37-43, :118-135) on NHWC views.  Contract:
// include/ppyolo_hip.h (ppy_group_norm_f32, ppy_mish_f32), DESIGN.md section 9.
//
// Both are streaming kernels: every access is 16 bytes along C, a row of 64 lanes covers 1 KB of one pixel.  GroupNorm is three
// launches -- (1) partial sums per (image, pixel chunk, group): a workgroup owns a chunk of pixels over ALL channels, so its loads
// are whole rows whatever C / groups is and no wave owns a whole image's group; (2) one thread per (image, group) adds the chunks
// in chunk order and leaves mean (double) and 1 / sqrt(var + eps); (3) apply + residual + activation (+ the 2 x 2 upsampled store).
// The sums are SHIFTED and double: every group subtracts its own first element k (channel g * C / groups of pixel 0 of the image, the
// same value in every chunk) before it adds d = x - k and d * d.  x - k is exact in double, so mean = k + E[d] and
// var = E[d^2] - E[d]^2 carry no cancellation when the mean is large against the spread (raw double moments would still lose
// mean^2 / var * 2^-53, visible in float32 from a ratio of 1e4 on), and every order of addition is fixed -- no atomics.
#include "common.h"
#include "norm_act.h"

namespace {

constexpr int GN_THREADS = 256;
constexpr int GN_MIN_CHUNK = 32;      // pixels: below it a chunk is not worth a workgroup

// grid (nchunks, N, slabs).  Threads are (tx, ty) = (channel quad, pixel) with TX = 1 << tx_log2 <= 64 lanes along C.  slabs > 1: a
// workgroup owns the 4 * TX channels of its slab only (whole groups: the host checks 4 * TX % (C / G) == 0), which gives the small,
// wide maps (19 x 19 x 2048: 12 chunks) eight times the workgroups; slabs == 1: it walks all channel quads, TX at a time.
// LDS: red[256][8] doubles, then chan[C][2] doubles.  part[((n * nchunks + chunk) * G + g) * 2 + {0: sum of d, 1: sum of d * d}].
__global__ __launch_bounds__(GN_THREADS) void gn_partial_kernel(const float *__restrict__ x, int ld, int P, int C, int G,
                                                                int rows_per, int tx_log2, double *__restrict__ part) {
    extern __shared__ double gn_lds[];
    double *red = gn_lds, *chan = gn_lds + GN_THREADS * 8;
    const int n = blockIdx.y, chunk = blockIdx.x, nchunks = gridDim.x;
    const int t = threadIdx.x, TX = 1 << tx_log2, tx = t & (TX - 1), ty = t >> tx_log2, TY = GN_THREADS >> tx_log2;
    const int p0 = chunk * rows_per, p1 = min(P, p0 + rows_per), Q = C >> 2, cpg = C / G;
    const float *xb = x + (long long)n * P * ld;
    const bool slab = gridDim.z > 1;
    const int q_begin = slab ? (int)blockIdx.z * TX : 0, q_end = slab ? min(Q, q_begin + TX) : Q;
    for (int q0 = q_begin; q0 < q_end; q0 += TX) {          // (uniform trip count: the barriers below are reached by every thread)
        const int q = q0 + tx;
        double s[4] = {0., 0., 0., 0.}, ss[4] = {0., 0., 0., 0.}, k[4] = {0., 0., 0., 0.};
        if (q < Q) {
#pragma unroll
            for (int j = 0; j < 4; ++j) k[j] = (double)xb[(4 * q + j) / cpg * cpg];      // the group's shift
            for (int p = p0 + ty; p < p1; p += TY) {
                const floatx4 v = *reinterpret_cast<const floatx4 *>(xb + (long long)p * ld + 4 * q);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double d = (double)v[j] - k[j];
                    s[j] += d;
                    ss[j] += d * d;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            red[t * 8 + j] = s[j];
            red[t * 8 + 4 + j] = ss[j];
        }
        __syncthreads();
        for (int st = TY >> 1; st > 0; st >>= 1) {      // fixed tree over the pixel lanes
            if (ty < st) {
#pragma unroll
                for (int e = 0; e < 8; ++e) red[t * 8 + e] += red[(t + st * TX) * 8 + e];
            }
            __syncthreads();
        }
        if (ty == 0 && q < Q) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                chan[(4 * q + j) * 2] = red[t * 8 + j];
                chan[(4 * q + j) * 2 + 1] = red[t * 8 + 4 + j];
            }
        }
        __syncthreads();
    }
    const int g_begin = slab ? 4 * q_begin / cpg : 0, g_end = slab ? min(G, 4 * (q_begin + TX) / cpg) : G;
    for (int g = g_begin + t; g < g_end; g += GN_THREADS) {
        double a = 0., b = 0.;
        for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
            a += chan[2 * c];
            b += chan[2 * c + 1];
        }
        double *o = part + (((long long)n * nchunks + chunk) * G + g) * 2;
        o[0] = a;
        o[1] = b;
    }
}

// One thread per (image, group): chunks in order.  mean[N * G] doubles, rstd[N * G] floats.
__global__ void gn_finalize_kernel(const double *__restrict__ part, const float *__restrict__ x, int ld, int P, int cpg, int NG, int G,
                                   int nchunks, double count, float eps, double *__restrict__ mean, float *__restrict__ rstd) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NG) return;
    const int n = i / G, g = i - n * G;
    double a = 0., b = 0.;
    for (int c = 0; c < nchunks; ++c) {
        const double *p = part + (((long long)n * nchunks + c) * G + g) * 2;
        a += p[0];
        b += p[1];
    }
    const double m = a / count;          // of d = x - shift
    double var = b / count - m * m;
    if (var < 0.) var = 0.;
    mean[i] = (double)x[(long long)n * P * ld + g * cpg] + m;
    rstd[i] = (float)(1.0 / sqrt(var + (double)eps));
}

// Grid-stride over (pixel, channel quad).  UPS: the store goes to the four positions of the [N, 2H, 2W] destination.
template <bool UPS>
__global__ __launch_bounds__(GN_THREADS) void gn_apply_kernel(const float *__restrict__ x, int x_ld, const float *__restrict__ gamma,
                                                              const float *__restrict__ beta, const double *__restrict__ mean,
                                                              const float *__restrict__ rstd, const float *__restrict__ res, int res_ld,
                                                              float *__restrict__ y, int y_ld, int N, int H, int W, int C, int G, int act) {
    const int Q = C >> 2, cpg = C / G;
    const long long P = (long long)H * W, total = (long long)N * P * Q;
    for (long long i = (long long)blockIdx.x * GN_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * GN_THREADS) {
        const long long pix = i / Q;
        const int q = (int)(i - pix * Q), c0 = 4 * q;
        const int n = (int)(pix / P);
        const floatx4 v = *reinterpret_cast<const floatx4 *>(x + pix * x_ld + c0);
        const floatx4 ga = *reinterpret_cast<const floatx4 *>(gamma + c0), be = *reinterpret_cast<const floatx4 *>(beta + c0);
        floatx4 r = {0.f, 0.f, 0.f, 0.f};
        if (res) r = *reinterpret_cast<const floatx4 *>(res + pix * res_ld + c0);
        floatx4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int s = n * G + (c0 + j) / cpg;
            const float d = (float)((double)v[j] - mean[s]);
            float u = d * rstd[s] * ga[j] + be[j];
            if (res) u += r[j];
            o[j] = norm_act(u, act);
        }
        if (UPS) {
            const long long pin = pix - (long long)n * P;
            const int h = (int)(pin / W), w = (int)(pin - (long long)h * W);
            float *yo = y + (((long long)n * 2 * H + 2 * h) * (2 * W) + 2 * w) * y_ld + c0;
            const long long row = (long long)2 * W * y_ld;
            *reinterpret_cast<floatx4 *>(yo) = o;
            *reinterpret_cast<floatx4 *>(yo + y_ld) = o;
            *reinterpret_cast<floatx4 *>(yo + row) = o;
            *reinterpret_cast<floatx4 *>(yo + row + y_ld) = o;
        } else {
            *reinterpret_cast<floatx4 *>(y + pix * y_ld + c0) = o;
        }
    }
}

__global__ __launch_bounds__(GN_THREADS) void mish_kernel(float *__restrict__ x, int ld, long long pixels, int Q) {
    const long long total = pixels * Q;
    for (long long i = (long long)blockIdx.x * GN_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * GN_THREADS) {
        const long long pix = i / Q;
        float *p = x + pix * ld + 4 * (int)(i - pix * Q);
        floatx4 v = *reinterpret_cast<floatx4 *>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = mish_f32(v[j]);
        *reinterpret_cast<floatx4 *>(p) = v;
    }
}

int stream_grid(long long total) {          // 256 CUs x 8 workgroups of four waves at the most: the loop strides over the rest
    const long long b = (total + GN_THREADS - 1) / GN_THREADS;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

bool view_ok(const void *p, int ld, int C) { return p && C > 0 && C % 4 == 0 && ld >= C && ld % 4 == 0 && ((uintptr_t)p & 15) == 0; }

// The three launches. mean [N * G] doubles and rstd [N * G] floats: inside the workspace (inference) or the caller's own (training).
int gn_forward(const float *x, int x_ld, const float *gamma, const float *beta, int groups, float eps, int act, const float *residual,
               int res_ld, float *y, int y_ld, int upsample2x, int N, int H, int W, int C, void *ws, size_t ws_bytes, double *mean_out,
               float *rstd_out, bool own_stats, void *stream) {
    ppy_drop_stale_error();
    PPY_CHECK_ARG(N > 0 && H > 0 && W > 0 && view_ok(x, x_ld, C) && view_ok(y, y_ld, C));
    PPY_CHECK_ARG(gamma && beta && ((uintptr_t)gamma & 15) == 0 && ((uintptr_t)beta & 15) == 0);
    PPY_CHECK_ARG(residual == nullptr || view_ok(residual, res_ld, C));
    PPY_CHECK_ARG(groups > 0 && C % groups == 0 && eps >= 0.f);
    PPY_CHECK_ARG(act == PPY_ACT_NONE || act == PPY_ACT_RELU || act == PPY_ACT_LEAKY || act == PPY_ACT_MISH);
    PPY_CHECK_ARG((long long)N * groups < (1LL << 24) && (long long)H * W < (1LL << 30) && N < 65536);
    PPY_CHECK_ARG(!own_stats || (mean_out && rstd_out && ((uintptr_t)mean_out & 7) == 0 && ((uintptr_t)rstd_out & 3) == 0));
    if (C > 2048) return PPY_ERR_UNSUPPORTED;
    if (!ws || ((uintptr_t)ws & 7) || ws_bytes < PPY_GN_WS_BYTES(N, groups)) return PPY_ERR_WORKSPACE;
    const int P = H * W, Q = C / 4;
    int rows_per = (P + PPY_GN_MAX_CHUNKS - 1) / PPY_GN_MAX_CHUNKS;
    if (rows_per < GN_MIN_CHUNK) rows_per = GN_MIN_CHUNK;
    const int nchunks = (P + rows_per - 1) / rows_per;          // <= PPY_GN_MAX_CHUNKS, none empty
    int tx_log2 = 0;
    while ((1 << tx_log2) < Q && tx_log2 < 6) ++tx_log2;
    const long long NG = (long long)N * groups;
    double *part = static_cast<double *>(ws);                   // [N][nchunks][G][2]
    double *mean = own_stats ? mean_out : part + NG * PPY_GN_MAX_CHUNKS * 2;           // [N][G]
    float *rstd = own_stats ? rstd_out : reinterpret_cast<float *>(mean + NG);         // [N][G]
    const size_t lds = (size_t)(GN_THREADS * 8 + 2 * C) * sizeof(double);      // <= 48 KB
    hipStream_t st = (hipStream_t)stream;
    const int TX = 1 << tx_log2, slabs = (4 * TX) % (C / groups) == 0 ? (Q + TX - 1) / TX : 1;      // <= 8 (C <= 2048)
    hipLaunchKernelGGL(gn_partial_kernel, dim3(nchunks, N, slabs), dim3(GN_THREADS), lds, st, x, x_ld, P, C, groups, rows_per, tx_log2, part);
    hipLaunchKernelGGL(gn_finalize_kernel, dim3((unsigned)((NG + 63) / 64)), dim3(64), 0, st, part, x, x_ld, P, C / groups, (int)NG, groups,
                       nchunks, (double)P * (C / groups), eps, mean, rstd);
    const int grid = stream_grid((long long)N * P * Q);
    if (upsample2x)
        hipLaunchKernelGGL(gn_apply_kernel<true>, dim3(grid), dim3(GN_THREADS), 0, st, x, x_ld, gamma, beta, mean, rstd, residual, res_ld, y,
                           y_ld, N, H, W, C, groups, act);
    else
        hipLaunchKernelGGL(gn_apply_kernel<false>, dim3(grid), dim3(GN_THREADS), 0, st, x, x_ld, gamma, beta, mean, rstd, residual, res_ld, y,
                           y_ld, N, H, W, C, groups, act);
    return ppy_launch_status();
}

}  // namespace

extern "C" int ppy_group_norm_f32(const float *x, int x_ld, const float *gamma, const float *beta, int groups, float eps, int act,
                                  const float *residual, int res_ld, float *y, int y_ld, int upsample2x, int N, int H, int W, int C,
                                  void *ws, size_t ws_bytes, void *stream) {
    return gn_forward(x, x_ld, gamma, beta, groups, eps, act, residual, res_ld, y, y_ld, upsample2x, N, H, W, C, ws, ws_bytes, nullptr,
                      nullptr, false, stream);
}

// The training forward: the same three launches, the statistics left in the caller's mean / rstd for ppy_group_norm_bwd_f32.
extern "C" int ppy_group_norm_train_f32(const float *x, int x_ld, const float *gamma, const float *beta, int groups, float eps, int act,
                                        const float *residual, int res_ld, float *y, int y_ld, int N, int H, int W, int C, double *mean,
                                        float *rstd, void *ws, size_t ws_bytes, void *stream) {
    return gn_forward(x, x_ld, gamma, beta, groups, eps, act, residual, res_ld, y, y_ld, 0, N, H, W, C, ws, ws_bytes, mean, rstd, true,
                      stream);
}

extern "C" int ppy_mish_f32(float *x, int x_ld, int N, int H, int W, int C, void *stream) {
    ppy_drop_stale_error();
    PPY_CHECK_ARG(N > 0 && H > 0 && W > 0 && view_ok(x, x_ld, C));
    const long long pixels = (long long)N * H * W;
    hipLaunchKernelGGL(mish_kernel, dim3(stream_grid(pixels * (C / 4))), dim3(GN_THREADS), 0, (hipStream_t)stream, x, x_ld, pixels, C / 4);
    return ppy_launch_status();
}
