// Backward of GroupNorm, AffineChannel and Mish of Conv2dUnit for the training step (reference model/custom_layers.py:37-62,
// :118-135, :142-253).  Contract: include/ppyolo_hip.h (ppy_group_norm_bwd_f32, ppy_affine_act_f32, ppy_affine_bwd_f32,
// ppy_mish_bwd_f32), DESIGN.md section 9b.  The training FORWARD of GroupNorm is ppy_group_norm_train_f32 in norm_act.hip.
//
// The rules of norm_act.hip hold: NHWC views, every access 16 bytes along C, sums in double combined in a fixed order, no
// floating-point atomics, no host synchronisation, workspace from the caller.  GroupNorm backward is three launches with the
// forward's geometry -- (1) a workgroup owns a chunk of pixels of one image (and, on wide maps, a slab of channels) and leaves
// per channel sum dz and sum dz * xhat, and per group those sums weighted by gamma; (2) one wave per (image, group) and one per
// channel add the chunks in a fixed order; (3) dx.  dz = dy * act'(z) is recomputed from the raw x in both passes with the
// forward's own expression for z (Mish cannot be inverted from y), so relu / leaky slopes follow the signs the forward saw.
#include "common.h"
#include "norm_act.h"

namespace {

constexpr int NT = 256;
constexpr int MIN_CHUNK = 32;      // pixels: below it a chunk is not worth a workgroup
constexpr int AF_MAX_CHUNKS = 512;

// Fixed tree over the pixel lanes of red[NT][8]; on return the lanes with ty == 0 hold the sums of their channel quad.
__device__ __forceinline__ void reduce_pixels(double *red, const double *s, const double *ss, int t, int ty, int TX, int TY) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        red[t * 8 + j] = s[j];
        red[t * 8 + 4 + j] = ss[j];
    }
    __syncthreads();
    for (int st = TY >> 1; st > 0; st >>= 1) {
        if (ty < st) {
#pragma unroll
            for (int e = 0; e < 8; ++e) red[t * 8 + e] += red[(t + st * TX) * 8 + e];
        }
        __syncthreads();
    }
}

// grid (nchunks, N, slabs): the geometry of gn_partial_kernel.  LDS: red[NT][8] doubles, then chan[C][2] doubles.
// pc[((n * nchunks + chunk) * C + c) * 2 + {0: sum dz, 1: sum dz * xhat}]; pg[((n * nchunks + chunk) * G + g) * 2 + {0: A, 1: B}].
__global__ __launch_bounds__(NT) void gn_bwd_partial_kernel(const float *__restrict__ x, int x_ld, const float *__restrict__ dy, int dy_ld,
                                                            const float *__restrict__ res, int res_ld, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, const double *__restrict__ mean,
                                                            const float *__restrict__ rstd, int P, int C, int G, int rows_per, int tx_log2,
                                                            int act, double *__restrict__ pc, double *__restrict__ pg) {
    extern __shared__ double gnb_lds[];
    double *red = gnb_lds, *chan = gnb_lds + NT * 8;
    const int n = blockIdx.y, chunk = blockIdx.x, nchunks = gridDim.x;
    const int t = threadIdx.x, TX = 1 << tx_log2, tx = t & (TX - 1), ty = t >> tx_log2, TY = NT >> tx_log2;
    const int p0 = chunk * rows_per, p1 = min(P, p0 + rows_per), Q = C >> 2, cpg = C / G;
    const long long base = (long long)n * P;
    const bool slab = gridDim.z > 1;
    const int q_begin = slab ? (int)blockIdx.z * TX : 0, q_end = slab ? min(Q, q_begin + TX) : Q;
    for (int q0 = q_begin; q0 < q_end; q0 += TX) {          // (uniform trip count: every thread reaches the barriers)
        const int q = q0 + tx, c0 = 4 * q;
        double s[4] = {0., 0., 0., 0.}, ss[4] = {0., 0., 0., 0.};
        if (q < Q) {
            const floatx4 ga = *reinterpret_cast<const floatx4 *>(gamma + c0), be = *reinterpret_cast<const floatx4 *>(beta + c0);
            double mu[4];
            float rs[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int si = n * G + (c0 + j) / cpg;
                mu[j] = mean[si];
                rs[j] = rstd[si];
            }
            for (int p = p0 + ty; p < p1; p += TY) {
                const floatx4 v = *reinterpret_cast<const floatx4 *>(x + (base + p) * x_ld + c0);
                const floatx4 g = *reinterpret_cast<const floatx4 *>(dy + (base + p) * dy_ld + c0);
                floatx4 r = {0.f, 0.f, 0.f, 0.f};
                if (res) r = *reinterpret_cast<const floatx4 *>(res + (base + p) * res_ld + c0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float d = (float)((double)v[j] - mu[j]);
                    const float xh = d * rs[j];
                    float u = xh * ga[j] + be[j];
                    if (res) u += r[j];
                    const float dz = g[j] * norm_act_grad(u, act);
                    s[j] += (double)dz;
                    ss[j] += (double)dz * (double)xh;
                }
            }
        }
        reduce_pixels(red, s, ss, t, ty, TX, TY);
        if (ty == 0 && q < Q) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                chan[(c0 + j) * 2] = red[t * 8 + j];
                chan[(c0 + j) * 2 + 1] = red[t * 8 + 4 + j];
            }
        }
        __syncthreads();
    }
    const long long blk = (long long)n * nchunks + chunk;
    const int c_begin = 4 * q_begin, c_end = 4 * q_end;
    for (int c = c_begin + t; c < c_end; c += NT) {
        pc[(blk * C + c) * 2] = chan[2 * c];
        pc[(blk * C + c) * 2 + 1] = chan[2 * c + 1];
    }
    const int g_begin = c_begin / cpg, g_end = slab ? min(G, c_end / cpg) : G;
    for (int g = g_begin + t; g < g_end; g += NT) {
        double a = 0., b = 0.;
        for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
            const double w = (double)gamma[c];
            a += w * chan[2 * c];
            b += w * chan[2 * c + 1];
        }
        pg[(blk * G + g) * 2] = a;
        pg[(blk * G + g) * 2 + 1] = b;
    }
}

// Sum of a lane's value over the 64 lanes of a wave by a fixed butterfly: every lane ends with the same double, in the same order
// of additions whatever the machine does.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One wave per item.  Items [0, N * G): A / m and B / m of an (image, group) -> ab[i * 2]; items [N * G, N * G + C), when the
// parameters train: dbeta / dgamma of a channel over images and chunks.  Lane l adds entries l, l + 64, ... in that order, then the
// butterfly: a fixed order (a single thread per item walked 1008 entries on a 76 x 76 map of 8 images: most of the backward's time).
__global__ __launch_bounds__(64) void gn_bwd_combine_kernel(const double *__restrict__ pc, const double *__restrict__ pg, int N, int G, int C,
                                                            int nchunks, double count, double *__restrict__ ab, float *__restrict__ dgamma,
                                                            float *__restrict__ dbeta) {
    const int i = blockIdx.x, NG = N * G, lane = threadIdx.x;
    double a = 0., b = 0.;
    if (i < NG) {
        const int n = i / G, g = i - n * G;
        for (int k = lane; k < nchunks; k += 64) {
            const double *p = pg + (((long long)n * nchunks + k) * G + g) * 2;
            a += p[0];
            b += p[1];
        }
        a = wave_sum(a);
        b = wave_sum(b);
        if (lane == 0) {
            ab[2 * i] = a / count;
            ab[2 * i + 1] = b / count;
        }
    } else {
        const int c = i - NG;          // (the grid holds these items only when dgamma / dbeta are wanted)
        const long long total = (long long)N * nchunks;
        for (long long k = lane; k < total; k += 64) {
            a += pc[(k * C + c) * 2];
            b += pc[(k * C + c) * 2 + 1];
        }
        a = wave_sum(a);
        b = wave_sum(b);
        if (lane == 0) {
            dbeta[c] = (float)a;
            dgamma[c] = (float)b;
        }
    }
}

// Grid-stride over (pixel, channel quad): dx = rstd * (gamma * dz - A / m - xhat * B / m), the bracket in double (with m = 1 it is
// exactly 0); dz_out (or NULL): dz for the shortcut branch.
__global__ __launch_bounds__(NT) void gn_bwd_apply_kernel(const float *__restrict__ x, int x_ld, const float *__restrict__ dy, int dy_ld,
                                                          const float *__restrict__ res, int res_ld, const float *__restrict__ gamma,
                                                          const float *__restrict__ beta, const double *__restrict__ mean,
                                                          const float *__restrict__ rstd, const double *__restrict__ ab,
                                                          float *__restrict__ dx, int dx_ld, float *__restrict__ dz_out, int dz_ld,
                                                          int N, long long P, int C, int G, int act) {
    const int Q = C >> 2, cpg = C / G;
    const long long total = (long long)N * P * Q;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const long long pix = i / Q;
        const int q = (int)(i - pix * Q), c0 = 4 * q;
        const int n = (int)(pix / P);
        const floatx4 v = *reinterpret_cast<const floatx4 *>(x + pix * x_ld + c0);
        const floatx4 g = *reinterpret_cast<const floatx4 *>(dy + pix * dy_ld + c0);
        const floatx4 ga = *reinterpret_cast<const floatx4 *>(gamma + c0), be = *reinterpret_cast<const floatx4 *>(beta + c0);
        floatx4 r = {0.f, 0.f, 0.f, 0.f};
        if (res) r = *reinterpret_cast<const floatx4 *>(res + pix * res_ld + c0);
        floatx4 o, z;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int si = n * G + (c0 + j) / cpg;
            const float rs = rstd[si];
            const float d = (float)((double)v[j] - mean[si]);
            const float xh = d * rs;
            float u = xh * ga[j] + be[j];
            if (res) u += r[j];
            const float dz = g[j] * norm_act_grad(u, act);
            z[j] = dz;
            o[j] = (float)((double)rs * ((double)ga[j] * (double)dz - ab[2 * si] - (double)xh * ab[2 * si + 1]));
        }
        *reinterpret_cast<floatx4 *>(dx + pix * dx_ld + c0) = o;
        if (dz_out) *reinterpret_cast<floatx4 *>(dz_out + pix * dz_ld + c0) = z;
    }
}

// y = act(x * w + b [+ res]): the training forward of a trainable AffineChannel unit (its backward recomputes z with this expression).
__global__ __launch_bounds__(NT) void affine_act_kernel(const float *__restrict__ x, int x_ld, const float *__restrict__ w,
                                                        const float *__restrict__ b, const float *__restrict__ res, int res_ld,
                                                        float *__restrict__ y, int y_ld, long long pixels, int Q, int act) {
    const long long total = pixels * Q;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const long long pix = i / Q;
        const int c0 = 4 * (int)(i - pix * Q);
        const floatx4 v = *reinterpret_cast<const floatx4 *>(x + pix * x_ld + c0);
        const floatx4 sc = *reinterpret_cast<const floatx4 *>(w + c0), sh = *reinterpret_cast<const floatx4 *>(b + c0);
        floatx4 r = {0.f, 0.f, 0.f, 0.f};
        if (res) r = *reinterpret_cast<const floatx4 *>(res + pix * res_ld + c0);
        floatx4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float u = v[j] * sc[j] + sh[j];
            if (res) u += r[j];
            o[j] = norm_act(u, act);
        }
        *reinterpret_cast<floatx4 *>(y + pix * y_ld + c0) = o;
    }
}

// grid (nchunks, slabs) over the N * H * W pixels: a workgroup owns rows_per pixels x 4 * TX channels, writes dx = dz * w (and dz for
// the shortcut) and, when the parameters train, leaves pc[(chunk * C + c) * 2 + {0: sum dz, 1: sum dz * x}].  LDS: red[NT][8] doubles.
__global__ __launch_bounds__(NT) void affine_bwd_kernel(const float *__restrict__ x, int x_ld, const float *__restrict__ dy, int dy_ld,
                                                        const float *__restrict__ res, int res_ld, const float *__restrict__ w,
                                                        const float *__restrict__ b, float *__restrict__ dx, int dx_ld,
                                                        float *__restrict__ dz_out, int dz_ld, long long pixels, int C, int rows_per,
                                                        int tx_log2, int act, double *__restrict__ pc) {
    __shared__ double red[NT * 8];
    const int chunk = blockIdx.x, t = threadIdx.x, TX = 1 << tx_log2, tx = t & (TX - 1), ty = t >> tx_log2, TY = NT >> tx_log2;
    const int Q = C >> 2, q = (int)blockIdx.y * TX + tx, c0 = 4 * q;
    const long long p0 = (long long)chunk * rows_per, p1 = min(pixels, p0 + rows_per);
    double s[4] = {0., 0., 0., 0.}, ss[4] = {0., 0., 0., 0.};
    if (q < Q) {
        const floatx4 sc = *reinterpret_cast<const floatx4 *>(w + c0), sh = *reinterpret_cast<const floatx4 *>(b + c0);
        for (long long p = p0 + ty; p < p1; p += TY) {
            const floatx4 v = *reinterpret_cast<const floatx4 *>(x + p * x_ld + c0);
            const floatx4 g = *reinterpret_cast<const floatx4 *>(dy + p * dy_ld + c0);
            floatx4 r = {0.f, 0.f, 0.f, 0.f};
            if (res) r = *reinterpret_cast<const floatx4 *>(res + p * res_ld + c0);
            floatx4 o, z;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float u = v[j] * sc[j] + sh[j];
                if (res) u += r[j];
                const float dz = g[j] * norm_act_grad(u, act);
                z[j] = dz;
                o[j] = dz * sc[j];
                s[j] += (double)dz;
                ss[j] += (double)dz * (double)v[j];
            }
            *reinterpret_cast<floatx4 *>(dx + p * dx_ld + c0) = o;
            if (dz_out) *reinterpret_cast<floatx4 *>(dz_out + p * dz_ld + c0) = z;
        }
    }
    if (pc == nullptr) return;          // (uniform: frozen parameters)
    reduce_pixels(red, s, ss, t, ty, TX, TY);
    if (ty == 0 && q < Q) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pc[((long long)chunk * C + c0 + j) * 2] = red[t * 8 + j];
            pc[((long long)chunk * C + c0 + j) * 2 + 1] = red[t * 8 + 4 + j];
        }
    }
}

// One wave per channel: lane l adds chunks l, l + 64, ... in that order, then the fixed butterfly.
__global__ __launch_bounds__(64) void affine_bwd_combine_kernel(const double *__restrict__ pc, int C, int nchunks, float *__restrict__ dw,
                                                                float *__restrict__ db) {
    const int c = blockIdx.x, lane = threadIdx.x;
    double a = 0., b = 0.;
    for (int k = lane; k < nchunks; k += 64) {
        a += pc[((long long)k * C + c) * 2];
        b += pc[((long long)k * C + c) * 2 + 1];
    }
    a = wave_sum(a);
    b = wave_sum(b);
    if (lane == 0) {
        db[c] = (float)a;
        dw[c] = (float)b;
    }
}

// dx = dy * mish'(x * scale + shift): behind a bn + mish / af + mish unit, the pre-activation recomputed from the raw convolution output.
__global__ __launch_bounds__(NT) void mish_bwd_kernel(const float *__restrict__ x, int x_ld, const float *__restrict__ scale,
                                                      const float *__restrict__ shift, const float *__restrict__ dy, int dy_ld,
                                                      float *__restrict__ dx, int dx_ld, long long pixels, int Q) {
    const long long total = pixels * Q;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const long long pix = i / Q;
        const int c0 = 4 * (int)(i - pix * Q);
        const floatx4 v = *reinterpret_cast<const floatx4 *>(x + pix * x_ld + c0);
        const floatx4 g = *reinterpret_cast<const floatx4 *>(dy + pix * dy_ld + c0);
        floatx4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
        if (scale) sc = *reinterpret_cast<const floatx4 *>(scale + c0);
        if (shift) sh = *reinterpret_cast<const floatx4 *>(shift + c0);
        floatx4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = g[j] * mish_grad_f32(v[j] * sc[j] + sh[j]);
        *reinterpret_cast<floatx4 *>(dx + pix * dx_ld + c0) = o;
    }
}

int stream_grid(long long total) {          // 256 CUs x 8 workgroups of four waves at the most: the loop strides over the rest
    const long long b = (total + NT - 1) / NT;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

bool view_ok(const void *p, int ld, int C) { return p && C > 0 && C % 4 == 0 && ld >= C && ld % 4 == 0 && ((uintptr_t)p & 15) == 0; }
bool vec_ok(const void *p) { return p && ((uintptr_t)p & 15) == 0; }
bool act_ok(int act) { return act == PPY_ACT_NONE || act == PPY_ACT_RELU || act == PPY_ACT_LEAKY || act == PPY_ACT_MISH; }

// The forward's chunking of the H * W pixels of an image (gn_forward in norm_act.hip).
void gn_chunks(int P, int *rows_per, int *nchunks) {
    int r = (P + PPY_GN_MAX_CHUNKS - 1) / PPY_GN_MAX_CHUNKS;
    if (r < MIN_CHUNK) r = MIN_CHUNK;
    *rows_per = r;
    *nchunks = (P + r - 1) / r;
}

void af_chunks(long long pixels, int *rows_per, int *nchunks) {
    long long r = (pixels + AF_MAX_CHUNKS - 1) / AF_MAX_CHUNKS;
    if (r < MIN_CHUNK) r = MIN_CHUNK;
    *rows_per = (int)r;
    *nchunks = (int)((pixels + r - 1) / r);
}

}  // namespace

extern "C" size_t ppy_group_norm_bwd_workspace_bytes(int N, int H, int W, int C, int groups) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || groups <= 0 || (long long)H * W >= (1LL << 30)) return 0;
    int rows_per, nchunks;
    gn_chunks(H * W, &rows_per, &nchunks);
    return ((size_t)N * nchunks * ((size_t)C + groups) * 2 + (size_t)N * groups * 2) * sizeof(double);
}

extern "C" int ppy_group_norm_bwd_f32(const float *x, int x_ld, const double *mean, const float *rstd, const float *gamma,
                                      const float *beta, int groups, int act, const float *residual, int res_ld, const float *dy,
                                      int dy_ld, float *dx, int dx_ld, float *dz, int dz_ld, float *dgamma, float *dbeta,
                                      int param_grads, int N, int H, int W, int C, void *ws, size_t ws_bytes, void *stream) {
    ppy_drop_stale_error();
    PPY_CHECK_ARG(N > 0 && H > 0 && W > 0 && view_ok(x, x_ld, C) && view_ok(dy, dy_ld, C) && view_ok(dx, dx_ld, C));
    PPY_CHECK_ARG(vec_ok(gamma) && vec_ok(beta) && mean && rstd && ((uintptr_t)mean & 7) == 0 && ((uintptr_t)rstd & 3) == 0);
    PPY_CHECK_ARG(residual == nullptr || view_ok(residual, res_ld, C));
    PPY_CHECK_ARG(dz == nullptr || view_ok(dz, dz_ld, C));
    PPY_CHECK_ARG(groups > 0 && C % groups == 0 && act_ok(act));
    PPY_CHECK_ARG(!param_grads || (dgamma && dbeta));
    PPY_CHECK_ARG((long long)N * groups < (1LL << 24) && (long long)H * W < (1LL << 30) && N < 65536);
    if (C > 2048) return PPY_ERR_UNSUPPORTED;
    if (!ws || ((uintptr_t)ws & 7) || ws_bytes < ppy_group_norm_bwd_workspace_bytes(N, H, W, C, groups)) return PPY_ERR_WORKSPACE;
    const int P = H * W, Q = C / 4;
    int rows_per, nchunks;
    gn_chunks(P, &rows_per, &nchunks);
    int tx_log2 = 0;
    while ((1 << tx_log2) < Q && tx_log2 < 6) ++tx_log2;
    const int TX = 1 << tx_log2, slabs = (4 * TX) % (C / groups) == 0 ? (Q + TX - 1) / TX : 1;      // <= 8 (C <= 2048)
    double *pc = static_cast<double *>(ws);                               // [N][nchunks][C][2]
    double *pg = pc + (size_t)N * nchunks * C * 2;                        // [N][nchunks][G][2]
    double *ab = pg + (size_t)N * nchunks * groups * 2;                   // [N][G][2]
    const size_t lds = (size_t)(NT * 8 + 2 * C) * sizeof(double);         // <= 48 KB
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gn_bwd_partial_kernel, dim3(nchunks, N, slabs), dim3(NT), lds, st, x, x_ld, dy, dy_ld, residual, res_ld, gamma, beta,
                       mean, rstd, P, C, groups, rows_per, tx_log2, act, pc, pg);
    const int items = N * groups + (param_grads ? C : 0);
    hipLaunchKernelGGL(gn_bwd_combine_kernel, dim3(items), dim3(64), 0, st, pc, pg, N, groups, C, nchunks,
                       (double)P * (C / groups), ab, param_grads ? dgamma : nullptr, param_grads ? dbeta : nullptr);
    hipLaunchKernelGGL(gn_bwd_apply_kernel, dim3(stream_grid((long long)N * P * Q)), dim3(NT), 0, st, x, x_ld, dy, dy_ld, residual, res_ld,
                       gamma, beta, mean, rstd, ab, dx, dx_ld, dz, dz_ld, N, (long long)P, C, groups, act);
    return ppy_launch_status();
}

extern "C" int ppy_affine_act_f32(const float *x, int x_ld, const float *weight, const float *bias, int act, const float *residual,
                                  int res_ld, float *y, int y_ld, int N, int H, int W, int C, void *stream) {
    ppy_drop_stale_error();
    PPY_CHECK_ARG(N > 0 && H > 0 && W > 0 && view_ok(x, x_ld, C) && view_ok(y, y_ld, C) && vec_ok(weight) && vec_ok(bias) && act_ok(act));
    PPY_CHECK_ARG(residual == nullptr || view_ok(residual, res_ld, C));
    const long long pixels = (long long)N * H * W;
    hipLaunchKernelGGL(affine_act_kernel, dim3(stream_grid(pixels * (C / 4))), dim3(NT), 0, (hipStream_t)stream, x, x_ld, weight, bias,
                       residual, res_ld, y, y_ld, pixels, C / 4, act);
    return ppy_launch_status();
}

extern "C" size_t ppy_affine_bwd_workspace_bytes(int N, int H, int W, int C) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
    int rows_per, nchunks;
    af_chunks((long long)N * H * W, &rows_per, &nchunks);
    return (size_t)nchunks * C * 2 * sizeof(double);
}

extern "C" int ppy_affine_bwd_f32(const float *x, int x_ld, const float *weight, const float *bias, int act, const float *residual,
                                  int res_ld, const float *dy, int dy_ld, float *dx, int dx_ld, float *dz, int dz_ld, float *dweight,
                                  float *dbias, int param_grads, int N, int H, int W, int C, void *ws, size_t ws_bytes, void *stream) {
    ppy_drop_stale_error();
    PPY_CHECK_ARG(N > 0 && H > 0 && W > 0 && view_ok(x, x_ld, C) && view_ok(dy, dy_ld, C) && view_ok(dx, dx_ld, C));
    PPY_CHECK_ARG(vec_ok(weight) && vec_ok(bias) && act_ok(act));
    PPY_CHECK_ARG(residual == nullptr || view_ok(residual, res_ld, C));
    PPY_CHECK_ARG(dz == nullptr || view_ok(dz, dz_ld, C));
    PPY_CHECK_ARG(!param_grads || (dweight && dbias));
    PPY_CHECK_ARG((long long)N * H * W < (1LL << 40));
    if (param_grads && (!ws || ((uintptr_t)ws & 7) || ws_bytes < ppy_affine_bwd_workspace_bytes(N, H, W, C))) return PPY_ERR_WORKSPACE;
    const long long pixels = (long long)N * H * W;
    const int Q = C / 4;
    int rows_per, nchunks;
    af_chunks(pixels, &rows_per, &nchunks);
    int tx_log2 = 0;
    while ((1 << tx_log2) < Q && tx_log2 < 6) ++tx_log2;
    const int TX = 1 << tx_log2;
    hipStream_t st = (hipStream_t)stream;
    double *pc = param_grads ? static_cast<double *>(ws) : nullptr;
    hipLaunchKernelGGL(affine_bwd_kernel, dim3(nchunks, (Q + TX - 1) / TX), dim3(NT), 0, st, x, x_ld, dy, dy_ld, residual, res_ld, weight,
                       bias, dx, dx_ld, dz, dz_ld, pixels, C, rows_per, tx_log2, act, pc);
    if (param_grads)
        hipLaunchKernelGGL(affine_bwd_combine_kernel, dim3(C), dim3(64), 0, st, pc, C, nchunks, dweight, dbias);
    return ppy_launch_status();
}

extern "C" int ppy_mish_bwd_f32(const float *x, int x_ld, const float *scale, const float *shift, const float *dy, int dy_ld, float *dx,
                                int dx_ld, int N, int H, int W, int C, void *stream) {
    ppy_drop_stale_error();
    PPY_CHECK_ARG(N > 0 && H > 0 && W > 0 && view_ok(x, x_ld, C) && view_ok(dy, dy_ld, C) && view_ok(dx, dx_ld, C));
    PPY_CHECK_ARG((scale == nullptr || vec_ok(scale)) && (shift == nullptr || vec_ok(shift)));
    const long long pixels = (long long)N * H * W;
    hipLaunchKernelGGL(mish_bwd_kernel, dim3(stream_grid(pixels * (C / 4))), dim3(NT), 0, (hipStream_t)stream, x, x_ld, scale, shift, dy,
                       dy_ld, dx, dx_ld, pixels, C / 4);
    return ppy_launch_status();
}
