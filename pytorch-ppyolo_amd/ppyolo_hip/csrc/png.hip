// PNG reconstruction on the device: inflated scanline streams -> uint8 HWC BGR images, the pixels cv2.imread(path) gives for a
// PNG file (pinned to Pillow / libpng: DESIGN.md section 10e).  The host has walked the chunks and inflated IDAT
// (ppyolo_hip/png.py, or a C caller's own zlib); what is left is per byte: reverse the five scanline filters, then expand
// (bit unpacking, palette lookup, grey replication, alpha drop, high byte of a 16-bit sample) and, for Adam7, scatter.
//
// Schedule.  A reconstructed byte needs its left neighbour (one UNIT = max(1, channels * depth / 8) bytes back), the byte
// above and the byte above-left; Avg and Paeth are not associative, so a row cannot be scanned in parallel -- but rows can
// be skewed.  One workgroup per (image, Adam7 pass); thread r owns row r of the band in flight (blockDim.x rows, at most
// 1024) and at step s works on unit x = s - r:
//     b      the output of thread r - 1 at step s - 1: one cross-lane move; between waves the last lane's outputs pass
//            through a two-slot LDS ring, and every step ends in the workgroup barrier that orders the ring;
//     c      last step's b;      a      the thread's own last output.
// Steps come in tiles of PNG_TILE.  A wave stages the filtered bytes of its 64 rows for a tile through LDS with coalesced
// dword loads (the next tile's loads are in flight in registers while this tile is worked on), reconstructs IN PLACE in
// LDS, and after the tile's last step stores the tile expanded to BGR with 16 consecutive lanes on consecutive units of a
// row.  Images taller than the band are walked band by band; the last row of a band goes to the workspace (raw
// reconstructed bytes) and comes back as the row above thread 0 through the same LDS staging.
// All arithmetic is integer: Avg is (a + b) >> 1 on 9 bits, Paeth keeps `pa <= pb && pa <= pc`, then `pb <= pc`.
// No atomics: every output byte has one writer.
#include <string.h>

#include "common.h"

namespace {

constexpr int PNG_TILE = 16;            // steps per LDS tile
constexpr int PNG_MAX_THREADS = 1024;   // rows in flight
constexpr int PNG_RING_BYTES = (PNG_MAX_THREADS / 64) * 2 * 8;

struct PngDev {                         // device descriptor, one per image
    unsigned char *out;                 // pixel (y, x) channel c at y * row_stride + 3 * x + c
    long long row_stride;
    long long scan_off;                 // the image's stream, bytes from the start of the scan buffer (% 16 == 0)
    long long ws_off;                   // its band hand-over rows, bytes from the start of the workspace
    int W, H, depth, ctype, interlace, unit, ws_row, pad_;
    unsigned char pal[256][4];          // B, G, R, 0
};

__host__ __device__ inline int png_channels(int ctype) { return ctype == 2 ? 3 : ctype == 4 ? 2 : ctype == 6 ? 4 : 1; }
__host__ __device__ inline int png_unit(int ctype, int depth) {
    const int bits = png_channels(ctype) * depth;
    return bits < 8 ? 1 : bits / 8;
}
__host__ __device__ inline long long png_row_bytes(int cols, int ctype, int depth) {
    return ((long long)cols * png_channels(ctype) * depth + 7) / 8;
}
// Adam7: pass p covers pixels (ys + yd * r, xs + xd * x)
__host__ __device__ inline void png_pass_geometry(int interlace, int p, int W, int H, int *xs, int *ys, int *xd, int *yd, int *cols,
                                                  int *rows) {
    if (!interlace) {
        *xs = *ys = 0;
        *xd = *yd = 1;
        *cols = p == 0 ? W : 0;
        *rows = p == 0 ? H : 0;
        return;
    }
    // packed tables: pass 0..6, four bits each
    const int XS = 0x0102040, YS = 0x1020400, XD = 0x1224488, YD = 0x2244888;
    *xs = (XS >> (4 * p)) & 15;
    *ys = (YS >> (4 * p)) & 15;
    *xd = (XD >> (4 * p)) & 15;
    *yd = (YD >> (4 * p)) & 15;
    *cols = W > *xs ? (W - *xs + *xd - 1) / *xd : 0;
    *rows = H > *ys ? (H - *ys + *yd - 1) / *yd : 0;
    if (*cols == 0 || *rows == 0) *cols = *rows = 0;
}

static bool png_format_ok(int ctype, int depth) {
    switch (ctype) {
        case 0: return depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16;
        case 3: return depth == 1 || depth == 2 || depth == 4 || depth == 8;
        case 2: case 4: case 6: return depth == 8 || depth == 16;
        default: return false;
    }
}
static long long png_expected_bytes(const ppy_png_desc_t &s) {
    long long total = 0;
    for (int p = 0; p < (s.interlace ? 7 : 1); ++p) {
        int xs, ys, xd, yd, cols, rows;
        png_pass_geometry(s.interlace, p, s.width, s.height, &xs, &ys, &xd, &yd, &cols, &rows);
        if (rows) total += (long long)rows * (1 + png_row_bytes(cols, s.colour_type, s.bit_depth));
    }
    return total;
}
static int png_ws_row(const ppy_png_desc_t &s) { return (int)((png_row_bytes(s.width, s.colour_type, s.bit_depth) + 15) / 16 * 16 + 16); }
static bool png_desc_ok(const ppy_png_desc_t &s) {
    return s.width >= 1 && s.width <= 65535 && s.height >= 1 && s.height <= 65535 && png_format_ok(s.colour_type, s.bit_depth) &&
           (s.interlace == 0 || s.interlace == 1) && s.palette_entries >= (s.colour_type == 3 ? 1 : 0) && s.palette_entries <= 256 &&
           s.scan_offset >= 0 && (s.scan_offset & 15) == 0 && s.scan_bytes == png_expected_bytes(s);
}

#ifndef PPY_PNG_HOST_ONLY
template <int U>
__device__ __forceinline__ unsigned long long png_lds_read_unit(const unsigned char *p) {
    unsigned long long v = 0;
#pragma unroll
    for (int k = 0; k < U; ++k) v |= (unsigned long long)p[k] << (8 * k);
    return v;
}
template <int U>
__device__ __forceinline__ void png_lds_write_unit(unsigned char *p, unsigned long long v) {
#pragma unroll
    for (int k = 0; k < U; ++k) p[k] = (unsigned char)(v >> (8 * k));
}

// one unit of one row: x (filtered), a (left), b (above), c (above-left), U bytes packed low byte first
template <int U>
__device__ __forceinline__ unsigned long long png_unfilter(int ft, unsigned long long x, unsigned long long a, unsigned long long b,
                                                           unsigned long long c) {
    unsigned long long out = 0;
#pragma unroll
    for (int k = 0; k < U; ++k) {
        const int xv = (int)(x >> (8 * k)) & 255, av = (int)(a >> (8 * k)) & 255, bv = (int)(b >> (8 * k)) & 255,
                  cv = (int)(c >> (8 * k)) & 255;
        const int pa = abs(bv - cv), pb = abs(av - cv), pc = abs(av + bv - 2 * cv);
        const int paeth = (pa <= pb && pa <= pc) ? av : (pb <= pc ? bv : cv);
        const int pred = ft == 1 ? av : ft == 2 ? bv : ft == 3 ? (av + bv) >> 1 : ft == 4 ? paeth : 0;
        out |= (unsigned long long)((xv + pred) & 255) << (8 * k);
    }
    return out;
}

template <int U>
__device__ __forceinline__ unsigned long long png_shfl_up1(unsigned long long v) {
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
    lo = __shfl_up(lo, 1);
    if (U > 4) hi = __shfl_up(hi, 1);
    return U > 4 ? ((unsigned long long)hi << 32 | lo) : (unsigned long long)lo;
}

// What the store needs of the descriptor, read ONCE into registers: the output stores are byte stores, which for all the
// compiler knows alias the table, so fields read through it would be loaded again after every store.
struct PngOut {
    unsigned char *out;
    long long row_stride;
    const unsigned char (*pal)[4];
    int depth, ctype;
};

// expand one reconstructed unit of pass-row `row` to BGR and store it
template <int U>
__device__ __forceinline__ void png_store_unit(const PngOut &d, unsigned long long v, int row, int x, int cols, int xs, int ys, int xd,
                                               int yd) {
    unsigned char *orow = d.out + (long long)(ys + yd * row) * d.row_stride;
    if (U == 1 && d.depth < 8) {      // several pixels in the byte, first pixel in the high bits
        const int depth = d.depth, ppb = 8 / depth, mask = (1 << depth) - 1;
        const int scale = d.ctype == 3 ? 1 : 255 / mask;      // 255 / 85 / 17
        for (int q = 0; q < ppb; ++q) {
            const int col = x * ppb + q;
            if (col >= cols) break;
            const int s = ((int)v >> (8 - depth * (q + 1))) & mask;
            unsigned char *o = orow + 3LL * (xs + xd * col);
            if (d.ctype == 3) {
                o[0] = d.pal[s][0];
                o[1] = d.pal[s][1];
                o[2] = d.pal[s][2];
            } else {
                o[0] = o[1] = o[2] = (unsigned char)(s * scale);
            }
        }
        return;
    }
    unsigned char *o = orow + 3LL * (xs + xd * x);
    const int v0 = (int)v & 255;      // first sample: its only byte, or the high byte of a 16-bit one
    if (d.ctype == 3) {
        o[0] = d.pal[v0][0];
        o[1] = d.pal[v0][1];
        o[2] = d.pal[v0][2];
    } else if (d.ctype == 0 || d.ctype == 4) {
        o[0] = o[1] = o[2] = (unsigned char)v0;
    } else {                          // RGB / RGBA, sample stride 1 or 2 bytes
        const int st = d.depth == 16 ? 16 : 8;
        o[0] = (unsigned char)(v >> (2 * st));
        o[1] = (unsigned char)(v >> st);
        o[2] = (unsigned char)v0;
    }
}

template <int U>
__device__ void png_pass(const PngOut d, const unsigned char *scan, long long poff, unsigned char *wsrow, int cols, int rows, int xs,
                         int ys, int xd, int yd, unsigned char *lds) {
    constexpr int T = PNG_TILE;
    constexpr int RB = T * U + 4;      // bytes of one row's LDS buffer: a tile + the dword alignment slack; RB / 4 is odd
    constexpr int D = RB / 4;
    constexpr int DP = U == 1 ? 4 : U == 2 ? 8 : U <= 4 ? 16 : 32;      // the power of two in [D - 1, D]
    constexpr int K = 64 / DP;
    constexpr bool TAIL = D > DP;
    static_assert(DP == D - 1 || DP >= D, "every dword of a row's segment has a lane");
    const int tid = threadIdx.x, lane = tid & 63, R = blockDim.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rb = (int)png_row_bytes(cols, d.ctype, d.depth);      // bytes of a row after its filter byte
    const int units = rb / U;
    const int pitch = rb + 1;
    unsigned char *ring = lds;                                       // [wave][2][8]
    unsigned char *uprow = lds + PNG_RING_BYTES;                     // the row above thread 0: RB bytes (136 reserved)
    unsigned char *rowbuf0 = uprow + 136 + wave * (64 * RB);         // this wave's 64 row buffers
    unsigned char *myrow = rowbuf0 + lane * RB;

    for (int band0 = 0; band0 < rows; band0 += R) {
        const int Rb = min(R, rows - band0);
        const int nsteps = units + Rb - 1;
        const bool rowvalid = tid < Rb;
        const bool has_up = band0 > 0;
        const bool hand_over = band0 + R < rows;      // thread R - 1's row is the row above the next band
        // byte 0 of the wave's first row, from `scan` (16-byte aligned): wave-uniform and 64-bit; what a lane adds fits 32 bits
        const long long wbase = poff + (long long)(band0 + wave * 64) * pitch + 1;
        const unsigned char *wscan = scan + wbase;
        const int wlow = (int)(wbase & 3);
        const unsigned char *wscan4 = wscan - wlow;      // the dword loads: an aligned base and an unsigned 32-bit offset
        int ft = 0;
        if (rowvalid) ft = wscan[lane * pitch - 1];
        const bool first_row = band0 + tid == 0;

        unsigned regs[DP + 1];
        unsigned upreg = 0;
        unsigned long long a = 0, bprev = 0, outp = 0;
        for (int s0 = -T; s0 < nsteps; s0 += T) {
            const bool more = s0 + T < nsteps;
            if (more) {
                // the loads of the tile that starts at step n0.  Iteration `it` covers rows it * K .. it * K + K - 1 of the wave,
                // DP lanes on the first DP dwords of each; the rows whose segment needs a dword more get it from their own lane.
                const int n0 = s0 + T;
                auto load = [&](int rr, int dw) -> unsigned {
                    const int r = wave * 64 + rr;
                    const int xlo = max(n0 - r, 0), xhi = min(n0 - r + T, units);
                    unsigned v = 0;
                    if (r < Rb && xlo < xhi) {
                        const int loff = rr * pitch + xlo * U, al = (wlow + loff) & 3;
                        const int count = (al + (xhi - xlo) * U + 3) >> 2;
                        if (dw < count) v = *reinterpret_cast<const unsigned *>(wscan4 + (unsigned)(wlow + loff - al + 4 * dw));
                    }
                    return v;
                };
#pragma unroll
                for (int it = 0; it < DP; ++it) regs[it] = load(it * K + lane / DP, lane % DP);
                if (TAIL) regs[DP] = load(lane, DP);
                if (has_up && wave == 0 && lane < D) {
                    const int xhi = min(n0 + T, units);
                    if (n0 < xhi) {
                        const int glo = n0 * U, count = ((glo & 3) + (xhi - n0) * U + 3) >> 2;
                        if (lane < count) upreg = *reinterpret_cast<const unsigned *>(wsrow + (glo & ~3) + 4 * lane);
                    }
                }
            }
            if (s0 >= 0) {
                // where this thread's units of the tile lie in its row buffer
                const int xlo = max(s0 - tid, 0);
                const int align = (wlow + lane * pitch + xlo * U) & 3;
                const int upalign = (s0 * U) & 3;
                const int send = min(s0 + T, nsteps);
                for (int s = s0; s < send; ++s) {
                    // wave-uniform: is any row of this wave inside the image at this step?
                    if (s >= wave * 64 && s - (wave * 64 + 63) < units && wave * 64 < Rb) {
                        const int x = s - tid;
                        const bool active = rowvalid && x >= 0 && x < units;
                        unsigned long long up = png_shfl_up1<U>(outp);
                        if (lane == 0) {
                            if (wave > 0) up = *reinterpret_cast<const unsigned long long *>(ring + (wave - 1) * 16 + ((s - 1) & 1) * 8);
                            else if (has_up && active) up = png_lds_read_unit<U>(uprow + upalign + (x - s0) * U);
                            else up = 0;
                        }
                        if (first_row) up = 0;
                        unsigned long long out = 0;
                        if (active) {
                            unsigned char *p = myrow + align + (x - xlo) * U;
                            const unsigned long long f = png_lds_read_unit<U>(p);
                            out = png_unfilter<U>(ft, f, x > 0 ? a : 0ull, up, x > 0 ? bprev : 0ull);
                            png_lds_write_unit<U>(p, out);
                            a = out;
                        }
                        bprev = up;
                        outp = out;
                    }
                    if (lane == 63) *reinterpret_cast<unsigned long long *>(ring + wave * 16 + (s & 1) * 8) = outp;
                    __syncthreads();
                }
                // the tile, expanded: element e = it * 64 + lane -> (row e / T of the wave, unit e % T of the row's tile)
#pragma unroll 2
                for (int it = 0; it < T; ++it) {
                    const int e = it * 64 + lane, rr = e / T, j = e % T, r = wave * 64 + rr;
                    const int x = s0 - r + j;
                    if (r < Rb && x >= 0 && x < units) {
                        const int rxlo = max(s0 - r, 0);
                        const int al = (wlow + rr * pitch + rxlo * U) & 3;
                        const unsigned long long v = png_lds_read_unit<U>(rowbuf0 + rr * RB + al + (x - rxlo) * U);
                        png_store_unit<U>(d, v, band0 + r, x, cols, xs, ys, xd, yd);
                        if (hand_over && r == R - 1) {
#pragma unroll
                            for (int k = 0; k < U; ++k) wsrow[x * U + k] = (unsigned char)(v >> (8 * k));
                        }
                    }
                }
            }
            if (more) {
#pragma unroll
                for (int it = 0; it < DP; ++it)
                    if (DP <= D || lane % DP < D)      // (a row buffer has D dwords)
                        *reinterpret_cast<unsigned *>(rowbuf0 + (it * K + lane / DP) * RB + 4 * (lane % DP)) = regs[it];
                if (TAIL) *reinterpret_cast<unsigned *>(myrow + 4 * DP) = regs[DP];
                if (has_up && wave == 0 && lane < D) *reinterpret_cast<unsigned *>(uprow + 4 * lane) = upreg;
            }
            __syncthreads();
        }
    }
}

// One instantiation per unit size, so that each gets its own register allocation; a launch takes the images of its unit size
// and the workgroups of the others leave at once.
template <int U>
__global__ __launch_bounds__(PNG_MAX_THREADS) void png_reconstruct_kernel(const PngDev *__restrict__ table,
                                                                           const unsigned char *__restrict__ scan_base,
                                                                           unsigned char *__restrict__ ws_base) {
    extern __shared__ __attribute__((aligned(16))) unsigned char png_lds[];
    const PngDev &d = table[blockIdx.y];
    const int pass = blockIdx.x;
    if (d.unit != U || (pass > 0 && !d.interlace)) return;
    int xs, ys, xd, yd, cols, rows;
    long long off = 0;      // of this pass in the image's stream: the non-empty passes before it
    for (int p = 0; p < pass; ++p) {
        png_pass_geometry(d.interlace, p, d.W, d.H, &xs, &ys, &xd, &yd, &cols, &rows);
        if (rows) off += (long long)rows * (1 + png_row_bytes(cols, d.ctype, d.depth));
    }
    png_pass_geometry(d.interlace, pass, d.W, d.H, &xs, &ys, &xd, &yd, &cols, &rows);
    if (rows == 0) return;
    const unsigned char *scan = scan_base + d.scan_off;      // 16-byte aligned: the staging loads are dwords
    unsigned char *wsrow = ws_base + d.ws_off + (long long)pass * d.ws_row;
    PngOut o;
    o.out = d.out;
    o.row_stride = d.row_stride;
    o.pal = d.pal;
    o.depth = d.depth;
    o.ctype = d.ctype;
    png_pass<U>(o, scan, off, wsrow, cols, rows, xs, ys, xd, yd, png_lds);
}

template <int U>
int png_launch(int passes, int n, int threads, hipStream_t stream, const void *table, const void *scan, void *ws) {
    const int lds = PNG_RING_BYTES + 136 + threads * (PNG_TILE * U + 4);
    static PpyLdsAttr attr;
    if (ppy_lds_attr(attr, (const void *)png_reconstruct_kernel<U>, lds) != PPY_OK) return PPY_ERR_LAUNCH;
    hipLaunchKernelGGL(png_reconstruct_kernel<U>, dim3(passes, n), dim3(threads), lds, stream, (const PngDev *)table,
                       (const unsigned char *)scan, (unsigned char *)ws);
    return PPY_OK;
}
#endif  // PPY_PNG_HOST_ONLY

}  // namespace

extern "C" size_t ppy_png_table_bytes(int n) { return n > 0 ? (size_t)n * sizeof(PngDev) : 0; }

extern "C" size_t ppy_png_workspace_bytes(int n, const ppy_png_desc_t *h_descs) {
    if (n <= 0 || h_descs == nullptr) return 0;
    long long s = 0;
    for (int i = 0; i < n; ++i) {
        if (!png_desc_ok(h_descs[i])) return 0;
        s += (long long)(h_descs[i].interlace ? 7 : 1) * png_ws_row(h_descs[i]);
    }
    return (size_t)s;
}

extern "C" int ppy_png_pack_table(int n, const ppy_png_desc_t *h_descs, unsigned char *const *h_out, const long long *h_row_stride,
                                  void *h_table, size_t table_bytes) {
    PPY_CHECK_ARG(n > 0 && n <= 65535 && h_descs && h_out && h_row_stride && h_table && table_bytes >= (size_t)n * sizeof(PngDev));
    PngDev *tab = static_cast<PngDev *>(h_table);
    long long ws = 0;
    for (int i = 0; i < n; ++i) {
        const ppy_png_desc_t &s = h_descs[i];
        PPY_CHECK_ARG(png_desc_ok(s) && h_out[i] != nullptr && h_row_stride[i] >= 3LL * s.width);
        PngDev d;
        memset(&d, 0, sizeof(d));
        d.out = h_out[i];
        d.row_stride = h_row_stride[i];
        d.scan_off = s.scan_offset;
        d.ws_off = ws;
        d.W = s.width;
        d.H = s.height;
        d.depth = s.bit_depth;
        d.ctype = s.colour_type;
        d.interlace = s.interlace;
        d.unit = png_unit(s.colour_type, s.bit_depth);
        d.ws_row = png_ws_row(s);
        ws += (long long)(s.interlace ? 7 : 1) * d.ws_row;
        for (int k = 0; k < s.palette_entries; ++k) {      // PLTE is R, G, B; entries past its end stay black
            d.pal[k][0] = s.palette[3 * k + 2];
            d.pal[k][1] = s.palette[3 * k + 1];
            d.pal[k][2] = s.palette[3 * k];
        }
        tab[i] = d;
    }
    return PPY_OK;
}

#ifndef PPY_PNG_HOST_ONLY
extern "C" int ppy_png_reconstruct_u8(int n, const ppy_png_desc_t *h_descs, const void *table, const void *scan, size_t scan_bytes,
                                      void *ws, size_t ws_bytes, void *stream) {
    ppy_drop_stale_error();
    PPY_CHECK_ARG(n > 0 && n <= 65535 && h_descs && table && scan && ((uintptr_t)table & 15) == 0 && ((uintptr_t)scan & 15) == 0);
    long long need = 0;
    int max_rows = 1, passes = 1;
    unsigned units_seen = 0;      // bit u: an image of unit size u
    for (int i = 0; i < n; ++i) {
        const ppy_png_desc_t &s = h_descs[i];
        // the stream and the dword the staging loads may touch past its end lie inside the buffer
        PPY_CHECK_ARG(png_desc_ok(s) &&
                      (unsigned long long)s.scan_offset + ((unsigned long long)s.scan_bytes + 15) / 16 * 16 <= scan_bytes);
        need += (long long)(s.interlace ? 7 : 1) * png_ws_row(s);
        if (s.interlace) passes = 7;
        max_rows = s.height > max_rows ? s.height : max_rows;      // (an interlaced pass has at most (H + 1) / 2 rows: not worth a case)
        units_seen |= 1u << png_unit(s.colour_type, s.bit_depth);
    }
    if (ws == nullptr || ws_bytes < (size_t)need || ((uintptr_t)ws & 15) != 0) return PPY_ERR_WORKSPACE;
    const int threads = max_rows >= PNG_MAX_THREADS ? PNG_MAX_THREADS : (max_rows + 63) / 64 * 64;
    int rc = PPY_OK;
    if (rc == PPY_OK && (units_seen & 1u << 1)) rc = png_launch<1>(passes, n, threads, (hipStream_t)stream, table, scan, ws);
    if (rc == PPY_OK && (units_seen & 1u << 2)) rc = png_launch<2>(passes, n, threads, (hipStream_t)stream, table, scan, ws);
    if (rc == PPY_OK && (units_seen & 1u << 3)) rc = png_launch<3>(passes, n, threads, (hipStream_t)stream, table, scan, ws);
    if (rc == PPY_OK && (units_seen & 1u << 4)) rc = png_launch<4>(passes, n, threads, (hipStream_t)stream, table, scan, ws);
    if (rc == PPY_OK && (units_seen & 1u << 6)) rc = png_launch<6>(passes, n, threads, (hipStream_t)stream, table, scan, ws);
    if (rc == PPY_OK && (units_seen & 1u << 8)) rc = png_launch<8>(passes, n, threads, (hipStream_t)stream, table, scan, ws);
    if (rc != PPY_OK) return rc;
    return ppy_launch_status();
}
#endif  // PPY_PNG_HOST_ONLY
