// Drawing detections onto uint8 images on the device: the reference's Decode.draw (model/decode_np.py:98-123) with Pillow's
// bitmap font in place of cv2.putText.  Contract: include/ppyolo_hip.h (ppy_draw_detections_u8), DESIGN.md section 10c.
//
// ONE launch per batch, one workgroup per (image, row).  A row paints, in this order, its outline, its label background and
// its label text; a later row overwrites an earlier one.  The kernel gets the sequential painter's result without any order
// between workgroups by giving every pixel exactly ONE writer: the LAST drawn row that covers it (covering = lying on that
// row's outline or inside its label rectangle, text included: the text lies inside the background).  So a workgroup
//   1. works out the geometry of every LATER drawn row of its image whose extent meets its own, marks the row in a K-bit
//      mask (one ballot per wave and 64 rows: no atomics) and keeps the marked rows in LDS as a dense list, each at the
//      position the mask gives it;
//   2. visits only the pixels of its own outline and label rectangle, clipped to the image, and stores a pixel unless one
//      of the listed rows covers it.  The colour of a pixel is black where the label's text has a set bit, else the class
//      colour -- outline and background have the same colour, so within a row the three primitives need no order either.
// Nothing is read from the image, nothing is accumulated: plain byte stores, the same bytes whatever the scheduling.
#include "common.h"

namespace {

constexpr int DRAW_THREADS = 256;
constexpr int DRAW_MAX_K = 1024;
constexpr int DRAW_NAME_MAX = 64;
constexpr int DRAW_LABEL_MAX = DRAW_NAME_MAX + 6;      // name + ": " + "d.dd"
constexpr int CELL_W = 6, CELL_H = 11;                 // the font's cell; th = CELL_H
constexpr int GLYPHS = 95, GLYPH_BYTES = 16;           // label_font.device_table()

struct DrawRow {
    int xa, ya, xb, yb;          // outline, corners sorted, inclusive
    int lx0, ly0, lx1, ly1;      // label background, inclusive; lx0 = left, ly1 = top
    int cls, hundredths;         // class index; rint(float64(score) * 100)
};

__device__ __forceinline__ bool draw_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }      // false for NaN

__device__ __forceinline__ int draw_round(float v) {
    float f = floorf(v + 0.5f);                                      // float32 sum and floor, as numpy >= 2 computes them
    f = fminf(fmaxf(f, -1073741824.0f), 1073741824.0f);
    return (int)f;
}

// The row's geometry if it is drawn.  name_len is read only for a class inside [0, C).
__device__ __forceinline__ bool draw_row(const float *__restrict__ p, float thresh, int C, int h, int w,
                                         const int *__restrict__ name_len, DrawRow &o) {
    const float cls = p[0], sc = p[1], x0 = p[2], y0 = p[3], x1 = p[4], y1 = p[5];
    if (!(draw_finite(cls) && draw_finite(sc) && draw_finite(x0) && draw_finite(y0) && draw_finite(x1) && draw_finite(y1))) return false;
    if (!(sc >= thresh) || !(cls >= 0.0f && cls < (float)C) || !(sc >= 0.0f && sc <= 1.0f)) return false;
    o.cls = (int)cls;
    const int left = max(0, draw_round(x0)), top = max(0, draw_round(y0));
    const int right = min(w, draw_round(x1)), bottom = min(h, draw_round(y1));
    o.xa = min(left, right);
    o.xb = max(left, right);
    o.ya = min(top, bottom);
    o.yb = max(top, bottom);
    const int nl = min(max(name_len[o.cls], 0), DRAW_NAME_MAX);
    o.lx0 = left;
    o.lx1 = left + CELL_W * (nl + 6);
    o.ly0 = top - CELL_H - 3;
    o.ly1 = top;
    o.hundredths = (int)rint((double)sc * 100.0);                    // exact product: 24 + 7 significant bits
    return true;
}

// ol = (xa, ya, xb - xa, yb - ya), lb = (lx0, ly0, lx1 - lx0, -): one unsigned compare per range (a negative difference wraps high)
__device__ __forceinline__ bool draw_covers(const int4 ol, const int4 lb, int x, int y) {
    const int dx = x - ol.x, dy = y - ol.y, u = x - lb.x, v = y - lb.y;
    const bool in_label = ((unsigned)u <= (unsigned)lb.z) & ((unsigned)v <= (unsigned)(CELL_H + 3));
    const bool in_box = ((unsigned)dx <= (unsigned)ol.z) & ((unsigned)dy <= (unsigned)ol.w);
    return in_label | (in_box & ((dx == 0) | (dx == ol.z) | (dy == 0) | (dy == ol.w)));
}

__global__ __launch_bounds__(DRAW_THREADS) void draw_detections_kernel(
    const ppy_draw_image_t *__restrict__ images, const float *__restrict__ dets, const int *__restrict__ count, int K, float thresh,
    const unsigned char *__restrict__ colors, int C, const unsigned char *__restrict__ names, const int *__restrict__ name_len,
    const unsigned char *__restrict__ font) {
    extern __shared__ int4 s_geo[];                                  // [K][2]: outline, label of the later rows that matter, dense
    __shared__ unsigned long long s_mask[DRAW_MAX_K / 64];
    __shared__ unsigned char s_glyph[DRAW_LABEL_MAX * GLYPH_BYTES];  // the font records of this row's label, in string order

    const int tid = threadIdx.x, r = blockIdx.x, img = blockIdx.y;
    const ppy_draw_image_t im = images[img];
    const int h = im.h, w = im.w;
    const int cnt = min(count[img], K);
    if (r >= cnt) return;                                            // (the whole workgroup: r is uniform)
    const float *rows = dets + (long long)img * K * 6;
    DrawRow own;
    if (!draw_row(rows + 6 * r, thresh, C, h, w, name_len, own)) return;
    // this row's extent, clipped: what a later row has to meet to matter here
    const int ex0 = max(min(own.xa, own.lx0), 0), ex1 = min(max(own.xb, own.lx1), w - 1);
    const int ey0 = max(min(own.ya, own.ly0), 0), ey1 = min(max(own.yb, own.ly1), h - 1);
    if (ex0 > ex1 || ey0 > ey1) return;                              // wholly outside the image

    // ---- 1: the later rows -------------------------------------------------------------------------------------------------
    // each thread keeps the geometry of its (at most 4) rows in registers; the ballots give the mask, the mask gives every
    // kept row its place in a dense list, written after the barrier
    const int words = (K + 63) >> 6, lane = tid & 63;
    int4 ga[DRAW_MAX_K / DRAW_THREADS], gb[DRAW_MAX_K / DRAW_THREADS];
    unsigned long long below[DRAW_MAX_K / DRAW_THREADS];             // the kept rows of this wave's word before this lane; ~0: not kept
#pragma unroll
    for (int it = 0; it < DRAW_MAX_K / DRAW_THREADS; ++it) {
        below[it] = ~0ull;
        if (it * DRAW_THREADS < words * 64) {                        // (uniform: every lane of the workgroup reaches the ballot)
            const int j = it * DRAW_THREADS + tid;
            bool hit = false;
            DrawRow o;
            if (j > r && j < cnt && draw_row(rows + 6 * j, thresh, C, h, w, name_len, o)) {
                hit = min(o.xa, o.lx0) <= ex1 && max(o.xb, o.lx1) >= ex0 && min(o.ya, o.ly0) <= ey1 && max(o.yb, o.ly1) >= ey0;
                ga[it] = make_int4(o.xa, o.ya, o.xb - o.xa, o.yb - o.ya);
                gb[it] = make_int4(o.lx0, o.ly0, o.lx1 - o.lx0, 0);
            }
            const unsigned long long m = __ballot(hit);
            if (hit) below[it] = m & ((1ull << lane) - 1ull);
            if (lane == 0 && (j >> 6) < words) s_mask[j >> 6] = m;
        }
    }
    // the label: name + ": " + d.dd, as font records
    const int nl = (own.lx1 - own.lx0) / CELL_W - 6, len = nl + 6;
    for (int i = tid; i < len * GLYPH_BYTES; i += DRAW_THREADS) {
        const int k = i / GLYPH_BYTES;
        int ch;
        if (k < nl) ch = names[(long long)own.cls * DRAW_NAME_MAX + k];
        else if (k == nl) ch = ':';
        else if (k == nl + 1) ch = ' ';
        else if (k == nl + 2) ch = '0' + own.hundredths / 100;
        else if (k == nl + 3) ch = '.';
        else if (k == nl + 4) ch = '0' + own.hundredths / 10 % 10;
        else ch = '0' + own.hundredths % 10;
        if (ch < 32 || ch > 126) ch = '?';
        s_glyph[i] = font[(ch - 32) * GLYPH_BYTES + (i % GLYPH_BYTES)];
    }
    __syncthreads();
    int nhit = 0;
#pragma unroll
    for (int it = 0; it < DRAW_MAX_K / DRAW_THREADS; ++it) {
        const int word = (it * DRAW_THREADS + tid) >> 6;             // (the same for every lane of a wave)
        if (below[it] != ~0ull) {
            int pos = __popcll(below[it]);
            for (int wd = 0; wd < word; ++wd) pos += __popcll(s_mask[wd]);
            s_geo[2 * pos] = ga[it];
            s_geo[2 * pos + 1] = gb[it];
        }
    }
    for (int wd = 0; wd < words; ++wd) nhit += __popcll(s_mask[wd]);
    __syncthreads();

    // ---- 2: this row's pixels ----------------------------------------------------------------------------------------------
    const unsigned char c0 = colors[3 * own.cls], c1 = colors[3 * own.cls + 1], c2 = colors[3 * own.cls + 2];
    const int cx0 = max(own.xa, 0), cx1 = min(own.xb, w - 1);                    // the horizontal edges' columns
    const int cy0 = max(own.ya + 1, 0), cy1 = min(own.yb - 1, h - 1);            // the vertical edges' rows, corners excluded
    const int nx = max(cx1 - cx0 + 1, 0), ny = max(cy1 - cy0 + 1, 0);
    const int n_top = own.ya >= 0 && own.ya < h ? nx : 0;
    const int n_bot = own.yb != own.ya && own.yb >= 0 && own.yb < h ? nx : 0;
    const int n_lft = own.xa >= 0 && own.xa < w ? ny : 0;
    const int n_rgt = own.xb != own.xa && own.xb >= 0 && own.xb < w ? ny : 0;
    const int bx0 = max(own.lx0, 0), bx1 = min(own.lx1, w - 1), by0 = max(own.ly0, 0), by1 = min(own.ly1, h - 1);
    const int bw = max(bx1 - bx0 + 1, 0), bh = max(by1 - by0 + 1, 0);
    const int n_out = n_top + n_bot + n_lft + n_rgt, total = n_out + bw * bh;
    const int tx0 = own.lx0, ty0 = own.ly1 - CELL_H - 2, tw = len * CELL_W;      // the text's cell grid
    for (int idx = tid; idx < total; idx += DRAW_THREADS) {
        int x, y;
        bool label = false;
        if (idx >= n_out) {
            const int k = idx - n_out;
            y = by0 + k / bw;
            x = bx0 + k % bw;
            label = true;
        } else {
            int k = idx;
            if (k < n_top) {
                x = cx0 + k, y = own.ya;
            } else if ((k -= n_top) < n_bot) {
                x = cx0 + k, y = own.yb;
            } else if ((k -= n_bot) < n_lft) {
                x = own.xa, y = cy0 + k;
            } else {
                x = own.xb, y = cy0 + (k - n_lft);
            }
            if (x >= own.lx0 && x <= own.lx1 && y >= own.ly0 && y <= own.ly1) continue;      // the label's loop owns it
        }
        bool covered = false;
        for (int q = 0; q < nhit && !covered; q += 4) {              // four rows a turn: their eight LDS reads go out together
            const int q1 = min(q + 1, nhit - 1), q2 = min(q + 2, nhit - 1), q3 = min(q + 3, nhit - 1);
            const int4 a0 = s_geo[2 * q], b0 = s_geo[2 * q + 1], a1 = s_geo[2 * q1], b1 = s_geo[2 * q1 + 1];
            const int4 a2 = s_geo[2 * q2], b2 = s_geo[2 * q2 + 1], a3 = s_geo[2 * q3], b3 = s_geo[2 * q3 + 1];
            covered = draw_covers(a0, b0, x, y) | draw_covers(a1, b1, x, y) | draw_covers(a2, b2, x, y) | draw_covers(a3, b3, x, y);
        }
        if (covered) continue;
        bool ink = false;
        const int u = x - tx0, v = y - ty0;
        if (label && u >= 0 && u < tw && v >= 0 && v < CELL_H) {
            // the LAST glyph whose rectangle contains the pixel: glyph i + 1 reaches column 5 of cell i when its gx0 is -1
            const int i = u / CELL_W, c = u - CELL_W * i;
            bool found = false;
            if (c == CELL_W - 1 && i + 1 < len) {
                const unsigned char *g = s_glyph + (i + 1) * GLYPH_BYTES;
                if (g[0] == 0 && v >= g[1] && v < g[3]) {
                    found = true;
                    ink = g[5 + v] & 1;
                }
            }
            if (!found) {
                const unsigned char *g = s_glyph + i * GLYPH_BYTES;
                if (c + 1 >= g[0] && c + 1 < g[2] && v >= g[1] && v < g[3]) ink = (g[5 + v] >> (c + 1)) & 1;
            }
        }
        unsigned char *px = im.base + (long long)y * im.pitch + 3 * x;
        px[0] = ink ? 0 : c0;
        px[1] = ink ? 0 : c1;
        px[2] = ink ? 0 : c2;
    }
}

}  // namespace

extern "C" int ppy_draw_detections_u8(int n, const ppy_draw_image_t *h_images, const ppy_draw_image_t *images, const float *dets,
                                      const int *count, int K, float draw_thresh, const unsigned char *colors, int num_classes,
                                      const unsigned char *names, const int *name_len, const int *h_name_len,
                                      const unsigned char *font, void *stream) {
    ppy_drop_stale_error();
    PPY_CHECK_ARG(n > 0 && n <= 65535 && h_images && images && dets && count && colors && names && name_len && h_name_len && font);
    if (K < 1 || K > DRAW_MAX_K || num_classes < 1) return PPY_ERR_UNSUPPORTED;
    for (int c = 0; c < num_classes; ++c) {
        PPY_CHECK_ARG(h_name_len[c] >= 0);
        if (h_name_len[c] > DRAW_NAME_MAX) return PPY_ERR_UNSUPPORTED;
    }
    for (int i = 0; i < n; ++i) {
        const ppy_draw_image_t &d = h_images[i];
        PPY_CHECK_ARG(d.base && d.h >= 1 && d.h <= 65535 && d.w >= 1 && d.w <= 65535);
        PPY_CHECK_ARG(d.pitch >= 3LL * d.w || (d.h == 1 && d.pitch >= 0));
    }
    const size_t lds = (size_t)K * 2 * sizeof(int4);                 // <= 32 KB: inside the default dynamic limit
    hipLaunchKernelGGL(draw_detections_kernel, dim3(K, n), dim3(DRAW_THREADS), lds, (hipStream_t)stream, images, dets, count, K,
                       draw_thresh, colors, num_classes, names, name_len, font);
    return ppy_launch_status();
}
