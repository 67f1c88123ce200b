// Baseline JPEG encoding with libjpeg-turbo's defaults (what cv2.imwrite(path, img, [IMWRITE_JPEG_QUALITY, q]) runs;
// reference demo.py:50): integer RGB -> YCbCr tables, box downsampling with the alternating bias, JDCT_ISLOW forward DCT,
// quantisation rounding half away from zero, the standard Huffman tables, a JFIF 1.01 header.  The file is byte for byte the
// one libjpeg-turbo writes; tests/jpeg_enc_ref.py restates every step in numpy and tests/test_jpeg_enc_ref.py holds that
// restatement equal to Pillow.  DESIGN.md section 10b is the contract, with the two padding rules.
//
// The seam is the decoder's coefficient buffer (include/ppyolo_hip.h): int16, per component [block row][block column][64],
// whole-MCU block counts, transposed inside a block.
//   stage 1, device  jpeg_enc_fdct_kernel: one launch per BATCH; 8 lanes per block, as the decoder's inverse DCT.
//   stage 2, device  eight launches per batch, no host synchronisation; one LANE per block codes it, so no restart segment
//                    and no image serialises through one lane (the prefix sums run one workgroup per image).
//   stage 2, host    ppy_jpeg_enc_scan_host, the same bytes in plain C++: the CPU-testable definition of the bit-packer.
// The per-image descriptors travel as a table in device memory, packed on the host (ppy_jpeg_enc_pack_table), like the
// decoder's table and the blob of augment.hip.
#include <string.h>

#include <cstdio>

#ifndef PPY_JPEG_HOST_ONLY
#include "common.h"
#else      // the host part alone as plain C++ (tools/jpeg_encode_asan.cpp: AddressSanitizer build, no HIP headers)
#include <stddef.h>
#include <stdint.h>

#include "../../../include/ppyolo_hip.h"
#define PPY_CHECK_ARG(cond) \
    do {                    \
        if (!(cond)) return PPY_ERR_BAD_ARG; \
    } while (0)
#endif

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

// ---------------------------------------------------------------------------------------------------------------- host
const unsigned char ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                  41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                  30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
inline int stored_index(int zz) { return (ZIGZAG[zz] & 7) * 8 + (ZIGZAG[zz] >> 3); }      // transposed inside a block

// ISO/IEC 10918-1 Annex K.1 (natural order) and K.3
const unsigned char Q_BASE[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
const unsigned char DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const unsigned char DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const unsigned char AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
const unsigned char AC_VALS[2][162] = {
    {1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161, 8,   35,  66,  177,
     193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,  39,  40,  41,  42,  52,  53,  54,  55,
     56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106,
     115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
     164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211,
     212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
    {0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,  145, 161, 177, 193,
     9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,  26,  38,  39,  40,  41,  42,  53,  54,
     55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105,
     106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
     162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202,
     210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}};

// symbol -> length << 16 | code, the canonical assignment of Annex C; 0 = no such symbol
void build_codes(const unsigned char *bits, const unsigned char *vals, u32 *out, int n_out) {
    for (int i = 0; i < n_out; ++i) out[i] = 0;
    u32 code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) out[vals[k]] = (u32)l << 16 | code;
        code <<= 1;
    }
}

void set_reason(char *h_reason, const char *why) {
    if (h_reason) snprintf(h_reason, 64, "%s", why);
}
int refuse(char *h_reason, int code, const char *why) {
    set_reason(h_reason, why);
    return code;
}

int params_check(const ppy_jpeg_enc_params_t *p, char *h_reason) {
    if (p == nullptr) return refuse(h_reason, PPY_ERR_BAD_ARG, "no parameters");
    if (p->quality < 1 || p->quality > 100) return refuse(h_reason, PPY_ERR_BAD_ARG, "quality outside 1..100");
    if (p->restart_interval < 0 || p->restart_interval > 65535) return refuse(h_reason, PPY_ERR_BAD_ARG, "restart interval outside 0..65535");
    if (!((p->h_samp == 1 && p->v_samp == 1) || (p->h_samp == 2 && p->v_samp == 1) || (p->h_samp == 2 && p->v_samp == 2)))
        return refuse(h_reason, PPY_ERR_UNSUPPORTED, "sampling factors");
    return PPY_OK;
}

// jpeg_set_quality(q, force_baseline = TRUE), natural order
void quant_tables(int quality, unsigned short q[2][64]) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            int v = (Q_BASE[t][i] * scale + 50) / 100;
            q[t][i] = (unsigned short)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
}

const long long DEVICE_CAPACITY_MAX = 1ll << 29;      // the device stage keeps 32-bit bit positions
long long scan_capacity(long long blocks, long long segments) { return 416 * blocks + 4 * segments; }
long long align16(long long v) { return (v + 15) / 16 * 16; }
// stage 2 workspace of one image: bits / bit offset per block | segment byte offsets (segments + 1) | 0xFF count per 64-byte
// chunk | the unstuffed stream (208 bytes per block and one per segment bound it: see CAPACITY in the header)
long long stream_bound(long long blocks, long long segments) { return (208 * blocks + segments + 63) / 64 * 64 + 64; }      // whole chunks + one
long long chunks_bound(long long blocks, long long segments) { return (208 * blocks + segments + 63) / 64; }
struct WsLayout {
    long long bits, seg, ff, stream, total;
};
WsLayout ws_layout(long long blocks, long long segments) {
    WsLayout w;
    w.bits = 0;
    w.seg = w.bits + align16(4 * blocks);
    w.ff = w.seg + align16(4 * (segments + 1));
    w.stream = w.ff + align16(4 * (chunks_bound(blocks, segments) + 1));
    w.total = w.stream + stream_bound(blocks, segments);
    return w;
}

// The geometry of one image from (width, height, components, params): everything ppy_jpeg_enc_layout fills but the bases.
void fill_geometry(const ppy_jpeg_enc_params_t &p, ppy_jpeg_enc_desc_t &d) {
    const int nc = d.components;
    const int hm = nc == 3 ? p.h_samp : 1, vm = nc == 3 ? p.v_samp : 1;
    d.restart_interval = p.restart_interval;
    d.mcus_w = (d.width + 8 * hm - 1) / (8 * hm);
    d.mcus_h = (d.height + 8 * vm - 1) / (8 * vm);
    long long elems = 0;
    d.blocks = 0;
    for (int c = 0; c < 3; ++c) {
        if (c >= nc) {
            d.h_samp[c] = d.v_samp[c] = d.blocks_w[c] = d.blocks_h[c] = d.real_w[c] = d.real_h[c] = 0;
            d.coef_offset[c] = 0;
            continue;
        }
        const int h = c == 0 ? hm : 1, v = c == 0 ? vm : 1;
        d.h_samp[c] = h;
        d.v_samp[c] = v;
        d.blocks_w[c] = d.mcus_w * h;
        d.blocks_h[c] = d.mcus_h * v;
        const int cw = (d.width * h + hm - 1) / hm, ch = (d.height * v + vm - 1) / vm;      // component size in samples
        d.real_w[c] = (cw + 7) / 8;
        d.real_h[c] = (ch + 7) / 8;
        d.coef_offset[c] = elems;
        elems += (long long)d.blocks_w[c] * d.blocks_h[c] * 64;
        d.blocks += (long long)d.blocks_w[c] * d.blocks_h[c];
    }
    const long long mcus = (long long)d.mcus_w * d.mcus_h;
    d.segments = p.restart_interval ? (mcus + p.restart_interval - 1) / p.restart_interval : 1;
    d.coef_bytes = elems * 2;
    d.scan_capacity = scan_capacity(d.blocks, d.segments);
    d.ws_bytes = ws_layout(d.blocks, d.segments).total;
}

bool size_ok(int width, int height, int components) {
    return width >= 1 && width <= 65535 && height >= 1 && height <= 65535 && (components == 1 || components == 3);
}

// A descriptor is what ppy_jpeg_enc_layout would have written for its (width, height, components, restart interval, luma
// sampling): the later calls recompute the geometry and compare, so a descriptor edited by hand cannot size a grid.
bool desc_ok(const ppy_jpeg_enc_desc_t &s) {
    if (!size_ok(s.width, s.height, s.components)) return false;
    ppy_jpeg_enc_params_t p;
    p.quality = 50;
    p.h_samp = s.components == 3 ? s.h_samp[0] : 1;
    p.v_samp = s.components == 3 ? s.v_samp[0] : 1;
    p.restart_interval = s.restart_interval;
    if (params_check(&p, nullptr) != PPY_OK) return false;
    ppy_jpeg_enc_desc_t g;
    memset(&g, 0, sizeof(g));
    g.width = s.width;
    g.height = s.height;
    g.components = s.components;
    fill_geometry(p, g);
    if (g.mcus_w != s.mcus_w || g.mcus_h != s.mcus_h || g.blocks != s.blocks || g.segments != s.segments || g.coef_bytes != s.coef_bytes ||
        g.scan_capacity != s.scan_capacity || g.ws_bytes != s.ws_bytes)
        return false;
    for (int c = 0; c < 3; ++c)
        if (g.h_samp[c] != s.h_samp[c] || g.v_samp[c] != s.v_samp[c] || g.blocks_w[c] != s.blocks_w[c] || g.blocks_h[c] != s.blocks_h[c] ||
            g.real_w[c] != s.real_w[c] || g.real_h[c] != s.real_h[c] || g.coef_offset[c] != s.coef_offset[c])
            return false;
    return s.coef_base >= 0 && s.coef_base % 16 == 0 && s.ws_base >= 0 && s.ws_base % 16 == 0;
}

// The table: EncCommon, then one EncDev per image.
struct EncCommon {
    u32 recip[2][64];      // floor(2^32 / d) + 1 with d = 8 * q, STORED (transposed) order: see quantise()
    u32 half[2][64];       // d / 2
    u32 dc_code[2][16];    // length << 16 | code
    u32 ac_code[2][256];
    int n, pad[3];
};
struct EncDev {
    const unsigned char *src;
    long long row_stride;
    long long coef_off[3];            // int16 elements into the batch coefficient buffer
    long long ws_bits, ws_seg, ws_ff, ws_stream;      // bytes into the stage 2 workspace
    int ncomp, W, H, pad0;
    int bw[3], bh[3], rw[3], rh[3], blk_end[3];
    int hs[3], vs[3];                 // blocks of the component in one MCU
    int cw[3], ch[3];                 // component size in samples
    int mcus_w, mcus, dri, segments;
    int blocks, bpm, chunks_bound, stream_vec_bound;      // bpm: blocks per MCU; stream_vec_bound: 16-byte units
    int pad1[2];
};
static_assert(sizeof(EncCommon) % 16 == 0 && sizeof(EncDev) % 16 == 0, "table layout");
size_t enc_table_bytes(int n) { return n > 0 ? sizeof(EncCommon) + (size_t)n * sizeof(EncDev) : 0; }

// ---- the bit-packer, host twin (jchuff.c encode_one_block / flush_bits / emit_restart) -------------------------------
struct HostBits {
    unsigned char *out;
    size_t cap, len;
    u64 acc;
    int n;
    bool full;
    void byte(unsigned b) {
        if (len < cap) out[len++] = (unsigned char)b;
        else full = true;
    }
    void put(u32 v, int bits) {
        acc = acc << bits | v;
        n += bits;
        while (n >= 8) {
            const unsigned b = (unsigned)(acc >> (n - 8)) & 0xFFu;
            byte(b);
            if (b == 0xFF) byte(0);
            n -= 8;
        }
    }
    void flush() {      // the last byte is filled with 1-bits
        if (n) put((1u << (8 - n)) - 1u, 8 - n);
    }
};

inline int bit_size(int v) {
    v = v < 0 ? -v : v;
    int s = 0;
    while (v) {
        ++s;
        v >>= 1;
    }
    return s;
}

}  // namespace

extern "C" int ppy_jpeg_enc_quant(int quality, unsigned short *h_luma, unsigned short *h_chroma) {
    PPY_CHECK_ARG(quality >= 1 && quality <= 100 && h_luma && h_chroma);
    unsigned short q[2][64];
    quant_tables(quality, q);
    memcpy(h_luma, q[0], sizeof(q[0]));
    memcpy(h_chroma, q[1], sizeof(q[1]));
    return PPY_OK;
}

extern "C" size_t ppy_jpeg_enc_header_bytes(int components, int restart_interval) {
    if (components != 1 && components != 3) return 0;
    const int t = components == 3 ? 2 : 1;
    // SOI, APP0(16), DQT(67) per table, SOF0(8 + 3 per component), DHT(31) + DHT(181) per table, [DRI(4)], SOS(6 + 2 per component)
    return 2 + 18 + 69 * t + (2 + 8 + 3 * components) + (33 + 183) * t + (restart_interval ? 6 : 0) + (2 + 6 + 2 * components);
}

extern "C" int ppy_jpeg_enc_header(const ppy_jpeg_enc_params_t *h_params, int width, int height, int components, unsigned char *h_out,
                                   size_t capacity, size_t *h_used, char *h_reason) {
    set_reason(h_reason, "");
    const int rc = params_check(h_params, h_reason);
    if (rc != PPY_OK) return rc;
    if (!size_ok(width, height, components)) return refuse(h_reason, PPY_ERR_BAD_ARG, "width, height 1..65535, components 1 or 3");
    if (h_out == nullptr) return refuse(h_reason, PPY_ERR_BAD_ARG, "no output buffer");
    const size_t need = ppy_jpeg_enc_header_bytes(components, h_params->restart_interval);
    if (capacity < need) return refuse(h_reason, PPY_ERR_WORKSPACE, "header buffer too small");
    unsigned char *o = h_out;
    auto seg = [&o](int marker, int payload) {
        *o++ = 0xFF;
        *o++ = (unsigned char)marker;
        *o++ = (unsigned char)((payload + 2) >> 8);
        *o++ = (unsigned char)((payload + 2) & 0xFF);
    };
    *o++ = 0xFF;
    *o++ = 0xD8;
    seg(0xE0, 14);
    const unsigned char jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    memcpy(o, jfif, 14);
    o += 14;
    const int tables = components == 3 ? 2 : 1;
    unsigned short q[2][64];
    quant_tables(h_params->quality, q);
    for (int t = 0; t < tables; ++t) {
        seg(0xDB, 65);
        *o++ = (unsigned char)t;
        for (int k = 0; k < 64; ++k) *o++ = (unsigned char)q[t][ZIGZAG[k]];
    }
    seg(0xC0, 6 + 3 * components);
    *o++ = 8;
    *o++ = (unsigned char)(height >> 8);
    *o++ = (unsigned char)(height & 0xFF);
    *o++ = (unsigned char)(width >> 8);
    *o++ = (unsigned char)(width & 0xFF);
    *o++ = (unsigned char)components;
    for (int c = 0; c < components; ++c) {
        *o++ = (unsigned char)(c + 1);
        *o++ = (unsigned char)(c == 0 && components == 3 ? h_params->h_samp << 4 | h_params->v_samp : 0x11);
        *o++ = (unsigned char)(c ? 1 : 0);
    }
    for (int t = 0; t < tables; ++t) {
        seg(0xC4, 1 + 16 + 12);
        *o++ = (unsigned char)t;
        memcpy(o, DC_BITS[t], 16);
        memcpy(o + 16, DC_VALS, 12);
        o += 28;
        seg(0xC4, 1 + 16 + 162);
        *o++ = (unsigned char)(0x10 | t);
        memcpy(o, AC_BITS[t], 16);
        memcpy(o + 16, AC_VALS[t], 162);
        o += 178;
    }
    if (h_params->restart_interval) {
        seg(0xDD, 2);
        *o++ = (unsigned char)(h_params->restart_interval >> 8);
        *o++ = (unsigned char)(h_params->restart_interval & 0xFF);
    }
    seg(0xDA, 4 + 2 * components);
    *o++ = (unsigned char)components;
    for (int c = 0; c < components; ++c) {
        *o++ = (unsigned char)(c + 1);
        *o++ = (unsigned char)(c ? 0x11 : 0x00);
    }
    *o++ = 0;
    *o++ = 63;
    *o++ = 0;
    if ((size_t)(o - h_out) != need) return refuse(h_reason, PPY_ERR_BAD_ARG, "header size");      // (cannot happen)
    if (h_used) *h_used = need;
    return PPY_OK;
}

extern "C" size_t ppy_jpeg_enc_scan_capacity(long long blocks, long long segments) {
    if (blocks <= 0 || segments <= 0 || blocks > (1ll << 40) || segments > (1ll << 40)) return 0;
    return (size_t)scan_capacity(blocks, segments);
}

extern "C" int ppy_jpeg_enc_layout(const ppy_jpeg_enc_params_t *h_params, int n, ppy_jpeg_enc_desc_t *h_descs, ppy_jpeg_enc_sizes_t *h_sizes,
                                   char *h_reason) {
    set_reason(h_reason, "");
    const int rc = params_check(h_params, h_reason);
    if (rc != PPY_OK) return rc;
    if (n <= 0 || n > 65535 || h_descs == nullptr || h_sizes == nullptr) return refuse(h_reason, PPY_ERR_BAD_ARG, "batch of 1..65535 images expected");
    long long coef = 0, ws = 0, out = 0;
    for (int i = 0; i < n; ++i) {
        ppy_jpeg_enc_desc_t &d = h_descs[i];
        if (!size_ok(d.width, d.height, d.components)) {
            char why[64];
            snprintf(why, sizeof(why), "image %d: width, height 1..65535, components 1 or 3", i);
            return refuse(h_reason, PPY_ERR_BAD_ARG, why);
        }
        if (d.row_stride < (long long)d.components * d.width) {
            char why[64];
            snprintf(why, sizeof(why), "image %d: row stride below the row's bytes", i);
            return refuse(h_reason, PPY_ERR_BAD_ARG, why);
        }
        fill_geometry(*h_params, d);
        d.coef_base = coef;
        coef += align16(d.coef_bytes);
        d.ws_base = ws;
        ws += align16(d.ws_bytes);
        out += d.scan_capacity;
    }
    h_sizes->coef_bytes = (size_t)coef;
    h_sizes->ws_bytes = (size_t)ws + 16 * (size_t)n + 16;      // + the images' offsets in `out` (n + 1 of 8 bytes)
    h_sizes->out_bytes = (size_t)out;
    h_sizes->table_bytes = enc_table_bytes(n);
    return PPY_OK;
}

extern "C" int ppy_jpeg_enc_scan_host(const ppy_jpeg_enc_desc_t *h_desc, const int16_t *h_coef, size_t coef_bytes, unsigned char *h_out,
                                      size_t capacity, size_t *h_len, char *h_reason) {
    set_reason(h_reason, "");
    if (h_desc == nullptr || h_coef == nullptr || h_out == nullptr || h_len == nullptr) return refuse(h_reason, PPY_ERR_BAD_ARG, "null pointer");
    const ppy_jpeg_enc_desc_t &d = *h_desc;
    if (!desc_ok(d)) return refuse(h_reason, PPY_ERR_BAD_ARG, "descriptor is not one ppy_jpeg_enc_layout wrote");
    if (coef_bytes < (size_t)d.coef_bytes) return refuse(h_reason, PPY_ERR_BAD_ARG, "coefficient buffer smaller than coef_bytes");
    if (capacity < (size_t)d.scan_capacity) return refuse(h_reason, PPY_ERR_WORKSPACE, "output below ppy_jpeg_enc_scan_capacity");
    u32 dc_code[2][16], ac_code[2][256];
    for (int t = 0; t < 2; ++t) {
        build_codes(DC_BITS[t], DC_VALS, dc_code[t], 16);
        build_codes(AC_BITS[t], AC_VALS[t], ac_code[t], 256);
    }
    int zzs[64];
    for (int k = 0; k < 64; ++k) zzs[k] = stored_index(k);
    HostBits hb = {h_out, capacity, 0, 0, 0, false};
    int pred[3] = {0, 0, 0};
    const long long mcus = (long long)d.mcus_w * d.mcus_h;
    for (long long m = 0; m < mcus; ++m) {
        const int my = (int)(m / d.mcus_w), mx = (int)(m % d.mcus_w);
        if (d.restart_interval && m && m % d.restart_interval == 0) {
            hb.flush();
            hb.byte(0xFF);
            hb.byte(0xD0 + (unsigned)((m / d.restart_interval - 1) & 7));
            pred[0] = pred[1] = pred[2] = 0;
        }
        for (int c = 0; c < d.components; ++c) {
            const int t = c ? 1 : 0;
            for (int v = 0; v < d.v_samp[c]; ++v)
                for (int h = 0; h < d.h_samp[c]; ++h) {
                    const int16_t *b = h_coef + d.coef_offset[c] + ((long long)(my * d.v_samp[c] + v) * d.blocks_w[c] + mx * d.h_samp[c] + h) * 64;
                    // a DC difference beyond 11 bits or an AC value beyond 10 has no code in a baseline file
                    const int diff = b[0] - pred[c];
                    pred[c] = b[0];
                    int s = bit_size(diff);
                    if (s > 11) return refuse(h_reason, PPY_ERR_BAD_ARG, "DC difference out of the baseline range");
                    hb.put(dc_code[t][s] & 0xFFFFu, (int)(dc_code[t][s] >> 16));
                    if (s) hb.put((u32)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u), s);
                    int run = 0;
                    for (int k = 1; k < 64; ++k) {
                        const int a = b[zzs[k]];
                        if (a == 0) {
                            ++run;
                            continue;
                        }
                        while (run > 15) {
                            hb.put(ac_code[t][0xF0] & 0xFFFFu, (int)(ac_code[t][0xF0] >> 16));
                            run -= 16;
                        }
                        s = bit_size(a);
                        if (s > 10) return refuse(h_reason, PPY_ERR_BAD_ARG, "AC coefficient out of the baseline range");
                        const u32 code = ac_code[t][run << 4 | s];
                        hb.put(code & 0xFFFFu, (int)(code >> 16));
                        hb.put((u32)(a < 0 ? a - 1 : a) & ((1u << s) - 1u), s);
                        run = 0;
                    }
                    if (run) hb.put(ac_code[t][0] & 0xFFFFu, (int)(ac_code[t][0] >> 16));
                }
        }
    }
    hb.flush();
    if (hb.full) return refuse(h_reason, PPY_ERR_WORKSPACE, "output buffer too small");      // (the capacity bound excludes it)
    *h_len = hb.len;
    return PPY_OK;
}


extern "C" int ppy_jpeg_enc_pack_table(const ppy_jpeg_enc_params_t *h_params, int n, const ppy_jpeg_enc_desc_t *h_descs, void *h_table,
                                       size_t table_bytes) {
    PPY_CHECK_ARG(params_check(h_params, nullptr) == PPY_OK && n > 0 && n <= 65535 && h_descs && h_table &&
                  table_bytes >= enc_table_bytes(n));
    EncCommon C;
    memset(&C, 0, sizeof(C));
    unsigned short q[2][64];
    quant_tables(h_params->quality, q);
    for (int t = 0; t < 2; ++t) {
        for (int i = 0; i < 64; ++i) {      // natural index i = row * 8 + col -> stored col * 8 + row
            const u32 d = 8u * q[t][i];
            const int st = (i & 7) * 8 + (i >> 3);
            C.recip[t][st] = (u32)((1ull << 32) / d) + 1u;
            C.half[t][st] = d >> 1;
        }
        build_codes(DC_BITS[t], DC_VALS, C.dc_code[t], 16);
        build_codes(AC_BITS[t], AC_VALS[t], C.ac_code[t], 256);
    }
    C.n = n;
    memcpy(h_table, &C, sizeof(C));
    EncDev *tab = reinterpret_cast<EncDev *>(static_cast<unsigned char *>(h_table) + sizeof(EncCommon));
    for (int i = 0; i < n; ++i) {
        const ppy_jpeg_enc_desc_t &s = h_descs[i];
        PPY_CHECK_ARG(desc_ok(s) && s.src != nullptr && s.row_stride >= (long long)s.components * s.width);
        PPY_CHECK_ARG(s.restart_interval == h_params->restart_interval &&
                      (s.components == 1 || (s.h_samp[0] == h_params->h_samp && s.v_samp[0] == h_params->v_samp)));
        EncDev d;
        memset(&d, 0, sizeof(d));
        d.src = s.src;
        d.row_stride = s.row_stride;
        d.ncomp = s.components;
        d.W = s.width;
        d.H = s.height;
        int blocks = 0;
        for (int c = 0; c < s.components; ++c) {
            d.coef_off[c] = s.coef_base / 2 + s.coef_offset[c];
            d.bw[c] = s.blocks_w[c];
            d.bh[c] = s.blocks_h[c];
            d.rw[c] = s.real_w[c];
            d.rh[c] = s.real_h[c];
            blocks += s.blocks_w[c] * s.blocks_h[c];
            d.blk_end[c] = blocks;
            d.hs[c] = s.h_samp[c];
            d.vs[c] = s.v_samp[c];
            d.cw[c] = (s.width * s.h_samp[c] + s.h_samp[0] - 1) / s.h_samp[0];
            d.ch[c] = (s.height * s.v_samp[c] + s.v_samp[0] - 1) / s.v_samp[0];
            d.bpm += s.h_samp[c] * s.v_samp[c];
        }
        d.mcus_w = s.mcus_w;
        d.mcus = s.mcus_w * s.mcus_h;
        d.dri = s.restart_interval;
        d.segments = (int)s.segments;
        d.blocks = blocks;
        if (s.scan_capacity <= DEVICE_CAPACITY_MAX) {      // (else stage 2 refuses the batch; stage 1 does not read these)
            const WsLayout w = ws_layout(s.blocks, s.segments);
            d.ws_bits = s.ws_base + w.bits;
            d.ws_seg = s.ws_base + w.seg;
            d.ws_ff = s.ws_base + w.ff;
            d.ws_stream = s.ws_base + w.stream;
            d.chunks_bound = (int)chunks_bound(s.blocks, s.segments);
            d.stream_vec_bound = (int)(stream_bound(s.blocks, s.segments) / 16);
        }
        tab[i] = d;
    }
    return PPY_OK;
}

#ifndef PPY_JPEG_HOST_ONLY
namespace {

__device__ __forceinline__ const EncCommon &enc_common(const unsigned char *table) { return *reinterpret_cast<const EncCommon *>(table); }
__device__ __forceinline__ const EncDev &enc_dev(const unsigned char *table, int i) {
    return reinterpret_cast<const EncDev *>(table + sizeof(EncCommon))[i];
}

// ---- stage 1 ---------------------------------------------------------------------------------------------------------
// jccolor.c: 16-bit fixed point; Y rounds with ONE_HALF, Cb and Cr carry (128 << 16) + ONE_HALF - 1.
__device__ __forceinline__ int ycc_component(int c, int b, int g, int r) {
    if (c == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (c == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}
__device__ __forceinline__ int enc_pixel(const EncDev &d, int c, int y, int x) {
    const unsigned char *p = d.src + (long long)y * d.row_stride + (long long)x * d.ncomp;
    if (d.ncomp == 1) return p[0];
    return ycc_component(c, p[0], p[1], p[2]);
}

// One pass of jfdctint.c's jpeg_fdct_islow over 8 values (CONST_BITS 13, PASS1_BITS 2).  first: the row pass (outputs scaled
// up by 4); else the column pass (scaled down again, leaving the factor 8 the quantiser removes).  No intermediate leaves
// int32: |input| <= 128 in pass 1 and <= 2^13 in pass 2, the largest multiplier is 25172 < 2^15, at most 4 terms are summed.
__device__ __forceinline__ void fdct_pass(const int d[8], int o[8], bool first) {
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int sh = first ? 11 : 15, r = 1 << (sh - 1);
    if (first) {
        o[0] = (t10 + t11) << 2;
        o[4] = (t10 - t11) << 2;
    } else {
        o[0] = (t10 + t11 + 2) >> 2;
        o[4] = (t10 - t11 + 2) >> 2;
    }
    int z1 = (t12 + t13) * 4433;
    o[2] = (z1 + t13 * 6270 + r) >> sh;
    o[6] = (z1 - t12 * 15137 + r) >> sh;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    o[7] = (a4 + z1 + z3 + r) >> sh;
    o[5] = (a5 + z2 + z4 + r) >> sh;
    o[3] = (a6 + z2 + z3 + r) >> sh;
    o[1] = (a7 + z1 + z4 + r) >> sh;
}

// jcdctmgr.c: (|v| + d / 2) / d with the sign put back, d = 8 * q.  The division is a multiply-high by m = floor(2^32 / d) + 1
// = (2^32 + e) / d with 0 < e <= d: n * m / 2^32 = n / d + n * e / (d * 2^32), whose floor is floor(n / d) while n * e < 2^32;
// n = |v| + d / 2 < 2^15 and e <= d <= 2040.
__device__ __forceinline__ int quantise(int v, u32 recip, u32 half) {
    const u32 a = (u32)(v < 0 ? -v : v) + half;
    const int q = (int)__umulhi(a, recip);
    return v < 0 ? -q : q;
}

// 32 blocks per workgroup, 8 lanes per block.  Lane r fetches row r of the block's samples (colour conversion, edge
// replication and the box filter happen in the fetch) and runs the row pass; the block is transposed through LDS; lane k runs
// the column pass on column k, quantises and stores its 8 coefficients -- horizontal frequency k, the vertical ones in turn,
// which IS the stored (transposed) order -- with one 16-byte store.  Workgroup tile: 32 blocks of the image's block list
// (component after component); the last workgroup of an image is partly idle.
__global__ __launch_bounds__(256) void jpeg_enc_fdct_kernel(const unsigned char *__restrict__ table, int16_t *__restrict__ coef) {
    __shared__ int lds[32][8][9];
    const EncCommon &C = enc_common(table);
    const EncDev &d = enc_dev(table, blockIdx.z);
    const int total = d.blk_end[d.ncomp - 1];
    if ((int)blockIdx.x * 32 >= total) return;                      // uniform over the workgroup
    const int lane = threadIdx.x & 7, slot = threadIdx.x >> 3;
    const int b = blockIdx.x * 32 + slot;
    const bool live = b < total;
    int c = 0, first = 0, bi = 0;
    bool dummy = false;
    if (live) {
        if (d.ncomp == 3 && b >= d.blk_end[0]) {
            c = b >= d.blk_end[1] ? 2 : 1;
            first = d.blk_end[c - 1];
        }
        bi = b - first;
        const int by = bi / d.bw[c], bx = bi - by * d.bw[c];
        // A dummy block (outside the real blocks; the MCU grid is larger) has no AC and the DC of the block before it in its
        // MCU's block order (jccoefct.c): compute that block again.  The first block of an MCU is always real.
        int sby = by, sbx = bx;
        dummy = by >= d.rh[c] || bx >= d.rw[c];
        if (dummy) {
            const int hs = d.hs[c], ly = by % d.vs[c], lx = bx % hs;
            for (int j = ly * hs + lx - 1; j >= 0; --j) {
                const int y = by - ly + j / hs, x = bx - lx + j % hs;
                if (y < d.rh[c] && x < d.rw[c]) {
                    sby = y;
                    sbx = x;
                    break;
                }
            }
        }
        // fh x fv full-resolution pixels under one sample.  To the right the PIXELS replicate (the filter runs over copies of
        // the edge pixel); downwards the pixels replicate up to a whole row group and below that the SAMPLE rows do.
        const int fh = d.hs[0] / d.hs[c], fv = d.vs[0] / d.vs[c];
        int sy = sby * 8 + lane;
        sy = sy < d.ch[c] ? sy : d.ch[c] - 1;
        const int y0 = sy * fv, y1 = y0 + fv - 1 < d.H ? y0 + fv - 1 : d.H - 1;
        int in[8], out[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int sx = sbx * 8 + k;
            const int x0 = sx * fh < d.W ? sx * fh : d.W - 1, x1 = sx * fh + fh - 1 < d.W ? sx * fh + fh - 1 : d.W - 1;
            int v;
            if (fh == 1) v = enc_pixel(d, c, y0, x0);
            else if (fv == 1) v = (enc_pixel(d, c, y0, x0) + enc_pixel(d, c, y0, x1) + (sx & 1)) >> 1;
            else v = (enc_pixel(d, c, y0, x0) + enc_pixel(d, c, y0, x1) + enc_pixel(d, c, y1, x0) + enc_pixel(d, c, y1, x1) + 1 + (sx & 1)) >> 2;
            in[k] = v - 128;
        }
        fdct_pass(in, out, true);
#pragma unroll
        for (int k = 0; k < 8; ++k) lds[slot][lane][k] = out[k];
    }
    __syncthreads();
    if (live) {
        int in[8], out[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = lds[slot][r][lane];
        fdct_pass(in, out, false);
        const int t = c ? 1 : 0;
        u32 w[4];
#pragma unroll
        for (int u = 0; u < 8; u += 2) {
            int lo = quantise(out[u], C.recip[t][lane * 8 + u], C.half[t][lane * 8 + u]);
            int hi = quantise(out[u + 1], C.recip[t][lane * 8 + u + 1], C.half[t][lane * 8 + u + 1]);
            if (dummy) {
                hi = 0;
                if (u || lane) lo = 0;
            }
            w[u >> 1] = ((u32)lo & 0xFFFFu) | (u32)hi << 16;
        }
        uintx4 v = {w[0], w[1], w[2], w[3]};
        *reinterpret_cast<uintx4 *>(coef + d.coef_off[c] + (long long)bi * 64 + lane * 8) = v;
    }
}

// ---- stage 2 ---------------------------------------------------------------------------------------------------------
// zigzag position -> index inside a stored (transposed) block
__device__ const unsigned char ZZ_STORED[64] = {0, 8, 1, 2, 9, 16, 24, 17, 10, 3, 4, 11, 18, 25, 32, 40, 33, 26, 19, 12, 5, 6, 13, 20, 27, 34, 41, 48, 56, 49, 42, 35,
                                                28, 21, 14, 7, 15, 22, 29, 36, 43, 50, 57, 58, 51, 44, 37, 30, 23, 31, 38, 45, 52, 59, 60, 53, 46, 39, 47, 54, 61, 62, 55, 63};

// Where block s of an image's scan order (MCU after MCU; inside an MCU component after component, rows of blocks in turn)
// lies, and what precedes it.
struct ScanBlock {
    int c, by, bx, mcu, j;      // j: index inside the MCU
    bool seg_first, seg_last;   // first / last block of its restart segment
};
__device__ __forceinline__ ScanBlock scan_block(const EncDev &d, int s) {
    ScanBlock b;
    b.mcu = s / d.bpm;
    b.j = s - b.mcu * d.bpm;
    const int nl = d.hs[0] * d.vs[0];
    int jc = b.j;
    b.c = 0;
    if (b.j >= nl) {
        b.c = 1 + b.j - nl;
        jc = 0;
    }
    const int my = b.mcu / d.mcus_w, mx = b.mcu - my * d.mcus_w;
    const int hs = d.hs[b.c];
    b.by = my * d.vs[b.c] + jc / hs;
    b.bx = mx * hs + jc % hs;
    const bool mcu_first = d.dri ? b.mcu % d.dri == 0 : b.mcu == 0;
    const bool mcu_last = b.mcu == d.mcus - 1 || (d.dri && (b.mcu + 1) % d.dri == 0);
    b.seg_first = mcu_first && b.j == 0;
    b.seg_last = mcu_last && b.j == d.bpm - 1;
    return b;
}
__device__ __forceinline__ long long block_offset(const EncDev &d, int c, int by, int bx) {
    return d.coef_off[c] + ((long long)by * d.bw[c] + bx) * 64;
}
// The DC prediction of a block: the DC of the component's previous block in scan order, 0 at the start of a restart segment.
__device__ __forceinline__ int dc_prediction(const EncDev &d, const ScanBlock &b, const int16_t *__restrict__ coef) {
    const int hs = d.hs[b.c], vs = d.vs[b.c];
    const int ly = b.by % vs, lx = b.bx % hs;
    if (ly || lx) {
        const int j = ly * hs + lx - 1;
        return coef[block_offset(d, b.c, b.by - ly + j / hs, b.bx - lx + j % hs)];
    }
    if (d.dri ? b.mcu % d.dri == 0 : b.mcu == 0) return 0;
    const int pm = b.mcu - 1, my = pm / d.mcus_w, mx = pm - my * d.mcus_w;
    return coef[block_offset(d, b.c, my * vs + vs - 1, mx * hs + hs - 1)];
}

// Bits go out most significant first; a 32-bit word of the stream is stored byte-swapped, so memory holds the bytes in order.
template <bool WRITE>
struct BitSink {
    u64 acc;
    int n;             // bits waiting in acc (the low n bits)
    u32 count;
    u32 *words;
    u32 word;
    bool shared;       // the next word to leave may hold bits of another block
    __device__ __forceinline__ void put(u32 v, int bits) {
        if (!WRITE) {
            count += bits;
            return;
        }
        acc = acc << bits | v;
        n += bits;
        if (n >= 32) {
            const u32 w = __builtin_bswap32((u32)(acc >> (n - 32)));
            if (shared) atomicOr(words + word, w);
            else words[word] = w;
            shared = false;
            ++word;
            n -= 32;
        }
    }
    __device__ __forceinline__ void finish() {
        if (WRITE && n > 0) atomicOr(words + word, __builtin_bswap32((u32)(acc << (32 - n))));
    }
};

// One block in the order of jchuff.c's encode_one_block.  blk: the block in stored order; a value whose size has no code
// (|DC difference| >= 2048, |AC| >= 1024: stage 1 cannot produce them) is coded as size 11 / 10 of its low bits.
template <bool WRITE>
__device__ __forceinline__ void code_block(const short *blk, int diff, const u32 *dc_code, const u32 *ac_code, BitSink<WRITE> &o) {
    int s = 32 - __clz(diff < 0 ? -diff : diff);
    s = s > 11 ? 11 : s;
    o.put(dc_code[s] & 0xFFFFu, (int)(dc_code[s] >> 16));
    if (s) o.put((u32)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u), s);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int a = blk[ZZ_STORED[k]];
        if (a == 0) {
            ++run;
            continue;
        }
        while (run > 15) {
            o.put(ac_code[0xF0] & 0xFFFFu, (int)(ac_code[0xF0] >> 16));
            run -= 16;
        }
        s = 32 - __clz(a < 0 ? -a : a);
        s = s > 10 ? 10 : s;
        const u32 code = ac_code[run << 4 | s];
        o.put(code & 0xFFFFu, (int)(code >> 16));
        o.put((u32)(a < 0 ? a - 1 : a) & ((1u << s) - 1u), s);
        run = 0;
    }
    if (run) o.put(ac_code[0] & 0xFFFFu, (int)(ac_code[0] >> 16));
}

// 64 consecutive blocks of an image's scan order per workgroup, one lane per block.  The blocks are staged through LDS with
// coalesced 16-byte loads (8 lanes per block), rows 33 words apart so that the lanes' walks hit different banks.
// WRITE = false: bits per block -> ws_bits.  WRITE = true: ws_bits holds the block's bit offset inside its restart segment,
// ws_seg the segments' byte offsets; the bits are OR-ed into the zeroed stream, the segment's last block adds the 1-bit fill.
constexpr int PACK_TILE = 64;
template <bool WRITE>
__global__ __launch_bounds__(PACK_TILE) void jpeg_enc_pack_kernel(const unsigned char *__restrict__ table, const int16_t *__restrict__ coef,
                                                                  unsigned char *__restrict__ ws) {
    __shared__ u32 s_dc[2][16], s_ac[2][256];
    __shared__ u32 s_blk[PACK_TILE][33];
    __shared__ long long s_off[PACK_TILE];
    const EncCommon &C = enc_common(table);
    const EncDev &d = enc_dev(table, blockIdx.y);
    if ((int)blockIdx.x * PACK_TILE >= d.blocks) return;            // uniform over the workgroup
    const int tid = threadIdx.x;
    for (int i = tid; i < 32; i += PACK_TILE) s_dc[i >> 4][i & 15] = C.dc_code[i >> 4][i & 15];
    for (int i = tid; i < 512; i += PACK_TILE) s_ac[i >> 8][i & 255] = C.ac_code[i >> 8][i & 255];
    const int s = blockIdx.x * PACK_TILE + tid;
    const bool live = s < d.blocks;
    ScanBlock b;
    int diff = 0;
    if (live) {
        b = scan_block(d, s);
        const long long off = block_offset(d, b.c, b.by, b.bx);
        s_off[tid] = off;
        diff = coef[off] - dc_prediction(d, b, coef);
    } else {
        s_off[tid] = -1;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int slot = i * 8 + (tid >> 3), part = tid & 7;
        const long long off = s_off[slot];
        if (off >= 0) {
            const uintx4 v = *reinterpret_cast<const uintx4 *>(coef + off + part * 8);
            s_blk[slot][part * 4 + 0] = v[0];
            s_blk[slot][part * 4 + 1] = v[1];
            s_blk[slot][part * 4 + 2] = v[2];
            s_blk[slot][part * 4 + 3] = v[3];
        }
    }
    __syncthreads();
    if (!live) return;
    u32 *bits = reinterpret_cast<u32 *>(ws + d.ws_bits);
    BitSink<WRITE> o;
    o.acc = 0;
    o.n = 0;
    o.count = 0;
    o.words = nullptr;
    o.word = 0;
    o.shared = true;
    u64 pos = 0;
    if (WRITE) {
        const u32 *seg = reinterpret_cast<const u32 *>(ws + d.ws_seg);
        pos = (u64)seg[d.dri ? b.mcu / d.dri : 0] * 8u + bits[s];
        o.words = reinterpret_cast<u32 *>(ws + d.ws_stream);
        o.word = (u32)(pos >> 5);
        o.n = (int)(pos & 31);       // the bits of the word before this block: zeros here, OR-ed in by their owners
    }
    const int t = b.c ? 1 : 0;
    code_block<WRITE>(reinterpret_cast<const short *>(s_blk[tid]), diff, s_dc[t], s_ac[t], o);
    if (!WRITE) {
        bits[s] = o.count;
        return;
    }
    if (b.seg_last) {                // the last byte of a restart segment is filled with 1-bits
        const int fill = (8 - (o.n & 7)) & 7;
        if (fill) o.put((1u << fill) - 1u, fill);
    }
    o.finish();
}

// Inclusive segmented scan over the 1024 values of a workgroup: (flag, value), a set flag starts a new sum.
constexpr int SCAN_THREADS = 1024;
__device__ __forceinline__ void scan_1024(u32 &flag, u32 &value, u32 *s_flag, u32 *s_value) {
    const int tid = threadIdx.x;
    for (int o = 1; o < SCAN_THREADS; o <<= 1) {
        s_flag[tid] = flag;
        s_value[tid] = value;
        __syncthreads();
        if (tid >= o) {
            if (!flag) value += s_value[tid - o];
            flag |= s_flag[tid - o];
        }
        __syncthreads();
    }
}

// One workgroup per image.  ws_bits: bits per block -> the block's bit offset inside its restart segment; ws_seg[k]: byte
// offset of segment k in the unstuffed stream, ws_seg[segments] the stream's size.
__global__ __launch_bounds__(SCAN_THREADS) void jpeg_enc_offsets_kernel(const unsigned char *__restrict__ table, unsigned char *__restrict__ ws) {
    __shared__ u32 s_flag[SCAN_THREADS], s_value[SCAN_THREADS];
    __shared__ u32 s_carry;
    const EncDev &d = enc_dev(table, blockIdx.x);
    u32 *bits = reinterpret_cast<u32 *>(ws + d.ws_bits);
    u32 *seg = reinterpret_cast<u32 *>(ws + d.ws_seg);
    const int tid = threadIdx.x;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base < d.blocks; base += SCAN_THREADS) {
        const int s = base + tid;
        const bool live = s < d.blocks;
        ScanBlock b;
        u32 own = 0, flag = 0;
        if (live) {
            b = scan_block(d, s);
            own = bits[s];
            flag = b.seg_first ? 1u : 0u;
        }
        u32 f = flag, v = own;
        scan_1024(f, v, s_flag, s_value);
        const u32 carry = s_carry;
        const u32 incl = f ? v : v + carry;       // bits of the segment up to and including this block
        if (live) {
            bits[s] = incl - own;
            if (b.seg_last) seg[d.dri ? b.mcu / d.dri : 0] = (incl + 7u) >> 3;       // the segment's bytes, for now
        }
        __syncthreads();
        if (tid == SCAN_THREADS - 1) s_carry = incl;
        __syncthreads();
    }
    if (tid == 0) s_carry = 0;
    __syncthreads();                               // (also: the segment sizes written above are visible to the workgroup)
    for (int base = 0; base < d.segments; base += SCAN_THREADS) {
        const int k = base + tid;
        const u32 own = k < d.segments ? seg[k] : 0u;
        u32 f = 0, v = own;
        scan_1024(f, v, s_flag, s_value);
        const u32 carry = s_carry;
        if (k < d.segments) seg[k] = carry + v - own;
        __syncthreads();
        if (tid == SCAN_THREADS - 1) s_carry = carry + v;
        __syncthreads();
    }
    if (tid == 0) seg[d.segments] = s_carry;
}

// Zero the unstuffed stream: every whole 64-byte chunk its size touches, which is all the later kernels read or OR into.
__global__ __launch_bounds__(256) void jpeg_enc_zero_kernel(const unsigned char *__restrict__ table, unsigned char *__restrict__ ws) {
    const EncDev &d = enc_dev(table, blockIdx.y);
    const u32 total = reinterpret_cast<const u32 *>(ws + d.ws_seg)[d.segments];
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (u32)d.stream_vec_bound || i >= (total + 63u) / 64u * 4u) return;
    const uintx4 z = {0u, 0u, 0u, 0u};
    reinterpret_cast<uintx4 *>(ws + d.ws_stream)[i] = z;
}

// 0xFF bytes per 64-byte chunk of the unstuffed stream.
__global__ __launch_bounds__(256) void jpeg_enc_ffcount_kernel(const unsigned char *__restrict__ table, unsigned char *__restrict__ ws) {
    const EncDev &d = enc_dev(table, blockIdx.y);
    const u32 total = reinterpret_cast<const u32 *>(ws + d.ws_seg)[d.segments];
    const u32 ck = blockIdx.x * 256u + threadIdx.x;
    if (ck >= (u32)d.chunks_bound || ck * 64u >= total) return;
    const uintx4 *p = reinterpret_cast<const uintx4 *>(ws + d.ws_stream) + ck * 4u;
    const u32 end = total - ck * 64u < 64u ? total - ck * 64u : 64u;
    u32 n = 0;
    for (u32 i = 0; i < 4; ++i) {
        const uintx4 v = p[i];
        for (u32 j = 0; j < 16; ++j)
            if (i * 16 + j < end && ((v[j >> 2] >> ((j & 3) * 8)) & 0xFFu) == 0xFFu) ++n;
    }
    reinterpret_cast<u32 *>(ws + d.ws_ff)[ck] = n;
}

// One workgroup per image: exclusive prefix sum of the chunks' 0xFF counts, and the image's length.
__global__ __launch_bounds__(SCAN_THREADS) void jpeg_enc_length_kernel(const unsigned char *__restrict__ table, unsigned char *__restrict__ ws,
                                                                       u64 *__restrict__ lengths) {
    __shared__ u32 s_flag[SCAN_THREADS], s_value[SCAN_THREADS];
    __shared__ u32 s_carry;
    const EncDev &d = enc_dev(table, blockIdx.x);
    const u32 total = reinterpret_cast<const u32 *>(ws + d.ws_seg)[d.segments];
    const u32 chunks = (total + 63u) / 64u;
    u32 *ff = reinterpret_cast<u32 *>(ws + d.ws_ff);
    const int tid = threadIdx.x;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (u32 base = 0; base < chunks; base += SCAN_THREADS) {
        const u32 k = base + tid;
        const u32 own = k < chunks ? ff[k] : 0u;
        u32 f = 0, v = own;
        scan_1024(f, v, s_flag, s_value);
        const u32 carry = s_carry;
        if (k < chunks) ff[k] = carry + v - own;
        __syncthreads();
        if (tid == SCAN_THREADS - 1) s_carry = carry + v;
        __syncthreads();
    }
    if (tid == 0) lengths[blockIdx.x] = (u64)total + s_carry + 2ull * (u64)(d.segments - 1);
}

// One workgroup: out_off[i] = sum of the lengths before image i (the images lie back to back in `out`).
__global__ __launch_bounds__(SCAN_THREADS) void jpeg_enc_place_kernel(int n, const u64 *__restrict__ lengths, u64 *__restrict__ out_off) {
    __shared__ u64 s_value[SCAN_THREADS];
    __shared__ u64 s_carry;
    const int tid = threadIdx.x;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += SCAN_THREADS) {
        const int k = base + tid;
        const u64 own = k < n ? lengths[k] : 0ull;
        u64 v = own;
        for (int o = 1; o < SCAN_THREADS; o <<= 1) {
            s_value[tid] = v;
            __syncthreads();
            if (tid >= o) v += s_value[tid - o];
            __syncthreads();
        }
        const u64 carry = s_carry;
        if (k < n) out_off[k] = carry + v - own;
        __syncthreads();
        if (tid == SCAN_THREADS - 1) s_carry = carry + v;
        __syncthreads();
    }
}

// One lane per 64-byte chunk of the unstuffed stream: its bytes with a 00 after every FF, and the RSTn marker in front of
// every restart segment that starts in the chunk.  Byte p of segment k lands at p + (FFs before p) + 2 k.
__global__ __launch_bounds__(256) void jpeg_enc_stuff_kernel(const unsigned char *__restrict__ table, const unsigned char *__restrict__ ws,
                                                             const u64 *__restrict__ out_off, unsigned char *__restrict__ out) {
    const EncDev &d = enc_dev(table, blockIdx.y);
    const u32 *seg = reinterpret_cast<const u32 *>(ws + d.ws_seg);
    const u32 total = seg[d.segments];
    const u32 ck = blockIdx.x * 256u + threadIdx.x;
    if (ck >= (u32)d.chunks_bound || ck * 64u >= total) return;
    const u32 start = ck * 64u, end = total - start < 64u ? total : start + 64u;
    int lo = 0, hi = d.segments - 1;       // the last segment that starts at or before `start`
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[mid] <= start) lo = mid;
        else hi = mid - 1;
    }
    int k = lo;
    unsigned char *o = out + out_off[blockIdx.y] + start + reinterpret_cast<const u32 *>(ws + d.ws_ff)[ck] + 2ull * (u64)k;
    if (k > 0 && seg[k] == start) {        // the segment starts with this chunk: its marker is ours
        o[-2] = 0xFF;
        o[-1] = (unsigned char)(0xD0 + ((k - 1) & 7));
    }
    u32 next = seg[k + 1];
    const u32 *src = reinterpret_cast<const u32 *>(ws + d.ws_stream) + ck * 16u;
    for (u32 p = start; p < end; ++p) {
        if (p == next) {
            ++k;
            *o++ = 0xFF;
            *o++ = (unsigned char)(0xD0 + ((k - 1) & 7));
            next = seg[k + 1];
        }
        const u32 i = p - start;
        const u32 byte = (src[i >> 2] >> ((i & 3) * 8)) & 0xFFu;
        *o++ = (unsigned char)byte;
        if (byte == 0xFFu) *o++ = 0;
    }
}

int batch_check(int n, const ppy_jpeg_enc_desc_t *h_descs, size_t coef_bytes) {
    for (int i = 0; i < n; ++i) {
        const ppy_jpeg_enc_desc_t &s = h_descs[i];
        PPY_CHECK_ARG(desc_ok(s) && (unsigned long long)s.coef_base + (unsigned long long)s.coef_bytes <= coef_bytes);
    }
    return PPY_OK;
}

}  // namespace

extern "C" int ppy_jpeg_enc_coefficients(int n, const ppy_jpeg_enc_desc_t *h_descs, const void *table, int16_t *coef, size_t coef_bytes,
                                         void *stream) {
    ppy_drop_stale_error();
    PPY_CHECK_ARG(n > 0 && n <= 65535 && h_descs && table && coef && ((uintptr_t)table & 15) == 0 && ((uintptr_t)coef & 15) == 0);
    const int rc = batch_check(n, h_descs, coef_bytes);
    if (rc != PPY_OK) return rc;
    long long max_blocks = 0;
    for (int i = 0; i < n; ++i) max_blocks = h_descs[i].blocks > max_blocks ? h_descs[i].blocks : max_blocks;
    PPY_CHECK_ARG(max_blocks <= (1ll << 30));
    hipLaunchKernelGGL(jpeg_enc_fdct_kernel, dim3((unsigned)((max_blocks + 31) / 32), 1, n), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char *)table, coef);
    return ppy_launch_status();
}

extern "C" int ppy_jpeg_enc_scan_device(int n, const ppy_jpeg_enc_desc_t *h_descs, const void *table, const int16_t *coef, size_t coef_bytes,
                                        unsigned char *out, size_t out_bytes, unsigned long long *lengths, void *ws, size_t ws_bytes,
                                        void *stream) {
    ppy_drop_stale_error();
    PPY_CHECK_ARG(n > 0 && n <= 65535 && h_descs && table && coef && out && lengths && ((uintptr_t)table & 15) == 0 &&
                  ((uintptr_t)coef & 15) == 0 && ((uintptr_t)lengths & 7) == 0);
    const int rc = batch_check(n, h_descs, coef_bytes);
    if (rc != PPY_OK) return rc;
    long long need_ws = 0, need_out = 0, max_blocks = 0, max_chunks = 0, max_vec = 0;
    for (int i = 0; i < n; ++i) {
        const ppy_jpeg_enc_desc_t &s = h_descs[i];
        if (s.scan_capacity > DEVICE_CAPACITY_MAX) return PPY_ERR_UNSUPPORTED;
        PPY_CHECK_ARG(s.ws_base >= need_ws);                       // the images' workspaces do not overlap, in table order
        need_ws = s.ws_base + align16(s.ws_bytes);
        need_out += s.scan_capacity;
        max_blocks = s.blocks > max_blocks ? s.blocks : max_blocks;
        const long long ch = chunks_bound(s.blocks, s.segments), vec = stream_bound(s.blocks, s.segments) / 16;
        max_chunks = ch > max_chunks ? ch : max_chunks;
        max_vec = vec > max_vec ? vec : max_vec;
    }
    const long long off_bytes = need_ws;                           // out_off: n u64 after the images' workspaces
    need_ws += 16 * (long long)n + 16;
    if (ws == nullptr || ws_bytes < (size_t)need_ws || ((uintptr_t)ws & 15) != 0) return PPY_ERR_WORKSPACE;
    if (out_bytes < (size_t)need_out) return PPY_ERR_WORKSPACE;
    const unsigned char *tab = (const unsigned char *)table;
    unsigned char *w = (unsigned char *)ws;
    u64 *out_off = reinterpret_cast<u64 *>(w + off_bytes);
    hipStream_t st = (hipStream_t)stream;
    const dim3 pack_grid((unsigned)((max_blocks + PACK_TILE - 1) / PACK_TILE), n), chunk_grid((unsigned)((max_chunks + 255) / 256), n);
    hipLaunchKernelGGL(jpeg_enc_pack_kernel<false>, pack_grid, dim3(PACK_TILE), 0, st, tab, coef, w);
    hipLaunchKernelGGL(jpeg_enc_offsets_kernel, dim3(n), dim3(SCAN_THREADS), 0, st, tab, w);
    hipLaunchKernelGGL(jpeg_enc_zero_kernel, dim3((unsigned)((max_vec + 255) / 256), n), dim3(256), 0, st, tab, w);
    hipLaunchKernelGGL(jpeg_enc_pack_kernel<true>, pack_grid, dim3(PACK_TILE), 0, st, tab, coef, w);
    hipLaunchKernelGGL(jpeg_enc_ffcount_kernel, chunk_grid, dim3(256), 0, st, tab, w);
    hipLaunchKernelGGL(jpeg_enc_length_kernel, dim3(n), dim3(SCAN_THREADS), 0, st, tab, w, (u64 *)lengths);
    hipLaunchKernelGGL(jpeg_enc_place_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, n, (const u64 *)lengths, out_off);
    hipLaunchKernelGGL(jpeg_enc_stuff_kernel, chunk_grid, dim3(256), 0, st, tab, (const unsigned char *)w, (const u64 *)out_off, out);
    return ppy_launch_status();
}
#endif  // PPY_JPEG_HOST_ONLY
