// Baseline JPEG decoding with libjpeg-turbo's defaults (what cv2.imread / cv2.imdecode(buf, 1) run; reference demo.py:41,
// tools/cocotools.py:105, tools/transform.py:87): JDCT_ISLOW inverse DCT, fancy chroma upsampling, integer YCbCr tables, EXIF
// orientation.  Bit for bit with it wherever a block's inverse DCT stays in [-512, 511] before the range-limit table, which
// every encoder's output does.  Beyond that range this follows libjpeg's C code (the table wraps) where libjpeg-turbo's SIMD
// code saturates, and where an int32 intermediate overflows it wraps at 32 bits where libjpeg's JLONG has 64.  DESIGN.md
// section 10 is the numerics contract with the three zones; tests/jpeg_ref.py restates it in numpy.
//
// Host part (plain C++, no GPU call, no global state => one call per image on any thread): marker parsing and Huffman
// decoding into int16 coefficient blocks.  Device part: two launches per BATCH, whatever the number and sizes of the images --
//   jpeg_idct_kernel    dequantise + 8x8 inverse DCT, 8 lanes per block, into block-padded component planes (workspace);
//   jpeg_colour_kernel  upsample + YCbCr -> BGR + orientation + store into the caller's HWC tensors.
// The per-image descriptors travel as a table in device memory (packed on the host, copied with the coefficients), like the
// blob of augment.hip.  The opt-in device entropy mode fills the same coefficient buffer on the GPU (jpeg_entropy.hip); its
// host part, one linear pass per file that writes a scan record (jpeg_scan.h), is ppy_jpeg_scan_prepare below.
#include <string.h>

#include <cstdio>

#ifndef PPY_JPEG_HOST_ONLY
#include "common.h"
#else      // the host stage alone as plain C++ (tools/jpeg_host_asan.cpp: AddressSanitizer build, no HIP headers)
#include <stddef.h>
#include <stdint.h>

#include "../../../include/ppyolo_hip.h"
#define PPY_CHECK_ARG(cond) \
    do {                    \
        if (!(cond)) return PPY_ERR_BAD_ARG; \
    } while (0)
#endif
#include "jpeg_scan.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- host
const unsigned char ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                  41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                  30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Coefficients and quantisation tables are stored TRANSPOSED inside a block (index col * 8 + row): the column pass of the
// inverse DCT comes first, and a lane then reads its whole column with one 16-byte load.
inline int stored_index(int zz) { return (ZIGZAG[zz] & 7) * 8 + (ZIGZAG[zz] >> 3); }

struct HuffTab {
    bool defined;
    unsigned char look_len[512], look_sym[512];      // 9-bit lookahead
    int maxcode[18], valoff[18];
    unsigned char vals[256];
};

struct Parsed {
    int W, H, ncomp, orientation, dri;
    int id[3], h[3], v[3], tq[3], td[3], ta[3];
    int hmax, vmax, mcux, mcuy;
    int bw[3], bh[3];
    long long coef_off[3], coef_elems;
    bool qdef[4];
    unsigned short q[4][64];                         // zigzag order, as in the file
    HuffTab dc[4], ac[4];
    size_t data;                                     // offset of the entropy-coded data
    bool full, progressive;                          // read by the scan loop (decode_full), which latches the tables in ql
    unsigned short ql[3][64];                        // per component: the table in force when its first scan started
};

struct Fail {
    int code;
    char reason[64];
};
int fail(Fail &f, int code, const char *why) {
    f.code = code;
    snprintf(f.reason, sizeof(f.reason), "%s", why);
    return code;
}

bool build_huff(HuffTab &t, const unsigned char *cnt, const unsigned char *vals, int total) {
    memset(&t, 0, sizeof(t));
    memcpy(t.vals, vals, total);
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        t.valoff[l] = k - code;
        for (int i = 0; i < cnt[l - 1]; ++i, ++k, ++code) {
            if (code >= (1 << l)) return false;
            if (l <= 9) {
                const int lo = code << (9 - l);
                for (int j = 0; j < (1 << (9 - l)); ++j) {
                    t.look_len[lo + j] = (unsigned char)l;
                    t.look_sym[lo + j] = vals[k];
                }
            }
        }
        t.maxcode[l] = cnt[l - 1] ? code - 1 : -1;
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    t.defined = true;
    return true;
}

int exif_orientation(const unsigned char *s, size_t n) {      // payload of an APP1 segment
    if (n < 14 || memcmp(s, "Exif\0\0", 6) != 0) return 1;
    const unsigned char *t = s + 6;
    n -= 6;
    bool be;
    if (t[0] == 'I' && t[1] == 'I') be = false;
    else if (t[0] == 'M' && t[1] == 'M') be = true;
    else return 1;
    auto u16 = [&](size_t p) { return be ? (unsigned)(t[p] << 8 | t[p + 1]) : (unsigned)(t[p + 1] << 8 | t[p]); };
    auto u32 = [&](size_t p) { return be ? (u16(p) << 16 | u16(p + 2)) : (u16(p + 2) << 16 | u16(p)); };
    if (u16(2) != 42) return 1;
    const size_t off = u32(4);
    if (off > n || off + 2 > n) return 1;
    const unsigned cnt = u16(off);
    for (unsigned k = 0; k < cnt; ++k) {
        const size_t p = off + 2 + 12 * (size_t)k;
        if (p + 12 > n) return 1;
        if (u16(p) == 0x0112) {
            const unsigned v = u16(p + 8);
            return (u16(p + 2) == 3 && u32(p + 4) == 1 && v >= 1 && v <= 8) ? (int)v : 1;
        }
    }
    return 1;
}

struct Markers {      // what the segments before a scan leave behind, besides the tables in Parsed
    bool sof, jfif, have_orient;
    int adobe;
};

// The SOF segment of a Huffman-coded DCT frame (SOF0, SOF1, SOF2): payload s of sl bytes.
int frame_segment(const unsigned char *s, size_t sl, Parsed &P, Markers &M, Fail &f) {
    if (M.sof || sl < 6) return fail(f, PPY_ERR_CORRUPT, "bad SOF segment");
    const int prec = s[0], nc = s[5];
    P.H = s[1] << 8 | s[2];
    P.W = s[3] << 8 | s[4];
    if (sl < 6 + 3 * (size_t)nc) return fail(f, PPY_ERR_CORRUPT, "bad SOF segment");
    if (prec != 8) return fail(f, PPY_ERR_UNSUPPORTED, "sample precision other than 8 bits");
    if (P.H == 0 || P.W == 0) return fail(f, PPY_ERR_UNSUPPORTED, "zero image size (DNL)");
    if (nc != 1 && nc != 3) return fail(f, PPY_ERR_UNSUPPORTED, "component count other than 1 or 3");
    P.ncomp = nc;
    for (int k = 0; k < nc; ++k) {
        P.id[k] = s[6 + 3 * k];
        P.h[k] = s[7 + 3 * k] >> 4;
        P.v[k] = s[7 + 3 * k] & 15;
        P.tq[k] = s[8 + 3 * k];
    }
    M.sof = true;
    return PPY_OK;
}

// Every segment but SOF0-2 and SOS: the tables (DQT, DHT, DRI; they hold for whatever scan follows), the APPn segments that
// are read, the frame types that are refused.  Anything else is skipped.
int table_segment(int m, const unsigned char *s, size_t sl, Parsed &P, Markers &M, Fail &f) {
    if (m == 0xDB) {
        size_t j = 0;
        while (j < sl) {
            const int pq = s[j] >> 4, tq = s[j] & 15;
            ++j;
            if (pq > 1 || tq > 3 || j + 64 * (size_t)(pq + 1) > sl) return fail(f, PPY_ERR_CORRUPT, "bad DQT segment");
            for (int k = 0; k < 64; ++k) P.q[tq][k] = pq ? (unsigned short)(s[j + 2 * k] << 8 | s[j + 2 * k + 1]) : s[j + k];
            P.qdef[tq] = true;
            j += 64 * (size_t)(pq + 1);
        }
    } else if (m >= 0xC9 && m <= 0xCF) {      // SOF9-15 and DAC
        return fail(f, PPY_ERR_UNSUPPORTED, "arithmetic coding");
    } else if (m == 0xC3 || (m >= 0xC5 && m <= 0xC7)) {
        return fail(f, PPY_ERR_UNSUPPORTED, "lossless or hierarchical JPEG");
    } else if (m == 0xC4) {
        size_t j = 0;
        while (j < sl) {
            if (j + 17 > sl) return fail(f, PPY_ERR_CORRUPT, "bad DHT segment");
            const int tc = s[j] >> 4, th = s[j] & 15;
            int total = 0;
            for (int k = 0; k < 16; ++k) total += s[j + 1 + k];
            if (tc > 1 || th > 3 || total > 256 || j + 17 + (size_t)total > sl) return fail(f, PPY_ERR_CORRUPT, "bad DHT segment");
            if (!build_huff(tc ? P.ac[th] : P.dc[th], s + j + 1, s + j + 17, total))
                return fail(f, PPY_ERR_CORRUPT, "bad Huffman table");
            j += 17 + (size_t)total;
        }
    } else if (m == 0xDD) {
        if (sl < 2) return fail(f, PPY_ERR_CORRUPT, "bad DRI segment");
        P.dri = s[0] << 8 | s[1];
    } else if (m == 0xE0 && sl >= 5 && memcmp(s, "JFIF\0", 5) == 0) {
        M.jfif = true;
    } else if (m == 0xE1 && !M.have_orient && sl >= 6 && memcmp(s, "Exif\0\0", 6) == 0) {
        P.orientation = exif_orientation(s, sl);
        M.have_orient = true;
    } else if (m == 0xEE && sl >= 12 && memcmp(s, "Adobe", 5) == 0) {
        M.adobe = s[11];
    }
    return PPY_OK;
}

bool rgb_file(const Parsed &P, const Markers &M) {
    return M.adobe == 0 || (M.adobe < 0 && !M.jfif && P.id[0] == 'R' && P.id[1] == 'G' && P.id[2] == 'B');
}

void frame_geometry(Parsed &P) {      // from the sampling factors: MCU counts and the layout of the coefficient buffer
    P.hmax = P.h[0];
    P.vmax = P.v[0];
    P.mcux = (P.W + 8 * P.hmax - 1) / (8 * P.hmax);
    P.mcuy = (P.H + 8 * P.vmax - 1) / (8 * P.vmax);
    long long off = 0;
    for (int k = 0; k < P.ncomp; ++k) {
        P.bw[k] = P.mcux * P.h[k];
        P.bh[k] = P.mcuy * P.v[k];
        P.coef_off[k] = off;
        off += (long long)P.bw[k] * P.bh[k] * 64;
    }
    P.coef_elems = off;
}

// Markers up to and including SOS.  Every read is bounds-checked against n.
int parse(const unsigned char *d, size_t n, Parsed &P, Fail &f) {
    memset(&P, 0, sizeof(P));
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return fail(f, PPY_ERR_CORRUPT, "no SOI marker");
    size_t i = 2;
    Markers M = {false, false, false, -1};
    P.orientation = 1;
    for (;;) {
        if (i + 2 > n || d[i] != 0xFF) return fail(f, PPY_ERR_CORRUPT, "marker expected");
        const int m = d[i + 1];
        i += 2;
        if (m == 0xFF) {      // fill byte
            i -= 1;
            continue;
        }
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (m == 0xD9 || m == 0xD8 || m == 0) return fail(f, PPY_ERR_CORRUPT, "unexpected marker before the scan");
        if (i + 2 > n) return fail(f, PPY_ERR_CORRUPT, "truncated segment");
        const size_t L = (size_t)d[i] << 8 | d[i + 1];
        if (L < 2 || i + L > n) return fail(f, PPY_ERR_CORRUPT, "truncated segment");
        const unsigned char *s = d + i + 2;
        const size_t sl = L - 2;
        i += L;
        if (m == 0xC0 || m == 0xC1) {
            if (frame_segment(s, sl, P, M, f) != PPY_OK) return f.code;
        } else if (m == 0xC2) {
            return fail(f, PPY_ERR_UNSUPPORTED, "progressive JPEG");
        } else if (m != 0xDA) {
            if (table_segment(m, s, sl, P, M, f) != PPY_OK) return f.code;
        } else {
            if (!M.sof) return fail(f, PPY_ERR_CORRUPT, "SOS before SOF");
            if (sl < 1 || sl < 4 + 2 * (size_t)s[0]) return fail(f, PPY_ERR_CORRUPT, "bad SOS segment");
            if (s[0] != P.ncomp) return fail(f, PPY_ERR_UNSUPPORTED, "multiple scans");
            for (int k = 0; k < P.ncomp; ++k) {
                if (s[1 + 2 * k] != P.id[k]) return fail(f, PPY_ERR_UNSUPPORTED, "scan component order");
                P.td[k] = s[2 + 2 * k] >> 4;
                P.ta[k] = s[2 + 2 * k] & 15;
            }
            if (P.ncomp == 3) {
                if (rgb_file(P, M)) return fail(f, PPY_ERR_UNSUPPORTED, "RGB colour space (Adobe transform 0)");
                const bool luma = (P.h[0] == 1 && P.v[0] == 1) || (P.h[0] == 2 && P.v[0] == 1) || (P.h[0] == 2 && P.v[0] == 2);
                if (P.h[1] != 1 || P.v[1] != 1 || P.h[2] != 1 || P.v[2] != 1 || !luma)
                    return fail(f, PPY_ERR_UNSUPPORTED, "sampling factors other than 4:4:4, 4:2:2, 4:2:0");
            } else {
                if (P.h[0] < 1 || P.h[0] > 4 || P.v[0] < 1 || P.v[0] > 4) return fail(f, PPY_ERR_CORRUPT, "bad sampling factors");
                P.h[0] = P.v[0] = 1;      // a one-component scan is never interleaved
            }
            for (int k = 0; k < P.ncomp; ++k)
                if (P.tq[k] > 3 || !P.qdef[P.tq[k]] || P.td[k] > 3 || P.ta[k] > 3 || !P.dc[P.td[k]].defined || !P.ac[P.ta[k]].defined)
                    return fail(f, PPY_ERR_CORRUPT, "scan refers to a missing table");
            frame_geometry(P);
            P.data = i;
            return PPY_OK;
        }
    }
}

// Bit reader over the entropy-coded data.  It removes the stuffed zero after 0xFF, stops at a marker (or the end of the
// file) and feeds zero bits from there on, counting them: consuming one of those is the "data ends early" error.
struct BitReader {
    const unsigned char *d;
    size_t n, p;
    unsigned long long acc;
    int cnt, phantom;
    bool stopped;
    void reset(size_t at) {
        p = at;
        acc = 0;
        cnt = phantom = 0;
        stopped = false;
    }
    void fill() {
        while (cnt <= 56) {
            unsigned c = 0;
            if (!stopped) {
                if (p >= n) stopped = true;
                else if (d[p] != 0xFF) c = d[p++];
                else if (p + 1 < n && d[p + 1] == 0) {
                    c = 0xFF;
                    p += 2;
                } else stopped = true;
            }
            if (stopped) phantom += 8;
            acc = acc << 8 | c;
            cnt += 8;
        }
    }
    unsigned peek(int k) const { return (unsigned)(acc >> (cnt - k)) & ((1u << k) - 1u); }
    void skip(int k) { cnt -= k; }
    bool overrun() const { return cnt < phantom; }
};

inline int decode_symbol(BitReader &br, const HuffTab &t) {
    const unsigned look = br.peek(9);
    int l = t.look_len[look];
    if (l) {
        br.skip(l);
        return t.look_sym[look];
    }
    for (l = 10; l <= 16; ++l) {
        const int code = (int)br.peek(l);
        if (code <= t.maxcode[l]) {
            const unsigned idx = (unsigned)(code + t.valoff[l]);
            if (idx >= 256) return -1;
            br.skip(l);
            return t.vals[idx];
        }
    }
    return -1;
}

inline int extend(unsigned x, int s) { return x < (1u << (s - 1)) ? (int)x - (1 << s) + 1 : (int)x; }

// One block of a sequential scan; the reason of PPY_ERR_CORRUPT, or nullptr.
inline const char *seq_block(BitReader &br, const HuffTab &dc, const HuffTab &ac, unsigned &pred, int16_t *blk, const int *stored) {
    br.fill();
    const int t = decode_symbol(br, dc);
    if (t < 0 || t > 15) return "bad Huffman code in the entropy data";
    if (t) {
        pred += (unsigned)extend(br.peek(t), t);
        br.skip(t);
    }
    blk[0] = (int16_t)pred;
    for (int k = 1; k < 64;) {
        if (br.cnt < 32) br.fill();
        const int rs = decode_symbol(br, ac);
        if (rs < 0) return "bad Huffman code in the entropy data";
        const int r = rs >> 4, s = rs & 15;
        if (s == 0) {
            if (r != 15) break;
            k += 16;
            continue;
        }
        k += r;
        if (k > 63) return "coefficient index past 63";
        blk[stored[k]] = (int16_t)extend(br.peek(s), s);
        br.skip(s);
        ++k;
    }
    return br.overrun() ? "entropy data ends early" : nullptr;
}

int entropy_decode(const unsigned char *d, size_t n, const Parsed &P, int16_t *coef, Fail &f) {
    BitReader br;
    br.d = d;
    br.n = n;
    br.reset(P.data);
    unsigned pred[3] = {0, 0, 0};
    int stored[64];
    for (int k = 0; k < 64; ++k) stored[k] = stored_index(k);
    long long mcu = 0;
    for (int my = 0; my < P.mcuy; ++my) {
        for (int mx = 0; mx < P.mcux; ++mx, ++mcu) {
            if (P.dri && mcu && mcu % P.dri == 0) {
                if (br.overrun() || br.cnt - br.phantom >= 8) return fail(f, PPY_ERR_CORRUPT, "restart marker expected");
                size_t p = br.p;
                while (p + 1 < n && d[p] == 0xFF && d[p + 1] == 0xFF) ++p;
                if (p + 1 >= n || d[p] != 0xFF || d[p + 1] != 0xD0 + (int)((mcu / P.dri - 1) & 7))
                    return fail(f, PPY_ERR_CORRUPT, "restart marker expected");
                br.reset(p + 2);
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < P.ncomp; ++c) {
                const HuffTab &dc = P.dc[P.td[c]], &ac = P.ac[P.ta[c]];
                for (int v = 0; v < P.v[c]; ++v) {
                    for (int h = 0; h < P.h[c]; ++h) {
                        int16_t *blk = coef + P.coef_off[c] + ((long long)(my * P.v[c] + v) * P.bw[c] + (mx * P.h[c] + h)) * 64;
                        if (const char *why = seq_block(br, dc, ac, pred[c], blk, stored)) return fail(f, PPY_ERR_CORRUPT, why);
                    }
                }
            }
        }
    }
    return PPY_OK;
}

// ------------------------------------------------------------------------------------------- the scan loop (accept != 0)
// Frames whose coefficients arrive in more than one scan -- progressive (jdphuff.c) and sequential multi-scan -- and the
// further luma sampling factors.  The coefficient buffer is the one of the single-scan path; a scan of one component is not
// interleaved and covers the blocks that hold image samples only, so the MCU padding of the buffer stays zero there.
struct Scan {
    int ns, c[3], td[3], ta[3];      // c: component INDEX in the frame
    int ss, se, ah, al;
};

inline const char *dc_first(BitReader &br, const HuffTab &dc, unsigned &pred, int al, int16_t *blk) {
    br.fill();
    const int t = decode_symbol(br, dc);
    if (t < 0 || t > 15) return "bad Huffman code in the entropy data";
    if (t) {
        pred += (unsigned)extend(br.peek(t), t);
        br.skip(t);
    }
    blk[0] = (int16_t)(pred << al);
    return nullptr;
}

inline unsigned one_bit(BitReader &br) {
    if (br.cnt < 32) br.fill();
    const unsigned b = br.peek(1);
    br.skip(1);
    return b;
}

// The run length an EOBn symbol announces, less the block it ends.
inline int eob_run(BitReader &br, int r) {
    int run = 1 << r;
    if (r) {
        if (br.cnt < 32) br.fill();
        run += (int)br.peek(r);
        br.skip(r);
    }
    return run - 1;
}

inline const char *ac_first(BitReader &br, const HuffTab &ac, const Scan &S, int &eobrun, int16_t *blk, const int *stored) {
    if (eobrun > 0) {
        --eobrun;
        return nullptr;
    }
    for (int k = S.ss; k <= S.se; ++k) {
        if (br.cnt < 32) br.fill();
        const int rs = decode_symbol(br, ac);
        if (rs < 0) return "bad Huffman code in the entropy data";
        const int r = rs >> 4, s = rs & 15;
        if (s) {
            k += r;
            if (k > S.se) return "coefficient index past the end of the band";
            blk[stored[k]] = (int16_t)((unsigned)extend(br.peek(s), s) << S.al);
            br.skip(s);
        } else if (r == 15) {
            k += 15;
        } else {
            eobrun = eob_run(br, r);
            break;
        }
    }
    return nullptr;
}

// jdphuff.c decode_mcu_AC_refine: a new coefficient is +-1 << Al and lands after r still-zero positions; every coefficient
// that is already nonzero and is passed on the way takes one correction bit.
inline const char *ac_refine(BitReader &br, const HuffTab &ac, const Scan &S, int &eobrun, int16_t *blk, const int *stored) {
    const int p1 = 1 << S.al, m1 = -p1;
    auto correct = [&](int16_t &co) {
        if (one_bit(br) && (co & p1) == 0) co = (int16_t)(co + (co >= 0 ? p1 : m1));
    };
    int k = S.ss;
    if (eobrun == 0) {
        for (; k <= S.se; ++k) {
            if (br.cnt < 32) br.fill();
            const int rs = decode_symbol(br, ac);
            if (rs < 0) return "bad Huffman code in the entropy data";
            int r = rs >> 4, val = 0;
            const int s = rs & 15;
            if (s) {
                if (s != 1) return "bad value in a refinement scan";
                val = one_bit(br) ? p1 : m1;
            } else if (r != 15) {
                eobrun = eob_run(br, r) + 1;      // this block is still to be finished below
                break;
            }
            do {
                int16_t &co = blk[stored[k]];
                if (co != 0) correct(co);
                else if (--r < 0) break;
                ++k;
            } while (k <= S.se);
            if (val) {
                if (k > S.se) return "coefficient index past the end of the band";
                blk[stored[k]] = (int16_t)val;
            }
        }
    }
    if (eobrun > 0) {
        for (; k <= S.se; ++k)
            if (blk[stored[k]] != 0) correct(blk[stored[k]]);
        --eobrun;
    }
    return nullptr;
}

// The entropy-coded data of one scan, from pos to the marker that ends it (pos on return).
int run_scan(const unsigned char *d, size_t n, const Parsed &P, const Scan &S, int16_t *coef, size_t &pos, Fail &f) {
    BitReader br;
    br.d = d;
    br.n = n;
    br.reset(pos);
    int stored[64];
    for (int k = 0; k < 64; ++k) stored[k] = stored_index(k);
    const bool inter = S.ns > 1;
    const int c0 = S.c[0];
    // units: MCUs of an interleaved scan, otherwise the blocks of the one component that hold image samples
    const int ux = inter ? P.mcux : ((P.W * P.h[c0] + P.hmax - 1) / P.hmax + 7) / 8;
    const int uy = inter ? P.mcuy : ((P.H * P.v[c0] + P.vmax - 1) / P.vmax + 7) / 8;
    const int kind = !P.progressive ? 0 : S.ss == 0 ? (S.ah ? 2 : 1) : (S.ah ? 4 : 3);
    unsigned pred[3] = {0, 0, 0};
    int eobrun = 0;
    long long unit = 0;
    for (int y = 0; y < uy; ++y) {
        for (int x = 0; x < ux; ++x, ++unit) {
            if (P.dri && unit && unit % P.dri == 0) {      // RSTn counts from 0 in every scan
                if (br.overrun() || br.cnt - br.phantom >= 8) return fail(f, PPY_ERR_CORRUPT, "restart marker expected");
                size_t p = br.p;
                while (p + 1 < n && d[p] == 0xFF && d[p + 1] == 0xFF) ++p;
                if (p + 1 >= n || d[p] != 0xFF || d[p + 1] != 0xD0 + (int)((unit / P.dri - 1) & 7))
                    return fail(f, PPY_ERR_CORRUPT, "restart marker expected");
                br.reset(p + 2);
                pred[0] = pred[1] = pred[2] = 0;
                eobrun = 0;
            }
            for (int k = 0; k < S.ns; ++k) {
                const int c = S.c[k], nh = inter ? P.h[c] : 1, nv = inter ? P.v[c] : 1;
                for (int v = 0; v < nv; ++v) {
                    for (int h = 0; h < nh; ++h) {
                        int16_t *blk = coef + P.coef_off[c] + ((long long)(y * nv + v) * P.bw[c] + (x * nh + h)) * 64;
                        const char *why = nullptr;
                        switch (kind) {
                            case 0: why = seq_block(br, P.dc[S.td[k]], P.ac[S.ta[k]], pred[k], blk, stored); break;
                            case 1: why = dc_first(br, P.dc[S.td[k]], pred[k], S.al, blk); break;
                            case 2: if (one_bit(br)) blk[0] = (int16_t)(blk[0] | 1 << S.al); break;
                            case 3: why = ac_first(br, P.ac[S.ta[k]], S, eobrun, blk, stored); break;
                            default: why = ac_refine(br, P.ac[S.ta[k]], S, eobrun, blk, stored); break;
                        }
                        if (!why && br.overrun()) why = "entropy data ends early";
                        if (why) return fail(f, PPY_ERR_CORRUPT, why);
                    }
                }
            }
        }
    }
    pos = br.p;
    return PPY_OK;
}

// The SOS payload -> Scan, checked against the frame, the tables in force and the progression so far (bits: per component
// and coefficient -1 = never sent, else the Al it was last sent with: libjpeg's coef_bits).
int scan_header(const unsigned char *s, size_t sl, unsigned accept, const Parsed &P, const signed char bits[3][64], const bool *latched,
                Scan &S, Fail &f) {
    if (sl < 1 || sl < 4 + 2 * (size_t)s[0]) return fail(f, PPY_ERR_CORRUPT, "bad SOS segment");
    S.ns = s[0];
    if (!P.progressive && !(accept & PPY_JPEG_ACCEPT_MULTISCAN)) {
        if (S.ns != P.ncomp) return fail(f, PPY_ERR_UNSUPPORTED, "multiple scans");
        for (int k = 0; k < P.ncomp; ++k)
            if (s[1 + 2 * k] != P.id[k]) return fail(f, PPY_ERR_UNSUPPORTED, "scan component order");
    }
    if (S.ns < 1 || S.ns > P.ncomp) return fail(f, PPY_ERR_CORRUPT, "bad SOS segment");
    int mcu_blocks = 0;
    for (int k = 0; k < S.ns; ++k) {
        int c = 0;
        while (c < P.ncomp && P.id[c] != s[1 + 2 * k]) ++c;
        if (c == P.ncomp) return fail(f, PPY_ERR_CORRUPT, "scan names an unknown component");
        for (int j = 0; j < k; ++j)
            if (S.c[j] == c) return fail(f, PPY_ERR_CORRUPT, "scan names a component twice");
        S.c[k] = c;
        S.td[k] = s[2 + 2 * k] >> 4;
        S.ta[k] = s[2 + 2 * k] & 15;
        mcu_blocks += P.h[c] * P.v[c];
    }
    if (S.ns > 1 && mcu_blocks > 10) return fail(f, PPY_ERR_CORRUPT, "more than 10 blocks in an MCU");
    const unsigned char *t = s + 1 + 2 * S.ns;
    S.ss = t[0];
    S.se = t[1];
    S.ah = t[2] >> 4;
    S.al = t[2] & 15;
    bool need_dc = true, need_ac = true;
    if (P.progressive) {
        if (S.ss > 63 || S.se > 63 || S.se < S.ss || S.ah > 13 || S.al > 13) return fail(f, PPY_ERR_CORRUPT, "scan parameters out of range");
        if (S.ss == 0 && S.se != 0) return fail(f, PPY_ERR_CORRUPT, "DC scan with Se != 0");
        if (S.ss != 0 && S.ns != 1) return fail(f, PPY_ERR_CORRUPT, "AC scan with more than one component");
        if (S.ah != 0 && S.ah != S.al + 1) return fail(f, PPY_ERR_CORRUPT, "refinement scan with Ah != Al + 1");
        need_dc = S.ss == 0 && S.ah == 0;
        need_ac = S.ss != 0;
    } else {      // a sequential scan carries whole blocks whatever it says
        S.ss = 0;
        S.se = 63;
        S.ah = S.al = 0;
    }
    for (int k = 0; k < S.ns; ++k) {
        const int c = S.c[k];
        if (!latched[c] && (P.tq[c] > 3 || !P.qdef[P.tq[c]]))      // its first scan latches the quantisation table
            return fail(f, PPY_ERR_CORRUPT, "scan refers to a missing table");
        if ((need_dc && (S.td[k] > 3 || !P.dc[S.td[k]].defined)) || (need_ac && (S.ta[k] > 3 || !P.ac[S.ta[k]].defined)))
            return fail(f, PPY_ERR_CORRUPT, "scan refers to a missing table");
        for (int j = S.ss; j <= S.se; ++j) {
            if (!P.progressive && bits[c][j] >= 0) return fail(f, PPY_ERR_CORRUPT, "scan repeats a component");
            if (P.progressive && S.ah != (bits[c][j] < 0 ? 0 : bits[c][j])) return fail(f, PPY_ERR_CORRUPT, "scan out of progression order");
        }
    }
    return PPY_OK;
}

// The whole file under an accept mask.  coef == nullptr: the header pass -- it returns at the first SOS, frame and first
// scan header checked, P filled as parse() fills it.  Otherwise every scan up to EOI is decoded into coef, which the caller
// has zeroed, and the completeness rule is applied.
int decode_full(const unsigned char *d, size_t n, unsigned accept, Parsed &P, int16_t *coef, Fail &f) {
    memset(&P, 0, sizeof(P));
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return fail(f, PPY_ERR_CORRUPT, "no SOI marker");
    size_t i = 2;
    Markers M = {false, false, false, -1};
    P.orientation = 1;
    P.full = true;
    signed char bits[3][64];
    bool latched[3] = {false, false, false};
    memset(bits, -1, sizeof(bits));
    int scans = 0;
    for (;;) {
        if (i + 2 > n || d[i] != 0xFF) return fail(f, PPY_ERR_CORRUPT, scans ? "marker expected after a scan (no EOI)" : "marker expected");
        const int m = d[i + 1];
        i += 2;
        if (m == 0xFF) {      // fill byte
            i -= 1;
            continue;
        }
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (m == 0xD9 && scans) break;
        if (m == 0xD9 || m == 0xD8 || m == 0) return fail(f, PPY_ERR_CORRUPT, scans ? "unexpected marker between scans" : "unexpected marker before the scan");
        if (i + 2 > n) return fail(f, PPY_ERR_CORRUPT, "truncated segment");
        const size_t L = (size_t)d[i] << 8 | d[i + 1];
        if (L < 2 || i + L > n) return fail(f, PPY_ERR_CORRUPT, "truncated segment");
        const unsigned char *s = d + i + 2;
        const size_t sl = L - 2;
        i += L;
        if (m == 0xC0 || m == 0xC1 || m == 0xC2) {
            if (m == 0xC2 && !(accept & PPY_JPEG_ACCEPT_PROGRESSIVE)) return fail(f, PPY_ERR_UNSUPPORTED, "progressive JPEG");
            if (frame_segment(s, sl, P, M, f) != PPY_OK) return f.code;
            P.progressive = m == 0xC2;
        } else if (m != 0xDA) {
            if (table_segment(m, s, sl, P, M, f) != PPY_OK) return f.code;
        } else {
            if (!M.sof) return fail(f, PPY_ERR_CORRUPT, "SOS before SOF");
            if (scans == 0) {      // the frame, judged where parse() judges it
                if (P.ncomp == 3) {
                    if (rgb_file(P, M)) return fail(f, PPY_ERR_UNSUPPORTED, "RGB colour space (Adobe transform 0)");
                    const int h = P.h[0], v = P.v[0];
                    const bool chroma = P.h[1] == 1 && P.v[1] == 1 && P.h[2] == 1 && P.v[2] == 1;
                    if (!(accept & PPY_JPEG_ACCEPT_SAMPLING)) {
                        if (!chroma || !((h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2)))
                            return fail(f, PPY_ERR_UNSUPPORTED, "sampling factors other than 4:4:4, 4:2:2, 4:2:0");
                    } else {
                        if (h < 1 || h > 4 || v < 1 || v > 4) return fail(f, PPY_ERR_CORRUPT, "bad sampling factors");
                        if (!chroma) return fail(f, PPY_ERR_UNSUPPORTED, "chroma sampling factors other than 1x1");
                        if (h * v > 8) return fail(f, PPY_ERR_UNSUPPORTED, "sampling factors with more than 10 blocks in an MCU");
                    }
                } else {
                    if (P.h[0] < 1 || P.h[0] > 4 || P.v[0] < 1 || P.v[0] > 4) return fail(f, PPY_ERR_CORRUPT, "bad sampling factors");
                    P.h[0] = P.v[0] = 1;      // a one-component scan is never interleaved
                }
                frame_geometry(P);
            }
            Scan S;
            if (scan_header(s, sl, accept, P, bits, latched, S, f) != PPY_OK) return f.code;
            if (coef == nullptr) return PPY_OK;
            if (++scans > 256) return fail(f, PPY_ERR_UNSUPPORTED, "more than 256 scans");
            for (int k = 0; k < S.ns; ++k) {
                const int c = S.c[k];
                if (!latched[c]) memcpy(P.ql[c], P.q[P.tq[c]], sizeof(P.ql[c]));
                latched[c] = true;
                for (int j = S.ss; j <= S.se; ++j) bits[c][j] = (signed char)S.al;
            }
            if (run_scan(d, n, P, S, coef, i, f) != PPY_OK) return f.code;
            while (i < n && !(d[i] == 0xFF && i + 1 < n && d[i + 1] != 0 && d[i + 1] != 0xFF)) ++i;      // to the marker
        }
    }
    for (int c = 0; c < P.ncomp; ++c)
        for (int j = 0; j < 64; ++j)
            if (bits[c][j] != 0)
                return P.progressive ? fail(f, PPY_ERR_UNSUPPORTED, "incomplete progressive scan script")
                                     : fail(f, PPY_ERR_CORRUPT, "a component has no scan");
    return PPY_OK;
}

void oriented_size(int W, int H, int orientation, int *ow, int *oh) {
    const bool swap = orientation >= 5 && orientation <= 8;
    *ow = swap ? H : W;
    *oh = swap ? W : H;
}

// ------------------------------------------------------------------------------------------------------------- device
// One image of the batch as the kernels see it.  576 bytes, q 16-byte aligned.
struct JpegDev {
    long long coef_off[3];       // int16 elements into the batch coefficient buffer
    long long plane_off[3];      // bytes into the workspace; plane c is bw[c]*8 bytes wide, bh[c]*8 rows
    unsigned char *out;
    long long row_stride;
    int ncomp, W, H, ow, oh;
    int bw[3], bh[3], blk_end[3];      // blk_end: running block count over the components
    int mode[3], dw[3], dh[3];         // upsampling mode and downsampled size of each component
    int y0, yy, yx, x0, xy, xx;        // source (y, x) of output (oy, ox): y0 + yy*oy + yx*ox, x0 + xy*oy + xx*ox
    int pad[3];
    unsigned short q[3][64];           // quantisation table per component, stored order
};
static_assert(sizeof(JpegDev) == 576 && offsetof(JpegDev, q) % 16 == 0, "JpegDev layout");

// UP_H1V2_FANCY and UP_REPLICATE serve the further luma factors; UP_REPLICATE carries its two factors in the mode word
// (UP_REPLICATE | fx << 8 | fy << 16), so JpegDev keeps its size.
enum { UP_NONE = 0, UP_H2V1_FANCY = 1, UP_H2V2_FANCY = 2, UP_H2V1_BOX = 3, UP_H2V2_BOX = 4, UP_H1V2_FANCY = 5, UP_REPLICATE = 6 };

#ifndef PPY_JPEG_HOST_ONLY
typedef unsigned int u32;

// One pass of jidctint.c's jpeg_idct_islow over 8 values (CONST_BITS 13): the 8 outputs BEFORE the descale.  All
// arithmetic is modulo 2^32 (unsigned), which is int32 with wrap-around.
#define FIX(x) ((u32)(int)(x))
__device__ __forceinline__ void idct_pass(const u32 in[8], u32 out[8]) {
    u32 z1 = (in[2] + in[6]) * FIX(4433);
    const u32 tmp2 = z1 + in[6] * FIX(-15137);
    const u32 tmp3 = z1 + in[2] * FIX(6270);
    const u32 tmp0 = (in[0] + in[4]) << 13;
    const u32 tmp1 = (in[0] - in[4]) << 13;
    const u32 tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    u32 a0 = in[7], a1 = in[5], a2 = in[3], a3 = in[1];
    z1 = a0 + a3;
    u32 z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const u32 z5 = (z3 + z4) * FIX(9633);
    a0 *= FIX(2446);
    a1 *= FIX(16819);
    a2 *= FIX(25172);
    a3 *= FIX(12299);
    z1 *= FIX(-7373);
    z2 *= FIX(-20995);
    z3 = z3 * FIX(-16069) + z5;
    z4 = z4 * FIX(-3196) + z5;
    a0 += z1 + z3;
    a1 += z2 + z4;
    a2 += z2 + z3;
    a3 += z1 + z4;
    out[0] = tmp10 + a3;
    out[7] = tmp10 - a3;
    out[1] = tmp11 + a2;
    out[6] = tmp11 - a2;
    out[2] = tmp12 + a1;
    out[5] = tmp12 - a1;
    out[3] = tmp13 + a0;
    out[4] = tmp13 - a0;
}
__device__ __forceinline__ u32 descale(u32 v, int n) { return (u32)((int)(v + (1u << (n - 1))) >> n); }
// libjpeg's range-limit table (centred on 128, indexed & 1023) in closed form: it wraps, it does not clamp.  Inside
// [-512, 511] that IS a clamp; outside, libjpeg-turbo's SIMD inverse DCT saturates instead (zone B).
__device__ __forceinline__ u32 range_limit(u32 v) {
    const u32 x = v & 1023u;
    return x < 128u ? x + 128u : x < 512u ? 255u : x < 896u ? 0u : x - 896u;
}

// 32 blocks per workgroup, 8 lanes per block: lane k runs the column pass on column k, the block is transposed through LDS,
// lane r runs the row pass on row r and stores its 8 samples with one 8-byte store.
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const JpegDev *__restrict__ table, const int16_t *__restrict__ coef,
                                                        unsigned char *__restrict__ ws) {
    __shared__ u32 lds[32][8][9];
    const JpegDev &d = table[blockIdx.z];
    const int total = d.blk_end[d.ncomp - 1];
    if ((int)blockIdx.x * 32 >= total) return;                      // uniform over the workgroup
    const int lane = threadIdx.x & 7, slot = threadIdx.x >> 3;
    const int b = blockIdx.x * 32 + slot;
    const bool live = b < total;
    int c = 0, first = 0;
    if (live) {
        if (d.ncomp == 3 && b >= d.blk_end[0]) {
            c = b >= d.blk_end[1] ? 2 : 1;
            first = d.blk_end[c - 1];
        }
        const int16_t *src = coef + d.coef_off[c] + (long long)(b - first) * 64 + lane * 8;
        const uintx4 cv = *reinterpret_cast<const uintx4 *>(src);
        const uintx4 qv = *reinterpret_cast<const uintx4 *>(&d.q[c][lane * 8]);
        u32 in[8], out[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const u32 cw = cv[r >> 1], qw = qv[r >> 1];
            const int co = (r & 1) ? (int)cw >> 16 : (int)(short)(cw & 0xffffu);
            const u32 qq = (r & 1) ? qw >> 16 : qw & 0xffffu;
            in[r] = (u32)co * qq;
        }
        idct_pass(in, out);
#pragma unroll
        for (int r = 0; r < 8; ++r) lds[slot][r][lane] = descale(out[r], 11);
    }
    __syncthreads();
    if (live) {
        u32 in[8], out[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = lds[slot][lane][k];
        idct_pass(in, out);
        u32 px[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) px[k] = range_limit(descale(out[k], 18));
        const int bi = b - first, by = bi / d.bw[c], bx = bi - by * d.bw[c];
        unsigned char *dst = ws + d.plane_off[c] + (long long)(by * 8 + lane) * (d.bw[c] * 8) + bx * 8;
        uint2 v;
        v.x = px[0] | px[1] << 8 | px[2] << 16 | px[3] << 24;
        v.y = px[4] | px[5] << 8 | px[6] << 16 | px[7] << 24;
        *reinterpret_cast<uint2 *>(dst) = v;
    }
}

// One full-resolution sample of a component at (y, x) of the image: jdsample.c's fullsize / h2v1_fancy / h2v2_fancy /
// h2v1 / h2v2 upsamplers evaluated at one position.  Edges replicate at the DOWNSAMPLED size (dw x dh).
__device__ __forceinline__ int jpeg_sample(const unsigned char *__restrict__ p, int pitch, int mode, int dw, int dh, int y, int x) {
    if (mode == UP_NONE) return p[(long long)y * pitch + x];
    if (mode > UP_H2V2_BOX) {      // uniform over an image: jdsample.c's h1v2_fancy (vertical triangle filter) and int_upsample
        if (mode == UP_H1V2_FANCY) {
            const int j = y >> 1;
            const int jn = (y & 1) ? (j + 1 < dh ? j + 1 : dh - 1) : (j > 0 ? j - 1 : 0);
            return (3 * p[(long long)j * pitch + x] + p[(long long)jn * pitch + x] + ((y & 1) ? 2 : 1)) >> 2;
        }
        return p[(long long)(y / (mode >> 16)) * pitch + x / ((mode >> 8) & 255)];
    }
    const int i = x >> 1;
    if (mode == UP_H2V1_BOX) return p[(long long)y * pitch + i];
    if (mode == UP_H2V2_BOX) return p[(long long)(y >> 1) * pitch + i];
    if (mode == UP_H2V1_FANCY) {
        const unsigned char *row = p + (long long)y * pitch;
        const int cur = row[i];
        if (x & 1) return i == dw - 1 ? cur : (3 * cur + row[i + 1] + 2) >> 2;
        return i == 0 ? cur : (3 * cur + row[i - 1] + 1) >> 2;
    }
    const int j = y >> 1;
    const int jn = (y & 1) ? (j + 1 < dh ? j + 1 : dh - 1) : (j > 0 ? j - 1 : 0);
    const unsigned char *r0 = p + (long long)j * pitch, *r1 = p + (long long)jn * pitch;
    const int t = 3 * r0[i] + r1[i];
    if (x & 1) return i == dw - 1 ? (4 * t + 7) >> 4 : (3 * t + (3 * r0[i + 1] + r1[i + 1]) + 7) >> 4;
    return i == 0 ? (4 * t + 8) >> 4 : (3 * t + (3 * r0[i - 1] + r1[i - 1]) + 8) >> 4;
}
__device__ __forceinline__ u32 clamp255(int v) { return (u32)(v < 0 ? 0 : v > 255 ? 255 : v); }

// 4 output pixels of one output row per lane (12 bytes: three 4-byte stores when the row allows it).
__global__ __launch_bounds__(256) void jpeg_colour_kernel(const JpegDev *__restrict__ table, const unsigned char *__restrict__ ws) {
    const JpegDev &d = table[blockIdx.z];
    const int ox0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ox0 >= d.ow || oy >= d.oh) return;
    const int npx = d.ow - ox0 < 4 ? d.ow - ox0 : 4;
    unsigned char px[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ox = ox0 + (k < npx ? k : 0);
        const int y = d.y0 + d.yy * oy + d.yx * ox, x = d.x0 + d.xy * oy + d.xx * ox;
        const int Y = jpeg_sample(ws + d.plane_off[0], d.bw[0] * 8, d.mode[0], d.dw[0], d.dh[0], y, x);
        u32 B = Y, G = Y, R = Y;
        if (d.ncomp == 3) {
            const int cb = jpeg_sample(ws + d.plane_off[1], d.bw[1] * 8, d.mode[1], d.dw[1], d.dh[1], y, x) - 128;
            const int cr = jpeg_sample(ws + d.plane_off[2], d.bw[2] * 8, d.mode[2], d.dw[2], d.dh[2], y, x) - 128;
            R = clamp255(Y + ((91881 * cr + 32768) >> 16));
            B = clamp255(Y + ((116130 * cb + 32768) >> 16));
            G = clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
        }
        px[3 * k] = (unsigned char)B;
        px[3 * k + 1] = (unsigned char)G;
        px[3 * k + 2] = (unsigned char)R;
    }
    unsigned char *dst = d.out + (long long)oy * d.row_stride + (long long)ox0 * 3;
    if (npx == 4 && ((uintptr_t)dst & 3) == 0) {
        u32 *w = reinterpret_cast<u32 *>(dst);
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = px[4 * k] | (u32)px[4 * k + 1] << 8 | (u32)px[4 * k + 2] << 16 | (u32)px[4 * k + 3] << 24;
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < 3 * npx) dst[k] = px[k];
    }
}

#endif  // PPY_JPEG_HOST_ONLY

// ------------------------------------------------------------------------------------------- host side of the device part
bool desc_ok(const ppy_jpeg_desc_t &d) {
    if (d.width < 1 || d.width > 65535 || d.height < 1 || d.height > 65535) return false;
    if (d.components != 1 && d.components != 3) return false;
    if (d.orientation < 1 || d.orientation > 8) return false;
    const int hm = d.h_samp[0], vm = d.v_samp[0];
    if (!((hm == 1 && vm == 1) || (d.components == 3 && hm >= 1 && hm <= 4 && vm >= 1 && vm <= 4 && hm * vm <= 8))) return false;
    const int mcux = (d.width + 8 * hm - 1) / (8 * hm), mcuy = (d.height + 8 * vm - 1) / (8 * vm);
    long long off = 0;
    for (int c = 0; c < d.components; ++c) {
        if (c && (d.h_samp[c] != 1 || d.v_samp[c] != 1)) return false;
        if (d.blocks_w[c] != mcux * d.h_samp[c] || d.blocks_h[c] != mcuy * d.v_samp[c] || d.coef_offset[c] != off) return false;
        off += (long long)d.blocks_w[c] * d.blocks_h[c] * 64;
    }
    return d.coef_bytes == off * 2 && d.coef_base >= 0 && d.coef_base % 16 == 0;
}
long long planes_bytes(const ppy_jpeg_desc_t &d) {      // every plane a multiple of 64 bytes
    long long s = 0;
    for (int c = 0; c < d.components; ++c) s += (long long)d.blocks_w[c] * d.blocks_h[c] * 64;
    return s;
}

}  // namespace

static void fill_desc(const Parsed &P, ppy_jpeg_desc_t *h_desc) {      // everything but coef_base, which is the caller's
    const long long base = h_desc->coef_base;
    memset(h_desc, 0, sizeof(*h_desc));
    h_desc->coef_base = base;
    h_desc->width = P.W;
    h_desc->height = P.H;
    h_desc->components = P.ncomp;
    h_desc->orientation = P.orientation;
    h_desc->coef_bytes = P.coef_elems * 2;
    for (int c = 0; c < P.ncomp; ++c) {
        h_desc->h_samp[c] = P.h[c];
        h_desc->v_samp[c] = P.v[c];
        h_desc->blocks_w[c] = P.bw[c];
        h_desc->blocks_h[c] = P.bh[c];
        h_desc->coef_offset[c] = P.coef_off[c];
        const unsigned short *q = P.full ? P.ql[c] : P.q[P.tq[c]];
        for (int k = 0; k < 64; ++k) h_desc->quant[c][stored_index(k)] = q[k];
    }
}

static void fill_info(const Parsed &P, ppy_jpeg_info_t *info) {
    info->width = P.W;
    info->height = P.H;
    info->orientation = P.orientation;
    oriented_size(P.W, P.H, P.orientation, &info->out_width, &info->out_height);
    info->components = P.ncomp;
    info->restart_interval = P.dri;
    for (int c = 0; c < P.ncomp; ++c) {
        info->h_samp[c] = P.h[c];
        info->v_samp[c] = P.v[c];
        info->blocks_w[c] = P.bw[c];
        info->blocks_h[c] = P.bh[c];
    }
    info->coef_bytes = P.coef_elems * 2;
    info->progressive = P.progressive;
}

static const unsigned ACCEPT_ALL = PPY_JPEG_ACCEPT_PROGRESSIVE | PPY_JPEG_ACCEPT_MULTISCAN | PPY_JPEG_ACCEPT_SAMPLING;

// Mask 0 is the single-scan path, call for call what it was before the mask existed; any other mask goes through the scan loop.
extern "C" int ppy_jpeg_info_ex(const unsigned char *h_data, size_t bytes, unsigned accept, ppy_jpeg_info_t *h_info) {
    if (h_data == nullptr || h_info == nullptr || (accept & ~ACCEPT_ALL) != 0) return PPY_ERR_BAD_ARG;
    memset(h_info, 0, sizeof(*h_info));
    Parsed P;
    Fail f = {PPY_OK, ""};
    const int rc = accept ? decode_full(h_data, bytes, accept, P, nullptr, f) : parse(h_data, bytes, P, f);
    if (rc == PPY_OK) fill_info(P, h_info);
    h_info->status = rc;
    memcpy(h_info->reason, f.reason, sizeof(f.reason));
    return rc;
}

extern "C" int ppy_jpeg_info(const unsigned char *h_data, size_t bytes, ppy_jpeg_info_t *h_info) {
    return ppy_jpeg_info_ex(h_data, bytes, 0, h_info);
}

extern "C" int ppy_jpeg_entropy_decode_ex(const unsigned char *h_data, size_t bytes, unsigned accept, int16_t *h_coef, size_t coef_bytes,
                                          ppy_jpeg_desc_t *h_desc, char *h_reason) {
    if (h_reason) h_reason[0] = 0;
    if (h_data == nullptr || h_coef == nullptr || h_desc == nullptr || (accept & ~ACCEPT_ALL) != 0) return PPY_ERR_BAD_ARG;
    Parsed P;
    Fail f = {PPY_OK, ""};
    int rc = accept ? decode_full(h_data, bytes, accept, P, nullptr, f) : parse(h_data, bytes, P, f);
    if (rc == PPY_OK && (size_t)(P.coef_elems * 2) > coef_bytes) rc = fail(f, PPY_ERR_WORKSPACE, "coefficient buffer too small");
    if (rc == PPY_OK) {
        memset(h_coef, 0, (size_t)P.coef_elems * 2);      // the blocks no scan visits stay zero
        rc = accept ? decode_full(h_data, bytes, accept, P, h_coef, f) : entropy_decode(h_data, bytes, P, h_coef, f);
    }
    if (h_reason) memcpy(h_reason, f.reason, sizeof(f.reason));
    if (rc != PPY_OK) return rc;
    fill_desc(P, h_desc);
    return PPY_OK;
}

extern "C" int ppy_jpeg_entropy_decode(const unsigned char *h_data, size_t bytes, int16_t *h_coef, size_t coef_bytes,
                                       ppy_jpeg_desc_t *h_desc, char *h_reason) {
    return ppy_jpeg_entropy_decode_ex(h_data, bytes, 0, h_coef, coef_bytes, h_desc, h_reason);
}

// ------------------------------------------------------------------------------- host pre-pass of the device entropy mode
// Restart segments the file can hold: every segment but the last ends in a two-byte marker, so a file with fewer bytes
// than that is refused ("restart marker expected") before anything is sized from its header.
static long long scan_segments(const Parsed &P, size_t bytes) {
    const long long mcus = (long long)P.mcux * P.mcuy, want = P.dri ? (mcus + P.dri - 1) / P.dri : 1;
    const long long room = 1 + (long long)((bytes - P.data) / 2);
    return want < room ? want : room;
}
static size_t scan_bound(const Parsed &P, size_t bytes, long long nseg) {
    const size_t fixed = sizeof(ppy_jpeg_scan_t) + 2 * (size_t)P.ncomp * sizeof(JpegHuffDev);
    return (fixed + (size_t)nseg * (sizeof(JpegSeg) + 4) + (bytes - P.data) + 15) / 16 * 16;
}

extern "C" size_t ppy_jpeg_scan_bytes(const unsigned char *h_data, size_t bytes, long long *h_segments) {
    if (h_segments) *h_segments = 0;
    if (h_data == nullptr || bytes >= (1u << 28)) return 0;
    Parsed P;
    Fail f = {PPY_OK, ""};
    if (parse(h_data, bytes, P, f) != PPY_OK) return 0;
    const long long nseg = scan_segments(P, bytes);
    if (h_segments) *h_segments = nseg;
    return scan_bound(P, bytes, nseg);
}

static void pack_huff(const HuffTab &t, JpegHuffDev &o) {
    for (int i = 0; i < 512; ++i) o.look[i] = (uint16_t)(t.look_len[i] << 8 | t.look_sym[i]);
    for (int l = 0; l < 18; ++l) {
        o.maxcode[l] = t.maxcode[l];
        o.valoff[l] = t.valoff[l];
    }
    memcpy(o.vals, t.vals, 256);
}

extern "C" int ppy_jpeg_scan_prepare(const unsigned char *h_data, size_t bytes, void *h_scan, size_t scan_bytes, size_t *h_used,
                                     ppy_jpeg_desc_t *h_desc, char *h_reason) {
    if (h_reason) h_reason[0] = 0;
    if (h_used) *h_used = 0;
    if (h_data == nullptr || h_scan == nullptr || h_desc == nullptr || ((uintptr_t)h_scan & 15) != 0 || bytes >= (1u << 28)) return PPY_ERR_BAD_ARG;
    Parsed P;
    Fail f = {PPY_OK, ""};
    int rc = parse(h_data, bytes, P, f);
    const unsigned char *d = h_data;
    const size_t n = bytes;
    if (rc == PPY_OK) {
        const long long mcus = (long long)P.mcux * P.mcuy, nseg = P.dri ? (mcus + P.dri - 1) / P.dri : 1;
        if (nseg != scan_segments(P, n)) rc = fail(f, PPY_ERR_CORRUPT, "restart marker expected");
        else if (scan_bound(P, n, nseg) > scan_bytes) rc = fail(f, PPY_ERR_WORKSPACE, "scan buffer too small");
        else {
            unsigned char *rec = static_cast<unsigned char *>(h_scan);
            ppy_jpeg_scan_t H;
            memset(&H, 0, sizeof(H));
            H.components = P.ncomp;
            H.mcus_w = P.mcux;
            H.mcus_h = P.mcuy;
            H.restart_interval = P.dri;
            H.segments = (int)nseg;
            H.mcus = (int)mcus;
            H.coef_elems = P.coef_elems;
            for (int c = 0; c < P.ncomp; ++c) {
                H.h_samp[c] = P.h[c];
                H.v_samp[c] = P.v[c];
                H.blocks_w[c] = P.bw[c];
                H.coef_offset[c] = P.coef_off[c];
            }
            H.table_offset = (unsigned)sizeof(H);
            H.segment_offset = H.table_offset + 2 * (unsigned)P.ncomp * (unsigned)sizeof(JpegHuffDev);
            H.data_offset = H.segment_offset + (unsigned)nseg * (unsigned)sizeof(JpegSeg);
            JpegHuffDev *tabs = reinterpret_cast<JpegHuffDev *>(rec + H.table_offset);
            for (int c = 0; c < P.ncomp; ++c) {
                pack_huff(P.dc[P.td[c]], tabs[c]);
                pack_huff(P.ac[P.ta[c]], tabs[P.ncomp + c]);
            }
            JpegSeg *seg = reinterpret_cast<JpegSeg *>(rec + H.segment_offset);
            unsigned char *out = rec + H.data_offset;
            size_t p = P.data, o = 0;
            for (long long s = 0; s < nseg; ++s) {
                const size_t start = o;
                while (p < n) {      // the one walk over the entropy-coded bytes: unstuff, stop at a marker
                    const unsigned char c = d[p];
                    if (c != 0xFF) {
                        out[o++] = c;
                        ++p;
                    } else if (p + 1 < n && d[p + 1] == 0) {
                        out[o++] = 0xFF;
                        p += 2;
                    } else break;
                }
                seg[s].byte_off = (uint32_t)start;
                seg[s].bit_len = (uint32_t)((o - start) * 8);
                seg[s].first_mcu = (uint32_t)(P.dri ? s * P.dri : 0);
                seg[s].mcu_count = (uint32_t)(P.dri && (s + 1) * P.dri < mcus ? P.dri : mcus - (P.dri ? s * P.dri : 0));
                while (o & 3) out[o++] = 0;
                if (s + 1 < nseg) {
                    while (p + 1 < n && d[p] == 0xFF && d[p + 1] == 0xFF) ++p;
                    if (p + 1 >= n || d[p] != 0xFF || d[p + 1] != 0xD0 + (int)(s & 7)) {
                        rc = fail(f, PPY_ERR_CORRUPT, "restart marker expected");
                        break;
                    }
                    p += 2;
                }
            }
            if (rc == PPY_OK) {
                H.data_bytes = (unsigned)o;
                const size_t used = ((size_t)H.data_offset + o + 15) / 16 * 16;
                memset(out + o, 0, used - H.data_offset - o);
                H.record_bytes = (unsigned)used;
                memcpy(rec, &H, sizeof(H));
                if (h_used) *h_used = used;
            }
        }
    }
    if (h_reason) memcpy(h_reason, f.reason, sizeof(f.reason));
    if (rc != PPY_OK) return rc;
    fill_desc(P, h_desc);
    return PPY_OK;
}

extern "C" size_t ppy_jpeg_workspace_bytes(int n, const ppy_jpeg_desc_t *h_descs) {
    if (n <= 0 || h_descs == nullptr) return 0;
    long long s = 0;
    for (int i = 0; i < n; ++i) {
        if (!desc_ok(h_descs[i])) return 0;
        s += planes_bytes(h_descs[i]);
    }
    return (size_t)s;
}

extern "C" size_t ppy_jpeg_table_bytes(int n) { return n > 0 ? (size_t)n * sizeof(JpegDev) : 0; }

extern "C" int ppy_jpeg_pack_table(int n, const ppy_jpeg_desc_t *h_descs, unsigned char *const *h_out, const long long *h_row_stride,
                                   int apply_orientation, void *h_table, size_t table_bytes) {
    PPY_CHECK_ARG(n > 0 && n <= 65535 && h_descs && h_out && h_row_stride && h_table && table_bytes >= (size_t)n * sizeof(JpegDev));
    JpegDev *tab = static_cast<JpegDev *>(h_table);
    long long plane = 0;
    for (int i = 0; i < n; ++i) {
        const ppy_jpeg_desc_t &s = h_descs[i];
        PPY_CHECK_ARG(desc_ok(s) && h_out[i] != nullptr);
        JpegDev d;
        memset(&d, 0, sizeof(d));
        const int o = apply_orientation ? s.orientation : 1;
        d.ncomp = s.components;
        d.W = s.width;
        d.H = s.height;
        oriented_size(d.W, d.H, o, &d.ow, &d.oh);
        PPY_CHECK_ARG(h_row_stride[i] >= 3LL * d.ow);
        d.out = h_out[i];
        d.row_stride = h_row_stride[i];
        // source (y, x) of output (oy, ox) for the eight EXIF orientations
        const int W1 = d.W - 1, H1 = d.H - 1;
        switch (o) {
            case 2: d.yy = 1; d.x0 = W1; d.xx = -1; break;                       // mirrored
            case 3: d.y0 = H1; d.yy = -1; d.x0 = W1; d.xx = -1; break;           // rotated 180
            case 4: d.y0 = H1; d.yy = -1; d.xx = 1; break;                       // flipped
            case 5: d.yx = 1; d.xy = 1; break;                                   // transposed
            case 6: d.y0 = H1; d.yx = -1; d.xy = 1; break;                       // rotate 90 clockwise to display
            case 7: d.y0 = H1; d.yx = -1; d.x0 = W1; d.xy = -1; break;           // transverse
            case 8: d.yx = 1; d.x0 = W1; d.xy = -1; break;                       // rotate 90 counter-clockwise to display
            default: d.yy = 1; d.xx = 1; break;
        }
        int blocks = 0;
        for (int c = 0; c < s.components; ++c) {
            d.coef_off[c] = s.coef_base / 2 + s.coef_offset[c];
            d.plane_off[c] = plane;
            plane += (long long)s.blocks_w[c] * s.blocks_h[c] * 64;
            d.bw[c] = s.blocks_w[c];
            d.bh[c] = s.blocks_h[c];
            blocks += s.blocks_w[c] * s.blocks_h[c];
            d.blk_end[c] = blocks;
            const int hm = s.h_samp[0], vm = s.v_samp[0];
            d.dw[c] = (s.width * s.h_samp[c] + hm - 1) / hm;
            d.dh[c] = (s.height * s.v_samp[c] + vm - 1) / vm;
            const int fx = hm / s.h_samp[c], fy = vm / s.v_samp[c];      // jdsample.c jinit_upsampler, fancy upsampling on
            if (fx == 1 && fy == 1) d.mode[c] = UP_NONE;
            else if (fx == 2 && fy == 1) d.mode[c] = d.dw[c] > 2 ? UP_H2V1_FANCY : UP_H2V1_BOX;      // fancy needs > 2 columns
            else if (fx == 2 && fy == 2) d.mode[c] = d.dw[c] > 2 ? UP_H2V2_FANCY : UP_H2V2_BOX;
            else if (fx == 1 && fy == 2) d.mode[c] = UP_H1V2_FANCY;                                  // whatever the width
            else d.mode[c] = UP_REPLICATE | fx << 8 | fy << 16;
            memcpy(d.q[c], s.quant[c], sizeof(d.q[c]));
        }
        tab[i] = d;
    }
    return PPY_OK;
}

#ifndef PPY_JPEG_HOST_ONLY
extern "C" int ppy_jpeg_reconstruct_u8(int n, const ppy_jpeg_desc_t *h_descs, int apply_orientation, const void *table,
                                       const int16_t *coef, size_t coef_bytes, void *ws, size_t ws_bytes, void *stream) {
    ppy_drop_stale_error();
    PPY_CHECK_ARG(n > 0 && n <= 65535 && h_descs && table && coef && ((uintptr_t)table & 15) == 0 && ((uintptr_t)coef & 15) == 0);
    long long need = 0;
    int max_blocks = 0, max_w = 0, max_h = 0;
    for (int i = 0; i < n; ++i) {
        const ppy_jpeg_desc_t &s = h_descs[i];
        PPY_CHECK_ARG(desc_ok(s) && (unsigned long long)s.coef_base + (unsigned long long)s.coef_bytes <= coef_bytes);
        need += planes_bytes(s);
        int blocks = 0;
        for (int c = 0; c < s.components; ++c) blocks += s.blocks_w[c] * s.blocks_h[c];
        max_blocks = blocks > max_blocks ? blocks : max_blocks;
        int ow, oh;      // the store kernel walks the OUTPUT raster
        oriented_size(s.width, s.height, apply_orientation ? s.orientation : 1, &ow, &oh);
        max_w = ow > max_w ? ow : max_w;
        max_h = oh > max_h ? oh : max_h;
    }
    if (ws == nullptr || ws_bytes < (size_t)need || ((uintptr_t)ws & 15) != 0) return PPY_ERR_WORKSPACE;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(ceil_div(max_blocks, 32), 1, n), dim3(256), 0, (hipStream_t)stream,
                       (const JpegDev *)table, coef, (unsigned char *)ws);
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3(ceil_div(max_w, 256), ceil_div(max_h, 4), n), dim3(256), 0, (hipStream_t)stream,
                       (const JpegDev *)table, (const unsigned char *)ws);
    return ppy_launch_status();
}
#endif  // PPY_JPEG_HOST_ONLY
