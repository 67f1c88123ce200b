// The scan record: what the host pre-pass of the device entropy mode (ppy_jpeg_scan_prepare, jpeg.hip) hands to the
// parallel Huffman decoder (jpeg_entropy.hip), and the decode step both the kernels and their host twin run.  Everything
// here compiles as plain C++ (PPY_JPEG_HOST_ONLY: the AddressSanitizer sweeps of tools/) and as HIP device code.
//
// Record layout (ppy_jpeg_scan_t is the public header of it, include/ppyolo_hip.h), all offsets from the record start:
//   ppy_jpeg_scan_t | JpegHuffDev dc[components], ac[components] | JpegSeg seg[segments] | unstuffed bytes
// Every segment's bytes start on a 4-byte boundary and are zero-padded to the next one, so the decoder reads aligned
// big-endian words and the pad reads as zero bits.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) && !defined(PPY_JPEG_HOST_ONLY)
#define PPY_HD __host__ __device__ __forceinline__
#else
#define PPY_HD inline
#endif

// The host decoder's table in compact form: 9-bit lookahead (length << 8 | symbol, 0 = longer than 9 bits) plus the
// maxcode / valoff / vals of the lengths 10..16.
struct JpegHuffDev {
    uint16_t look[512];
    int32_t maxcode[18], valoff[18];
    uint8_t vals[256];
};
static_assert(sizeof(JpegHuffDev) == 1424, "JpegHuffDev layout");

struct JpegSeg {
    uint32_t byte_off;       // from the start of the record's data, % 4 == 0
    uint32_t bit_len;        // unstuffed data bits up to the marker that ends the segment (a multiple of 8)
    uint32_t first_mcu, mcu_count;
};

// One image of the batch as ppy_jpeg_entropy_plan lays it out.  64 bytes.
struct JpegEntItem {
    long long scan_off;      // bytes from the start of the scan buffer to the image's record
    long long coef_base;     // int16 elements into the batch coefficient buffer
    long long coef_elems;
    long long sub_first_off; // bytes from the start of the plan to uint32 sub_first[segments + 1]
    uint32_t sub_base;       // the image's first subsequence in the batch-wide state arrays
    uint32_t nsub;
    uint32_t pad[6];
};
static_assert(sizeof(JpegEntItem) == 64, "JpegEntItem layout");

// Exit state of a subsequence: where its decoder stood when it crossed the subsequence's last bit.
struct JpegSubState {
    uint32_t p;              // bit position in the segment; JPEG_SUB_FAILED: the decode from this entry state failed
    uint32_t bk;             // block in MCU << 8 | zigzag index of the next symbol (0: a DC symbol)
    uint32_t count;          // coefficient slots consumed from the entry state (not part of the comparison)
    uint32_t pad;
};
static const uint32_t JPEG_SUB_FAILED = 0xFFFFFFFFu;

// reason ids of the status words (ppy_jpeg_reason_string)
enum { JPEG_R_OK = 0, JPEG_R_BAD_CODE = 1, JPEG_R_DC_SIZE = 2, JPEG_R_PAST_63 = 3, JPEG_R_ENDS_EARLY = 4, JPEG_R_RESTART = 5 };

#define PPY_ZIGZAG_INIT                                                                                                      \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}
#if defined(__HIP_DEVICE_COMPILE__)
__device__ const unsigned char JPEG_ZZ_DEV[64] = PPY_ZIGZAG_INIT;
#define JPEG_ZZ JPEG_ZZ_DEV
#else
static const unsigned char JPEG_ZZ_HOST[64] = PPY_ZIGZAG_INIT;
#define JPEG_ZZ JPEG_ZZ_HOST
#endif

// zigzag index -> index inside a stored (transposed) block, as stored_index() of the host decoder
PPY_HD int jpeg_stored_index(int zz) { return (JPEG_ZZ[zz] & 7) * 8 + (JPEG_ZZ[zz] >> 3); }

PPY_HD bool jpeg_state_equal(const JpegSubState &a, const JpegSubState &b) { return a.p == b.p && a.bk == b.bk; }

PPY_HD int jpeg_blocks_per_mcu(const ppy_jpeg_scan_t &H) { return H.components == 1 ? 1 : H.h_samp[0] * H.v_samp[0] + 2; }
PPY_HD int jpeg_block_comp(const ppy_jpeg_scan_t &H, int blk) {
    const int luma = H.h_samp[0] * H.v_samp[0];
    return blk < luma ? 0 : blk - luma + 1;
}

// (MCU, block in MCU) -> element offset of the block in the image's coefficients, or -1 outside the image's own range.
PPY_HD long long jpeg_block_base(const ppy_jpeg_scan_t &H, unsigned long long mcu, int blk) {
    if (mcu >= (unsigned long long)H.mcus) return -1;
    const int c = jpeg_block_comp(H, blk);
    if (c >= H.components) return -1;
    const int r = c ? 0 : blk, h = H.h_samp[c], v = H.v_samp[c];
    const int vv = r / h, hh = r - vv * h;
    const int my = (int)(mcu / (unsigned)H.mcus_w), mx = (int)(mcu - (unsigned long long)my * H.mcus_w);
    const long long block = (long long)(my * v + vv) * H.blocks_w[c] + (mx * h + hh);
    const long long at = H.coef_offset[c] + block * 64;
    return at >= 0 && at + 64 <= H.coef_elems ? at : -1;
}

// Bits of one segment, big-endian, through aligned 32-bit words; anything past the segment's words reads as zero (the
// host reader's phantom bits).  Two words are cached, so a symbol costs a load only when it crosses into a new word.
struct JpegBits {
    const uint32_t *words;
    uint32_t nwords, at;
    unsigned long long acc;
};
PPY_HD uint32_t jpeg_word(const JpegBits &b, uint32_t w) {
    if (w >= b.nwords) return 0;
    const uint32_t x = b.words[w];
    return x << 24 | (x & 0xff00u) << 8 | (x >> 8 & 0xff00u) | x >> 24;
}
PPY_HD void jpeg_bits_open(JpegBits &b, const uint32_t *words, uint32_t nwords) {
    b.words = words;
    b.nwords = nwords;
    b.at = 0xFFFFFFFFu;
    b.acc = 0;
}
PPY_HD uint32_t jpeg_peek32(JpegBits &b, uint32_t p) {      // the 32 bits from bit p on
    const uint32_t w = p >> 5;
    if (w != b.at) {
        b.acc = (unsigned long long)jpeg_word(b, w) << 32 | jpeg_word(b, w + 1);
        b.at = w;
    }
    return (uint32_t)((b.acc << (p & 31)) >> 32);
}

// One Huffman code from the top of v: its symbol and length, or -1 (decode_symbol of the host decoder).
PPY_HD int jpeg_huff(const JpegHuffDev &t, uint32_t v, int &len) {
    const uint32_t e = t.look[v >> 23];
    if (e >> 8) {
        len = (int)(e >> 8);
        return (int)(e & 255u);
    }
    for (int l = 10; l <= 16; ++l) {
        const int code = (int)(v >> (32 - l));
        if (code <= t.maxcode[l]) {
            const uint32_t idx = (uint32_t)(code + t.valoff[l]);
            if (idx >= 256) return -1;
            len = l;
            return t.vals[idx];
        }
    }
    return -1;
}
PPY_HD int jpeg_extend(uint32_t x, int s) { return x < (1u << (s - 1)) ? (int)x - (1 << s) + 1 : (int)x; }

// The per-subsequence decode step.  From the entry state (st.p, st.bk) decode whole symbols while the position is below
// `limit` (a symbol may end past it: that overhang is the next subsequence's entry position); st becomes the exit state
// and st.count the slots consumed.  A symbol takes at least one bit, so the loop runs at most limit - p times.
// WRITE = false: the synchronisation passes; a failure makes the state JPEG_SUB_FAILED and reports nothing.
// WRITE = true : the pass from the true entry state.  slot is the image-wide slot ((MCU * blocks per MCU + block) * 64 +
//   zigzag index) of the entry state; decoding also stops at slot_end (the segment's last slot + 1).  Non-zero coefficients
//   and the DC DIFFERENCE go to coef (the image's own, range-checked); the return value is a JPEG_R_* reason.
template <bool WRITE>
PPY_HD int jpeg_decode_sub(const ppy_jpeg_scan_t &H, const JpegHuffDev *tabs, JpegBits &bits, JpegSubState &st, uint32_t limit,
                           uint32_t bit_len, unsigned long long slot, unsigned long long slot_end, int16_t *coef) {
    const int B = jpeg_blocks_per_mcu(H), nc = H.components;
    uint32_t p = st.p;
    int blk = (int)(st.bk >> 8), k = (int)(st.bk & 255u);
    const unsigned long long slot0 = slot;
    long long base = -1;
    if (WRITE && k) base = jpeg_block_base(H, (slot >> 6) / (unsigned)B, blk);
    int reason = JPEG_R_OK;
    while (p < limit && (!WRITE || slot < slot_end)) {
        const uint32_t v = jpeg_peek32(bits, p);
        const int c = jpeg_block_comp(H, blk);
        int len = 0;
        if (k == 0) {
            const int t = jpeg_huff(tabs[c], v, len);
            if (t < 0 || t > 15) {
                reason = t < 0 ? JPEG_R_BAD_CODE : JPEG_R_DC_SIZE;
                break;
            }
            if (WRITE) {
                base = jpeg_block_base(H, (slot >> 6) / (unsigned)B, blk);
                if (t && base >= 0) coef[base] = (int16_t)jpeg_extend((v << len) >> (32 - t), t);
            }
            p += (uint32_t)(len + t);
            k = 1;
            slot += 1;
        } else {
            const int rs = jpeg_huff(tabs[nc + c], v, len);
            if (rs < 0) {
                reason = JPEG_R_BAD_CODE;
                break;
            }
            const int r = rs >> 4, s = rs & 15;
            if (s == 0) {      // end of block, or a run of 16 zeros (one that passes index 63 ends the block, as on the host)
                const int adv = r == 15 && k + 16 < 64 ? 16 : 64 - k;
                p += (uint32_t)len;
                slot += (unsigned)adv;
                k += adv;
            } else {
                k += r;
                if (k > 63) {
                    reason = JPEG_R_PAST_63;
                    break;
                }
                if (WRITE && base >= 0) coef[base + jpeg_stored_index(k)] = (int16_t)jpeg_extend((v << len) >> (32 - s), s);
                p += (uint32_t)(len + s);
                slot += (unsigned)(r + 1);
                ++k;
            }
        }
        if (k >= 64) {
            k = 0;
            blk = blk + 1 == B ? 0 : blk + 1;
            if (WRITE && p > bit_len) {      // the host's check after every block: it consumed bits the data does not have
                reason = JPEG_R_ENDS_EARLY;
                break;
            }
        }
    }
    st.p = reason ? JPEG_SUB_FAILED : p;
    st.bk = (uint32_t)blk << 8 | (uint32_t)k;
    st.count = (uint32_t)(slot - slot0);
    return reason;
}
