// Device entropy stage of the JPEG decoder: self-synchronising parallel Huffman decoding (Klein and Wiseman; Weissenberger
// and Schmidt for JPEG) of the scan records ppy_jpeg_scan_prepare writes (jpeg_scan.h), into the coefficient buffer the
// reconstruction kernels of jpeg.hip read.  DESIGN.md section 10.
//
// A restart segment is cut into subsequences of subseq_bytes, one lane each.  Four kernels per BATCH, blockIdx.y (or .x of
// the per-image kernels) selecting the image, the image's Huffman tables in LDS:
//   jpeg_huff_sync_kernel   every lane decodes its subsequence from the assumed state (its first bit, block 0, index 0; the
//                           first subsequence of a segment from the true one) and records the exit state; then, inside the
//                           workgroup, a lane whose predecessor's exit state changed decodes again from it, until nothing
//                           changes.  Round r leaves the first r lanes final, so SUB_LANES rounds bound the loop.
//   jpeg_huff_link_kernel   one workgroup per image walks the workgroups of the first kernel in order: the now-true exit
//                           state of the last lane before it is the entry state of a group's first lane, and the same
//                           rounds repair the group where that differs from the assumption.  The walk also prefix-sums the
//                           slot counts.  It is bounded by the subsequence count.
//   jpeg_huff_write_kernel  decodes every subsequence once more from its true entry state and writes the non-zero
//                           coefficients and the DC differences; it alone reports damage (the status words).
//   jpeg_dc_scan_kernel     DC differences -> values.
// No kernel waits for another workgroup: the launches are the only synchronisation across workgroups, so no input can make
// one spin.  A stream that never synchronises (fixed-length codes) costs SUB_LANES rounds per group: serial speed, still
// correct.  ppy_jpeg_entropy_twin runs the same phases on the host through the same decode step.
#include <string.h>

#ifndef PPY_JPEG_HOST_ONLY
#include "common.h"
#else
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

enum { SUB_LANES = 256 };      // subsequences per workgroup of the sync and write kernels (and per group of the link walk)

// One lane's view of its subsequence.
struct SubView {
    const uint32_t *words;
    uint32_t nwords, bit_len, limit, assumed_p;
    unsigned long long slot_first, slot_end;      // image-wide slots of the segment
    uint32_t first_sub;                           // the segment's first subsequence
    bool first, last_segment;
};

PPY_HD const ppy_jpeg_scan_t &scan_header(const unsigned char *scan, const JpegEntItem &it) {
    return *reinterpret_cast<const ppy_jpeg_scan_t *>(scan + it.scan_off);
}

// Subsequence j of an image -> its segment (the last one whose first subsequence is <= j) and its bit range.
PPY_HD void sub_view(const ppy_jpeg_scan_t &H, const unsigned char *rec, const uint32_t *sub_first, uint32_t j, uint32_t subseq_bits,
                     SubView &v) {
    uint32_t lo = 0, hi = (uint32_t)H.segments - 1;
    while (lo < hi) {      // at most 32 rounds
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (sub_first[mid] <= j) lo = mid;
        else hi = mid - 1;
    }
    const JpegSeg sg = reinterpret_cast<const JpegSeg *>(rec + H.segment_offset)[lo];
    const uint32_t jj = j - sub_first[lo];
    const int B = jpeg_blocks_per_mcu(H);
    v.words = reinterpret_cast<const uint32_t *>(rec + H.data_offset + sg.byte_off);
    v.nwords = (sg.bit_len + 31) >> 5;
    v.bit_len = sg.bit_len;
    v.assumed_p = jj * subseq_bits;
    const unsigned long long end = (unsigned long long)(jj + 1) * subseq_bits;
    v.limit = end < sg.bit_len ? (uint32_t)end : sg.bit_len;
    v.slot_first = (unsigned long long)sg.first_mcu * B * 64;
    v.slot_end = v.slot_first + (unsigned long long)sg.mcu_count * B * 64;
    v.first_sub = sub_first[lo];
    v.first = jj == 0;
    v.last_segment = lo + 1 == (uint32_t)H.segments;
}

PPY_HD JpegSubState assumed_state(const SubView &v) {
    JpegSubState s = {v.first ? 0u : v.assumed_p, 0u, 0u, 0u};
    return s;
}

// The synchronisation decode of one subsequence from `entry` (an exit state of its predecessor, or the assumed state).
PPY_HD JpegSubState sync_decode(const ppy_jpeg_scan_t &H, const JpegHuffDev *tabs, const SubView &v, const JpegSubState &entry) {
    JpegSubState s = entry;
    s.count = 0;
    if (entry.p == JPEG_SUB_FAILED) return s;
    JpegBits bits;
    jpeg_bits_open(bits, v.words, v.nwords);
    jpeg_decode_sub<false>(H, tabs, bits, s, v.limit, v.bit_len, 0, 0, nullptr);
    return s;
}

// The writing decode of subsequence j: entry state `entry` (true), slots before it in its segment `before`.
PPY_HD int write_decode(const ppy_jpeg_scan_t &H, const JpegHuffDev *tabs, const SubView &v, const JpegSubState &entry,
                        unsigned long long before, int16_t *coef) {
    if (entry.p == JPEG_SUB_FAILED) return JPEG_R_OK;      // the lane that met the failure reports it
    const unsigned long long slot = v.slot_first + before;
    if (slot >= v.slot_end) return JPEG_R_OK;              // the segment's MCUs are complete: bytes after them are not read
    JpegSubState s = entry;
    JpegBits bits;
    jpeg_bits_open(bits, v.words, v.nwords);
    int reason = jpeg_decode_sub<true>(H, tabs, bits, s, v.limit, v.bit_len, slot, v.slot_end, coef);
    if (reason) return reason;
    const unsigned long long at = slot + s.count;
    if (at >= v.slot_end) {      // this lane completed the segment
        if (s.p > v.bit_len) return JPEG_R_ENDS_EARLY;
        if (!v.last_segment && v.bit_len - s.p >= 8) return JPEG_R_RESTART;      // unread bytes before the restart marker
    } else if (v.limit == v.bit_len) {
        return JPEG_R_ENDS_EARLY;                                                 // the data ends before the segment's MCUs
    }
    return JPEG_R_OK;
}

// DC item q of component c in scan order (MCU by MCU, inside an MCU v then h) -> its coefficient, and whether the
// prediction restarts there.
PPY_HD long long dc_item(const ppy_jpeg_scan_t &H, int c, long long q, bool &reset) {
    const int hv = H.h_samp[c] * H.v_samp[c];
    const long long mcu = q / hv;
    const int r = (int)(q - mcu * hv);
    reset = r == 0 && (mcu == 0 || (H.restart_interval && mcu % H.restart_interval == 0));
    return jpeg_block_base(H, (unsigned long long)mcu, c ? H.h_samp[0] * H.v_samp[0] + c - 1 : r);
}

bool plan_ok(int n, const void *h_plan, int subseq_bytes, uint32_t *max_nsub, unsigned long long *total_sub) {
    if (n <= 0 || n > 65535 || h_plan == nullptr) return false;
    if (subseq_bytes < PPY_JPEG_SUBSEQ_MIN || subseq_bytes > PPY_JPEG_SUBSEQ_MAX || (subseq_bytes & (subseq_bytes - 1))) return false;
    const JpegEntItem *it = static_cast<const JpegEntItem *>(h_plan);
    uint32_t mx = 0;
    unsigned long long tot = 0;
    for (int i = 0; i < n; ++i) {
        if (it[i].sub_base != tot || it[i].nsub == 0) return false;
        tot += it[i].nsub;
        mx = it[i].nsub > mx ? it[i].nsub : mx;
    }
    if (tot >= (1ull << 31)) return false;
    *max_nsub = mx;
    *total_sub = tot;
    return true;
}
size_t state_bytes(unsigned long long total_sub) { return (size_t)total_sub * sizeof(JpegSubState); }

#ifndef PPY_JPEG_HOST_ONLY
// ------------------------------------------------------------------------------------------------------------- device
struct GroupLds {
    JpegHuffDev tabs[6];
    JpegSubState st[SUB_LANES];
    int changed[SUB_LANES];
};

__device__ __forceinline__ void load_tables(const ppy_jpeg_scan_t &H, const unsigned char *rec, JpegHuffDev *tabs) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(rec + H.table_offset);
    uint32_t *dst = reinterpret_cast<uint32_t *>(tabs);
    const int words = 2 * H.components * (int)(sizeof(JpegHuffDev) / 4);
    for (int i = threadIdx.x; i < words; i += SUB_LANES) dst[i] = src[i];
    __syncthreads();
}

// The rounds inside a group of SUB_LANES consecutive subsequences.  lane0_entry / lane0_dirty: the first lane's entry
// state when it is known to differ from the assumption (the link walk); all_dirty: the first round recomputes every lane
// that has a predecessor in the group (after the assumed-state pass).  Returns how often this lane recomputed.  Every lane
// of the workgroup calls; at most SUB_LANES rounds.
__device__ __forceinline__ unsigned group_rounds(GroupLds &L, const ppy_jpeg_scan_t &H, const SubView &v, bool live, JpegSubState &mine,
                                                 const JpegSubState &lane0_entry, bool lane0_dirty, bool all_dirty) {
    const int t = threadIdx.x;
    unsigned runs = 0;
    L.st[t] = mine;
    L.changed[t] = all_dirty;
    for (int round = 1; round <= SUB_LANES; ++round) {
        __syncthreads();
        const bool dirty = live && !v.first && (t == 0 ? (round == 1 && lane0_dirty) : L.changed[t - 1] != 0);
        const JpegSubState prev = t == 0 ? lane0_entry : L.st[t - 1];
        __syncthreads();
        int ch = 0;
        if (dirty) {
            const JpegSubState nw = sync_decode(H, L.tabs, v, prev);
            ch = !jpeg_state_equal(nw, mine);
            mine = nw;
            ++runs;
        }
        L.st[t] = mine;
        L.changed[t] = ch;
        if (!__syncthreads_or(ch)) break;
    }
    return runs;
}

__global__ __launch_bounds__(SUB_LANES) void jpeg_huff_sync_kernel(const JpegEntItem *__restrict__ items, const unsigned char *__restrict__ scan,
                                                                   const unsigned char *__restrict__ plan, uint32_t subseq_bits,
                                                                   JpegSubState *__restrict__ states) {
    __shared__ GroupLds L;
    const JpegEntItem it = items[blockIdx.y];
    if (blockIdx.x * SUB_LANES >= it.nsub) return;      // uniform over the workgroup
    const unsigned char *rec = scan + it.scan_off;
    const ppy_jpeg_scan_t &H = scan_header(scan, it);
    load_tables(H, rec, L.tabs);
    const uint32_t j = blockIdx.x * SUB_LANES + threadIdx.x;
    const bool live = j < it.nsub;
    SubView v;
    sub_view(H, rec, reinterpret_cast<const uint32_t *>(plan + it.sub_first_off), live ? j : it.nsub - 1, subseq_bits, v);
    JpegSubState mine = assumed_state(v);
    if (live) mine = sync_decode(H, L.tabs, v, mine);
    group_rounds(L, H, v, live, mine, mine, false, true);
    if (live) states[it.sub_base + j] = mine;
}

__global__ __launch_bounds__(SUB_LANES) void jpeg_huff_link_kernel(const JpegEntItem *__restrict__ items, const unsigned char *__restrict__ scan,
                                                                   const unsigned char *__restrict__ plan, uint32_t subseq_bits,
                                                                   JpegSubState *__restrict__ states, unsigned long long *__restrict__ before,
                                                                   int *__restrict__ status, int n) {
    __shared__ GroupLds L;
    __shared__ unsigned long long sums[SUB_LANES];
    const JpegEntItem it = items[blockIdx.x];
    const unsigned char *rec = scan + it.scan_off;
    const ppy_jpeg_scan_t &H = scan_header(scan, it);
    load_tables(H, rec, L.tabs);
    const int t = threadIdx.x;
    unsigned long long carry = 0;
    unsigned fixed = 0;
    const uint32_t groups = (it.nsub + SUB_LANES - 1) / SUB_LANES;
    for (uint32_t g = 0; g < groups; ++g) {
        const uint32_t j = g * SUB_LANES + t;
        const bool live = j < it.nsub;
        SubView v;
        sub_view(H, rec, reinterpret_cast<const uint32_t *>(plan + it.sub_first_off), live ? j : it.nsub - 1, subseq_bits, v);
        JpegSubState mine = states[it.sub_base + (live ? j : it.nsub - 1)];
        JpegSubState entry = assumed_state(v);
        bool dirty0 = false;
        if (g && t == 0 && !v.first) {      // the last lane of the group before: its final state is still in LDS
            entry = L.st[SUB_LANES - 1];
            dirty0 = !jpeg_state_equal(entry, assumed_state(v));
        }
        __syncthreads();      // L.st[] of the group before is read; group_rounds overwrites it
        fixed += group_rounds(L, H, v, live, mine, entry, dirty0, false);
        if (live) states[it.sub_base + j] = mine;
        // exclusive prefix of the slot counts over the image (the write pass subtracts the value at its segment's start)
        sums[t] = live ? mine.count : 0;
        __syncthreads();
        for (int o = 1; o < SUB_LANES; o <<= 1) {
            const unsigned long long a = t >= o ? sums[t - o] : 0;
            __syncthreads();
            sums[t] += a;
            __syncthreads();
        }
        if (live) before[it.sub_base + j] = carry + sums[t] - mine.count;
        carry += sums[SUB_LANES - 1];
        __syncthreads();      // sums[] and L.st[] of this group are read before the next one overwrites them
    }
    if (fixed) atomicAdd(reinterpret_cast<unsigned *>(status) + 2 * n + blockIdx.x, fixed);
}

__global__ __launch_bounds__(SUB_LANES) void jpeg_huff_write_kernel(const JpegEntItem *__restrict__ items, const unsigned char *__restrict__ scan,
                                                                    const unsigned char *__restrict__ plan, uint32_t subseq_bits,
                                                                    const JpegSubState *__restrict__ states,
                                                                    const unsigned long long *__restrict__ before, int16_t *__restrict__ coef,
                                                                    int *__restrict__ status, int n) {
    __shared__ JpegHuffDev tabs[6];
    const JpegEntItem it = items[blockIdx.y];
    if (blockIdx.x * SUB_LANES >= it.nsub) return;      // uniform over the workgroup
    const unsigned char *rec = scan + it.scan_off;
    const ppy_jpeg_scan_t &H = scan_header(scan, it);
    load_tables(H, rec, tabs);
    const uint32_t j = blockIdx.x * SUB_LANES + threadIdx.x;
    if (j >= it.nsub) return;
    SubView v;
    sub_view(H, rec, reinterpret_cast<const uint32_t *>(plan + it.sub_first_off), j, subseq_bits, v);
    const JpegSubState entry = v.first ? assumed_state(v) : states[it.sub_base + j - 1];
    const unsigned long long done = before[it.sub_base + j] - before[it.sub_base + v.first_sub];
    const int reason = write_decode(H, tabs, v, entry, done, coef + it.coef_base);
    if (reason) {      // any of the lanes that found damage names the reason
        status[blockIdx.y] = PPY_ERR_CORRUPT;
        status[n + blockIdx.y] = reason;
    }
}

// One workgroup per (component, image): a segmented inclusive scan over the component's DC terms in scan order, in tiles
// of SUB_LANES, modulo 2^32 and truncated to int16 -- the host's (int16_t)pred[c].
__global__ __launch_bounds__(SUB_LANES) void jpeg_dc_scan_kernel(const JpegEntItem *__restrict__ items, const unsigned char *__restrict__ scan,
                                                                 int16_t *__restrict__ coef_all) {
    __shared__ uint32_t val[SUB_LANES];
    __shared__ int flag[SUB_LANES];
    const JpegEntItem it = items[blockIdx.y];
    const ppy_jpeg_scan_t &H = scan_header(scan, it);
    const int c = blockIdx.x, t = threadIdx.x;
    if (c >= H.components) return;
    int16_t *coef = coef_all + it.coef_base;
    const long long total = (long long)H.mcus * H.h_samp[c] * H.v_samp[c];
    uint32_t carry = 0;
    for (long long base = 0; base < total; base += SUB_LANES) {
        const long long q = base + t;
        bool reset = false;
        const long long at = q < total ? dc_item(H, c, q, reset) : -1;
        uint32_t x = at >= 0 ? (uint32_t)(int)coef[at] : 0u;
        int f = reset;
        val[t] = x;
        flag[t] = f;
        __syncthreads();
        for (int o = 1; o < SUB_LANES; o <<= 1) {      // (reset, sum since the reset) composes associatively
            const uint32_t ax = t >= o ? val[t - o] : 0u;
            const int af = t >= o ? flag[t - o] : 0;
            __syncthreads();
            if (!f) x += ax;
            f |= af;
            val[t] = x;
            flag[t] = f;
            __syncthreads();
        }
        if (!f) x += carry;      // no reset in the tile up to this lane: the earlier tiles join
        if (at >= 0) coef[at] = (int16_t)x;
        if (t == SUB_LANES - 1) val[0] = x;
        __syncthreads();
        carry = val[0];
        __syncthreads();
    }
}
#endif  // PPY_JPEG_HOST_ONLY

}  // namespace

// --------------------------------------------------------------------------------------------------------- host entries
extern "C" const char *ppy_jpeg_reason_string(int reason) {
    switch (reason) {
        case JPEG_R_OK: return "";
        case JPEG_R_BAD_CODE: return "bad Huffman code in the entropy data";
        case JPEG_R_DC_SIZE: return "bad Huffman code in the entropy data (DC size above 15)";
        case JPEG_R_PAST_63: return "coefficient index past 63";
        case JPEG_R_ENDS_EARLY: return "entropy data ends early";
        case JPEG_R_RESTART: return "restart marker expected";
        default: return "?";
    }
}

extern "C" size_t ppy_jpeg_entropy_plan_bytes(int n, long long segments) {
    if (n <= 0 || segments < n) return 0;
    return ((size_t)n * sizeof(JpegEntItem) + ((size_t)segments + (size_t)n) * 4 + 15) / 16 * 16;
}

extern "C" int ppy_jpeg_entropy_plan(int n, const ppy_jpeg_desc_t *h_descs, const void *h_scan, size_t scan_bytes, const long long *h_scan_off,
                                     int subseq_bytes, void *h_plan, size_t plan_bytes, size_t *h_ws_bytes) {
    PPY_CHECK_ARG(n > 0 && n <= 65535 && h_descs && h_scan && h_scan_off && h_plan && h_ws_bytes && ((uintptr_t)h_plan & 15) == 0);
    if (subseq_bytes == 0) subseq_bytes = PPY_JPEG_SUBSEQ_DEFAULT;
    PPY_CHECK_ARG(subseq_bytes >= PPY_JPEG_SUBSEQ_MIN && subseq_bytes <= PPY_JPEG_SUBSEQ_MAX && (subseq_bytes & (subseq_bytes - 1)) == 0);
    PPY_CHECK_ARG(plan_bytes >= (size_t)n * sizeof(JpegEntItem));
    JpegEntItem *items = static_cast<JpegEntItem *>(h_plan);
    size_t at = (size_t)n * sizeof(JpegEntItem);
    unsigned long long total = 0;
    for (int i = 0; i < n; ++i) {
        // the record must be one ppy_jpeg_scan_prepare wrote for this descriptor: every offset the decoder follows is checked here
        const long long off = h_scan_off[i];
        PPY_CHECK_ARG(off >= 0 && off % 16 == 0 && (size_t)off + sizeof(ppy_jpeg_scan_t) <= scan_bytes);
        const unsigned char *rec = static_cast<const unsigned char *>(h_scan) + off;
        ppy_jpeg_scan_t H;
        memcpy(&H, rec, sizeof(H));
        const ppy_jpeg_desc_t &d = h_descs[i];
        PPY_CHECK_ARG(H.record_bytes <= scan_bytes - (size_t)off && (H.components == 1 || H.components == 3) && H.components == d.components);
        PPY_CHECK_ARG(H.segments >= 1 && H.mcus >= 1 && H.mcus_w >= 1 && (long long)H.mcus_w * H.mcus_h == H.mcus);
        PPY_CHECK_ARG(H.coef_elems * 2 == d.coef_bytes && d.coef_base >= 0 && d.coef_base % 16 == 0);
        PPY_CHECK_ARG(H.table_offset == sizeof(ppy_jpeg_scan_t) &&
                      H.segment_offset == H.table_offset + 2 * (unsigned)H.components * sizeof(JpegHuffDev) &&
                      H.data_offset == H.segment_offset + (unsigned long long)H.segments * sizeof(JpegSeg) &&
                      (unsigned long long)H.data_offset + H.data_bytes <= H.record_bytes);
        const int luma = H.h_samp[0] * H.v_samp[0];
        PPY_CHECK_ARG(H.h_samp[0] >= 1 && H.h_samp[0] <= 2 && H.v_samp[0] >= 1 && H.v_samp[0] <= 2 && (H.components == 3 || luma == 1));
        for (int c = 0; c < H.components; ++c) {
            PPY_CHECK_ARG((c == 0 || (H.h_samp[c] == 1 && H.v_samp[c] == 1)) && H.blocks_w[c] == H.mcus_w * H.h_samp[c] &&
                          H.coef_offset[c] == d.coef_offset[c] && d.blocks_w[c] == H.blocks_w[c] && d.blocks_h[c] == H.mcus_h * H.v_samp[c]);
        }
        PPY_CHECK_ARG(at + ((size_t)H.segments + 1) * 4 <= plan_bytes);
        uint32_t *sub_first = reinterpret_cast<uint32_t *>(static_cast<unsigned char *>(h_plan) + at);
        const JpegSeg *seg = reinterpret_cast<const JpegSeg *>(rec + H.segment_offset);
        unsigned long long subs = 0, mcu = 0;
        for (int s = 0; s < H.segments; ++s) {
            const unsigned long long bytes = seg[s].bit_len / 8, padded = (bytes + 3) / 4 * 4;
            PPY_CHECK_ARG(seg[s].byte_off % 4 == 0 && seg[s].bit_len % 8 == 0 && seg[s].byte_off + padded <= H.data_bytes);
            PPY_CHECK_ARG(seg[s].first_mcu == mcu && seg[s].mcu_count >= 1);
            mcu += seg[s].mcu_count;
            sub_first[s] = (uint32_t)subs;
            const unsigned long long k = (bytes + (unsigned)subseq_bytes - 1) / (unsigned)subseq_bytes;
            subs += k ? k : 1;      // a segment without data still has a lane: it reports that the data ends early
        }
        PPY_CHECK_ARG(mcu == (unsigned long long)H.mcus && subs < (1ull << 31) && total + subs < (1ull << 31));
        sub_first[H.segments] = (uint32_t)subs;
        JpegEntItem it;
        memset(&it, 0, sizeof(it));
        it.scan_off = off;
        it.coef_base = d.coef_base / 2;
        it.coef_elems = H.coef_elems;
        it.sub_first_off = (long long)at;
        it.sub_base = (uint32_t)total;
        it.nsub = (uint32_t)subs;
        items[i] = it;
        total += subs;
        at += ((size_t)H.segments + 1) * 4;
    }
    *h_ws_bytes = (state_bytes(total) + (size_t)total * 8 + 15) / 16 * 16;
    return PPY_OK;
}

// The rounds of group_rounds, lane by lane: st[0 .. m) are the group's states; every round reads the states of the round before.
static unsigned twin_rounds(const ppy_jpeg_scan_t &H, const JpegHuffDev *tabs, const SubView *v, int m, JpegSubState *st,
                            const JpegSubState &lane0_entry, bool lane0_dirty, bool all_dirty) {
    unsigned runs = 0;
    int changed[SUB_LANES], now[SUB_LANES];
    JpegSubState before[SUB_LANES];
    for (int t = 0; t < m; ++t) changed[t] = all_dirty;
    for (int round = 1; round <= SUB_LANES; ++round) {
        int any = 0;
        for (int t = 0; t < m; ++t) before[t] = st[t];
        for (int t = 0; t < m; ++t) {
            now[t] = 0;
            const bool dirty = !v[t].first && (t == 0 ? (round == 1 && lane0_dirty) : changed[t - 1] != 0);
            if (!dirty) continue;
            const JpegSubState nw = sync_decode(H, tabs, v[t], t == 0 ? lane0_entry : before[t - 1]);
            now[t] = !jpeg_state_equal(nw, st[t]);
            st[t] = nw;
            any |= now[t];
            ++runs;
        }
        for (int t = 0; t < m; ++t) changed[t] = now[t];
        if (!any) break;
    }
    return runs;
}

extern "C" int ppy_jpeg_entropy_twin(int n, const void *h_plan, const void *plan, const void *scan, int subseq_bytes, int16_t *coef,
                                     size_t coef_bytes, int *status, void *ws, size_t ws_bytes) {
    if (subseq_bytes == 0) subseq_bytes = PPY_JPEG_SUBSEQ_DEFAULT;
    uint32_t max_nsub = 0;
    unsigned long long total = 0;
    PPY_CHECK_ARG(plan_ok(n, h_plan, subseq_bytes, &max_nsub, &total) && plan && scan && coef && status);
    if (ws == nullptr || ws_bytes < state_bytes(total) + (size_t)total * 8) return PPY_ERR_WORKSPACE;
    const JpegEntItem *items = static_cast<const JpegEntItem *>(plan);
    const unsigned char *sc = static_cast<const unsigned char *>(scan), *pl = static_cast<const unsigned char *>(plan);
    JpegSubState *states = static_cast<JpegSubState *>(ws);
    unsigned long long *before = reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(ws) + state_bytes(total));
    const uint32_t bits = (uint32_t)subseq_bytes * 8;
    for (int i = 0; i < n; ++i) PPY_CHECK_ARG((unsigned long long)(items[i].coef_base + items[i].coef_elems) * 2 <= coef_bytes);
    memset(coef, 0, coef_bytes);
    memset(status, 0, (size_t)n * 3 * sizeof(int));
    for (int i = 0; i < n; ++i) {
        const JpegEntItem &it = items[i];
        const unsigned char *rec = sc + it.scan_off;
        const ppy_jpeg_scan_t &H = scan_header(sc, it);
        const JpegHuffDev *tabs = reinterpret_cast<const JpegHuffDev *>(rec + H.table_offset);
        const uint32_t *sub_first = reinterpret_cast<const uint32_t *>(pl + it.sub_first_off);
        JpegSubState *st = states + it.sub_base;
        SubView v[SUB_LANES];
        const uint32_t groups = (it.nsub + SUB_LANES - 1) / SUB_LANES;
        for (uint32_t g = 0; g < groups; ++g) {      // jpeg_huff_sync_kernel
            const uint32_t j0 = g * SUB_LANES;
            const int m = (int)(it.nsub - j0 < SUB_LANES ? it.nsub - j0 : SUB_LANES);
            for (int t = 0; t < m; ++t) {
                sub_view(H, rec, sub_first, j0 + t, bits, v[t]);
                st[j0 + t] = sync_decode(H, tabs, v[t], assumed_state(v[t]));
            }
            twin_rounds(H, tabs, v, m, st + j0, st[j0], false, true);
        }
        unsigned long long carry = 0;
        unsigned fixed = 0;
        for (uint32_t g = 0; g < groups; ++g) {      // jpeg_huff_link_kernel
            const uint32_t j0 = g * SUB_LANES;
            const int m = (int)(it.nsub - j0 < SUB_LANES ? it.nsub - j0 : SUB_LANES);
            for (int t = 0; t < m; ++t) sub_view(H, rec, sub_first, j0 + t, bits, v[t]);
            JpegSubState entry = assumed_state(v[0]);
            bool dirty0 = false;
            if (g && !v[0].first) {
                entry = st[j0 - 1];
                dirty0 = !jpeg_state_equal(entry, assumed_state(v[0]));
            }
            fixed += twin_rounds(H, tabs, v, m, st + j0, entry, dirty0, false);
            for (int t = 0; t < m; ++t) {
                before[it.sub_base + j0 + t] = carry;
                carry += st[j0 + t].count;
            }
        }
        status[2 * n + i] = (int)fixed;
        for (uint32_t j = 0; j < it.nsub; ++j) {      // jpeg_huff_write_kernel
            SubView w;
            sub_view(H, rec, sub_first, j, bits, w);
            const JpegSubState entry = w.first ? assumed_state(w) : st[j - 1];
            const int reason = write_decode(H, tabs, w, entry, before[it.sub_base + j] - before[it.sub_base + w.first_sub], coef + it.coef_base);
            if (reason) {
                status[i] = PPY_ERR_CORRUPT;
                status[n + i] = reason;
            }
        }
        for (int c = 0; c < H.components; ++c) {      // jpeg_dc_scan_kernel
            const long long cnt = (long long)H.mcus * H.h_samp[c] * H.v_samp[c];
            uint32_t pred = 0;
            for (long long q = 0; q < cnt; ++q) {
                bool reset = false;
                const long long at = dc_item(H, c, q, reset);
                if (reset) pred = 0;
                if (at < 0) continue;
                pred += (uint32_t)(int)coef[it.coef_base + at];
                coef[it.coef_base + at] = (int16_t)pred;
            }
        }
    }
    return PPY_OK;
}

#ifndef PPY_JPEG_HOST_ONLY
extern "C" int ppy_jpeg_entropy_device(int n, const void *h_plan, const void *plan, const void *scan, int subseq_bytes, int16_t *coef,
                                       size_t coef_bytes, int *status, void *ws, size_t ws_bytes, void *stream) {
    ppy_drop_stale_error();
    if (subseq_bytes == 0) subseq_bytes = PPY_JPEG_SUBSEQ_DEFAULT;
    uint32_t max_nsub = 0;
    unsigned long long total = 0;
    PPY_CHECK_ARG(plan_ok(n, h_plan, subseq_bytes, &max_nsub, &total) && plan && scan && coef && status);
    PPY_CHECK_ARG((((uintptr_t)plan | (uintptr_t)scan | (uintptr_t)coef | (uintptr_t)ws) & 15) == 0 && ((uintptr_t)status & 3) == 0);
    const JpegEntItem *h_items = static_cast<const JpegEntItem *>(h_plan);
    for (int i = 0; i < n; ++i) PPY_CHECK_ARG((unsigned long long)(h_items[i].coef_base + h_items[i].coef_elems) * 2 <= coef_bytes);
    if (ws == nullptr || ws_bytes < state_bytes(total) + (size_t)total * 8) return PPY_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const JpegEntItem *items = static_cast<const JpegEntItem *>(plan);
    const unsigned char *sc = static_cast<const unsigned char *>(scan), *pl = static_cast<const unsigned char *>(plan);
    JpegSubState *states = static_cast<JpegSubState *>(ws);
    unsigned long long *before = reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(ws) + state_bytes(total));
    const uint32_t bits = (uint32_t)subseq_bytes * 8;
    if (hipMemsetAsync(coef, 0, coef_bytes, st) != hipSuccess || hipMemsetAsync(status, 0, (size_t)n * 3 * sizeof(int), st) != hipSuccess)
        return ppy_launch_status();
    const dim3 grid((max_nsub + SUB_LANES - 1) / SUB_LANES, n);
    hipLaunchKernelGGL(jpeg_huff_sync_kernel, grid, dim3(SUB_LANES), 0, st, items, sc, pl, bits, states);
    hipLaunchKernelGGL(jpeg_huff_link_kernel, dim3(n), dim3(SUB_LANES), 0, st, items, sc, pl, bits, states, before, status, n);
    hipLaunchKernelGGL(jpeg_huff_write_kernel, grid, dim3(SUB_LANES), 0, st, items, sc, pl, bits, (const JpegSubState *)states,
                       (const unsigned long long *)before, coef, status, n);
    hipLaunchKernelGGL(jpeg_dc_scan_kernel, dim3(3, n), dim3(SUB_LANES), 0, st, items, sc, coef);
    return ppy_launch_status();
}
#endif  // PPY_JPEG_HOST_ONLY
