// Sweep of the host side of the JPEG encoder (ppy_jpeg_enc_quant, _header, _layout, _pack_table, _scan_host) for an
// AddressSanitizer build.  Host code only: the device side of csrc/jpeg_encode.hip and csrc/jpeg.hip is compiled out, nothing
// here touches a GPU.
//
//   clang++ -x c++ -DPPY_JPEG_HOST_ONLY -std=c++17 -g -O1 \
//       -fsanitize=address,undefined -fno-sanitize-recover=all \
//       pytorch-ppyolo_amd/ppyolo_hip/csrc/jpeg_encode.hip pytorch-ppyolo_amd/ppyolo_hip/csrc/jpeg.hip \
//       tools/jpeg_encode_asan.cpp -o /tmp/jpeg_encode_asan
//   /tmp/jpeg_encode_asan
//
// Every buffer is a heap block of exactly the size the library asked for (header, coefficients, scan capacity, table), so a
// read or write one byte outside any of them is reported.  Coefficients are seeded: sparse, dense, and at the ends of the
// baseline range.  Each produced file goes back through the decoder's host stage and must return the same coefficients; bad
// parameters, short buffers and edited descriptors must return a status code.  Exit status 0 = all of that held.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../include/ppyolo_hip.h"

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 32);
}

static int fails = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("line %d: %s does not hold\n", __LINE__, #cond);   \
            ++fails;                                                  \
        }                                                             \
    } while (0)

static void one(int w, int h, int comps, int hs, int vs, int quality, int dri, int fill) {
    ppy_jpeg_enc_params_t p = {quality, hs, vs, dri};
    ppy_jpeg_enc_desc_t d;
    memset(&d, 0, sizeof(d));
    d.width = w;
    d.height = h;
    d.components = comps;
    d.row_stride = (long long)comps * w;
    ppy_jpeg_enc_sizes_t sz;
    char reason[64];
    EXPECT(ppy_jpeg_enc_layout(&p, 1, &d, &sz, reason) == PPY_OK);
    const size_t n = (size_t)d.coef_bytes / 2;
    int16_t *coef = (int16_t *)malloc(n * 2);
    for (size_t i = 0; i < n; ++i) {
        const bool dc = i % 64 == 0;
        int v = 0;
        if (fill == 0) v = rnd() % 8 == 0 ? (int)(rnd() % 61) - 30 : 0;              // sparse
        else if (fill == 1) v = (int)(rnd() % 2047) - 1023;                          // dense, the whole AC range
        else if (fill == 2) v = dc ? ((i / 64) & 1 ? 1023 : -1023) : (i % 64 == 63 ? -1023 : 0);      // DC size 11, long zero runs
        coef[i] = (int16_t)(dc && fill == 1 ? v / 2 : v);
    }
    unsigned char *out = (unsigned char *)malloc((size_t)d.scan_capacity);
    size_t len = 0;
    EXPECT(ppy_jpeg_enc_scan_host(&d, coef, n * 2, out, (size_t)d.scan_capacity, &len, reason) == PPY_OK);
    EXPECT(len <= (size_t)d.scan_capacity);
    const size_t hb = ppy_jpeg_enc_header_bytes(comps, dri);
    unsigned char *file = (unsigned char *)malloc(hb + len + 2);
    size_t used = 0;
    EXPECT(ppy_jpeg_enc_header(&p, w, h, comps, file, hb, &used, reason) == PPY_OK && used == hb);
    memcpy(file + hb, out, len);
    file[hb + len] = 0xFF;
    file[hb + len + 1] = 0xD9;
    int16_t *back = (int16_t *)malloc(n * 2);
    ppy_jpeg_desc_t dd;
    memset(&dd, 0, sizeof(dd));
    EXPECT(ppy_jpeg_entropy_decode(file, hb + len + 2, back, n * 2, &dd, reason) == PPY_OK);
    EXPECT(memcmp(back, coef, n * 2) == 0);
    // short buffers and an edited descriptor
    size_t len2 = 0;
    if (d.scan_capacity > 1) {
        unsigned char *tiny = (unsigned char *)malloc((size_t)d.scan_capacity - 1);
        EXPECT(ppy_jpeg_enc_scan_host(&d, coef, n * 2, tiny, (size_t)d.scan_capacity - 1, &len2, reason) == PPY_ERR_WORKSPACE);
        free(tiny);
    }
    EXPECT(ppy_jpeg_enc_scan_host(&d, coef, n * 2 - 2, out, (size_t)d.scan_capacity, &len2, reason) == PPY_ERR_BAD_ARG);
    unsigned char *shorthead = (unsigned char *)malloc(hb - 1);
    EXPECT(ppy_jpeg_enc_header(&p, w, h, comps, shorthead, hb - 1, &used, reason) == PPY_ERR_WORKSPACE);
    free(shorthead);
    ppy_jpeg_enc_desc_t bad = d;
    bad.blocks_h[0] += 1;
    EXPECT(ppy_jpeg_enc_scan_host(&bad, coef, n * 2, out, (size_t)d.scan_capacity, &len2, reason) == PPY_ERR_BAD_ARG);
    // the device table is packed into host memory of exactly its size
    d.src = (const unsigned char *)coef;      // any non-null pointer: it is stored, not read
    unsigned char *table = (unsigned char *)malloc(sz.table_bytes);
    EXPECT(ppy_jpeg_enc_pack_table(&p, 1, &d, table, sz.table_bytes) == PPY_OK);
    EXPECT(ppy_jpeg_enc_pack_table(&p, 1, &d, table, sz.table_bytes - 1) == PPY_ERR_BAD_ARG);
    EXPECT(ppy_jpeg_enc_pack_table(&p, 1, &bad, table, sz.table_bytes) == PPY_ERR_BAD_ARG);
    free(table);
    free(back);
    free(file);
    free(out);
    free(coef);
}

int main() {
    const int sizes[][2] = {{1, 1}, {7, 9}, {8, 8}, {17, 1}, {1, 17}, {33, 35}, {65, 33}, {200, 120}};
    const int samp[][3] = {{1, 1, 1}, {3, 1, 1}, {3, 2, 1}, {3, 2, 2}};
    const int quality[] = {1, 50, 95, 100}, dri[] = {0, 1, 3, 65535};
    int runs = 0;
    for (auto &s : sizes)
        for (auto &c : samp)
            for (int k = 0; k < 4; ++k)
                for (int fill = 0; fill < 3; ++fill, ++runs) one(s[0], s[1], c[0], c[1], c[2], quality[k], dri[(k + fill) % 4], fill);
    // parameters and sizes outside the contract
    ppy_jpeg_enc_sizes_t sz;
    ppy_jpeg_enc_desc_t d;
    char reason[64];
    unsigned char buf[1024];
    size_t used;
    const ppy_jpeg_enc_params_t badp[] = {{0, 2, 2, 0}, {101, 2, 2, 0}, {95, 2, 2, -1}, {95, 2, 2, 65536}, {95, 1, 2, 0}, {95, 4, 1, 0}, {95, 0, 0, 0}};
    for (auto &p : badp) {
        memset(&d, 0, sizeof(d));
        d.width = d.height = 16;
        d.components = 3;
        d.row_stride = 48;
        const int rc = ppy_jpeg_enc_layout(&p, 1, &d, &sz, reason);
        EXPECT(rc == PPY_ERR_BAD_ARG || rc == PPY_ERR_UNSUPPORTED);
        EXPECT(ppy_jpeg_enc_header(&p, 16, 16, 3, buf, sizeof(buf), &used, reason) == rc);
    }
    const ppy_jpeg_enc_params_t p = {95, 2, 2, 0};
    const int bads[][3] = {{0, 1, 3}, {1, 0, 3}, {65536, 1, 3}, {1, 65536, 1}, {8, 8, 2}, {8, 8, 0}};
    for (auto &b : bads) {
        memset(&d, 0, sizeof(d));
        d.width = b[0];
        d.height = b[1];
        d.components = b[2];
        d.row_stride = 1 << 20;
        EXPECT(ppy_jpeg_enc_layout(&p, 1, &d, &sz, reason) == PPY_ERR_BAD_ARG);
        EXPECT(ppy_jpeg_enc_header(&p, b[0], b[1], b[2], buf, sizeof(buf), &used, reason) == PPY_ERR_BAD_ARG);
    }
    EXPECT(ppy_jpeg_enc_layout(&p, 0, &d, &sz, reason) == PPY_ERR_BAD_ARG);
    EXPECT(ppy_jpeg_enc_layout(nullptr, 1, &d, &sz, nullptr) == PPY_ERR_BAD_ARG);
    // the largest image the format allows lays out without overflow (nothing is allocated from it here)
    memset(&d, 0, sizeof(d));
    d.width = d.height = 65535;
    d.components = 3;
    d.row_stride = 3ll * 65535;
    const ppy_jpeg_enc_params_t p444 = {95, 1, 1, 1};
    EXPECT(ppy_jpeg_enc_layout(&p444, 1, &d, &sz, reason) == PPY_OK && d.blocks == 3ll * 8192 * 8192 && d.segments == 8192ll * 8192);
    EXPECT((long long)sz.out_bytes == 416 * d.blocks + 4 * d.segments);
    printf("%d images swept, %d expectations failed\n", runs, fails);
    return fails ? 1 : 0;
}
