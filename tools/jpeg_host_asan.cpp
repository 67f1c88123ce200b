// Prefix and byte-flip sweep of the host JPEG stage (ppy_jpeg_info_ex, ppy_jpeg_entropy_decode_ex) for an AddressSanitizer build.
// Host code only: the device side of csrc/jpeg.hip is compiled out, nothing here touches a GPU.
//
//   clang++ -x c++ -DPPY_JPEG_HOST_ONLY -std=c++17 -g -O1 \
//       -fsanitize=address,undefined -fno-sanitize-recover=all \
//       pytorch-ppyolo_amd/ppyolo_hip/csrc/jpeg.hip tools/jpeg_host_asan.cpp -o /tmp/jpeg_host_asan
//   /tmp/jpeg_host_asan [--accept MASK] FILE.jpg [FILE.jpg ...]
//
// MASK: the PPY_JPEG_ACCEPT_* bits, default 0 (the baseline subset); 7 takes progressive files, several scans and the further
// luma sampling factors through the scan loop.
//
// Every input is copied into a heap block of exactly its size and the coefficient buffer has exactly coef_bytes, so a read or
// write one byte outside either is reported.  Prints one line per file; exit status 0 = every call returned a status code.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/ppyolo_hip.h"

static unsigned accept_mask = 0;

static int run(const unsigned char *src, size_t n, long long *counts) {
    unsigned char *d = (unsigned char *)malloc(n ? n : 1);
    if (n) memcpy(d, src, n);
    ppy_jpeg_info_t info;
    int rc = ppy_jpeg_info_ex(d, n, accept_mask, &info);
    if (rc == PPY_OK && info.coef_bytes <= (1ll << 26)) {
        int16_t *coef = (int16_t *)malloc((size_t)info.coef_bytes);
        ppy_jpeg_desc_t desc;
        memset(&desc, 0, sizeof(desc));
        char reason[64];
        rc = ppy_jpeg_entropy_decode_ex(d, n, accept_mask, coef, (size_t)info.coef_bytes, &desc, reason);
        free(coef);
    }
    free(d);
    if (rc != PPY_OK && rc != PPY_ERR_UNSUPPORTED && rc != PPY_ERR_CORRUPT) return 1;
    counts[rc == PPY_OK ? 0 : rc == PPY_ERR_UNSUPPORTED ? 1 : 2]++;
    return 0;
}

int main(int argc, char **argv) {
    int bad = 0;
    int first = 1;
    if (argc > 2 && strcmp(argv[1], "--accept") == 0) {
        accept_mask = (unsigned)strtoul(argv[2], nullptr, 0);
        first = 3;
    }
    for (int a = first; a < argc; ++a) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) return 2;
        std::vector<unsigned char> b;
        unsigned char buf[4096];
        for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) b.insert(b.end(), buf, buf + k);
        fclose(f);
        long long counts[3] = {0, 0, 0};
        const size_t stride = b.size() > 8192 ? 97 : 1;
        for (size_t n = 0; n <= b.size(); n += stride) bad += run(b.data(), n, counts);
        bad += run(b.data(), b.size(), counts);
        if (stride == 1) {
            std::vector<unsigned char> m(b);
            for (size_t i = 0; i < b.size(); ++i) {
                const unsigned char vals[3] = {0, 0xFF, (unsigned char)(b[i] ^ 0xFF)};
                for (unsigned char v : vals) {
                    m[i] = v;
                    bad += run(m.data(), m.size(), counts);
                }
                m[i] = b[i];
            }
        }
        printf("%s: %zu bytes, ok %lld, unsupported %lld, corrupt %lld\n", argv[a], b.size(), counts[0], counts[1], counts[2]);
    }
    return bad ? 1 : 0;
}
