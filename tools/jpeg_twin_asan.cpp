// Prefix and byte-flip sweep of the DEVICE entropy stage's host side for an AddressSanitizer / UBSan build: the pre-pass
// (ppy_jpeg_scan_prepare), the batch plan and ppy_jpeg_entropy_twin, the host twin that runs the kernels' decode step, state
// comparison and slot-to-address map lane by lane.  Host code only: the kernels of csrc/jpeg_entropy.hip are compiled out,
// nothing here touches a GPU.  The sibling of tools/jpeg_host_asan.cpp, which sweeps the host entropy stage.
//
//   clang++ -x c++ -DPPY_JPEG_HOST_ONLY -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       pytorch-ppyolo_amd/ppyolo_hip/csrc/jpeg.hip pytorch-ppyolo_amd/ppyolo_hip/csrc/jpeg_entropy.hip \
//       tools/jpeg_twin_asan.cpp -o /tmp/jpeg_twin_asan
//   /tmp/jpeg_twin_asan [--subseq BYTES] FILE.jpg [FILE.jpg ...]
//
// Every buffer -- input, scan record, plan, coefficients, workspace, status -- is a heap block of exactly the size the library
// asked for, so a read or write one byte outside any of them is reported.  For every input the status class of (pre-pass,
// twin) must equal that of (ppy_jpeg_info, ppy_jpeg_entropy_decode), and where both are OK the coefficients must be equal.
// Prints one line per file; exit status 0 = no mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/ppyolo_hip.h"

static int g_subseq = PPY_JPEG_SUBSEQ_MIN;

static void *block(size_t n) {      // 16-byte aligned, exact size
    void *p = nullptr;
    if (posix_memalign(&p, 16, n ? n : 1) != 0) abort();
    return p;
}

static int host_stage(const unsigned char *d, size_t n, std::vector<int16_t> &coef) {
    ppy_jpeg_info_t info;
    int rc = ppy_jpeg_info(d, n, &info);
    if (rc != PPY_OK || info.coef_bytes > (1ll << 27)) return rc;
    coef.assign((size_t)info.coef_bytes / 2, 0x5a5a);
    ppy_jpeg_desc_t desc;
    memset(&desc, 0, sizeof(desc));
    char reason[64];
    return ppy_jpeg_entropy_decode(d, n, coef.data(), (size_t)info.coef_bytes, &desc, reason);
}

static int device_stage(const unsigned char *d, size_t n, std::vector<int16_t> &out) {
    long long segs = 0;
    const size_t bound = ppy_jpeg_scan_bytes(d, n, &segs);
    void *scan = block(bound ? bound : 16);
    ppy_jpeg_desc_t desc;
    memset(&desc, 0, sizeof(desc));
    char reason[64];
    size_t used = 0;
    int rc = ppy_jpeg_scan_prepare(d, n, scan, bound, &used, &desc, reason);
    if (rc == PPY_OK && desc.coef_bytes <= (1ll << 27)) {
        void *exact = block(used);      // the record alone: the decoder must not read past it
        memcpy(exact, scan, used);
        const size_t plan_bytes = ppy_jpeg_entropy_plan_bytes(1, segs);
        void *plan = block(plan_bytes);
        const long long off = 0;
        size_t ws_bytes = 0;
        rc = ppy_jpeg_entropy_plan(1, &desc, exact, used, &off, g_subseq, plan, plan_bytes, &ws_bytes);
        if (rc == PPY_OK) {
            int16_t *coef = (int16_t *)block((size_t)desc.coef_bytes);
            void *ws = block(ws_bytes);
            int *status = (int *)block(3 * sizeof(int));
            rc = ppy_jpeg_entropy_twin(1, plan, plan, exact, g_subseq, coef, (size_t)desc.coef_bytes, status, ws, ws_bytes);
            if (rc == PPY_OK) {
                rc = status[0];
                out.assign(coef, coef + desc.coef_bytes / 2);
            } else {
                rc = 100 + rc;      // not a status class: counted as a mismatch
            }
            free(status);
            free(ws);
            free(coef);
        } else {
            rc = 200 + rc;
        }
        free(plan);
        free(exact);
    }
    free(scan);
    return rc;
}

static int run(const unsigned char *src, size_t n, long long *counts) {
    unsigned char *d = (unsigned char *)malloc(n ? n : 1);
    memcpy(d, src, n);
    std::vector<int16_t> want, got;
    const int host = host_stage(d, n, want), dev = device_stage(d, n, got);
    free(d);
    if (host != dev || (host != PPY_OK && host != PPY_ERR_UNSUPPORTED && host != PPY_ERR_CORRUPT)) return 1;
    if (host == PPY_OK && want != got) return 1;
    counts[host == PPY_OK ? 0 : host == PPY_ERR_UNSUPPORTED ? 1 : 2]++;
    return 0;
}

int main(int argc, char **argv) {
    int bad = 0, a = 1;
    if (argc > 2 && strcmp(argv[1], "--subseq") == 0) {
        g_subseq = atoi(argv[2]);
        a = 3;
    }
    for (; a < argc; ++a) {
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
        printf("%s: %zu bytes, subsequences of %d, ok %lld, unsupported %lld, corrupt %lld, mismatches so far %d\n", argv[a], b.size(),
               g_subseq, counts[0], counts[1], counts[2], bad);
    }
    return bad ? 1 : 0;
}
