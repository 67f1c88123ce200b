// Sweep of the host planner of the Pillow resize (ppy_pil_resize_plan_bytes, ppy_pil_resize_plan) for an AddressSanitizer
// build.  Host code only: the kernels and launches of csrc/pil_resize.hip are compiled out, nothing here touches a GPU.
//
//   clang++ -x c++ -DPPY_PIL_HOST_ONLY -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       pytorch-ppyolo_amd/ppyolo_hip/csrc/pil_resize.hip tools/pil_resize_asan.cpp -o /tmp/pil_resize_asan
//   /tmp/pil_resize_asan
//
// Every blob is a heap block of exactly the size the library asked for, so a write one byte outside it is reported.  Each
// blob is then walked as the kernels walk it: every table a descriptor names lies inside the blob, every tap inside the
// source axis, every intermediate inside the workspace.  Batches outside the limits, short buffers and bad arguments must
// return a status code.  Exit status 0 = all of that held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

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

static unsigned char pixel;      // the descriptors only carry the address

static void walk_axis(const unsigned char *blob, long long blob_bytes, int off, int in, int out) {
    EXPECT(off >= 64 && off + 16 <= blob_bytes);
    int t[4];
    memcpy(t, blob + off, 16);
    EXPECT(t[0] == in && t[1] == out && t[2] >= 0 && t[2] <= 1024);
    const long long end = off + 16 + (long long)out * 8 + (long long)out * t[2] * 4;
    EXPECT(end <= blob_bytes);
    if (end > blob_bytes) return;
    const int *bounds = reinterpret_cast<const int *>(blob + off + 16);
    for (int x = 0; x < out; ++x) {
        EXPECT(bounds[2 * x] >= 0 && bounds[2 * x + 1] >= 1 && bounds[2 * x] + bounds[2 * x + 1] <= in);
        EXPECT(t[2] == 0 ? bounds[2 * x + 1] == 1 : bounds[2 * x + 1] <= t[2]);
    }
}

static void one(const std::vector<ppy_pil_image_t> &im, int ow, int oh, int filter) {
    const int n = (int)im.size();
    const size_t bytes = ppy_pil_resize_plan_bytes(n, im.data(), ow, oh, filter);
    bool long_taps = false;      // ksize = ceil(support * max(in / out, 1)) * 2 + 1 above 1024 on a resampled axis
    const double support = filter == 4 ? 0.5 : (filter == 2 || filter == 5) ? 1.0 : filter == 3 ? 2.0 : 3.0;
    for (const auto &d : im) {
        const int in[2] = {d.w, d.h}, out[2] = {ow, oh};
        for (int a = 0; a < 2; ++a)
            if (filter > 0 && in[a] != out[a] && std::ceil(support * std::fmax((double)in[a] / out[a], 1.0)) * 2 + 1 > 1024) long_taps = true;
    }
    if (long_taps) {
        char why[96];
        EXPECT(bytes == 0 && ppy_pil_resize_plan(n, im.data(), ow, oh, filter, nullptr, 0, nullptr, why) == PPY_ERR_UNSUPPORTED &&
               strstr(why, "ksize"));
        return;
    }
    EXPECT(bytes >= 64 + 48 * (size_t)n);
    if (!bytes) return;
    unsigned char *blob = static_cast<unsigned char *>(malloc(bytes));
    size_t ws = ~(size_t)0;
    char reason[96];
    EXPECT(ppy_pil_resize_plan(n, im.data(), ow, oh, filter, blob, bytes - 1, &ws, reason) == PPY_ERR_WORKSPACE);
    EXPECT(ppy_pil_resize_plan(n, im.data(), ow, oh, filter, blob, bytes, &ws, reason) == PPY_OK);
    int hi[8], ho[2];
    long long hl[2];
    memcpy(hi, blob, 32);
    memcpy(hl, blob + 32, 16);
    memcpy(ho, blob + 48, 8);
    EXPECT(hi[1] == n && hi[2] == ow && hi[3] == oh && hi[4] == filter && hl[0] == (long long)bytes && hl[1] == (long long)ws);
    EXPECT(hi[7] >= 3 * ow && ho[0] == 64);
    for (int i = 0; i < n; ++i) {
        const unsigned char *d = blob + 64 + 48 * (size_t)i;
        int q[4];
        long long mid;
        memcpy(q, d + 16, 16);
        memcpy(&mid, d + 32, 8);
        EXPECT(q[0] == im[i].h && q[1] == im[i].w);
        EXPECT((q[2] < 0) == (im[i].w == ow));
        if (q[2] >= 0) {
            walk_axis(blob, hl[0], q[2], im[i].w, ow);
            EXPECT(mid >= 0 && mid + (long long)im[i].h * hi[7] <= hl[1] && hi[6] >= im[i].h);
        }
        walk_axis(blob, hl[0], q[3], im[i].h, oh);
    }
    free(blob);
}

int main() {
    const int side[] = {1, 2, 3, 7, 16, 37, 53, 64, 200, 375, 480, 640, 1080, 1920};
    const int outs[] = {1, 2, 8, 16, 20, 32, 64, 608};
    for (int f = 0; f < 6; ++f)
        for (int round = 0; round < 60; ++round) {
            std::vector<ppy_pil_image_t> im(1 + rnd() % 6);
            for (auto &d : im) {
                d.base = &pixel;
                d.h = side[rnd() % 14];
                d.w = side[rnd() % 14];
                d.pitch = 3LL * d.w + rnd() % 9;
            }
            one(im, outs[rnd() % 8], outs[rnd() % 8], f);
        }
    for (int f = 0; f < 6; ++f) {      // the limits themselves: the longest tables the planner accepts
        one({{&pixel, 3, 65535, 1}}, 1, 8192, f);
        one({{&pixel, 3 * 65535, 1, 65535}}, 8192, 1, f);
    }
    one({{&pixel, 3 * 511, 511, 511}}, 1, 1, 2);                  // bilinear, ksize 1023
    one({{&pixel, 3 * 3840, 2160, 3840}}, 608, 608, 1);
    // refusals: a status code and a reason, nothing written
    char reason[96];
    unsigned char small[64];
    const ppy_pil_image_t ok = {&pixel, 30, 10, 10};
    const ppy_pil_image_t bad[] = {{&pixel, 30, 0, 10}, {&pixel, 30, 10, 65536}, {&pixel, 3 * 65535, 10, 65535}};
    EXPECT(ppy_pil_resize_plan_bytes(1, &bad[0], 16, 16, 3) == 0 && ppy_pil_resize_plan_bytes(1, &bad[1], 16, 16, 3) == 0);
    EXPECT(ppy_pil_resize_plan_bytes(1, &bad[2], 64, 16, 1) == 0);      // lanczos 65535 -> 64: ksize 6145
    EXPECT(ppy_pil_resize_plan(1, &bad[2], 64, 16, 1, small, sizeof small, nullptr, reason) == PPY_ERR_UNSUPPORTED && strstr(reason, "6145"));
    EXPECT(ppy_pil_resize_plan(1, &ok, 8193, 16, 3, small, sizeof small, nullptr, reason) == PPY_ERR_UNSUPPORTED && strstr(reason, "8193"));
    EXPECT(ppy_pil_resize_plan(1, &ok, 16, 16, 6, small, sizeof small, nullptr, reason) == PPY_ERR_UNSUPPORTED);
    EXPECT(ppy_pil_resize_plan(0, &ok, 16, 16, 3, small, sizeof small, nullptr, reason) == PPY_ERR_BAD_ARG);
    EXPECT(ppy_pil_resize_plan(1025, &ok, 16, 16, 3, small, sizeof small, nullptr, nullptr) == PPY_ERR_BAD_ARG);
    EXPECT(ppy_pil_resize_plan(1, nullptr, 16, 16, 3, small, sizeof small, nullptr, nullptr) == PPY_ERR_BAD_ARG);
    EXPECT(ppy_pil_resize_plan(1, &ok, 16, 16, 3, nullptr, 1 << 20, nullptr, nullptr) == PPY_ERR_BAD_ARG);
    const ppy_pil_image_t short_pitch = {&pixel, 29, 10, 10}, null_base = {nullptr, 30, 10, 10};
    void *big = malloc(1 << 16);
    EXPECT(ppy_pil_resize_plan(1, &short_pitch, 16, 16, 3, big, 1 << 16, nullptr, nullptr) == PPY_ERR_BAD_ARG);
    EXPECT(ppy_pil_resize_plan(1, &null_base, 16, 16, 3, big, 1 << 16, nullptr, nullptr) == PPY_ERR_BAD_ARG);
    free(big);
    printf(fails ? "%d checks failed\n" : "all planner checks held\n", fails);
    return fails ? 1 : 0;
}
