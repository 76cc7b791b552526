// Stand-alone driver of the host table code (csrc/resample_host.cpp) for a sanitizer build: compiled together with that file by
// the host compiler, with the Makefile's flags for it plus -fsanitize=address,undefined -fno-sanitize-recover=all, and run as a
// child process by tests/test_image_refs_cpu.py.  Every table goes into heap buffers of exactly out_size * 2 and
// out_size * ksize ints, so a write one element past either is an AddressSanitizer report.  Exit status 0: nothing reported and
// every structural property below holds.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "omr_hip.h"

namespace {

int failures = 0;

#define EXPECT(cond, ...)                      \
    do {                                       \
        if (!(cond)) {                         \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fputc('\n', stderr);          \
            ++failures;                        \
        }                                      \
    } while (0)

void one_pair(int in_size, int out_size, double* worst_headroom) {
    const int ks = omr_resample_ksize(in_size, out_size);
    EXPECT(ks >= 5 && ks % 2 == 1, "ksize(%d, %d) = %d", in_size, out_size, ks);
    if (ks <= 0) return;
    int* bounds = (int*)std::malloc(sizeof(int) * 2 * (size_t)out_size);
    int* coefs = (int*)std::malloc(sizeof(int) * (size_t)ks * (size_t)out_size);
    EXPECT(omr_resample_coeffs(in_size, out_size, bounds, coefs) == ks, "coeffs(%d, %d) != ksize", in_size, out_size);
    for (int x = 0; x < out_size; ++x) {
        const int xmin = bounds[2 * x], n = bounds[2 * x + 1];
        EXPECT(xmin >= 0 && n >= 1 && n <= ks && xmin + n <= in_size, "(%d, %d) pixel %d: window [%d, %d + %d)", in_size, out_size, x, xmin, xmin, n);
        long sum = 0, sum_abs = 0;
        for (int t = 0; t < ks; ++t) {
            const long c = coefs[(long)x * ks + t];
            EXPECT(t < n || c == 0, "(%d, %d) pixel %d: tap %d behind the window is %ld", in_size, out_size, x, t, c);
            sum += c;
            sum_abs += c < 0 ? -c : c;
        }
        EXPECT(sum >= (1L << 22) - ks && sum <= (1L << 22) + ks, "(%d, %d) pixel %d: taps sum to %ld", in_size, out_size, x, sum);
        const double headroom = (255.0 * (double)sum_abs + (double)(1L << 21)) / 2147483648.0;      // of the kernels' int32 accumulator
        EXPECT(headroom < 1.0, "(%d, %d) pixel %d: 255 sum |coef| + 2^21 = %.4f x 2^31", in_size, out_size, x, headroom);
        if (headroom > *worst_headroom) *worst_headroom = headroom;
    }
    std::free(bounds);
    std::free(coefs);
}

}  // namespace

int main() {
    double worst = 0.0;
    for (int in_size = 1; in_size <= 48; ++in_size)
        for (int out_size = 1; out_size <= 48; ++out_size) one_pair(in_size, out_size, &worst);
    const std::pair<int, int> extra[] = {{2048, 33}, {3000, 1500}, {699, 279}, {4096, 128}, {128, 4096}};
    for (const auto& p : extra) one_pair(p.first, p.second, &worst);

    // error paths: nothing may be written through the (exactly sized, or null) buffers
    int one_bounds[2] = {77, 77}, one_coef[5] = {77, 77, 77, 77, 77};
    EXPECT(omr_resample_ksize(0, 5) < 0 && omr_resample_ksize(5, 0) < 0 && omr_resample_ksize(-1, 5) < 0 && omr_resample_ksize(5, -7) < 0, "ksize accepts a size <= 0");
    EXPECT(omr_resample_coeffs(0, 1, one_bounds, one_coef) < 0 && omr_resample_coeffs(1, 0, one_bounds, one_coef) < 0, "coeffs accepts a size <= 0");
    EXPECT(omr_resample_coeffs(-4, 1, one_bounds, one_coef) < 0 && omr_resample_coeffs(1, -4, one_bounds, one_coef) < 0, "coeffs accepts a size < 0");
    EXPECT(omr_resample_coeffs(4, 4, nullptr, nullptr) < 0 && omr_resample_coeffs(1, 1, nullptr, one_coef) < 0 && omr_resample_coeffs(1, 1, one_bounds, nullptr) < 0,
           "coeffs accepts a null table");
    bool untouched = one_bounds[0] == 77 && one_bounds[1] == 77;
    for (int v : one_coef) untouched = untouched && v == 77;
    EXPECT(untouched, "a refused call wrote to its tables");

    std::printf("resample tables: %d failures, largest 255 sum |coef| + 2^21 = %.4f x 2^31\n", failures, worst);
    return failures == 0 ? 0 : 1;
}
