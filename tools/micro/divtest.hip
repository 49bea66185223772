// Is the division by a constant of the box-grid kernels (div_const in csrc/kernels.hip: inside a window of exponents three instructions on a
// reciprocal refined once per thread, outside it the plain division for the whole wave) bitwise the compiler's own fp64 division?
// Numerators, in contiguous blocks so that whole waves stay on the fast path where the block allows it:
//   A  2^24 random bit patterns (all exponents, denormals, infinities, NaNs; every third with a moderate exponent), +-0, denormals, +-inf, NaN
//   B  2^22 random mantissas and signs with exponents drawn uniformly from E = 1023 - W - 4 .. 1023 + W + 4: both edges, from both sides
//   C  2^22 the same with E = 1023 - W .. 1023 + W: every wave on the fast path
// Divisors: ordinary, negative and extreme ones, and divisors just inside and just outside the divisor window.  For each divisor
//   wave  div_const as the kernels call it (a wave with one numerator outside the window takes the plain division)
//   lane  the three-instruction form on every numerator inside the window, whatever its neighbours are (plain division outside)
// are compared bit for bit against the device's a / b, and that against the host's.  Also counts the lanes that left the fast path.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/micro/divtest.hip -o tools/micro/divtest && tools/micro/divtest
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include <cstdint>
constexpr int kDivWindow = 256;
constexpr unsigned kDivWindowWidth = (unsigned)(2 * kDivWindow + 1) << 20;
struct DivConst {
    double b, r0;
    unsigned fast;
};
__device__ __forceinline__ unsigned div_window_pos(double v)
{
    return ((unsigned)__double2hiint(v) & 0x7fffffffu) - ((unsigned)(1023 - kDivWindow) << 20);
}
__device__ __forceinline__ DivConst make_div_const(double b)
{
    DivConst c;
    c.b = b;
    bool f;
    const double bs0 = __builtin_amdgcn_div_scale(1.0, b, false, &f);
    double r = __builtin_amdgcn_rcp(bs0);
    double e = __builtin_fma(-bs0, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-bs0, r, 1.0);
    r = __builtin_fma(r, e, r);
    c.r0 = r;
    c.fast = div_window_pos(b) < kDivWindowWidth && bs0 == b ? kDivWindowWidth : 0u;
    return c;
}
__device__ __forceinline__ double div_const(double a, const DivConst &c)
{
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(div_window_pos(a) >= c.fast) != 0ull, 0)) return a / c.b;  // wave-uniform
    const double q0 = a * c.r0;
    const double rem = __builtin_fma(-c.b, q0, a);
    return __builtin_fma(rem, c.r0, q0);
}
// counts[0]: lanes outside the window (or all lanes, divisor not fast); counts[1]: lanes of waves that took the plain division; counts[2]: c.fast
__global__ void k(const double *a, int n, double b, double *o1, double *o2, double *o3, unsigned long long *counts)
{
    const DivConst c = make_div_const(b);
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double ai = a[i];
    o1[i] = ai / b;
    const bool out = div_window_pos(ai) >= c.fast;
    if (out) atomicAdd(counts, 1ull);
    if (__builtin_amdgcn_ballot_w64(out) != 0ull) atomicAdd(counts + 1, 1ull);
    if (i == 0) counts[2] = c.fast;
    o2[i] = div_const(ai, c);
    double q = ai / b;
    if (!out) {
        const double q0 = ai * c.r0;
        const double rem = __builtin_fma(-c.b, q0, ai);
        q = __builtin_fma(rem, c.r0, q0);
    }
    o3[i] = q;
}
#define HIP_OK(x)                                                              \
    do {                                                                       \
        hipError_t e_ = (x);                                                   \
        if (e_ != hipSuccess) {                                                \
            printf("%s: %s\n", #x, hipGetErrorString(e_));                     \
            return 2;                                                          \
        }                                                                      \
    } while (0)
int main()
{
    const int nA = 1 << 24, nB = 1 << 22, nC = 1 << 22, n = nA + nB + nC;
    std::vector<double> h(n);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < n; ++i) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        uint64_t bits = s;
        const uint64_t draw = s >> 52;
        if (i < nA) {
            if (i % 3 == 0) bits = (bits & 0x800FFFFFFFFFFFFFull) | ((uint64_t)(1023 - 40 + draw % 80) << 52);  // moderate exponents
        } else if (i < nA + nB) {
            bits = (bits & 0x800FFFFFFFFFFFFFull) | ((uint64_t)(1023 - kDivWindow - 4 + draw % (2 * kDivWindow + 9)) << 52);
        } else {
            bits = (bits & 0x800FFFFFFFFFFFFFull) | ((uint64_t)(1023 - kDivWindow + draw % (2 * kDivWindow + 1)) << 52);
        }
        std::memcpy(&h[i], &bits, 8);
    }
    h[0] = 0.0; h[1] = -0.0; h[2] = 1e-320; h[3] = 1e308; h[4] = -1e308; h[5] = 5e-324;
    h[6] = INFINITY; h[7] = -INFINITY; h[8] = NAN; h[9] = -5e-324; h[10] = 2.2250738585072009e-308;  // (the largest denormal)
    // the window's own corners: smallest and largest numerators inside, their neighbours outside
    h[nA + 0] = std::ldexp(1.0, -kDivWindow); h[nA + 1] = std::nextafter(h[nA + 0], 0.0);
    h[nA + 2] = std::nextafter(std::ldexp(1.0, kDivWindow + 1), 0.0); h[nA + 3] = std::ldexp(1.0, kDivWindow + 1);
    for (int j = 0; j < 4; ++j) h[nA + 64 + j] = -h[nA + j];
    for (int j = 0; j < 4; ++j) h[nA + nB + 64 * j] = h[nA + 2 * (j & 1)] * (j & 2 ? -1.0 : 1.0);  // the inside corners in all-fast waves
    double *a, *o1, *o2, *o3; unsigned long long *counts;
    HIP_OK(hipMalloc(&a, (size_t)n * 8)); HIP_OK(hipMalloc(&o1, (size_t)n * 8)); HIP_OK(hipMalloc(&o2, (size_t)n * 8));
    HIP_OK(hipMalloc(&o3, (size_t)n * 8)); HIP_OK(hipMalloc(&counts, 24));
    HIP_OK(hipMemcpy(a, h.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    const double W2 = std::ldexp(1.0, kDivWindow);
    const double bs[] = {6.0, 10.0, 16.0, 28.0, 3.0, 7.123456789, 1e-300, 1e300, 4.9e-324, 44.0,      // the earlier list
                         2.0, 12.0, 0.1, 1.0 / 3.0, 1e10, 1e-10, 5.999999999999999, 1e77, 1e-77,      // ordinary ones
                         -6.0, -7.123456789, -1e-77,                                                  // negative ones
                         W2, 1.9999999 * W2, -1.7 * W2, 2.0 * W2, -2.0 * W2, 2.0000001 * W2,          // the upper edge of the divisor window, from both sides
                         1.0 / W2, 1.3 / W2, -1.0 / W2, 0.9999999 / W2, -0.9999999 / W2, 0.5 / W2};   // the lower edge
    std::vector<double> r1(n), r2(n), r3(n);
    printf("div_const against a / b: window W = %d (|E - 1023| <= W for divisor and numerator), %d numerators per divisor\n", kDivWindow, n);
    long total_bad = 0;
    for (double b : bs) {
        HIP_OK(hipMemset(counts, 0, 24));
        hipLaunchKernelGGL(k, dim3(n / 256), dim3(256), 0, 0, a, n, b, o1, o2, o3, counts);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(r1.data(), o1, (size_t)n * 8, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(r2.data(), o2, (size_t)n * 8, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(r3.data(), o3, (size_t)n * 8, hipMemcpyDeviceToHost));
        unsigned long long cnt[3];
        HIP_OK(hipMemcpy(cnt, counts, 24, hipMemcpyDeviceToHost));
        long bad = 0, badlane = 0, baddev = 0, badhost = 0;
        for (int i = 0; i < n; ++i) {
            if (std::memcmp(&r1[i], &r2[i], 8)) { if (bad < 3) printf("  wave: a=%a: %a vs %a\n", h[i], r1[i], r2[i]); ++bad; }
            if (std::memcmp(&r1[i], &r3[i], 8)) { if (badlane < 3) printf("  lane: a=%a: %a vs %a\n", h[i], r1[i], r3[i]); ++badlane; }
            const double c = h[i] / b;
            const bool nans = c != c;  // (NaN payloads are not compared: the host's and the device's differ)
            if (std::memcmp(&r1[i], &c, 8) && !(nans && r1[i] != r1[i])) ++baddev;
            if (std::memcmp(&r2[i], &c, 8) && !(nans && r2[i] != r2[i])) ++badhost;
        }
        total_bad += bad + badlane + baddev + badhost;
        printf("b=%-24.17g %s: differ from device '/': %ld (wave) %ld (lane); div_const differs from host '/': %ld; device '/' from host '/': %ld; "
               "lanes outside the window %llu, lanes of waves off the fast path %llu\n",
               b, cnt[2] ? "fast    " : "not fast", bad, badlane, badhost, baddev, cnt[0], cnt[1]);
    }
    printf("total differences: %ld\n", total_bad);
    return total_bad ? 1 : 0;
}
