// stage4_identities_test.cpp -- the scaling identities behind the scan kernel's unscaled staging (csrc/eval_tile_stage.h Quad,
// EvalEngine::stage4_eligible; the limits: exact_math.h stage4_coef_ok / stage4_tap_ok), replayed on the host with the device's
// operations (std::fmaf is v_fma_f32; build with -ffp-contract=off) over everything the eligibility rule admits:
//   1. div25(4 x) == 4 div25(x)                         the device's three operations and the host's division
//   2. a * (4 s) + b * (4 m) == 4 (a * s + b * m)        s = n / 4, n = a [1 2 1] sum with its bias, m = the sample maximum
//   3. (k / 4) * (4 w - 4 mu) == k * (w - mu)            and the multiply-add form fma(k / 4, 4 w, acc) == fma(k, w, acc)
//   4. the bin rule: (int)med3(4 m, 0, 1020) >> 5 == (int)med3(m, 0, 255) >> 3
// and shows for each limit that one operand below it already breaks an identity.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "exact_math.h"

using namespace amt;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}
static uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float float_of(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static bool same(float a, float b) { return bits_of(a) == bits_of(b) || (a == 0.0f && b == 0.0f); }      // (a zero's sign cannot reach a score: exact_math.h)
// a float with a random sign and mantissa and an exponent in [lo, hi] (2^lo <= |f| < 2^(hi + 1))
static float rnd_float(int lo, int hi)
{
    const uint64_t r = rnd();
    const int e = lo + (int)((r >> 40) % (uint64_t)(hi - lo + 1));
    return float_of(((uint32_t)(r >> 63) << 31) | ((uint32_t)(e + 127) << 23) | ((uint32_t)r & 0x7FFFFFu));
}

static float div25_device(float x)
{
    const float z = 0.04f;
    const float q = x * z;
    const float r = std::fmaf(-25.0f, q, x);
    return std::fmaf(r, z, q);
}
// v_med3_f32 (a NaN operand: the minimum of the three, and v_min_f32 returns the operand that is a number)
static float med3(float a, float b, float c)
{
    if (a != a || b != b || c != c) return std::fmin(std::fmin(a, b), c);
    return std::fmax(std::fmin(a, b), std::fmin(std::fmax(a, b), c));
}
static int bin_plain(float m) { return (int)med3(m, 0.0f, 255.0f) >> 3; }
static int bin_scaled(float m4) { return (int)med3(m4, 0.0f, 1020.0f) >> 5; }

static long long failures = 0;
static void fail(const char* what, float a, float b, float c)
{
    if (failures++ < 10) std::printf("DIFFERENCE in %s: operands %a %a %a\n", what, a, b, c);
}

static void check_div25(float x)
{
    if (!same(div25_device(4.0f * x), 4.0f * div25_device(x))) fail("div25 (device)", x, 0, 0);
    if (!same(div25(4.0f * x), 4.0f * div25(x))) fail("div25 (host)", x, 0, 0);
    if (!same(div25_device(x), div25(x))) fail("div25 device against host", x, 0, 0);
}
static const float kMaxv[] = {255.0f, 1023.0f, 4095.0f, 65535.0f};
static void check_bg(float a, float b, unsigned n, float maxv)
{
    if (!stage4_coef_ok(a, b)) return;
    const float s = std::ldexp((float)n, -2), s4 = (float)n;
    const float bg = a * s + b * maxv;                               // (two roundings of the products, one of the sum: -ffp-contract=off)
    const float bg4 = a * s4 + b * (4.0f * maxv);
    if (!same(bg4, 4.0f * bg)) fail("a s + b maxv", a, b, s);
}
static void check_tap(float k, float w, float mu, float acc)
{
    if (!stage4_tap_ok(k)) return;
    const float k4 = 0.25f * k;
    if (!same(k4 * (4.0f * w - 4.0f * mu), k * (w - mu))) fail("k (w - m)", k, w, mu);
    if (!same(std::fmaf(k4, 4.0f * w, acc), std::fmaf(k, w, acc))) fail("fma(k, w, acc)", k, w, acc);
    if (!same(std::fmaf(-k4, 4.0f * mu, acc), std::fmaf(-k, mu, acc))) fail("fma(-sum k, M, acc)", k, mu, acc);
}
static void check_bins(float m)
{
    const float m4 = 4.0f * m;
    if (m4 - m4 == 0.0f && bin_scaled(m4) != bin_plain(m)) fail("bin >> 5 against >> 3", m, 0, 0);       // (4 m finite: |m| < 2^126)
    if (m != m && bin_scaled(m) != bin_plain(m)) fail("bin of a NaN", m, 0, 0);
}
int main()
{
    // ---- 1. div25.  The dividend is a window sum: 0, or a multiple of 2^-89 (stage4_eligible) up to 25 * 8192 * 65535 < 2^38 ----
    for (int e = -89; e <= 38; ++e)
        for (uint32_t mant : {0u, 1u, 0x400000u, 0x7FFFFFu, 0x2AAAAAu})
            for (uint32_t sign : {0u, 0x80000000u}) check_div25(float_of(sign | ((uint32_t)(e + 127) << 23) | mant));
    check_div25(0.0f);
    for (int i = 0; i <= 25 * 255 * 4; ++i) check_div25((float)i * 0.25f);                     // the sums of 8-bit s windows
    for (int i = 0; i < 3000000; ++i) check_div25(rnd_float(-89, 38));
    // ---- 2. bg.  Every [1 2 1] sum of 8-bit samples, the edges of the wider ones, the coefficient limits ----
    const float coefs[] = {0.0f, kStage4MinCoef, -kStage4MinCoef, float_of(bits_of(kStage4MinCoef) + 1), 1.0f, -1.0f, 1.0f / 3.0f, 8191.0f, -8191.0f, 4095.5f,
                           float_of(bits_of(8192.0f) - 1), 1e-10f, -3e-7f, 8100.0f, -90.0f};
    for (float a : coefs)
        for (float b : coefs)
            for (float maxv : kMaxv) {
                for (unsigned n = 0; n <= 4u * 255u + 2u; ++n) check_bg(a, b, n, maxv);
                for (unsigned n : {4u * 1023u, 4u * 1023u + 2u, 4u * 65535u - 1u, 4u * 65535u, 4u * 65535u + 1u, 4u * 65535u + 2u}) check_bg(a, b, n, maxv);
            }
    for (int i = 0; i < 3000000; ++i) {
        const float a = (rnd() & 15) == 0 ? 0.0f : rnd_float(-64, 12), b = (rnd() & 15) == 0 ? 0.0f : rnd_float(-64, 12);
        check_bg(a, b, (unsigned)(rnd() % (4u * 65535u + 3u)), kMaxv[rnd() & 3]);
    }
    // ---- 3. taps.  Window values and means up to 4 * 2^30; taps from the limit up; products in the denormal range included ----
    const float taps[] = {0.0f, kStage4MinTap, -kStage4MinTap, float_of(bits_of(kStage4MinTap) + 1), 1.0f, -0.3f, 123.456f, 1e-30f, 3e20f};
    const float vals[] = {0.0f, 0.25f, 0.5f, 255.0f, 254.75f, 65535.0f, 1e-20f, 1e-38f, 5.36e8f, -5.36e8f, 1.0f / 3.0f, float_of(1u)};
    for (float k : taps)
        for (float w : vals)
            for (float mu : vals)
                for (float acc : {0.0f, 1.0f, -1e-30f, 1e10f}) check_tap(k, w, mu, acc);
    for (int i = 0; i < 3000000; ++i) {
        const float k = rnd_float((rnd() & 7) == 0 ? -124 : -20, (rnd() & 7) == 0 ? -100 : 20);
        const float w = rnd_float(-40, 30), mu = (rnd() & 3) == 0 ? float_of(bits_of(w) + (uint32_t)(rnd() & 7)) : rnd_float(-40, 30);
        check_tap(k, w, mu, (rnd() & 1) ? rnd_float(-60, 40) : 0.0f);
    }
    // ---- 4. bins ----
    for (int c = 0; c <= 40; ++c)
        for (int d = -3; d <= 3; ++d) {
            check_bins(float_of(bits_of((float)(c * 8)) + (uint32_t)d));            // (around 0 this walks into the denormals / a NaN pattern: both checked)
        }
    for (float v : {-0.0f, 0.0f, -1e-45f, 1e-45f, -1e-20f, 1e-20f, 254.99998f, 255.0f, 255.25f, 255.99998f, 256.0f, 1e9f, -1e9f, 2.1e9f, 3e9f, 1e30f, -1e30f,
                    8388607.5f, 8388608.0f, 8388609.0f, 31.999998f, 32.0f, -0.99999994f, -1.0f, NAN}) {
        check_bins(v);
    }
    for (int i = 0; i < 3000000; ++i) {
        check_bins(rnd_float(-30, 12));
        check_bins((float)(rnd() % 2600000) * 1e-4f);                               // dense over [0, 260)
    }
    // ---- one operand below a limit already gives another result ----
    {
        const float a = float_of(bits_of(std::ldexp(1.0f, -126)) | 1u);             // a normal number, but a * 0.25 is rounded in the denormal range
        const float unscaled = a * 0.25f, scaled = a * 1.0f;
        if (stage4_coef_ok(a, 0.0f) || same(scaled, 4.0f * unscaled)) { std::printf("the coefficient limit admits %a\n", a); return 1; }
        const float k = float_of(bits_of(std::ldexp(1.0f, -126)) | 1u);             // k / 4 is not exact
        if (stage4_tap_ok(k) || same((0.25f * k) * 4.0f, k)) { std::printf("the tap limit admits %a\n", k); return 1; }
        if (!stage4_coef_ok(8100.0f, -90.0f) || stage4_coef_ok(8100.0f, -92.0f) || stage4_coef_ok(NAN, 0.0f) || stage4_tap_ok(NAN)) { std::printf("limits\n"); return 1; }
    }
    if (failures) { std::printf("%lld differences\n", failures); return 1; }
    std::printf("no difference\n");
    return 0;
}
