// ref_sanitize_main.cpp — the reference harness and its stand-in headers under AddressSanitizer / UndefinedBehaviorSanitizer.
//
// TEST INFRASTRUCTURE ONLY, written by this project; a stand-alone CPU program (`make -C oracle _ref_sanitize` builds and runs it), never loaded
// into Python.  It drives every entry point of ref_harness.cpp, under both readings of the UV fetch, over planes in which a share of the texels
// holds what the parity tests poison with: NaN, infinities, motions beyond the int range, -0.0, denormals, the depth sentinel, random half bits.
// The sanitizers (float -> integer casts included) stop the program at the first finding, in the stand-ins or in the filter source.
#include "ref_harness.cpp"

#include <cmath>
#include <cstdio>

static uint32_t state = 12345u;
static uint32_t rnd() { state = state * 1664525u + 1013904223u; return state >> 8; }
static float unit() { return (float)(rnd() & 0xffff) / 65536.0f; }
static uint16_t half_of(float f) { return __float2half(f).bits; }

int main() {
    const int W = 37, H = 29;
    const size_t n = (size_t)W * H;
    const float special[] = {NAN, INFINITY, -INFINITY, 1e20f, -1e20f, 3e9f, -3e9f, 2147483520.0f, -2147483648.0f, -0.0f, 1e30f, 0.0f, 1e-40f};
    const int nspecial = (int)(sizeof special / sizeof special[0]);
    std::vector<float> motion_c(4 * n), motion_p(4 * n), tone_in(4 * n), tone_out(4 * n);
    std::vector<uint16_t> normal_c(4 * n), normal_p(4 * n), uv_c(4 * n), uv_p(4 * n), prev(4 * n), cur(4 * n), out(4 * n), render(4 * n), mom_c(2 * n), mom_p(2 * n);
    std::vector<uint8_t> hist(n);
    for (int mode = 0; mode < 2; mode++) {
        if (svgf_ref_set_uv_fetch(mode)) return 2;
        for (size_t i = 0; i < n; i++) {
            for (int k = 0; k < 4; k++) {
                const size_t j = 4 * i + k;
                motion_c[j] = motion_p[j] = k < 2 ? unit() * 6.0f - 3.0f : 1.0f + unit();
                if (rnd() % 7 == 0) motion_c[j] = special[rnd() % nspecial];
                if (rnd() % 7 == 0) motion_p[j] = special[rnd() % nspecial];
                tone_in[j] = rnd() % 9 ? unit() * 1.5f - 0.1f : special[rnd() % nspecial];
                normal_c[j] = rnd() % 11 ? half_of(unit() * 2.0f - 1.0f) : (uint16_t)rnd();
                normal_p[j] = rnd() % 11 ? normal_c[j] : (uint16_t)rnd();
                uv_c[j] = rnd() % 5 ? half_of((float)(rnd() % 6)) : (uint16_t)rnd();
                uv_p[j] = rnd() % 5 ? uv_c[j] : (uint16_t)rnd();
                prev[j] = rnd() % 13 ? half_of(unit() * 1.5f - 0.2f) : (uint16_t)rnd();
                cur[j] = rnd() % 13 ? half_of(unit() * 1.5f - 0.2f) : (uint16_t)rnd();
            }
            mom_p[2 * i] = (uint16_t)rnd();
            mom_p[2 * i + 1] = half_of(unit());
            hist[i] = (uint8_t)rnd();
        }
        int rc = svgf_ref_temporal(W, H, prev.data(), cur.data(), motion_c.data(), normal_c.data(), uv_c.data(), motion_p.data(), normal_p.data(),
                                   uv_p.data(), hist.data(), mom_c.data(), mom_p.data(), 0.8f, 0.9f, 24);
        for (size_t i = 0; i < n; i++) hist[i] = (uint8_t)(rnd() % 8);
        rc |= svgf_ref_moments(W, H, prev.data(), out.data(), mom_p.data(), motion_c.data(), normal_c.data(), hist.data(), 10.0f, 128.0f);
        for (int step : {1, 2, 4, 16})
            rc |= svgf_ref_atrous(W, H, prev.data(), motion_c.data(), normal_c.data(), hist.data(), out.data(), render.data(), step, 0.05f, 0.5f, 0);
        rc |= svgf_ref_atrous(W, H, prev.data(), motion_c.data(), normal_c.data(), hist.data(), out.data(), nullptr, 2, 10.0f, 128.0f, 1);
        rc |= svgf_ref_taa(W, H, prev.data(), out.data());
        rc |= svgf_ref_tonemap(W, H, tone_in.data(), tone_out.data());
        std::printf("uv fetch %d: rc %d\n", mode, rc);
        if (rc) return 1;
    }
    std::vector<uint8_t> plane(n);
    if (svgf_ref_guard_selftest(W, H, 5, 5, 0, 0, plane.data()) != 0 || svgf_ref_guard_selftest(W, H, 5, 5, 1, 2, plane.data()) != -2) return 3;
    std::printf("sanitizers: nothing found\n");
    return 0;
}
