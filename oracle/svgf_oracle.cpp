// svgf_oracle.cpp — scalar CPU restatement of the SVGF hot path of jacquespillet/SVGF.
//
// TEST INFRASTRUCTURE ONLY.  Nothing under svgf_amd/ (the product) may include,
// link, import or execute this file.  Only tests/, __graft_entry__.smoke() and the
// cpu_baseline leg of bench.py use it, and only as the checker / reported baseline.
//
// PARITY: the reference repository has no tests, golden vectors or CPU implementation of the filter, and its
// application cannot be built without its toolchain.  Its filter source can: ref_harness.cpp compiles it for the host against the
// stand-in headers of ref_shim/, and the fp16 path of this restatement is held to that build bit for bit
// (tests/test_reference_parity.py).  The fp32 storage path and the G-buffer adapter are pinned by (a) hand-derivable known-answer
// cases and (b) an independently written NumPy restatement (oracle/svgf_numpy.py); see tests/test_oracle_*.py.
//
// Each function cites the reference lines (under /root/reference/) it follows.
// Arithmetic is fp32 with the reference's fp64 islands kept;
// compile with -ffp-contract=off so no FMA contraction changes the rounding.
//
// Geometry: every plane holds `rows` local rows of a W-wide, H-high global frame,
// local row 0 being global row y0 (single GPU / whole frame: y0 = 0, rows = H).
// Stages compute global rows [yb, ye).  "Inside the frame" always means the
// GLOBAL frame, exactly as the reference kernels test it.

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

namespace {

// The reference's fp64 islands are evaluated in `wide_t`.  The oracle proper keeps them (double).  A SECOND build of this
// file — libsvgf_oracle_fp32fma.so: -DSVGF_ORACLE_ALL_FP32 -ffp-contract=fast -mfma — evaluates them in fp32 and lets the compiler contract
// a*b+c into FMAs, as nvcc's default does to Filter.cuh:393-398,498-499,608: a second "correct" implementation of the same source.  The
// distance between the two, free-running on the same frames, is the envelope inside which the HIP path must sit (tests/test_gpu_parity.py,
// profiles/r05_parity_report.json: VERDICT r04 #4).
#ifdef SVGF_ORACLE_ALL_FP32
typedef float wide_t;
#else
typedef double wide_t;
#endif

struct Geo { int W, H, y0, rows, yb, ye; };

// ---------------------------------------------------------------- storage ----
// half <-> float: round-to-nearest-even like __float2half / exact like __half2float
// (reference Filter.cuh:15-52).
inline float h2f(uint16_t h) {
    uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    uint32_t exp  = (h >> 10) & 0x1fu;
    uint32_t man  = h & 0x3ffu;
    uint32_t out;
    if (exp == 0) {
        if (man == 0) out = sign;
        else {  // subnormal: value = man * 2^-24
            float v = (float)man * 5.9604644775390625e-8f;
            std::memcpy(&out, &v, 4);
            out |= sign;
        }
    } else if (exp == 31) out = sign | 0x7f800000u | (man << 13);
    else out = sign | ((exp + 112u) << 23) | (man << 13);
    float f; std::memcpy(&f, &out, 4); return f;
}

inline uint16_t f2h(float f) {
    uint32_t x; std::memcpy(&x, &f, 4);
    uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    uint32_t o;
    if (x >= 0x47800000u) {                 // >= 65536, inf or nan
        o = (x > 0x7f800000u) ? 0x7e00u : 0x7c00u;
    } else if (x < 0x38800000u) {           // below the smallest normal half: exact RNE through an fp32 add
        float a; std::memcpy(&a, &x, 4);
        const uint32_t magic_u = (uint32_t)((127 - 15) + (23 - 10) + 1) << 23;   // 0.5f
        float magic; std::memcpy(&magic, &magic_u, 4);
        a += magic;
        uint32_t au; std::memcpy(&au, &a, 4);
        o = au - magic_u;
    } else {
        uint32_t odd = (x >> 13) & 1u;
        x += 0xc8000fffu;                   // rebias exponent (15-127)<<23, plus rounding bias 0xfff
        x += odd;
        o = x >> 13;                        // [65520,65536) carries into the exponent -> 0x7c00
    }
    return (uint16_t)(o | sign);
}

struct F32 {                                 // "fp32 storage" extension (BASELINE configs #1-#4)
    static constexpr int kBytes4 = 16;
    static void ld4(const void* p, size_t i, float* v) { std::memcpy(v, (const float*)p + 4 * i, 16); }
    static void st4(void* p, size_t i, const float* v) { std::memcpy((float*)p + 4 * i, v, 16); }
    static void ld2(const void* p, size_t i, float* v) { std::memcpy(v, (const float*)p + 2 * i, 8); }
    static void st2(void* p, size_t i, const float* v) { std::memcpy((float*)p + 2 * i, v, 8); }
};
struct F16 {                                 // reference-native half4 / half2 (Filter.cuh:15-16)
    static void ld4(const void* p, size_t i, float* v) { const uint16_t* q = (const uint16_t*)p + 4 * i; for (int k = 0; k < 4; k++) v[k] = h2f(q[k]); }
    static void st4(void* p, size_t i, const float* v) { uint16_t* q = (uint16_t*)p + 4 * i; for (int k = 0; k < 4; k++) q[k] = f2h(v[k]); }
    static void ld2(const void* p, size_t i, float* v) { const uint16_t* q = (const uint16_t*)p + 2 * i; v[0] = h2f(q[0]); v[1] = h2f(q[1]); }
    static void st2(void* p, size_t i, const float* v) { uint16_t* q = (uint16_t*)p + 2 * i; q[0] = f2h(v[0]); q[1] = f2h(v[1]); }
};

inline float clamp01(float v) { return std::min(std::max(v, 0.0f), 1.0f); }   // glm::clamp = min(max(x,lo),hi)

// Envelope build "hwulp" only: v moved by -1, 0 or +1 unit in the last place, chosen by a hash of its own bits (deterministic: the same operand
// always gets the same nudge, as a hardware approximation does).  Every other build: the identity.
uint32_t g_hw_ulp_seed = 0u;      // svgf_oracle_set_hw_ulp_seed: another "unit" (another assignment of nudges to operands); set between frames only
inline float hw_ulp(float v, uint32_t salt) {
#ifdef SVGF_ORACLE_HW_ULP
    if (!(std::fabs(v) > 0.0f) || !(std::fabs(v) < 3.0e38f)) return v;           // zeros, infinities, NaN: as they are
    uint32_t b;
    std::memcpy(&b, &v, 4);
    uint32_t h = (b + salt + g_hw_ulp_seed * 0x9E3779B9u) * 2654435761u;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    b += (uint32_t)((int)(h % 3u) - 1);
    std::memcpy(&v, &b, 4);
#else
    (void)salt;
#endif
    return v;
}

// imageLoad (Filter.cuh:78-83): value clamped to [0,1] on all four channels.  The coordinate
// clamp never fires on this path (every caller tests "inside" first), so it is not restated.
template <class T> inline void image_load(const void* img, size_t idx, float* v) {
    T::ld4(img, idx, v);
    for (int k = 0; k < 4; k++) v[k] = clamp01(v[k]);
}
// imageStore (Filter.cuh:63-69)
template <class T> inline void image_store(void* img, size_t idx, const float* v) {
    float c[4]; for (int k = 0; k < 4; k++) c[k] = clamp01(v[k]);
    T::st4(img, idx, c);
}

// G-buffer fetches ------------------------------------------------------------
// GetDepth (Filter.cuh:199-207): (z,dz) = motion.zw ; z == 0 -> (1e30, 0)
inline void get_depth(const float* motion, size_t idx, float& z, float& dz) {
    z = motion[4 * idx + 2]; dz = motion[4 * idx + 3];
    if (z == 0.0f) { z = 1e30f; dz = 0.0f; }
}
// SampleCuTextureHalf4 (Filter.cuh:188-197): 4 x u16 half bits -> floats (xyz used)
inline void get_normal(const uint16_t* normal, size_t idx, float* n) {
    n[0] = h2f(normal[4 * idx]); n[1] = h2f(normal[4 * idx + 1]); n[2] = h2f(normal[4 * idx + 2]);
}
// int(x) / ivec2(vec2) on the device (Filter.cuh:232 `Coord + ivec2(MotionVector)`; the instance ID of :245-246) is PTX cvt.rzi.s32.f32:
// round toward zero, out-of-range values SATURATE, NaN converts to 0.  (A C++ cast of such a value is undefined — x86's cvttss2si
// returns INT_MIN for all of them, which is not what the reference's binary does: VERDICT r04.)  The sum with the pixel coordinate is a
// two's-complement add: INT_MAX + x wraps negative, so every saturated motion lands outside the frame and is rejected (:235).
inline int cvt_rzi_s32(float f) {
    if (f != f) return 0;
    if (f >= 2147483648.0f) return 2147483647;
    if (f <= -2147483648.0f) return -2147483647 - 1;
    return (int)f;
}
inline int add_wrap(int a, int b) { return (int)((uint32_t)a + (uint32_t)b); }
inline float dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }  // glm::dot
// CalculateLuminance (Filter.cuh:260-263)
inline float luminance(const float* c) { return 0.2126f * c[0] + 0.7152f * c[1] + 0.0722f * c[2]; }
inline float mixf(float x, float y, float a) { return x * (1.0f - a) + y * a; }                           // glm::mix

// computeWeight (Filter.cuh:407-427).  The double literals in :424 select CUDA's
// double max(float,double) and a double exp; the product with weightNormal is in double
// and rounds to float once.
inline float compute_weight(float zc, float zp, float phi_depth, const float* nc, const float* np,
                            float phi_normal, float lc, float lp, float phi_illum) {
    float d = clamp01(dot3(nc, np));
    if (!(d == d)) d = 0.0f;                                            // saturate(): NaN -> 0
#ifdef SVGF_ORACLE_FUSED_EXPONENT
    // Envelope build "fused" only (Makefile): the weight as ONE exp2 of a fused fp32 exponent, the divisions as multiplications by reciprocals —
    // the formulation of the HIP kernels (svgf_device.h: edge_weight), evaluated with libm.  A third correct reading of :407-427, like nvcc -use_fast_math.
    // Envelope build "hwulp" (-DSVGF_ORACLE_HW_ULP on top): the four results a GPU takes from its transcendental unit — log2, exp2 and the two
    // reciprocals — moved by -1 / 0 / +1 ulp (hw_ulp below): a model of v_log_f32 / v_exp_f32 / v_rcp_f32, which are 1-ulp approximations where
    // libm rounds correctly.  What that alone does to a free-running sequence is the envelope the fp16-under-a-pan case is held against.
    {
        const float ln = (phi_normal == 0.0f) ? 0.0f : phi_normal * hw_ulp(std::log2(d), 1u);
        const float wz1 = (phi_depth == 0) ? 0.0f : std::fabs(zc - zp) * hw_ulp(1.0f / phi_depth, 2u);
        const float wl1 = std::fabs(lc - lp) * hw_ulp(1.0f / phi_illum, 3u);
        return hw_ulp(std::exp2(ln - (std::fmax(wl1, 0.0f) + std::fmax(wz1, 0.0f)) * 1.4426950408889634f), 4u);
    }
#endif
    const float wn = std::pow(d, phi_normal);                           // powf
    const float wz = (phi_depth == 0) ? 0.0f : std::fabs(zc - zp) / phi_depth;
    const float wl = std::fabs(lc - lp) / phi_illum;
    const wide_t e = std::exp((wide_t)0.0 - std::fmax((wide_t)wl, (wide_t)0.0) - std::fmax((wide_t)wz, (wide_t)0.0)) * (wide_t)wn;
    return (float)e;
}

template <class F> void parallel_rows(int yb, int ye, int nthreads, F&& fn) {
    if (nthreads <= 1 || ye - yb < 2 * nthreads) { fn(yb, ye); return; }
    std::vector<std::thread> th;
    int n = ye - yb;
    for (int t = 0; t < nthreads; t++) {
        int a = yb + (int)((long long)n * t / nthreads), b = yb + (int)((long long)n * (t + 1) / nthreads);
        th.emplace_back([=, &fn] { fn(a, b); });
    }
    for (auto& t : th) t.join();
}

// ---------------------------------------------------------------- temporal ----
// TemporalFilter (Filter.cuh:359-404) with LoadPreviousData (Filter.cuh:225-258).
// History is ping-ponged (hist_prev read, hist_cur written): SURVEY.md App. B #1.
// mesh_id_test=1 implements the intended instance-ID comparison of :245-247, 0 the
// de-facto no-op (App. B #3).
template <class T>
void temporal(const Geo& g, const void* prev_colour, const void* cur_in, void* cur_out,
              const float* motion_c, const uint16_t* normal_c, const uint16_t* uv_c,
              const float* motion_p, const uint16_t* normal_p, const uint16_t* uv_p,
              const uint8_t* hist_prev, uint8_t* hist_cur, void* mom_cur, const void* mom_prev,
              float depth_thr, float normal_thr, int history_base, int mesh_id_test, int nthreads) {
    parallel_rows(g.yb, g.ye, nthreads, [&](int ya, int yb2) {
        for (int y = ya; y < yb2; y++)
            for (int x = 0; x < g.W; x++) {
                const size_t idx = (size_t)(y - g.y0) * g.W + x;
                float c[4]; image_load<T>(cur_in, idx, c);                        // :370
                float cp[3] = {0, 0, 0}, mp[2] = {0, 0};                          // :371,374
                int h = 1; float alpha;                                           // :372
                bool ok = false;
                const float mvx = motion_c[4 * idx], mvy = motion_c[4 * idx + 1]; // :230-231
                const int qx = add_wrap(x, cvt_rzi_s32(mvx)), qy = add_wrap(y, cvt_rzi_s32(mvy));   // :232 (toward 0, saturating, NaN -> 0)
                if (qx >= 0 && qx < g.W && qy >= 0 && qy < g.H) {                 // :235
                    const size_t q = (size_t)(qy - g.y0) * g.W + qx;
                    float zc, dzc, zp, dzp;
                    get_depth(motion_c, idx, zc, dzc); get_depth(motion_p, q, zp, dzp);   // :239-240
                    ok = !(std::fabs(zp - zc) > depth_thr);                       // :242
                    if (ok && mesh_id_test) {                                     // :245-247
                        const int idc = cvt_rzi_s32(h2f(uv_c[4 * idx + 3])), idp = cvt_rzi_s32(h2f(uv_p[4 * q + 3]));
                        ok = (idc == idp);
                    }
                    if (ok) {                                                     // :250-252
                        float nc[3], np[3]; get_normal(normal_c, idx, nc); get_normal(normal_p, q, np);
                        ok = !(dot3(nc, np) < normal_thr);
                    }
                    if (ok) {                                                     // :254-256
                        float pc[4]; image_load<T>(prev_colour, q, pc);
                        cp[0] = pc[0]; cp[1] = pc[1]; cp[2] = pc[2];
                        h = (int)hist_prev[q];
                        T::ld2(mom_prev, q, mp);
                    }
                }
                if (ok) { h = std::min(history_base, h + 1); alpha = (float)((wide_t)1.0 / (wide_t)h); }   // :380-381
                else    { alpha = 1.0f; h = 1; }                                                   // :385-386
                float m[2]; m[0] = luminance(c); m[1] = m[0] * m[0];              // :391-392
                m[0] = mixf(mp[0], m[0], alpha); m[1] = mixf(mp[1], m[1], alpha); // :393
                const float var = std::max(0.0f, m[1] - m[0] * m[0]);             // :396
                float out[4] = {mixf(cp[0], c[0], alpha), mixf(cp[1], c[1], alpha), mixf(cp[2], c[2], alpha), var}; // :398
                hist_cur[idx] = (uint8_t)h;                                       // :400
                image_store<T>(cur_out, idx, out);                                // :401
                T::st2(mom_cur, idx, m);                                          // :402
            }
    });
}

// ---------------------------------------------------------------- moments -----
// FilterMoments (Filter.cuh:430-525).  `radius` = 3 is the reference (:465).
template <class T>
void moments(const Geo& g, const void* colour, void* out, const void* mom, const float* motion,
             const uint16_t* normal, const uint8_t* hist, float phi_colour, float phi_normal,
             int radius, int nthreads) {
    parallel_rows(g.yb, g.ye, nthreads, [&](int ya, int yb2) {
        for (int y = ya; y < yb2; y++)
            for (int x = 0; x < g.W; x++) {
                const size_t idx = (size_t)(y - g.y0) * g.W + x;
                const float h = (float)hist[idx];                                 // :442
                float cc[4]; T::ld4(colour, idx, cc);                             // raw, :450
                if (h < 4.0f) {                                                   // :444
                    float sw = 0.0f, sc[3] = {0, 0, 0}, sm[2] = {0, 0};
                    const float lc = luminance(cc);                               // :451
                    float zc, dzc; get_depth(motion, idx, zc, dzc);               // :453
                    float nc[3]; get_normal(normal, idx, nc);                     // :459
                    const float phi_l = phi_colour;                               // :460
                    const float phi_d = (float)(std::fmax((wide_t)dzc, (wide_t)1e-8) * (wide_t)3.0);  // :461 (CUDA's max(float, double) is fmax: a NaN ddepth gives 1e-8)
                    for (int yy = -radius; yy <= radius; yy++)
                        for (int xx = -radius; xx <= radius; xx++) {              // :467-469
                            const int px = x + xx, py = y + yy;
                            if (!(px < g.W && py < g.H && px >= 0 && py >= 0)) continue;   // :473,477
                            const size_t p = (size_t)(py - g.y0) * g.W + px;
                            float cpix[4]; T::ld4(colour, p, cpix);               // :479 raw
                            float mpix[2]; T::ld2(mom, p, mpix);                  // :480
                            const float lp = luminance(cpix);                     // :481
                            float zp, dzp; get_depth(motion, p, zp, dzp);         // :482
                            float np[3]; get_normal(normal, p, np);               // :483
                            const float len = std::sqrt((float)(xx * xx + yy * yy));     // glm::length(vec2) :488
                            const float w = compute_weight(zc, zp, phi_d * len, nc, np, phi_normal, lc, lp, phi_l);
                            sw += w;                                              // :497
                            sc[0] += cpix[0] * w; sc[1] += cpix[1] * w; sc[2] += cpix[2] * w;   // :498
                            sm[0] += mpix[0] * w; sm[1] += mpix[1] * w;           // :499
                        }
                    sw = std::fmax(sw, 1e-6f);                                    // :505 (fmaxf)
                    float o[4] = {sc[0] / sw, sc[1] / sw, sc[2] / sw, 0};         // :507
                    sm[0] /= sw; sm[1] /= sw;                                     // :508
                    float var = sm[1] - sm[0] * sm[0];                            // :511
                    var = (float)((wide_t)var * ((wide_t)4.0 / (wide_t)h));               // :514
                    o[3] = var;
                    T::st4(out, idx, o);                                          // :516 unclamped
                } else {
                    T::st4(out, idx, cc);                                         // :521
                }
            }
    });
}

// ---------------------------------------------------------------- a-trous -----
// FilterKernel (Filter.cuh:527-624).
template <class T>
void atrous(const Geo& g, const void* in, void* out, void* feedback, const float* motion,
            const uint16_t* normal, int step, float phi_colour, float phi_normal, int iteration,
            int nthreads) {
    const float K[3] = {(float)1.0, (float)(2.0 / 3.0), (float)(1.0 / 6.0)};     // :540
    parallel_rows(g.yb, g.ye, nthreads, [&](int ya, int yb2) {
        for (int y = ya; y < yb2; y++)
            for (int x = 0; x < g.W; x++) {
                const size_t idx = (size_t)(y - g.y0) * g.W + x;
                float c[4]; image_load<T>(in, idx, c);                            // :543
                const float lc = luminance(c);                                    // :544
                const float var = c[3];                                           // :547
                float zc, dzc; get_depth(motion, idx, zc, dzc);                   // :552
                if (zc == 1e30f) { T::st4(out, idx, c); continue; }               // :554-558 (no feedback)
                float nc[3]; get_normal(normal, idx, nc);                         // :560
                const float eps = 1e-10f;
                const float phi_l = hw_ulp((float)((wide_t)phi_colour * std::sqrt(std::max((wide_t)0.0, (wide_t)(eps + var)))), 5u);  // :562 ("hwulp" build: a v_rsq_f32 result)
                const float phi_d = std::fmax(dzc, 1e-6f) * (float)step;          // :563 (CUDA's max(float, float) is fmaxf: a NaN ddepth gives 1e-6)
                float sw = 1.0f;                                                  // :567
                float s[4] = {c[0], c[1], c[2], c[3]};                            // :568
                for (int yy = -2; yy <= 2; yy++)
                    for (int xx = -2; xx <= 2; xx++) {                            // :571-573
                        const int px = x + xx * step, py = y + yy * step;         // :576
                        const bool inside = px < g.W && py < g.H && px >= 0 && py >= 0;   // :579
                        const float kern = K[std::abs(xx)] * K[std::abs(yy)];     // :582
                        if (!(inside && (xx != 0 || yy != 0))) continue;          // :584
                        const size_t p = (size_t)(py - g.y0) * g.W + px;
                        float q[4]; image_load<T>(in, p, q);                      // :586
                        const float lp = luminance(q);                            // :587
                        float zp, dzp; get_depth(motion, p, zp, dzp);             // :588
                        float np[3]; get_normal(normal, p, np);                   // :589
                        const float len = std::sqrt((float)(xx * xx + yy * yy));  // :595
                        const float w = compute_weight(zc, zp, phi_d * len, nc, np, phi_normal, lc, lp, phi_l);
                        const float iw = w * kern;                                // :604
                        sw += iw;                                                 // :607
                        s[0] += iw * q[0]; s[1] += iw * q[1]; s[2] += iw * q[2];  // :608
                        s[3] += (iw * iw) * q[3];
                    }
#ifdef SVGF_ORACLE_HW_ULP
                const float inv = hw_ulp(1.0f / sw, 6u);                          // ("hwulp" build: the normalisation by a v_rcp_f32 result, as the kernels do)
                float o[4] = {s[0] * inv, s[1] * inv, s[2] * inv, s[3] * (inv * inv)};
#else
                float o[4] = {s[0] / sw, s[1] / sw, s[2] / sw, s[3] / (sw * sw)};  // :615
#endif
                T::st4(out, idx, o);                                              // :618 unclamped
                if (iteration == 0 && feedback) T::st4(feedback, idx, o);         // :619-622
            }
    });
}


// ---------------------------------------------------------------- TAA + sRGB --
// TAAFilterKernel (Filter.cuh:288-357) with its helpers textureSample (:116-131: the bilinear path is dead code,
// it returns the nearest texel c00), encodePalYuv/decodePalYuv (:267-285) and ToSRGB (:145-157).
// The reference reads the history from the very buffer it writes (Output, App.cu:520) at a DIFFERENT pixel
// (the uv*(W-1) mapping below lands on pixel k-1), a cross-thread race; here the previous output is a separate
// plane (snapshot semantics), like the history-length fix of the temporal stage.
inline int tex_coord(float uv, int n) {                                  // :118-130
    const float x = uv * (float)(n - 1);
    const int x0 = (int)std::floor(x);
    return std::min(std::max(x0, 0), n - 1);
}
inline void enc_yuv(const float* rgb, float* yuv) {                       // :267-275
    const float r = std::pow(rgb[0], 2.0f), g = std::pow(rgb[1], 2.0f), b = std::pow(rgb[2], 2.0f);
    yuv[0] = (r * (float)0.299 + g * (float)0.587) + b * (float)0.114;
    yuv[1] = (r * (float)-0.14713 + g * (float)-0.28886) + b * (float)0.436;
    yuv[2] = (r * (float)0.615 + g * (float)-0.51499) + b * (float)-0.10001;
}
inline void dec_yuv(const float* yuv, float* rgb) {                       // :277-285
    const float r = (yuv[0] * 1.0f + yuv[1] * 0.0f) + yuv[2] * (float)1.13983;
    const float g = (yuv[0] * 1.0f + yuv[1] * (float)-0.39465) + yuv[2] * (float)-0.58060;
    const float b = (yuv[0] * 1.0f + yuv[1] * (float)2.03211) + yuv[2] * 0.0f;
    rgb[0] = std::pow(r, 0.5f); rgb[1] = std::pow(g, 0.5f); rgb[2] = std::pow(b, 0.5f);
}
inline float to_srgb(float c) {                                           // :145-148
    return (c <= 0.0031308f) ? 12.92f * c : (1 + 0.055f) * std::pow(c, 1 / 2.4f) - 0.055f;
}

template <class T>
void taa(const Geo& g, const void* input, const void* history, void* out, int nthreads) {
    const float inv_w = 1.0f / (float)g.W, inv_h = 1.0f / (float)g.H;     // InvTexResolution :294, off :304
    auto sample = [&](const void* img, float u, float v, float* c) {      // textureSample + imageLoad (value clamp)
        const int sx = tex_coord(u, g.W), sy = tex_coord(v, g.H);
        image_load<T>(img, (size_t)(sy - g.y0) * g.W + sx, c);
    };
    parallel_rows(g.yb, g.ye, nthreads, [&](int ya, int yb2) {
        for (int y = ya; y < yb2; y++)
            for (int x = 0; x < g.W; x++) {
                const float u = (float)x * inv_w, v = (float)y * inv_h;   // :296
                float last[4]; sample(history, u, v, last);               // :299
                float aa[3] = {last[0], last[1], last[2]};
                const float mix_rate = (float)std::fmin((double)last[3], 0.5);  // :302 min(float, double literal): CUDA's overload is fmin (a NaN alpha gives 0.5)
                float in[9][4];
                sample(input, u, v, in[0]);                               // :305
                for (int k = 0; k < 3; k++) aa[k] = std::sqrt(mixf(aa[k] * aa[k], in[0][k] * in[0][k], mix_rate));   // :307-308
                sample(input, u + inv_w, v, in[1]);          sample(input, u - inv_w, v, in[2]);            // :310-311
                sample(input, u, v + inv_h, in[3]);          sample(input, u, v - inv_h, in[4]);            // :312-313
                sample(input, u + inv_w, v + inv_h, in[5]);  sample(input, u - inv_w, v + inv_h, in[6]);    // :314-315
                sample(input, u + inv_w, v - inv_h, in[7]);  sample(input, u - inv_w, v - inv_h, in[8]);    // :316-317
                float ya_[3]; enc_yuv(aa, ya_);                           // :319
                float yin[9][3];
                for (int k = 0; k < 9; k++) enc_yuv(in[k], yin[k]);       // :320-328
                float mn[3], mx[3];
                for (int k = 0; k < 3; k++) {
                    mn[k] = std::min(std::min(std::min(yin[0][k], yin[1][k]), std::min(yin[2][k], yin[3][k])), yin[4][k]);   // :330
                    mx[k] = std::max(std::max(std::max(yin[0][k], yin[1][k]), std::max(yin[2][k], yin[3][k])), yin[4][k]);   // :331
                    const float mn2 = std::min(std::min(std::min(yin[5][k], yin[6][k]), std::min(yin[7][k], yin[8][k])), mn[k]);
                    const float mx2 = std::max(std::max(std::max(yin[5][k], yin[6][k]), std::max(yin[7][k], yin[8][k])), mx[k]);
                    mn[k] = mixf(mn[k], mn2, 0.5f);                       // :332-333
                    mx[k] = mixf(mx[k], mx2, 0.5f);                       // :334-335
                    ya_[k] = std::min(std::max(ya_[k], mn[k]), mx[k]);    // :338 (the mixRate update :340-346 has no effect on the output)
                }
                float rgb[3]; dec_yuv(ya_, rgb);                          // :348
                float o[4] = {rgb[0], rgb[1], rgb[2], 1.0f};              // :350
                if (std::isnan(o[0]) || std::isnan(o[1]) || std::isnan(o[2])) o[0] = o[1] = o[2] = o[3] = 0.0f;   // :351
                float res[4] = {to_srgb(o[0]), to_srgb(o[1]), to_srgb(o[2]), 1.0f};   // :353
                image_store<T>(out, (size_t)(y - g.y0) * g.W + x, res);   // :355
            }
    });
}

}  // namespace

// ---------------------------------------------------------------- C entry -----
// Albedo demodulation / re-modulation around the filter.  NOT in the reference — its README says so
// (README.md:14,172-174) — so this restates the build's own definition (include/svgf.h), not reference code:
//   demodulate: illumination.rgb = radiance.rgb / max(albedo.rgb, 1e-3), .w = radiance.w      (IEEE division; max = fmaxf)
//   modulate:   colour.rgb = illumination.rgb * max(albedo.rgb, 1e-3),   .w = illumination.w
template <class T> void albedo_op(int mode, size_t n, const void* in, const void* albedo, void* out) {
    for (size_t i = 0; i < n; i++) {
        float c[4], al[4], o[4];
        T::ld4(in, i, c);
        T::ld4(albedo, i, al);
        for (int k = 0; k < 3; k++) {
            const float d = std::fmax(al[k], 1e-3f);                                 // max(float, float) as CUDA has it: fmaxf — a NaN albedo reads as the floor
            o[k] = mode == 0 ? c[k] / d : c[k] * d;
        }
        o[3] = c[3];
        T::st4(out, i, o);
    }
}

extern "C" {

// storage: 0 = fp32 colour/moments, 1 = fp16 colour/moments (reference-native)
int svgf_oracle_temporal(int W, int H, int y0, int rows, int yb, int ye, int storage,
                         const void* prev_colour, const void* cur_in, void* cur_out,
                         const float* motion_c, const uint16_t* normal_c, const uint16_t* uv_c,
                         const float* motion_p, const uint16_t* normal_p, const uint16_t* uv_p,
                         const uint8_t* hist_prev, uint8_t* hist_cur, void* mom_cur, const void* mom_prev,
                         float depth_thr, float normal_thr, int history_base, int mesh_id_test, int nthreads) {
    Geo g{W, H, y0, rows, yb, ye};
    history_base = std::min(std::max(history_base, 1), 255);
    if (storage == 0) temporal<F32>(g, prev_colour, cur_in, cur_out, motion_c, normal_c, uv_c, motion_p, normal_p, uv_p, hist_prev, hist_cur, mom_cur, mom_prev, depth_thr, normal_thr, history_base, mesh_id_test, nthreads);
    else if (storage == 1) temporal<F16>(g, prev_colour, cur_in, cur_out, motion_c, normal_c, uv_c, motion_p, normal_p, uv_p, hist_prev, hist_cur, mom_cur, mom_prev, depth_thr, normal_thr, history_base, mesh_id_test, nthreads);
    else return -1;
    return 0;
}

int svgf_oracle_moments(int W, int H, int y0, int rows, int yb, int ye, int storage,
                        const void* colour, void* out, const void* mom, const float* motion,
                        const uint16_t* normal, const uint8_t* hist, float phi_colour, float phi_normal,
                        int radius, int nthreads) {
    Geo g{W, H, y0, rows, yb, ye};
    if (storage == 0) moments<F32>(g, colour, out, mom, motion, normal, hist, phi_colour, phi_normal, radius, nthreads);
    else if (storage == 1) moments<F16>(g, colour, out, mom, motion, normal, hist, phi_colour, phi_normal, radius, nthreads);
    else return -1;
    return 0;
}

int svgf_oracle_atrous(int W, int H, int y0, int rows, int yb, int ye, int storage,
                       const void* in, void* out, void* feedback, const float* motion,
                       const uint16_t* normal, int step, float phi_colour, float phi_normal,
                       int iteration, int nthreads) {
    Geo g{W, H, y0, rows, yb, ye};
    if (storage == 0) atrous<F32>(g, in, out, feedback, motion, normal, step, phi_colour, phi_normal, iteration, nthreads);
    else if (storage == 1) atrous<F16>(g, in, out, feedback, motion, normal, step, phi_colour, phi_normal, iteration, nthreads);
    else return -1;
    return 0;
}

int svgf_oracle_taa(int W, int H, int y0, int rows, int yb, int ye, int storage, const void* input, const void* history,
                    void* out, int nthreads) {
    Geo g{W, H, y0, rows, yb, ye};
    if (storage == 0) taa<F32>(g, input, history, out, nthreads);
    else if (storage == 1) taa<F16>(g, input, history, out, nthreads);
    else return -1;
    return 0;
}

int svgf_oracle_albedo(int mode, int W, int rows, int storage, const void* in, const void* albedo, void* out) {
    const size_t n = (size_t)W * rows;
    if (storage == 0) albedo_op<F32>(mode, n, in, albedo, out);
    else if (storage == 1) albedo_op<F16>(mode, n, in, albedo, out);
    else return -1;
    return 0;
}

// The stage in front of the path: what resources/shaders/GBuffer.frag:62-88 writes per fragment, given GBuffer.vert:21-34's
// interpolated attributes as linear planes (position {world xyz, primitive id}, normal {world normal, material id}, bary {b0,b1,b2, instance id};
// float4 each), MVP = view_proj, PreviousMVP = prev_view_proj (column-major, static geometry: ModelMatrix = identity), CameraPosition = cam.
//   GBuffer.vert:23,31      CurrentScreenPos = MVP * vec4(p, 1);  PrevScreenPos = PreviousMVP * vec4(p, 1)
//   GBuffer.frag:65-67      both / .w;  MotionVector = (prev.xy - cur.xy) * (0.5 * vec2(Width, Height))
//   GBuffer.frag:68         Depth = distance(CameraPosition, OutPosition.xyz)
//   GBuffer.frag:69         DepthDerivative = max(abs(dFdx(Depth)), abs(dFdy(Depth))): differences inside the fragment's 2x2 quad (x ^ 1, y ^ 1);
//                           a neighbour without geometry contributes 0 (OpenGL extrapolates the triangle there: no image-space adapter can)
//   GBuffer.frag:62,77,84   OutNormal = packHalf(normalize(FragNormal), MaterialIndex);  :61,76,85  OutUV = packHalf(BarycentricCoord, InstanceIndex)
// A texel whose normal is (0,0,0) has no geometry: the cleared texel, all zero (App.cu:383-384).  Unfused fp32, one rounding per operation
// (this file is built with -ffp-contract=off), written from the shader, not from the NumPy restatement (oracle/svgf_numpy.py:pack_gbuffer) it is
// checked against in tests/test_oracle_fuzz.py.
int svgf_oracle_pack_gbuffer(int W, int H, const float* position, const float* normal, const float* bary, const float* view_proj,
                             const float* prev_view_proj, const float* cam, float* motion_out, uint16_t* normal_out, uint16_t* uv_out) {
    if (W <= 0 || H <= 0 || !position || !normal || !bary || !view_proj || !prev_view_proj || !cam || !motion_out || !normal_out || !uv_out) return -1;
    auto covered = [&](int x, int y) { const float* n = normal + ((size_t)y * W + x) * 4; return !(n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f); };
    auto depth_at = [&](int x, int y) {
        const float* p = position + ((size_t)y * W + x) * 4;
        const float dx = cam[0] - p[0], dy = cam[1] - p[1], dz = cam[2] - p[2];
        return std::sqrt((dx * dx + dy * dy) + dz * dz);                              // distance()
    };
    auto mul = [](const float* m, const float* p, float* o) {                         // column-major m * vec4(p, 1)
        for (int r = 0; r < 4; r++) o[r] = ((m[r] * p[0] + m[4 + r] * p[1]) + m[8 + r] * p[2]) + m[12 + r];
    };
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t i = (size_t)y * W + x;
            float* mo = motion_out + i * 4;
            uint16_t* no = normal_out + i * 4;
            uint16_t* uo = uv_out + i * 4;
            if (!covered(x, y)) {
                for (int k = 0; k < 4; k++) { mo[k] = 0.0f; no[k] = 0; uo[k] = 0; }
                continue;
            }
            const float* p = position + i * 4;
            float cur[4], prev[4];
            mul(view_proj, p, cur);
            mul(prev_view_proj, p, prev);
            mo[0] = (prev[0] / prev[3] - cur[0] / cur[3]) * (0.5f * (float)W);
            mo[1] = (prev[1] / prev[3] - cur[1] / cur[3]) * (0.5f * (float)H);
            const float d = depth_at(x, y);
            float ddx = 0.0f, ddy = 0.0f;
            const int xp = x ^ 1, yp = y ^ 1;
            if (xp < W && covered(xp, y)) ddx = std::fabs(depth_at(xp, y) - d);
            if (yp < H && covered(x, yp)) ddy = std::fabs(depth_at(x, yp) - d);
            mo[2] = d;
            mo[3] = std::fmax(ddx, ddy);
            const float* n = normal + i * 4;
            const float len = std::sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);    // normalize()
            no[0] = f2h(n[0] / len); no[1] = f2h(n[1] / len); no[2] = f2h(n[2] / len); no[3] = f2h(n[3]);
            const float* b = bary + i * 4;
            for (int k = 0; k < 4; k++) uo[k] = f2h(b[k]);
        }
    return 0;
}

// envelope build "hwulp" only (a no-op in every other build): which of its possible "transcendental units" the build models
void svgf_oracle_set_hw_ulp_seed(uint32_t seed) { g_hw_ulp_seed = seed; }

// ToSRGB (Filter.cuh:145-148) on n floats: what TonemapKernel (:159-175) stores and what TAAFilterKernel ends with (:353), exported so that
// it can be held to the reference build on its own (tests/test_reference_parity.py)
void svgf_oracle_srgb(const float* in, float* out, size_t n) { for (size_t i = 0; i < n; i++) out[i] = to_srgb(in[i]); }

// converters exported so the tests can pin them against numpy's float16
uint16_t svgf_oracle_f2h(float f) { return f2h(f); }
float svgf_oracle_h2f(uint16_t h) { return h2f(h); }

}  // extern "C"
