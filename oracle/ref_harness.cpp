// ref_harness.cpp — runs the reference's own filter kernels on the host, one thread at a time.
//
// TEST INFRASTRUCTURE ONLY, written by this project.  `make _ref` copies the reference's src/Filter.cuh, unmodified, to oracle/_ref/src/ and
// compiles it here against the stand-in headers of oracle/ref_shim/ (our text; each definition cites what it restates).  Nothing of the
// reference's, and nothing compiled from it, is committed: oracle/_ref/ is ignored by git.  What results is the second, independent
// implementation that oracle/svgf_oracle.cpp is held to (tests/test_reference_parity.py).
//
// Only the reference-native fp16 storage exists on this side: the kernels take half4* / half2*.
//
// One launch = the reference's grid (App.cu:471-472: 16x16 blocks, W/16+1 by H/16+1 of them, so threads outside the frame run too).  The
// reference works in place: TemporalFilter reads and writes CurrentImage, reads HistoryLengths at the reprojected pixel and writes it at its
// own, and TAAFilterKernel reads the plane it writes.  Which neighbour's write a thread sees is a race on the device;
// this project resolved it as "every thread reads the state before the launch" (include/svgf.h), and the runner implements exactly that:
// after every thread it takes what the thread stored at its own pixel into a separate result plane and puts the previous contents back.
// Every written buffer must then equal its copy from before the launch again, and that is checked after EVERY thread (whole buffers, the
// threads outside the frame included): a store to any pixel but the thread's own is reported (return value -2) and undone before the next
// thread runs, so no thread ever reads another's store.  When the launch is over the result planes replace the buffers.

#include <cstdint>
#include <cstring>
#include <vector>

#include "_ref/src/Filter.cuh"

// The fp64 islands of SURVEY.md App. A.5, as overload resolution inside the filter source's own namespace picks them (`using namespace glm`
// against CUDA's global overload set, ref_cuda_runtime.h): checked on the return type, here where the filter source's calls are made.
#include <type_traits>
namespace filter {
static_assert(std::is_same<decltype(min(1.0f, 0.5)), double>::value, ":302 min(float, double literal) is CUDA's double fmin");
static_assert(std::is_same<decltype(max(1.0f, 1e-8)), double>::value, ":461 / :424 max(float, double literal) is CUDA's double fmax");
static_assert(std::is_same<decltype(max(0.0, 1e-10f + 1.0f)), double>::value, ":562 max(double literal, float) is CUDA's double fmax");
static_assert(std::is_same<decltype(sqrt(max(0.0, 1.0f))), double>::value, ":562 sqrt of it is the double sqrt");
static_assert(std::is_same<decltype(exp(0.0 - max(1.0f, 0.0) - max(1.0f, 0.0))), double>::value, ":424 the exponential is the double exp");
static_assert(std::is_same<decltype(max(0.f, 1.0f)), float>::value, ":396 max(float, float) is fmaxf");
static_assert(std::is_same<decltype(max(1.0f, 1e-6f)), float>::value, ":505 / :563 max(float, float) is fmaxf");
static_assert(std::is_same<decltype(pow(1.0f, 1 / 2.4f)), float>::value, ":147 / :419 pow(float, float) is powf");
static_assert(std::is_same<decltype(abs(1.0f - 2.0f) > 0.7), bool>::value && std::is_same<decltype(abs(1.0f)), float>::value, ":242 abs(float) is fabsf");
static_assert(std::is_same<decltype(min(24, 2)), int>::value, ":380 min(int, int)");
static_assert(std::is_same<decltype(1.0 / 2), double>::value, ":381 1.0 / HistoryLength is a double division");
}  // namespace filter

uint3 threadIdx, blockIdx;
dim3 blockDim, gridDim;
namespace ref_shim { int uv_fetch_mode = UV_FETCH_AS_HALF; }

namespace {

struct Written {                 // a buffer the launch stores to: base, bytes per pixel
    void* base; size_t elem;
    std::vector<unsigned char> before, result;
};

template <class Thread>
int launch(int W, int H, std::vector<Written>& outs, Thread&& thread) {
    const size_t n = (size_t)W * H;
    for (auto& o : outs) {
        if (!o.base) continue;
        o.before.assign((unsigned char*)o.base, (unsigned char*)o.base + n * o.elem);
        o.result = o.before;
    }
    blockDim.x = 16; blockDim.y = 16; blockDim.z = 1;
    gridDim.x = (unsigned)(W / 16) + 1; gridDim.y = (unsigned)(H / 16) + 1; gridDim.z = 1;   // App.cu:472
    int rc = 0;
    for (unsigned gy = 0; gy < gridDim.y * 16; gy++)
        for (unsigned gx = 0; gx < gridDim.x * 16; gx++) {
            blockIdx.x = gx / 16; threadIdx.x = gx % 16;
            blockIdx.y = gy / 16; threadIdx.y = gy % 16;
            blockIdx.z = threadIdx.z = 0;
            thread();
            if ((int)gx < W && (int)gy < H) {
                const size_t own = (size_t)gy * W + gx;
                for (auto& o : outs) {
                    if (!o.base) continue;
                    unsigned char* p = (unsigned char*)o.base + own * o.elem;
                    memcpy(o.result.data() + own * o.elem, p, o.elem);
                    memcpy(p, o.before.data() + own * o.elem, o.elem);
                }
            }
            for (auto& o : outs)
                if (o.base && memcmp(o.base, o.before.data(), n * o.elem) != 0) {     // this thread stored outside its own pixel
                    rc = -2;
                    memcpy(o.base, o.before.data(), n * o.elem);
                }
        }
    for (auto& o : outs)
        if (o.base) memcpy(o.base, o.result.data(), n * o.elem);
    return rc;
}

cudaTextureObject_t handle(const ref_shim::plane& p) { return (cudaTextureObject_t)(uintptr_t)&p; }

}  // namespace

extern "C" {

// what the float4 fetch of the 8-byte UV texel returns (ref_cuda_runtime.h): 0 = the raw 16-bit integers as float bits, 1 = decoded halves
int svgf_ref_set_uv_fetch(int mode) {
    if (mode != ref_shim::UV_FETCH_RAW_BITS && mode != ref_shim::UV_FETCH_AS_HALF) return -1;
    ref_shim::uv_fetch_mode = mode;
    return 0;
}

// TemporalFilter.  cur_image, hist: in place (read and written).  mom_cur: written.
int svgf_ref_temporal(int W, int H, void* prev_image, void* cur_image,
                      const float* motion_c, const uint16_t* normal_c, const uint16_t* uv_c,
                      const float* motion_p, const uint16_t* normal_p, const uint16_t* uv_p,
                      uint8_t* hist, void* mom_cur, void* mom_prev,
                      float depth_thr, float normal_thr, int history_base) {
    using namespace ref_shim;
    const plane mc{motion_c, W, H, TEXEL_F32X4}, nc{normal_c, W, H, TEXEL_U16X4}, uc{uv_c, W, H, TEXEL_U16X4};
    const plane mp{motion_p, W, H, TEXEL_F32X4}, np{normal_p, W, H, TEXEL_U16X4}, up{uv_p, W, H, TEXEL_U16X4};
    gpupt::cudaFramebuffer fc{0, handle(nc), handle(uc), handle(mc)}, fp{0, handle(np), handle(up), handle(mp)};
    std::vector<Written> outs{{cur_image, 8, {}, {}}, {hist, 1, {}, {}}, {mom_cur, 4, {}, {}}};
    return launch(W, H, outs, [&] {
        filter::TemporalFilter((filter::half4*)prev_image, (filter::half4*)cur_image, fc, fp, hist, (filter::half2*)mom_cur,
                               (filter::half2*)mom_prev, W, H, depth_thr, normal_thr, history_base);
    });
}

// FilterMoments.  output: written.
int svgf_ref_moments(int W, int H, void* cur_image, void* output, void* moments, const float* motion, const uint16_t* normal,
                     uint8_t* hist, float phi_colour, float phi_normal) {
    using namespace ref_shim;
    const plane m{motion, W, H, TEXEL_F32X4}, nr{normal, W, H, TEXEL_U16X4};
    std::vector<Written> outs{{output, 8, {}, {}}};
    return launch(W, H, outs, [&] {
        filter::FilterMoments((filter::half4*)cur_image, (filter::half4*)output, (filter::half2*)moments, handle(m), handle(nr), hist, W, H,
                              phi_colour, phi_normal);
    });
}

// FilterKernel (one à-trous iteration).  output: written; render_output: written when iteration == 0 (may be null otherwise).
int svgf_ref_atrous(int W, int H, void* input, const float* motion, const uint16_t* normal, uint8_t* hist, void* output,
                    void* render_output, int step, float phi_colour, float phi_normal, int iteration) {
    using namespace ref_shim;
    if (iteration == 0 && !render_output) return -1;
    const plane m{motion, W, H, TEXEL_F32X4}, nr{normal, W, H, TEXEL_U16X4};
    std::vector<Written> outs{{output, 8, {}, {}}, {iteration == 0 ? render_output : nullptr, 8, {}, {}}};
    return launch(W, H, outs, [&] {
        filter::FilterKernel((filter::half4*)input, handle(m), handle(nr), hist, (filter::half4*)output, (filter::half4*)render_output, W, H,
                             step, phi_colour, phi_normal, iteration);
    });
}

// TAAFilterKernel.  output: in place (its previous contents are the history).
int svgf_ref_taa(int W, int H, void* input, void* output) {
    std::vector<Written> outs{{output, 8, {}, {}}};
    return launch(W, H, outs, [&] { filter::TAAFilterKernel((filter::half4*)input, (filter::half4*)output, W, H); });
}

// The runner's own check, on a kernel of this file's: every thread stores 1 at its own pixel of `plane` (W x H bytes), and the thread of pixel
// (x, y) also stores 0xff at (x + dx, y + dy).  -> what launch() returns: 0 for dx = dy = 0, -2 for any stray store inside the frame, whether
// the pixel it hits comes earlier or later in the order the threads run.
int svgf_ref_guard_selftest(int W, int H, int x, int y, int dx, int dy, uint8_t* plane) {
    std::vector<Written> outs{{plane, 1, {}, {}}};
    return launch(W, H, outs, [&] {
        const glm::uvec2 id = ref_shim::global_id();
        const int tx = (int)id.x, ty = (int)id.y;
        if (tx >= W || ty >= H) return;
        plane[(size_t)ty * W + tx] = 1;
        if (tx == x && ty == y && (dx || dy)) plane[(size_t)(y + dy) * W + (x + dx)] = 0xff;
    });
}

// TonemapKernel (fp32 vec4 planes).  output: written.
int svgf_ref_tonemap(int W, int H, float* input, float* output) {
    std::vector<Written> outs{{output, 16, {}, {}}};
    return launch(W, H, outs, [&] { filter::TonemapKernel((glm::vec4*)input, (glm::vec4*)output, W, H, 0); });
}

}  // extern "C"
