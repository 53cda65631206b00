// Internal: the context behind the C ABI and the helpers shared by svgf_api.hip (stages, frame driver, lifecycle) and
// svgf_strip.hip (the multi-GPU strip driver).
#pragma once
#include "../../include/svgf.h"
#include "../../include/svgf_ext.h"
#include "../../include/svgf_test.h"
#include "svgf_kernels.h"

#include <memory>
#include <string>
#include <type_traits>
#include <vector>

struct svgf_strip_driver;

namespace svgf_host {

// Owning handles: every device buffer, host-mapped word, stream and event the library creates has exactly one of these as its owner,
// and the owner's destruction (or reset, or a move onto it) is the one place it is released.
struct FreeDevice { void operator()(void* p) const { (void)hipFree(p); } };
struct FreeHost { void operator()(void* p) const { (void)hipHostFree(p); } };
struct DestroyEvent { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
struct DestroyStream { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
template <class T> using DevicePtr = std::unique_ptr<T, FreeDevice>;
template <class T> using HostPtr = std::unique_ptr<T, FreeHost>;
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, DestroyEvent>;
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, DestroyStream>;

// make(&tmp, args...) acquires into a temporary (hipMalloc<T>, hipEventCreateWithFlags, ...); `h` takes it, releasing what it held, only on
// success — a failure leaves `h` as it was
template <class H, class F, class... A> hipError_t acquire(H& h, F make, A... args) {
    typename H::pointer p = nullptr;
    const hipError_t e = make(&p, args...);
    if (e == hipSuccess) h.reset(p);
    return e;
}

struct Rows { int a, b; };              // global rows [a, b): what ONE launch computes — an argument of every stage helper, never context state

// Which kernel serves a frame's young pixels: the drivers' decision for one frame (choose_moments_kernel), handed to that frame's temporal and
// moments launches.  The stage entry points pass the default: their temporal launch appends to the list and adds to the sample.
struct MomentsChoice {
    bool cold = false, crowded = false;     // one of the first three frames after a reset; the sample says too many young pixels for the list
    bool dense() const { return cold || crowded; }   // the streaming kernel visits every pixel: the temporal launch appends to no list
};

// Scratch a temporal launch hands to the moments launch of the same frame (TemporalArgs / MomentsArgs, svgf_kernels.h).  All of it or none
// (alloc_flags).  The three device counters are pairs used in turn: a frame's temporal launch appends to the current one and zeroes the next.
struct YoungScratch {
    DevicePtr<unsigned long long> masks;   // per (row, 64-column segment) the lanes whose pixel (history < 4) needs the spatial estimate
    DevicePtr<uint32_t> list;              // the indices of the pixels of the partly young segments (svgf::young_list_entries)
    DevicePtr<unsigned long long> count;   // {appends, pixels} counters of `list`, svgf::kYoungCounterStride words apart
    DevicePtr<uint32_t> nan_list;          // the pixels whose accumulated colour / moments are NaN or inf (kNanListCap entries)
    DevicePtr<unsigned> nan_count;         // ... and its counters
    DevicePtr<unsigned long long> sample_count;   // 64-bit counters 128 B apart: the sampled number of young pixels of a frame (TemporalArgs::sample_count)
    HostPtr<unsigned long long> estimate_host;   // host-mapped: the latest sample a temporal launch has published (read without synchronising: some frames old)
    int phase = 0;                         // which counter of each pair is the current one
    bool pending = false;                  // a temporal launch wrote the masks / appended to the current counters and no moments launch has consumed them yet
    bool complete() const { return masks && list && count && nan_list && nan_count && sample_count && estimate_host; }
    void reset() { *this = YoungScratch(); }
    unsigned long long* counter(bool next = false) const { return count.get() + (phase ^ (int)next) * svgf::kYoungCounterStride; }
    unsigned* nan_counter(bool next = false) const { return nan_count.get() + (phase ^ (int)next); }
    unsigned long long* sample_counter(bool next = false) const { return sample_count.get() + (phase ^ (int)next) * 16; }
    void turn() { phase ^= 1; pending = false; }   // the moments launch has consumed the lists: the next frame appends to the counters this frame's temporal launch zeroed
};

}  // namespace svgf_host

#ifndef SVGF_PREV_GUIDE_DEFAULT
#define SVGF_PREV_GUIDE_DEFAULT 0      // opt-in (svgf_set_prev_guide): it relies on the host not rewriting the previous G-buffer's planes
#endif

#ifndef SVGF_FUSE01_DEFAULT
#define SVGF_FUSE01_DEFAULT 0         // off: the pair launch is bit-identical and ~10 % slower than two launches
#endif

struct svgf_ctx {
    int W = 0, H = 0;
    svgf_strip strip{};
    int rb = 0, re = 0;                 // svgf_set_rows: the rows the stage entry points and svgf_denoise_frame compute (they pass them down; a strip driver's launches bring their own)
    svgf_params p{};
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // context-owned state (frame driver): RenderBuffer[2], MomentsBuffer[2], FilterBuffer[2] (App.h:138-140)
    // and the ping-ponged history plane (App.h:141 + SURVEY App. B #1)
    svgf_host::DevicePtr<void> colour[2], moments[2], filter[2];
    svgf_host::DevicePtr<uint8_t> hist[2];
    svgf_host::DevicePtr<void> guide;      // {depth, ddepth, normal, instance ID} of the current G-buffer repacked by the temporal launch for the wavelet iterations
    svgf_host::DevicePtr<void> guide_prev; // ... and the plane the previous frame wrote (the two swap at the end of a frame): the next reprojection test reads it
    svgf_gbuffer guide_prev_of{};          // the G-buffer guide_prev was made from (the planes' addresses), valid while guide_prev_valid
    bool guide_prev_valid = false;
    bool prev_guide_enabled = SVGF_PREV_GUIDE_DEFAULT != 0;   // svgf_set_prev_guide
    bool fuse01 = SVGF_FUSE01_DEFAULT != 0;   // svgf_set_iteration_fusion: iterations 0 and 1 in one launch (frame / strip drivers)
    // svgf_set_frames_in_flight(2) / svgf_strips_set_frames_in_flight(2): the frame and strip drivers run iterations 1.. of a frame on `side`
    // while the NEXT frame's temporal, moments and first-iteration launches run on `stream` (the HBM-bound launch beside the arithmetic-bound
    // ones).  Frames then alternate between two pairs of filter planes (the guide planes alternate anyway), and a frame's result is ordered
    // on `stream` by the next frame / svgf_flush / svgf_sync.
    int frames_in_flight = 1;
    svgf_host::Stream side;
    svgf_host::Event ev_first, ev_done;    // iteration 0 of the frame being enqueued is on `stream`; the last iteration of the frame in flight is on `side`
    svgf_host::DevicePtr<void> filter_alt[2];   // the other pair: `filter` always names the pair the last frame enqueued wrote
    bool swap_pairs = false;               // frames_in_flight == 2: the next frame takes the other pair (false for the first one after the switch or a resize)
    bool in_flight = false;                // a frame's tail is on `side` and `stream` has not been made to wait for it yet
    unsigned long long in_flight_capture = 0;   // ... and the stream capture that tail was recorded in (0: none; svgf.h, Stream capture)
    svgf_host::YoungScratch young;         // temporal -> moments scratch (alloc_flags)
    bool adaptive_moments = true;          // svgf_set_adaptive_moments
    bool dense_moments = false;            // the drivers' current choice between the two moments kernels (hysteresis, choose_moments_kernel)
    int vy0 = 0, vy1 = 0;                  // global rows of the previous-frame planes that hold valid state (svgf_set_valid_rows; default: all held)
    svgf_host::DevicePtr<unsigned> halo_violations;   // strips: device counter of reprojections that left the rows this strip holds (temporal_kernel)
    int pingpong = 0;                      // PingPongInx, App.cu:374
    int frames_since_reset = 0;
    int result_index = 0;                  // which filter plane holds the last result (the reference copies it back into FilterBuffer[0], App.cu:510-513)
    int debug_mode = SVGF_DEBUG_FINAL;     // SVGFDebugOutput, App.cu:545-649
    bool have_state = false;
    svgf_strip_driver* strip_drv = nullptr;
    svgf_host::DevicePtr<unsigned long long> path_stats;   // svgf_path_stats_enable: device counters, a pair per step 1 << i (svgf_kernels.h: AtrousArgs::path_stats), or null
    // per-stage timing
    int timing = 0;               // 0 = off, n = stage events on every n-th frame
    int timing_phase = 0;
    // stage i ran between ev[i] and ev[i + 1]; from stage `split` on (the launches on the side stream) between ev[i + 1] and ev[i + 2]
    struct FrameEvents { std::vector<svgf_host::Event> ev; int nstage = 0; int split = 1 << 30; };
    std::vector<FrameEvents> pending;      // each event is in exactly one of the two: a frame's events go back to the pool once it has been read
    std::vector<svgf_host::Event> pool;
    double ms_sum[2 + SVGF_MAX_STEPS] = {0};
    int timed_frames = 0;
};

namespace svgf_host {

// Every entry point runs with the context's device current and restores the caller's on the way out: a host that drives
// several devices from one thread (or whose current device is not the context's) finds its own device unchanged.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) == hipSuccess && prev != device) {
            switched = hipSetDevice(device) == hipSuccess;
            if (!switched) (void)hipGetLastError();        // (a device that does not exist: the caller's entry point fails on its own; nothing is left pending for the host)
        }
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

int fail(svgf_ctx* c, int code, const std::string& msg);
int hip_fail(svgf_ctx* c, hipError_t e, const char* what);
#define SVGF_HIP(c, call)                                                    \
    do {                                                                     \
        hipError_t e_ = (call);                                              \
        if (e_ != hipSuccess) return svgf_host::hip_fail((c), e_, #call);    \
    } while (0)

size_t colour_bytes(const svgf_ctx* c);
size_t moments_bytes(const svgf_ctx* c);
size_t hist_bytes(const svgf_ctx* c);
bool is_strip(const svgf_ctx* c);
int reset_history(svgf_ctx* c);
int read_halo_violations(svgf_ctx* c, unsigned long long* count, int clear);

// Two frames in flight, one mechanism for the frame and the strip driver (svgf_api.hip)
int set_frames_in_flight(svgf_ctx* c, int frames, int side_priority);   // 2: creates the side stream (at that priority) and its events; 1: joins the frame in flight
int join_side(svgf_ctx* c, hipStream_t onto);   // `onto` waits for the frame in flight on the side stream (frames_in_flight == 2); no-op otherwise
bool tail_may_leave(const svgf_ctx* c, int first);   // iterations first.. of this frame may run on the side stream
int fork_side(svgf_ctx* c);             // the launches from here on go to the side stream, behind what c->stream holds and the frame in flight
hipError_t join_back(svgf_ctx* c, hipStream_t caller, unsigned long long capture);   // ... what went there is the frame in flight; c->stream = caller
int begin_frame(svgf_ctx* c);           // allocates what a frame needs and picks its pair of filter planes: c->filter
void finish_frame(svgf_ctx* c, int result_index, const svgf_gbuffer* cur, bool guide_written);   // result, guide and ping-pong move on

// the stages on caller- or driver-owned planes, each on the rows its caller passes (the context is not consulted for them); the device is already current
// temporal launch on rows `rt`, moments launch on `rm` inside them; `choice`: which moments kernel (the stage entry point: the default)
int temporal_moments_impl(svgf_ctx* c, Rows rt, Rows rm, MomentsChoice choice, const void* prev_colour, const void* radiance, void* colour_out,
                          void* filter_out, const svgf_gbuffer* cur, const svgf_gbuffer* prev, const uint8_t* hist_prev, uint8_t* hist_cur,
                          void* moments_cur, const void* moments_prev, int feedback_follows, void* guide_out = nullptr, const void* guide_prev = nullptr);
MomentsChoice choose_moments_kernel(svgf_ctx* c, Rows rt);   // frame / strip drivers, before the temporal launch (rows rt) of a frame (svgf_api.hip)
int atrous_impl(svgf_ctx* c, Rows rows, const void* in, void* out, void* feedback, const svgf_gbuffer* g, int step, int iteration, const void* guide = nullptr);
// one iteration over several row ranges in one launch, the first ranges signalled (the strip driver's edge rows; svgf_kernels.h: AtrousRanges); `hull` spans them
bool atrous_ranges_ok(const svgf_ctx* c, int step);
int atrous_ranges_impl(svgf_ctx* c, Rows hull, const void* in, void* out, void* feedback, const svgf_gbuffer* g, int step, int iteration, const void* guide, const svgf::AtrousRanges& r);
// iterations 0 and 1 in one launch on `rows` (iteration 1's; iteration 0 and the feedback store cover 4 more rows either side)
int atrous_pair_impl(svgf_ctx* c, Rows rows, const void* in, void* out, void* feedback, const svgf_gbuffer* g, const void* guide = nullptr);
bool can_fuse01(const svgf_ctx* c);     // the drivers run iterations 0 and 1 as one launch
const void* prev_guide_for(const svgf_ctx* c, const svgf_gbuffer* cur, const svgf_gbuffer* prev);   // the guide plane that stands in for `prev`, or null
bool use_guide(const svgf_ctx* c);      // the frame / strip drivers repack {depth, ddepth, normal, instance ID} for the iterations (any storage, >= 1 iteration, LDS kernels)

}  // namespace svgf_host
