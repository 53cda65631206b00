// ref_cuda_runtime.h — stand-in for what the CUDA toolchain gives device code implicitly, as far as the reference's filter source uses it.
//
// TEST INFRASTRUCTURE ONLY, written by this project; included by the App.h stand-in so that it is in force before the filter source.
// Each definition states the documented behaviour of what it replaces and names the document.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

// CUDA C++ Programming Guide, "Function Execution Space Specifiers": no meaning on the host
#define __device__
#define __global__
#define __host__

// CUDA C++ Programming Guide, "Built-in Vector Types" and "Built-in Variables"
struct float4 { float x, y, z, w; };
struct ushort4 { unsigned short x, y, z, w; };
struct uint3 { unsigned x, y, z; };
struct dim3 { unsigned x = 1, y = 1, z = 1; };
typedef unsigned long long cudaTextureObject_t;      // driver_types.h
extern uint3 threadIdx, blockIdx;                    // set per thread by the runner (oracle/ref_harness.cpp)
extern dim3 blockDim, gridDim;

// ---- CUDA's overload set of min / max in the global namespace (CUDA Math API; crt/math_functions.hpp) -----------------------------
// The float and double forms are fminf/fmaxf and fmin/fmax: a NaN operand gives the OTHER operand.  A call that mixes float and double
// has no matching GLM template (its two parameters are one genType), so it resolves here and is evaluated in double.  A call with two
// floats or two ints matches these non-templates exactly and prefers them to GLM's templates, as it does under nvcc.
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }
inline unsigned min(unsigned a, unsigned b) { return a < b ? a : b; }
inline unsigned max(unsigned a, unsigned b) { return a > b ? a : b; }
inline unsigned min(int a, unsigned b) { return min((unsigned)a, b); }
inline unsigned min(unsigned a, int b) { return min(a, (unsigned)b); }
inline unsigned max(int a, unsigned b) { return max((unsigned)a, b); }
inline unsigned max(unsigned a, int b) { return max(a, (unsigned)b); }
inline float min(float a, float b) { return fminf(a, b); }
inline float max(float a, float b) { return fmaxf(a, b); }
inline double min(double a, double b) { return fmin(a, b); }
inline double max(double a, double b) { return fmax(a, b); }
inline double min(float a, double b) { return fmin((double)a, b); }
inline double min(double a, float b) { return fmin(a, (double)b); }
inline double max(float a, double b) { return fmax((double)a, b); }
inline double max(double a, float b) { return fmax(a, (double)b); }

// device_functions.h: saturate(x) is __saturatef(x) — PTX cvt.sat.f32.f32: clamps to [+0.0, 1.0], NaN becomes +0.0
inline float saturate(float x) {
    if (x != x) return 0.0f;
    return fminf(fmaxf(x, 0.0f), 1.0f);
}

// ---- texture objects ----------------------------------------------------------------------------------------------------------------
// A texture object here is the address of a plane descriptor.  The reference creates every texture object from a zeroed cudaTextureDesc
// with readMode = cudaReadModeElementType (CudaUtil.h:58-63 and :90-95): filterMode 0 = point, normalizedCoords 0, addressMode 0 =
// cudaAddressModeWrap — which the CUDA Runtime API documents as honoured with normalized coordinates only; with unnormalized coordinates
// the access clamps to the edge.  tex2D(tex, x, y) with integer arguments converts them to float and point-samples texel floor(x), floor(y).
namespace ref_shim {
enum texel_format { TEXEL_F32X4 = 0, TEXEL_U16X4 = 1 };
struct plane { const void* data; int W, H, format; };
inline const plane& plane_of(cudaTextureObject_t t) { return *reinterpret_cast<const plane*>((uintptr_t)t); }
inline size_t texel_index(const plane& p, int x, int y) {
    x = x < 0 ? 0 : (x > p.W - 1 ? p.W - 1 : x);
    y = y < 0 ? 0 : (y > p.H - 1 ? p.H - 1 : y);
    return (size_t)y * p.W + x;
}
// What tex2D<float4> returns from an 8-byte four-channel 16-bit texel (Filter.cuh:245-246 fetch the RGBA16UI UV plane this way):
//   UV_FETCH_RAW_BITS  the de-facto reading: each channel's 16-bit integer arrives in a 32-bit register and is read as float bits — a denormal
//   UV_FETCH_AS_HALF   the intended reading: each channel decoded from IEEE half to float
enum uv_fetch { UV_FETCH_RAW_BITS = 0, UV_FETCH_AS_HALF = 1 };
extern int uv_fetch_mode;
float half_bits_to_float(unsigned short h);          // cuda_fp16.h stand-in
}  // namespace ref_shim

template <class T> T tex2D(cudaTextureObject_t tex, float x, float y);
template <> inline float4 tex2D<float4>(cudaTextureObject_t tex, float x, float y) {
    const ref_shim::plane& p = ref_shim::plane_of(tex);
    const size_t i = ref_shim::texel_index(p, (int)floorf(x), (int)floorf(y));
    float4 r;
    if (p.format == ref_shim::TEXEL_F32X4) {
        memcpy(&r, (const float*)p.data + 4 * i, sizeof r);
        return r;
    }
    const unsigned short* q = (const unsigned short*)p.data + 4 * i;
    float v[4];
    for (int k = 0; k < 4; k++) {
        if (ref_shim::uv_fetch_mode == ref_shim::UV_FETCH_RAW_BITS) {
            const uint32_t bits = q[k];
            memcpy(&v[k], &bits, 4);
        } else {
            // The reference converts the fetched channel with a built-in `int id = value.w`, which no header can intercept: the device does
            // cvt.rzi.s32.f32 (NaN -> 0, +-inf saturate), the host's cvttss2si gives INT_MIN for all three.  The ids are only ever compared for
            // equality (Filter.cuh:247), so the channel is handed over as a float whose host truncation compares as the device's result does:
            // NaN -> 0 ; +inf -> the largest float below 2^31 (distinct from every finite half, equal to itself) ; -inf -> -2^31.
            float f = ref_shim::half_bits_to_float(q[k]);
            if (f != f) f = 0.0f;
            else if (f > 65504.0f) f = 2147483520.0f;
            else if (f < -65504.0f) f = -2147483648.0f;
            v[k] = f;
        }
    }
    r.x = v[0]; r.y = v[1]; r.z = v[2]; r.w = v[3];
    return r;
}
template <> inline ushort4 tex2D<ushort4>(cudaTextureObject_t tex, float x, float y) {
    const ref_shim::plane& p = ref_shim::plane_of(tex);
    const size_t i = ref_shim::texel_index(p, (int)floorf(x), (int)floorf(y));
    ushort4 r;
    memcpy(&r, (const unsigned short*)p.data + 4 * i, sizeof r);
    return r;
}
