// Common.cuh — stand-in for the four things the reference's filter source takes from its Common.cuh.
//
// TEST INFRASTRUCTURE ONLY, written by this project.  The path tracer that the rest of that file holds is not restated.
// Only the names and what they mean are taken over (the filter source spells them); every body below is this project's own wording.
//   FN_DECL      Common.cuh:8    the device-function marker
//   GLOBAL_ID()  Common.cuh:13   uvec2 of the thread's global x and y index
//   INOUT(Type)  Common.cuh:16   a parameter passed by reference, written through to the caller
//   commonCu::IsFinite  Common.cuh:85-93   "is not a NaN", per component (infinities count as finite)
#pragma once

#include <glm/glm.hpp>
#include <cuda_fp16.h>
#include "App.h"
#include <initializer_list>

#define FN_DECL          /* marks a device function; an execution-space specifier means nothing on the host (ref_cuda_runtime.h) */

namespace ref_shim {
// CUDA C++ Programming Guide, "Thread Hierarchy": a thread's index in the grid is its block's index times the block's extent plus its index in the block
inline unsigned grid_index(unsigned block, unsigned extent, unsigned lane) { return lane + extent * block; }
inline glm::uvec2 global_id() {
    const unsigned column = grid_index(blockIdx.x, blockDim.x, threadIdx.x);
    const unsigned row = grid_index(blockIdx.y, blockDim.y, threadIdx.y);
    return glm::uvec2(column, row);
}
}  // namespace ref_shim
#define GLOBAL_ID() ref_shim::global_id()

// The reference hands temporaries to INOUT parameters (`Vec4ToHalf4(clamp(...))`, `Half4ToVec4({...})`), which the host compiler it is built
// with binds to `Type &` and ISO C++ does not.  ref_shim::inout<Type> is that reference: bound to the caller's object when given one (writes
// go through, as with `Type &`), and to a copy of its own when given a temporary.  Members are reached through references of the same names.
namespace ref_shim {
template <class T> struct inout {                        // scalars
    T own; T& r;
    inout(T& l) : own(), r(l) {}
    inout(T&& t) : own(t), r(own) {}
    inout(const inout& o) = delete;
    operator T&() const { return r; }
    template <class V> inout& operator=(const V& v) { r = v; return *this; }
};
#define REF_SHIM_INOUT_HEAD(SELF, TYPE)                                              \
    TYPE own; TYPE& r;                                                               \
    SELF(const SELF& o) = delete;                                                    \
    operator TYPE&() const { return r; }                                             \
    SELF& operator=(const TYPE& v) { r = v; return *this; }
template <> struct inout<glm::vec2> {
    REF_SHIM_INOUT_HEAD(inout, glm::vec2)
    float &x, &y;
    inout(glm::vec2& l) : own(), r(l), x(r.x), y(r.y) {}
    inout(glm::vec2&& t) : own(t), r(own), x(r.x), y(r.y) {}
};
template <> struct inout<glm::vec3> {
    REF_SHIM_INOUT_HEAD(inout, glm::vec3)
    float &x, &y, &z;
    inout(glm::vec3& l) : own(), r(l), x(r.x), y(r.y), z(r.z) {}
    inout(glm::vec3&& t) : own(t), r(own), x(r.x), y(r.y), z(r.z) {}
};
template <> struct inout<glm::vec4> {
    REF_SHIM_INOUT_HEAD(inout, glm::vec4)
    float &x, &y, &z, &w;
    inout(glm::vec4& l) : own(), r(l), x(r.x), y(r.y), z(r.z), w(r.w) {}
    inout(glm::vec4&& t) : own(t), r(own), x(r.x), y(r.y), z(r.z), w(r.w) {}
};
// the filter source's own half4 / half2 (declared there, after this header): any struct of x,y,z,w or x,y halves
template <class T> struct inout_h4 {
    REF_SHIM_INOUT_HEAD(inout_h4, T)
    half &x, &y, &z, &w;
    inout_h4(T& l) : own(), r(l), x(r.x), y(r.y), z(r.z), w(r.w) {}
    inout_h4(T&& t) : own(t), r(own), x(r.x), y(r.y), z(r.z), w(r.w) {}
    inout_h4(half a, half b, half c, half d) : own{a, b, c, d}, r(own), x(r.x), y(r.y), z(r.z), w(r.w) {}
};
template <class T> struct inout_h2 {
    REF_SHIM_INOUT_HEAD(inout_h2, T)
    half &x, &y;
    inout_h2(T& l) : own(), r(l), x(r.x), y(r.y) {}
    inout_h2(T&& t) : own(t), r(own), x(r.x), y(r.y) {}
};
template <class T> struct inout_of { typedef inout<T> type; };
}  // namespace ref_shim
namespace filter { struct half4; struct half2; }
namespace ref_shim {
template <> struct inout_of<filter::half4> { typedef inout_h4<filter::half4> type; };
template <> struct inout_of<filter::half2> { typedef inout_h2<filter::half2> type; };
}
#define INOUT(Type) typename ref_shim::inout_of<Type>::type

namespace commonCu {
// a NaN is the one value that differs from itself (IEEE 754); an infinity passes
inline bool IsFinite(float value) { return value == value; }
inline bool IsFinite(glm::vec3 v) {
    for (float c : {v.x, v.y, v.z})
        if (c != c) return false;
    return true;
}
}  // namespace commonCu
