// glm/glm.hpp — stand-in for the part of GLM (g-truc/glm, 0.9.9 series) that the reference's filter source uses.
//
// TEST INFRASTRUCTURE ONLY, written by this project.  The reference's glm submodule is empty, so its filter source is
// compiled on the host against this header instead (oracle/Makefile, target _ref).  Every definition restates the GLM
// definition it replaces and names the GLM file it restates; only what the filter source uses is provided.
//
// Two things here are not GLM's but the device compiler's, and are restated because they are observable:
//   * static_cast<int>(float) inside GLM's converting constructors is, in device code, PTX cvt.rzi.s32.f32
//     (PTX ISA, "cvt": round toward zero, out-of-range values saturate, NaN converts to 0).  A host cast of such a
//     value is undefined behaviour; ref_shim::cvt_rzi_s32 states the device rule.
//   * signed integer addition and multiplication on the device are two's-complement (PTX add.s32 / mul.lo.s32 wrap);
//     ivec arithmetic goes through unsigned here so that the host build has no signed-overflow UB either.
#pragma once

#include <math.h>      // the C++ <math.h>: puts the float and double overloads of pow/exp/sqrt/abs/floor/sin in the global namespace, as the CUDA math API does
#include <stdint.h>
#include <stdlib.h>
#include <type_traits>

namespace ref_shim {

// PTX ISA, cvt.rzi.s32.f32
inline int cvt_rzi_s32(float f) {
    if (f != f) return 0;
    if (f >= 2147483648.0f) return 2147483647;
    if (f <= -2147483648.0f) return -2147483647 - 1;
    return (int)f;
}
// PTX ISA, cvt.rzi.u32.f32 (same rules, unsigned range)
inline unsigned cvt_rzi_u32(float f) {
    if (f != f) return 0u;
    if (f >= 4294967296.0f) return 4294967295u;
    if (f <= 0.0f) return 0u;
    return (unsigned)f;
}

// component conversion as GLM's converting constructors spell it, static_cast<T>(u), with the device's float -> integer rule
template <class T, class U> inline T conv(U u) {
    if constexpr (std::is_same<T, int>::value && std::is_floating_point<U>::value) return cvt_rzi_s32((float)u);
    else if constexpr (std::is_same<T, unsigned>::value && std::is_floating_point<U>::value) return cvt_rzi_u32((float)u);
    else return static_cast<T>(u);
}

// a + b, a - b, a * b, a / b on components: two's-complement for integers (PTX add/sub/mul.lo wrap), IEEE for floats
template <class T> inline T add(T a, T b) { if constexpr (std::is_integral<T>::value) return (T)((typename std::make_unsigned<T>::type)a + (typename std::make_unsigned<T>::type)b); else return a + b; }
template <class T> inline T sub(T a, T b) { if constexpr (std::is_integral<T>::value) return (T)((typename std::make_unsigned<T>::type)a - (typename std::make_unsigned<T>::type)b); else return a - b; }
template <class T> inline T mul(T a, T b) { if constexpr (std::is_integral<T>::value) return (T)((typename std::make_unsigned<T>::type)a * (typename std::make_unsigned<T>::type)b); else return a * b; }
template <class T> inline T quo(T a, T b) { return a / b; }

}  // namespace ref_shim

namespace glm {

typedef int length_t;
template <length_t L, typename T> struct vec;

// glm/detail/type_vec2.hpp, type_vec3.hpp, type_vec4.hpp: components x/r, y/g, z/b, w/a share storage; the converting
// constructors are implicit (GLM_EXPLICIT is empty unless GLM_FORCE_EXPLICIT_CTOR is defined, and the reference does not define it).
template <typename T> struct vec<2, T> {
    union { T x, r; };
    union { T y, g; };
    vec() : x(), y() {}
    vec(const vec&) = default;
    vec& operator=(const vec&) = default;
    explicit vec(T s) : x(s), y(s) {}
    template <class A, class B, class = typename std::enable_if<std::is_arithmetic<A>::value && std::is_arithmetic<B>::value>::type>
    vec(A a, B b) : x(ref_shim::conv<T>(a)), y(ref_shim::conv<T>(b)) {}
    template <class U> vec(const vec<2, U>& v) : x(ref_shim::conv<T>(v.x)), y(ref_shim::conv<T>(v.y)) {}
    template <class U> vec(const vec<3, U>& v);
    template <class U> vec(const vec<4, U>& v);
};
template <typename T> struct vec<3, T> {
    union { T x, r; };
    union { T y, g; };
    union { T z, b; };
    vec() : x(), y(), z() {}
    vec(const vec&) = default;
    vec& operator=(const vec&) = default;
    explicit vec(T s) : x(s), y(s), z(s) {}
    template <class A, class B, class C, class = typename std::enable_if<std::is_arithmetic<A>::value && std::is_arithmetic<B>::value && std::is_arithmetic<C>::value>::type>
    vec(A a, B b, C c) : x(ref_shim::conv<T>(a)), y(ref_shim::conv<T>(b)), z(ref_shim::conv<T>(c)) {}
    template <class U> vec(const vec<3, U>& v) : x(ref_shim::conv<T>(v.x)), y(ref_shim::conv<T>(v.y)), z(ref_shim::conv<T>(v.z)) {}
    template <class U> vec(const vec<4, U>& v);
};
template <typename T> struct vec<4, T> {
    union { T x, r; };
    union { T y, g; };
    union { T z, b; };
    union { T w, a; };
    vec() : x(), y(), z(), w() {}
    vec(const vec&) = default;
    vec& operator=(const vec&) = default;
    explicit vec(T s) : x(s), y(s), z(s), w(s) {}
    template <class A, class B, class C, class D, class = typename std::enable_if<std::is_arithmetic<A>::value && std::is_arithmetic<B>::value && std::is_arithmetic<C>::value && std::is_arithmetic<D>::value>::type>
    vec(A a_, B b_, C c_, D d_) : x(ref_shim::conv<T>(a_)), y(ref_shim::conv<T>(b_)), z(ref_shim::conv<T>(c_)), w(ref_shim::conv<T>(d_)) {}
    template <class U, class D, class = typename std::enable_if<std::is_arithmetic<D>::value>::type>
    vec(const vec<3, U>& v, D d_) : x(ref_shim::conv<T>(v.x)), y(ref_shim::conv<T>(v.y)), z(ref_shim::conv<T>(v.z)), w(ref_shim::conv<T>(d_)) {}
    template <class U> vec(const vec<4, U>& v) : x(ref_shim::conv<T>(v.x)), y(ref_shim::conv<T>(v.y)), z(ref_shim::conv<T>(v.z)), w(ref_shim::conv<T>(v.w)) {}
};
// the truncating conversions (type_vec2.inl, type_vec3.inl: "vec(vec<4, U, P> const& v)" keeps the leading components)
template <typename T> template <class U> vec<2, T>::vec(const vec<3, U>& v) : x(ref_shim::conv<T>(v.x)), y(ref_shim::conv<T>(v.y)) {}
template <typename T> template <class U> vec<2, T>::vec(const vec<4, U>& v) : x(ref_shim::conv<T>(v.x)), y(ref_shim::conv<T>(v.y)) {}
template <typename T> template <class U> vec<3, T>::vec(const vec<4, U>& v) : x(ref_shim::conv<T>(v.x)), y(ref_shim::conv<T>(v.y)), z(ref_shim::conv<T>(v.z)) {}

typedef vec<2, float> vec2;
typedef vec<3, float> vec3;
typedef vec<4, float> vec4;
typedef vec<2, int> ivec2;
typedef vec<2, unsigned> uvec2;

// Arithmetic operators (type_vecN.inl): component-wise; a scalar operand is applied to every component.
#define REF_SHIM_VEC_OP(OP, FN)                                                                                                                 \
    template <typename T> inline vec<2, T> operator OP(const vec<2, T>& a, const vec<2, T>& b) { return vec<2, T>(ref_shim::FN(a.x, b.x), ref_shim::FN(a.y, b.y)); }                                       \
    template <typename T> inline vec<3, T> operator OP(const vec<3, T>& a, const vec<3, T>& b) { return vec<3, T>(ref_shim::FN(a.x, b.x), ref_shim::FN(a.y, b.y), ref_shim::FN(a.z, b.z)); }              \
    template <typename T> inline vec<4, T> operator OP(const vec<4, T>& a, const vec<4, T>& b) { return vec<4, T>(ref_shim::FN(a.x, b.x), ref_shim::FN(a.y, b.y), ref_shim::FN(a.z, b.z), ref_shim::FN(a.w, b.w)); } \
    template <typename T> inline vec<2, T> operator OP(const vec<2, T>& a, T s) { return vec<2, T>(ref_shim::FN(a.x, s), ref_shim::FN(a.y, s)); }                                                          \
    template <typename T> inline vec<3, T> operator OP(const vec<3, T>& a, T s) { return vec<3, T>(ref_shim::FN(a.x, s), ref_shim::FN(a.y, s), ref_shim::FN(a.z, s)); }                                    \
    template <typename T> inline vec<4, T> operator OP(const vec<4, T>& a, T s) { return vec<4, T>(ref_shim::FN(a.x, s), ref_shim::FN(a.y, s), ref_shim::FN(a.z, s), ref_shim::FN(a.w, s)); }              \
    template <typename T> inline vec<2, T> operator OP(T s, const vec<2, T>& a) { return vec<2, T>(ref_shim::FN(s, a.x), ref_shim::FN(s, a.y)); }                                                          \
    template <typename T> inline vec<3, T> operator OP(T s, const vec<3, T>& a) { return vec<3, T>(ref_shim::FN(s, a.x), ref_shim::FN(s, a.y), ref_shim::FN(s, a.z)); }                                    \
    template <typename T> inline vec<4, T> operator OP(T s, const vec<4, T>& a) { return vec<4, T>(ref_shim::FN(s, a.x), ref_shim::FN(s, a.y), ref_shim::FN(s, a.z), ref_shim::FN(s, a.w)); }              \
    template <length_t L, typename T, class B> inline vec<L, T>& operator OP##=(vec<L, T>& a, const B& b) { a = a OP b; return a; }
REF_SHIM_VEC_OP(+, add)
REF_SHIM_VEC_OP(-, sub)
REF_SHIM_VEC_OP(*, mul)
REF_SHIM_VEC_OP(/, quo)
#undef REF_SHIM_VEC_OP

}  // namespace glm
namespace ref_shim {
// The reference passes the sum `uv + vec2(...)` to a `vec2&` parameter (its textureSample).  The host compiler it is built with binds a
// temporary there; ISO C++ does not.  The float vec2 sum is therefore returned as an object that converts to an lvalue of vec2: the value
// and every use of it are those of GLM's operator+, and the reference's call compiles as written.
template <class V> struct bindable { V v; operator V&() { return v; } };
}  // namespace ref_shim
namespace glm {
inline ref_shim::bindable<vec<2, float>> operator+(const vec<2, float>& a, const vec<2, float>& b) { return {vec<2, float>(a.x + b.x, a.y + b.y)}; }

// glm/detail/func_common.inl:  min(x, y) = (y < x) ? y : x ;  max(x, y) = (x < y) ? y : x ;  clamp(x, lo, hi) = min(max(x, lo), hi)
template <typename genType> inline genType min(genType x, genType y) { return (y < x) ? y : x; }
template <typename genType> inline genType max(genType x, genType y) { return (x < y) ? y : x; }
template <typename genType> inline genType clamp(genType x, genType lo, genType hi) { return min(max(x, lo), hi); }
template <typename T> inline vec<3, T> min(const vec<3, T>& a, const vec<3, T>& b) { return vec<3, T>(min(a.x, b.x), min(a.y, b.y), min(a.z, b.z)); }
template <typename T> inline vec<3, T> max(const vec<3, T>& a, const vec<3, T>& b) { return vec<3, T>(max(a.x, b.x), max(a.y, b.y), max(a.z, b.z)); }
template <typename T> inline vec<4, T> min(const vec<4, T>& a, const vec<4, T>& b) { return vec<4, T>(min(a.x, b.x), min(a.y, b.y), min(a.z, b.z), min(a.w, b.w)); }
template <typename T> inline vec<4, T> max(const vec<4, T>& a, const vec<4, T>& b) { return vec<4, T>(max(a.x, b.x), max(a.y, b.y), max(a.z, b.z), max(a.w, b.w)); }
template <typename T> inline vec<3, T> clamp(const vec<3, T>& x, const vec<3, T>& lo, const vec<3, T>& hi) { return min(max(x, lo), hi); }
template <typename T> inline vec<4, T> clamp(const vec<4, T>& x, const vec<4, T>& lo, const vec<4, T>& hi) { return min(max(x, lo), hi); }

// glm/detail/func_common.inl, compute_mix_scalar / compute_mix_vector:
//   mix(x, y, a) = vec<L, T>( vec<L, U>(x) * (static_cast<U>(1) - a) + vec<L, U>(y) * a )
// The arithmetic is in the type U of the weight: a double literal as `a` makes the whole blend double, rounded to T once.
template <typename T, typename U, class = typename std::enable_if<std::is_arithmetic<T>::value>::type>
inline T mix(T x, T y, U a) { return static_cast<T>(static_cast<U>(x) * (static_cast<U>(1) - a) + static_cast<U>(y) * a); }
template <length_t L, typename T, typename U, class = typename std::enable_if<std::is_arithmetic<U>::value>::type>
inline vec<L, T> mix(const vec<L, T>& x, const vec<L, T>& y, U a) { return vec<L, T>(vec<L, U>(x) * (static_cast<U>(1) - a) + vec<L, U>(y) * a); }

// glm/detail/func_common.inl: abs, floor, fract(x) = x - floor(x) (scalar forms; the std functions on the component type)
template <typename genType> inline genType abs(genType x) { return x < genType(0) ? -x : x; }
template <typename genType> inline genType fract(genType x) { return x - ::floor(x); }

// glm/detail/func_geometric.inl: dot(vec2) = tmp.x + tmp.y ; dot(vec3) = tmp.x + tmp.y + tmp.z with tmp = x * y ; length(v) = sqrt(dot(v, v))
template <typename T> inline T dot(const vec<2, T>& a, const vec<2, T>& b) { const vec<2, T> tmp(a * b); return tmp.x + tmp.y; }
template <typename T> inline T dot(const vec<3, T>& a, const vec<3, T>& b) { const vec<3, T> tmp(a * b); return tmp.x + tmp.y + tmp.z; }
template <length_t L, typename T> inline T length(const vec<L, T>& v) { return ::sqrt(dot(v, v)); }

// glm/detail/func_exponential.inl: pow and sqrt component-wise through the std function of the component type (powf, sqrtf for float)
template <typename T> inline vec<3, T> pow(const vec<3, T>& b, const vec<3, T>& e) { return vec<3, T>(::pow(b.x, e.x), ::pow(b.y, e.y), ::pow(b.z, e.z)); }
template <typename T> inline vec<3, T> sqrt(const vec<3, T>& v) { return vec<3, T>(::sqrt(v.x), ::sqrt(v.y), ::sqrt(v.z)); }

}  // namespace glm
