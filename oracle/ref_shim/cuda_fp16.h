// cuda_fp16.h — stand-in for the half type and the four conversions the reference's filter source uses.
//
// TEST INFRASTRUCTURE ONLY, written by this project.  The conversions are the CPU's own F16C instructions (build with -mf16c), NOT the
// software converter of oracle/svgf_oracle.cpp: the reference build must not share the oracle's reading of IEEE half.
//   __float2half   CUDA Math API: round-to-nearest-even (PTX cvt.rn.f16.f32)           -> vcvtps2ph, rounding control 0 (nearest even)
//   __half2float   exact                                                               -> vcvtph2ps
// One documented difference remains: cvt.rn.f16.f32 turns every NaN into the canonical 0x7fff, vcvtps2ph keeps sign and payload (quieted).
// Comparisons of reference results therefore treat all NaN encodings as one value.
#pragma once

#include <immintrin.h>
#include <stdint.h>

struct half { unsigned short bits; };

inline half __float2half(float f) { half h; h.bits = _cvtss_sh(f, _MM_FROUND_TO_NEAREST_INT); return h; }
inline float __half2float(half h) { return _cvtsh_ss(h.bits); }
inline half __ushort_as_half(unsigned short u) { half h; h.bits = u; return h; }   // reinterpretation, no conversion
inline unsigned short __half_as_ushort(half h) { return h.bits; }

namespace ref_shim {
inline float half_bits_to_float(unsigned short h) { return _cvtsh_ss(h); }
}
