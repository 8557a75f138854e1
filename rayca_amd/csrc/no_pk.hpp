// no_pk.hpp -- RAYCA_NO_PK_BEGIN / RAYCA_NO_PK_END: the region of a device translation unit (kernels.hip, refill.hip) that is
// compiled without packed f32 arithmetic.  Included before <hip/hip_runtime.h>, which goes inside the region.
#pragma once
// RAYCA_NO_PK_F32: no packed f32 arithmetic (v_pk_add / v_pk_mul / v_pk_fma_f32) in the traversal, leaf, shading and BRDF code.
// The vectoriser pairs the (x, y) lanes of the F4 / Color arithmetic wherever it can; on this chip a packed f32 instruction issues
// in the 4.1-cycle class where v_fma / v_add / v_mul_f32 take 2.3-2.5 (profiles/peaks_r03.json), and the pairs cost register-pair
// moves and re-cut loads on top.  The functions concerned are compiled for a target without the packed operations (a function
// attribute; device pass only).  A function only inlines into one whose target features contain its own, so the runtime header's
// inline functions are declared under the same attribute, or they would become calls.  The same holds for anything new in the
// region: a device function that is not __forceinline__ and is declared outside it, a device-library function (threadIdx.x:
// trace_core.inc rc_tid), an implicit constructor -- each stays a call without a word from the compiler.
// tests/device_calls.py lists the functions left in a unit's code object; there must be none.
#ifndef RAYCA_NO_PK_F32
#define RAYCA_NO_PK_F32 1
#endif
#if RAYCA_NO_PK_F32 && defined(__HIP_DEVICE_COMPILE__)
#define RAYCA_NO_PK_BEGIN _Pragma("clang attribute push(__attribute__((target(\"no-packed-fp32-ops\"))), apply_to = function)")
#define RAYCA_NO_PK_END _Pragma("clang attribute pop")
#else
#define RAYCA_NO_PK_BEGIN
#define RAYCA_NO_PK_END
#endif
