// oracle/ref_shim/curand_kernel.h -- TEST INFRASTRUCTURE ONLY.
//
// Stands in for cuRAND's header when the reference's per-child functions
// (statePropagator.cu, collisionCheck.cu, the tail of KGMT.cu) are compiled for
// the host by `make -C oracle ref`.  It supplies the only outside names those
// functions use:
//   curandState / curand_uniform   the oracle's XORWOW restatement (xorwow_ref.h;
//                                  its seeding constants stay unpinned, the
//                                  recurrence is held to rocRAND's vectors)
//   M_PI                           <math.h>
//   cosf / sinf / tanf             with -DREF_SHIM_D9_MATH routed to the project's
//                                  deterministic functions (decision D9): libdevice's
//                                  bits are not knowable here.  Without the macro
//                                  the reference's text calls libm.
// The routed functions are defined in ref_driver.cpp, which is compiled with
// -ffp-contract=off as sbmp_math.h requires; the reference's own text is compiled
// with -ffp-contract=fast (see oracle/Makefile).
#pragma once

#include <math.h>

#include "xorwow_ref.h"

typedef oracle::XorwowState curandState;

// x 2^-32 + 2^-33: the product is exact, so a contracted and an uncontracted build agree.
static inline float curand_uniform(curandState* state) { return oracle::xorwow_uniform(*state); }

#ifdef REF_SHIM_D9_MATH
float ref_shim_cosf(float x);
float ref_shim_sinf(float x);
float ref_shim_tanf(float x);
#define cosf(x) ref_shim_cosf(x)
#define sinf(x) ref_shim_sinf(x)
#define tanf(x) ref_shim_tanf(x)
#endif
