// The data terms of PDHG, SPDHG and PDHG's stripe variable (pdhg_kernels.hip, pdhg_stripe.hip): the three families promise
// the same bits per data term, so the prox and the checks of its arguments are this one copy.  Everything here is internal
// to the including translation unit (anonymous namespace).
#pragma once
#include "tomo_common.h"
#include <cmath>

namespace {

// the prox of the conjugate of the data term at y + sigma r (step 2 of the algorithms; the stripe variable passes r + s-bar)
template <int MODE>
__device__ __forceinline__ float data_prox(float y, float r, float b, float sigma, float one_sigma, float c4)
{
    if (MODE == TOMO_PDHG_LS) return (y + sigma * (r - b)) / one_sigma;
    if (MODE == TOMO_PDHG_L1) {
        const float v = y + sigma * (r - b);
        return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
    }
    const float v = y + sigma * r;
    const float t = v - 1.0f;
    const float bp = b > 0.0f ? b : 0.0f;
    return 0.5f * ((1.0f + v) - sqrtf(t * t + c4 * bp));
}

static bool positive_finite(float v) { return v > 0.0f && std::isfinite(v); }

static bool known_fidelity(int f) { return f == TOMO_PDHG_LS || f == TOMO_PDHG_L1 || f == TOMO_PDHG_KL; }

}  // namespace
