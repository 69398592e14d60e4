// gs_adam_field.h -- the Adam rule on one field, shared by gs_adam_rows_device (gs_adam.hip) and gs_adam_rows_raw_device
// (gs_raw.hip).  Device only.
#pragma once

#include "gs_internal.h"

namespace gs {

__device__ __forceinline__ float pick(const float (&t)[6], uint32_t g) {
    return g == 0u ? t[0] : g == 1u ? t[1] : g == 2u ? t[2] : g == 3u ? t[3] : g == 4u ? t[4] : t[5];
}

// One field.  The order of the operations is the contract of the header (bitwise reproducible: the files are built with
// -ffp-contract=off and correctly rounded division and square root).
__device__ __forceinline__ void adam_field(float& p, float& m, float& v, float g, const AdamStep& a, float step, float lo,
                                           float hi) {
    m = a.beta1 * m + a.c1 * g;
    v = a.beta2 * v + (a.c2 * g) * g;
    const float q = p - step * (m / (sqrtf(v) + a.eps));
    p = q < lo ? lo : (q > hi ? hi : q);        // every comparison with a NaN is false: a NaN stays
}

}  // namespace gs
