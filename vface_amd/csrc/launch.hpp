// Host-side helpers every launcher shares.  No device code: a plain C++ translation unit can include this file.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vface_hip.h"

// the ABI passes a stream as void*
inline hipStream_t vf_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// what a launcher returns after its last launch
inline int vf_launched() { return hipGetLastError() == hipSuccess ? VFACE_OK : VFACE_ERR_LAUNCH; }

// workgroups of a grid-stride kernel over `total` items, `per` items per workgroup, at most `cap` (and never 0)
inline unsigned vf_grid(long total, int per, int cap) {
    long g = (total + per - 1) / per;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (unsigned)g;
}

// runs CALL with TT = F16 or BF16 (common.hpp); any other dtype is refused
#define DISPATCH_DTYPE(dtype, CALL)                             \
    if ((dtype) == VFACE_F16) { using TT = F16; CALL; }         \
    else if ((dtype) == VFACE_BF16) { using TT = BF16; CALL; }  \
    else return VFACE_ERR_DTYPE;
