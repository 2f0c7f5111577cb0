// match_dev.h — the device arithmetic of a key's camera-space point, shared by the matcher's kernels (match.hip) and the
// bundler's closing launch (bundler.hip), so that both write the same EntryJ bits.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/bf/types.h"

namespace bf {

// float4x4 * float3 with w = 1 (cuda_SimpleMatrixUtil.h:937-945)
__device__ __forceinline__ void xform3(const float* e, float x, float y, float z, float* o) {
    o[0] = e[0] * x + e[1] * y + e[2] * z + e[3] * 1.0f;
    o[1] = e[4] * x + e[5] * y + e[6] * z + e[7] * 1.0f;
    o[2] = e[8] * x + e[9] * y + e[10] * z + e[11] * 1.0f;
}

// camera-space point of a key: intrinsicsInv * (depth * (x, y, 1))
__device__ __forceinline__ void key_point(const float* kinv, const BFSiftKeyPoint& k, float* o) {
    xform3(kinv, k.depth * k.x, k.depth * k.y, k.depth * 1.0f, o);
}

}  // namespace bf
