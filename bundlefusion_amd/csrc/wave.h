// wave.h — the integer wave and workgroup idioms every stream-compaction kernel shares: the lane index, the ballot
// mask of the lanes below one, and the exclusive scan / ordered compaction of one uint32 per lane over a 1-D workgroup.
// All sums are uint32 (they wrap), so any correct form gives the same bits; the floating-point reductions, whose
// order is their result, are not here (ba_dev.h, sift.hip).
//
// Contract of wg_exclusive_scan and wg_compact_offset: EVERY thread of the workgroup calls the helper (a thread with
// nothing to add passes 0 / false; never call under a per-lane condition), the workgroup is WAVES full waves, and
// sWave is WAVES words of LDS. The helper has one barrier, between its write of sWave and its reads; the caller puts
// a barrier before sWave is written again (the next call included), as a looping caller does at the end of a round.
#pragma once
#include <hip/hip_runtime.h>

namespace bf {

__device__ __forceinline__ unsigned lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// lanes of a wave below `lane`, as a ballot mask
__device__ __forceinline__ uint64_t lanes_below(uint32_t lane) { return lane == 0 ? 0ull : (~0ull >> (64 - lane)); }

// set bits of a ballot below `lane`: the lane's position among the wave's set flags
__device__ __forceinline__ uint32_t ballot_rank(uint64_t mask, uint32_t lane) { return (uint32_t)__popcll(mask & lanes_below(lane)); }

// inclusive scan over the wave
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v) {
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(v, o);
        if (lane >= (uint32_t)o) v += t;
    }
    return v;
}

// sums of the waves before this one and of all waves, from the per-wave totals in sWave
template <int WAVES>
__device__ __forceinline__ uint32_t wg_waves_before(const uint32_t* sWave, uint32_t& total) {
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < WAVES; w++) {
        const uint32_t s = sWave[w];
        before += (w < wave) ? s : 0u;
        all += s;
    }
    total = all;
    return before;
}

// exclusive scan of v over the workgroup; total = the workgroup's sum
template <int WAVES>
__device__ __forceinline__ uint32_t wg_exclusive_scan(uint32_t v, uint32_t* sWave, uint32_t& total) {
    const uint32_t incl = wave_inclusive_scan(v);
    if ((threadIdx.x & 63) == 63) sWave[threadIdx.x >> 6] = incl;
    __syncthreads();
    return wg_waves_before<WAVES>(sWave, total) + incl - v;
}

// position of this lane among the workgroup's set flags, in thread order; total = the number of set flags
template <int WAVES>
__device__ __forceinline__ uint32_t wg_compact_offset(bool flag, uint32_t* sWave, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t m = __ballot(flag);
    if (lane == 0) sWave[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    return wg_waves_before<WAVES>(sWave, total) + ballot_rank(m, lane);
}

}  // namespace bf
