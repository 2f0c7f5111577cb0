// wave_test.hip — bf_debug_wg_scan: wave.h's two workgroup helpers run directly, at sizes the kernels that use them
// never reach (tests/test_wave_gpu.py). One workgroup walks the input in rounds of its size with a carry, the shape
// of k_corr_pack.
#include <hip/hip_runtime.h>

#include "bf_runtime.h"
#include "wave.h"

namespace bf {

namespace {

template <int WG, bool FLAGS>
__global__ __launch_bounds__(WG) void k_wg_scan(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out,
                                                uint32_t* __restrict__ total) {
    __shared__ uint32_t sWave[WG / 64];
    uint32_t carry = 0;  // the same in every lane
    for (uint32_t r = 0; r < n; r += WG) {
        const uint32_t i = r + threadIdx.x;
        const uint32_t v = i < n ? in[i] : 0u;
        uint32_t all;
        const uint32_t at = carry + (FLAGS ? wg_compact_offset<WG / 64>(v != 0u, sWave, all) : wg_exclusive_scan<WG / 64>(v, sWave, all));
        if (i < n) out[i] = at;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

template <int WG>
void launch_wg_scan(const uint32_t* in, uint32_t n, bool flags, uint32_t* out, uint32_t* total) {
    if (flags) k_wg_scan<WG, true><<<1, WG>>>(in, n, out, total);
    else k_wg_scan<WG, false><<<1, WG>>>(in, n, out, total);
}

}  // namespace

// out[i] = the sum of in[0, i) (flags: the number of non-zero words in in[0, i)), *total = that of in[0, n); all DEVICE
void debug_wg_scan(const uint32_t* in, uint32_t n, uint32_t wg, bool flags, uint32_t* out, uint32_t* total) {
    BF_REQUIRE(wg == 256 || wg == 512 || wg == 1024, BF_ERR_ARG, "wg is 256, 512 or 1024");
    BF_REQUIRE(total != nullptr && (n == 0 || (in != nullptr && out != nullptr)), BF_ERR_ARG, "null pointer");
    if (wg == 256) launch_wg_scan<256>(in, n, flags, out, total);
    else if (wg == 512) launch_wg_scan<512>(in, n, flags, out, total);
    else launch_wg_scan<1024>(in, n, flags, out, total);
    BF_LAUNCH_CHECK();
    BF_HIP(hipDeviceSynchronize());
}

}  // namespace bf
