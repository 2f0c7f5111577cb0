// sift.hip — gfx950 SIFT detector: SiftGPU (FriedLiver/Source/SiftGPU) as SiftGPU::SetParams configures it, from the
// float intensity + depth image to BFSiftKeyPoint[n] + uint8 descriptors [n][128].
//
// The reference runs a frame in well over a hundred small launches (FilterH / FilterV per level, ComputeDOG per level,
// ComputeKEY per level, orientation / reshape / descriptor / normalise per level) with three device -> host count
// copies. Here a detect is 24 launches and no host round trip:
//
//  * k_sift_pyramid (18 launches): one Gaussian level per job, both filter directions through an LDS tile with halo;
//    a launch carries up to two jobs, so octave o + 1 starts (DownsampleKernel, then its levels) beside octave o's last
//    two levels. Taps are added in the reference's order from 0, contraction is off: levels are bit-identical.
//  * k_sift_keys (1 launch, all octaves x 3 key levels): ComputeKEY_Kernel with its early-outs; the DoG values are
//    differences of the Gaussian levels taken where they are read. A workgroup owns a band of rows, compacts its keys
//    with ballot + prefix in (row, col) order and counts them.
//  * k_sift_scan (one workgroup): band offsets, the per-level cap and LimitFeatureCount(0).
//  * k_sift_gather: the bands' keys to the levels' raw lists, in order.
//  * k_sift_orient: one wave per raw key; the gradient is taken from the Gaussian level where it is sampled.
//  * k_sift_reshape (one workgroup): ReshapeFeatureList's minKeyScale filter and orientation expansion, LimitFeature-
//    Count(1), the maxKeys cap, output offsets, the final list.
//  * k_sift_desc: one workgroup per final key over its 16 cells; normalisation, byte conversion and the key point.
// Later kernels are launched with worst-case grids and exit on the device-side counts.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/bf/bf.h"
#include "bf_runtime.h"
#include "sift.h"
#include "wave.h"

namespace bf {

namespace {

constexpr uint32_t kMinDim = 32, kMaxDim = 4096;
constexpr int FT = 32;           // pyramid tile edge
constexpr int FE = FT + 24;      // + halo of the widest filter the six tables reach (25 taps)
constexpr uint32_t kMaxBands = 3 * (1024 + 512 + 256 + 128);  // at kMaxDim rows and Sift::kBandRows

float powd(float b, float e) { return (float)std::pow((double)b, (double)e); }

}  // namespace

// ---- host: options and tables ------------------------------------------------------------------
SiftConfig make_sift_config(const BFSiftOptions* o) {
    BF_REQUIRE(o, BF_ERR_ARG, "null sift options");
    SiftConfig c;
    BF_REQUIRE(o->width >= kMinDim && o->height >= kMinDim && o->width <= kMaxDim && o->height <= kMaxDim, BF_ERR_ARG,
               "sift image size outside 32...4096: four octaves need (dim >> 3) >= 4");
    BF_REQUIRE(o->depthWidth >= 1 && o->depthHeight >= 1 && o->depthWidth <= kMaxDim && o->depthHeight <= kMaxDim, BF_ERR_ARG,
               "sift depth size outside 1...4096");
    c.width = o->width; c.height = o->height; c.depthWidth = o->depthWidth; c.depthHeight = o->depthHeight;
    BF_REQUIRE(o->maxKeys <= BF_MATCH_MAX_KEYS_PER_IMAGE, BF_ERR_ARG, "sift maxKeys above 1024");
    if (o->maxKeys) c.maxKeys = o->maxKeys;
    BF_REQUIRE(o->featureCountThreshold <= (1u << 30), BF_ERR_ARG, "sift featureCountThreshold");
    if (o->featureCountThreshold) c.featureCountThreshold = o->featureCountThreshold;
    const float th[5] = {o->sensorDepthMin, o->sensorDepthMax, o->minKeyScale, o->dogThreshold, o->edgeThreshold};
    for (float v : th) BF_REQUIRE(std::isfinite(v) && v >= 0.0f, BF_ERR_ARG, "sift threshold negative or not finite");
    if (o->sensorDepthMin > 0.0f) c.sensorDepthMin = o->sensorDepthMin;
    if (o->sensorDepthMax > 0.0f) c.sensorDepthMax = o->sensorDepthMax;
    BF_REQUIRE(c.sensorDepthMin <= c.sensorDepthMax, BF_ERR_ARG, "sift sensorDepthMin above sensorDepthMax");
    if (o->minKeyScale > 0.0f) c.minKeyScale = o->minKeyScale;
    if (o->dogThreshold > 0.0f) c.dogThreshold = o->dogThreshold;
    if (o->edgeThreshold > 0.0f) c.edgeThreshold = o->edgeThreshold;
    return c;
}

// SiftParam::ParseSiftParam (SiftGPU.cpp:127-174) at _dog_level_num 3, _level_min -1, _level_max 4, first octave 0, and
// ProgramCU::CreateFilterKernel (ProgramCU.cu:431-460). pow and exp are taken in double and rounded to float, so the
// tables do not depend on which float routine a C library ships.
void make_sift_tables(SiftTables& t) {
    std::memset(&t, 0, sizeof(t));
    const float sigmak = powd(2.0f, 1.0f / 3.0f);
    const float sigma0 = 1.6f * powd(2.0f, 1.0f / 3.0f);
    const float dsigma0 = sigma0 * std::sqrt(1.0f - 1.0f / (sigmak * sigmak));
    float sigmas[6];
    const float sa = sigma0 * powd(2.0f, -1.0f / 3.0f), sb = 0.5f / powd(2.0f, 0.0f);  // GetInitialSmoothSigma(0)
    sigmas[0] = (double)sa > (double)sb + 0.001 ? std::sqrt(sa * sa - sb * sb) : 0.0f;
    for (int i = 0; i < 5; i++) sigmas[i + 1] = dsigma0 * powd(sigmak, (float)i);
    for (int j = 0; j < 3; j++) t.levelSigma[j] = sigma0 * powd(2.0f, (float)j / 3.0f);  // GetLevelSigma
    for (int f = 0; f < 6; f++) {
        const float sigma = sigmas[f];
        int sz = (int)std::ceil(4.0f * sigma - 0.5);
        int width = 2 * sz + 1;
        if (width > BF_SIFT_MAX_FILTER) { sz = BF_SIFT_MAX_FILTER >> 1; width = BF_SIFT_MAX_FILTER; }
        else if (width < 5) { sz = 2; width = 5; }
        float rv = 1.0f / (sigma * sigma), ksum = 0.0f;
        for (int i = -sz; i <= sz; i++) {
            const float v = (float)std::exp((double)(-0.5f * (float)i * (float)i * rv));
            t.k[f][i + sz] = v;
            ksum += v;
        }
        rv = 1.0f / ksum;
        for (int i = 0; i < width; i++) t.k[f][i] *= rv;
        t.width[f] = (uint32_t)width;
    }
}

namespace {

// ---- intensity ----------------------------------------------------------------------------------
// resampleToIntensity_Kernel (CUDAImageUtil.cu:224-241) + convertToIntensity (:197-199)
__global__ __launch_bounds__(256) void k_sift_intensity(const uchar4* color, uint32_t cW, uint32_t cH, float* out, uint32_t W, uint32_t H) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= W * H) return;
    const uint32_t x = p % W, y = p / W;
    const float scaleWidth = (float)(cW - 1) / (float)(W - 1);
    const float scaleHeight = (float)(cH - 1) / (float)(H - 1);
    const uint32_t xi = (uint32_t)((float)x * scaleWidth + 0.5f), yi = (uint32_t)((float)y * scaleHeight + 0.5f);
    if (xi < cW && yi < cH) {
        const uchar4 c = color[yi * cW + xi];
        out[p] = (0.299f * (float)c.x + 0.587f * (float)c.y + 0.114f * (float)c.z) / 255.0f;
    }
}

// ---- pyramid ------------------------------------------------------------------------------------
struct PyrJob {
    const float* src;
    float* dst;
    int w, h;    // of dst (and of src when filtering)
    int sw;      // source row length when downsampling
    int fw;      // taps; 0: DownsampleKernel (every second pixel)
    int tilesX, blocks;
    float k[BF_SIFT_MAX_FILTER];
};
struct PyrArgs {
    PyrJob job[2];
};

// FilterH then FilterV (ProgramCU.cu:159-264) of one FT x FT tile: clamp-to-edge, value = 0, value += data[i] * k[i]
// for ascending i. The coefficients are kernel arguments (wave-uniform: scalar registers).
template <int FW>
__device__ __forceinline__ void filter_tile(const PyrJob& J, int tile, float* in, float* mid) {
    constexpr int HW = FW >> 1, E = FT + FW - 1;
    const int tx0 = (tile % J.tilesX) * FT, ty0 = (tile / J.tilesX) * FT;
    const int w = J.w, h = J.h;
    float kc[FW];
#pragma unroll
    for (int i = 0; i < FW; i++) kc[i] = J.k[i];
    for (int idx = threadIdx.x; idx < E * E; idx += 256) {
        const int ly = idx / E, lx = idx % E;
        const int gx = min(max(tx0 + lx - HW, 0), w - 1), gy = min(max(ty0 + ly - HW, 0), h - 1);
        in[idx] = J.src[(size_t)gy * w + gx];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < E * FT; idx += 256) {
        const int ly = idx / FT, lx = idx % FT;
        float v = 0.0f;
#pragma unroll
        for (int i = 0; i < FW; i++) v += in[ly * E + lx + i] * kc[i];
        mid[idx] = v;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < FT * FT; idx += 256) {
        const int ly = idx / FT, lx = idx % FT;
        const int gx = tx0 + lx, gy = ty0 + ly;
        if (gx < w && gy < h) {
            float v = 0.0f;
#pragma unroll
            for (int i = 0; i < FW; i++) v += mid[(ly + i) * FT + lx] * kc[i];
            J.dst[(size_t)gy * w + gx] = v;
        }
    }
}

__global__ __launch_bounds__(256) void k_sift_pyramid(PyrArgs A) {
    __shared__ float in[FE * FE];
    __shared__ float mid[FE * FT];
    const int j = (int)blockIdx.x < A.job[0].blocks ? 0 : 1;
    const PyrJob& J = A.job[j];
    const int tile = (int)blockIdx.x - (j ? A.job[0].blocks : 0);
    switch (J.fw) {
        case 0: {  // DownsampleKernel (ProgramCU.cu:330-341)
            const int tx0 = (tile % J.tilesX) * FT, ty0 = (tile / J.tilesX) * FT;
            for (int idx = threadIdx.x; idx < FT * FT; idx += 256) {
                const int gx = tx0 + idx % FT, gy = ty0 + idx / FT;
                if (gx < J.w && gy < J.h) J.dst[(size_t)gy * J.w + gx] = J.src[(size_t)(gy << 1) * J.sw + min(gx << 1, J.sw - 1)];
            }
            break;
        }
        case 11: filter_tile<11>(J, tile, in, mid); break;
        case 13: filter_tile<13>(J, tile, in, mid); break;
        case 17: filter_tile<17>(J, tile, in, mid); break;
        case 21: filter_tile<21>(J, tile, in, mid); break;
        case 25: filter_tile<25>(J, tile, in, mid); break;
        default: break;  // the host launches only the widths above
    }
}

// ---- key detection --------------------------------------------------------------------------------
struct KeyArgs {
    const float* g[4][6];
    uint32_t* stage[BF_SIFT_LEVELS];
    uint32_t* bandCount;
    const float* depth;
    int w[4], h[4], bandStart[5];
    int iw, ih, dw, dh;
    float dmin, dmax, thr, edge;
};

// ComputeKEY_Kernel (ProgramCU.cu:616-750) with subpixel_localization 0; c = DoG level of the key, p / n the levels
// below / above, each the difference of two Gaussian levels (ComputeDOG_Kernel :571-582) taken here.
__device__ __forceinline__ bool key_test(const KeyArgs& A, int o, const float* g0, const float* g1, const float* g2, const float* g3,
                                         int w, int h, int row, int col) {
    if (row < 1 || col < 1 || row >= h - 2 || col >= w - 2) return false;
    const float kls = (float)(1 << o);
    const int dx = (int)roundf((kls * (float)col + 0.5f) * (float)(A.dw - 1) / (float)(A.iw - 1));
    const int dy = (int)roundf((kls * (float)row + 0.5f) * (float)(A.dh - 1) / (float)(A.ih - 1));
    if (dx < 0 || dx >= A.dw || dy < 0 || dy >= A.dh) return false;
    const float depth = A.depth[(size_t)dy * A.dw + dx];
    if (!(depth >= A.dmin && depth <= A.dmax)) return false;  // -inf (and NaN) invalid
    const int i1 = row * w + col, i0 = i1 - w, i2 = i1 + w;
#define BF_DOG_C(i) (g2[i] - g1[i])
#define BF_DOG_P(i) (g1[i] - g0[i])
#define BF_DOG_N(i) (g3[i] - g2[i])
    const float v = BF_DOG_C(i1);
    if (fabsf(v) <= A.thr) return false;
    const float d10 = BF_DOG_C(i1 - 1), d12 = BF_DOG_C(i1 + 1);
    float nmax = fmaxf(d10, d12), nmin = fminf(d10, d12);
    if (v <= nmax && v >= nmin) return false;
    // READ_CMP_DOG_DATA (:598-614): the side is chosen again at every triple, ties pass
#define BF_CMP3(a, b, c)                                   \
    if (v > nmax) {                                        \
        nmax = fmaxf(fmaxf(fmaxf(nmax, a), b), c);         \
        if (v < nmax) return false;                        \
    } else {                                               \
        nmin = fminf(fminf(fminf(nmin, a), b), c);         \
        if (v > nmin) return false;                        \
    }
    const float d00 = BF_DOG_C(i0 - 1), d01 = BF_DOG_C(i0), d02 = BF_DOG_C(i0 + 1);
    BF_CMP3(d00, d01, d02)
    const float d20 = BF_DOG_C(i2 - 1), d21 = BF_DOG_C(i2), d22 = BF_DOG_C(i2 + 1);
    BF_CMP3(d20, d21, d22)
    const float vx2 = v * 2.0f;
    const float fxx = d10 + d12 - vx2;
    const float fyy = d01 + d21 - vx2;
    const float fxy = 0.25f * (d22 + d00 - d20 - d02);
    const float temp1 = fxx * fyy - fxy * fxy;
    const float temp2 = (fxx + fyy) * (fxx + fyy);
    if (temp1 <= 0 || temp2 > A.edge * temp1) return false;
    {
        const float a0 = BF_DOG_P(i0 - 1), a1 = BF_DOG_P(i0), a2 = BF_DOG_P(i0 + 1);
        BF_CMP3(a0, a1, a2)
        const float b0 = BF_DOG_P(i1 - 1), b1 = BF_DOG_P(i1), b2 = BF_DOG_P(i1 + 1);
        BF_CMP3(b0, b1, b2)
        const float c0 = BF_DOG_P(i2 - 1), c1 = BF_DOG_P(i2), c2 = BF_DOG_P(i2 + 1);
        BF_CMP3(c0, c1, c2)
    }
    {
        const float a0 = BF_DOG_N(i0 - 1), a1 = BF_DOG_N(i0), a2 = BF_DOG_N(i0 + 1);
        BF_CMP3(a0, a1, a2)
        const float b0 = BF_DOG_N(i1 - 1), b1 = BF_DOG_N(i1), b2 = BF_DOG_N(i1 + 1);
        BF_CMP3(b0, b1, b2)
        const float c0 = BF_DOG_N(i2 - 1), c1 = BF_DOG_N(i2), c2 = BF_DOG_N(i2 + 1);
        BF_CMP3(c0, c1, c2)
    }
#undef BF_CMP3
#undef BF_DOG_C
#undef BF_DOG_P
#undef BF_DOG_N
    return true;
}

// grid (bands of all octaves, 3 key levels); a band's keys go to its own stretch of the level's staging array
// (from pixel r0 * w on: a band never holds more keys than pixels), in (row, col) order
__global__ __launch_bounds__(256) void k_sift_keys(KeyArgs A) {
    __shared__ uint32_t waveCnt[4];
    const int b = blockIdx.x, jj = blockIdx.y;
    int o = 0;
    while (o < 3 && b >= A.bandStart[o + 1]) o++;
    const int band = b - A.bandStart[o], bands = A.bandStart[o + 1] - A.bandStart[o];
    const int w = A.w[o], h = A.h[o];
    const int r0 = band * (int)Sift::kBandRows, rows = min((int)Sift::kBandRows, h - r0), npix = rows * w;
    const float *g0 = A.g[o][jj], *g1 = A.g[o][jj + 1], *g2 = A.g[o][jj + 2], *g3 = A.g[o][jj + 3];
    uint32_t* stage = A.stage[o * 3 + jj] + (size_t)r0 * w;
    uint32_t running = 0;
    for (int base = 0; base < npix; base += 256) {
        const int idx = base + (int)threadIdx.x;
        bool flag = false;
        int row = 0, col = 0;
        if (idx < npix) {
            row = r0 + idx / w;
            col = idx % w;
            flag = key_test(A, o, g0, g1, g2, g3, w, h, row, col);
        }
        uint32_t total;
        const uint32_t off = running + wg_compact_offset<4>(flag, waveCnt, total);
        if (flag) stage[off] = ((uint32_t)row << 16) | (uint32_t)col;
        running += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) A.bandCount[3 * A.bandStart[o] + jj * bands + band] = running;
}

struct ScanArgs {
    uint32_t* bandCount;
    uint32_t* bandOffset;
    Sift::Counts* counts;
    int bandStart[5];
    uint32_t fmax[4];
    uint32_t featureCountThreshold;
};

// band offsets per level, the per-level cap (SiftPyramid::DetectKeypoints :387-393) and LimitFeatureCount(0) (:227-255,
// truncate method 0), whose while loop is stopped at the last level here
__global__ __launch_bounds__(1024) void k_sift_scan(ScanArgs A) {
    __shared__ uint32_t s[kMaxBands];
    __shared__ uint32_t tot[BF_SIFT_LEVELS];
    const int n = 3 * A.bandStart[4];
    for (int i = threadIdx.x; i < n; i += 1024) s[i] = A.bandCount[i];
    __syncthreads();
    if (threadIdx.x < BF_SIFT_LEVELS) {
        const int L = threadIdx.x, o = L / 3, jj = L % 3, bands = A.bandStart[o + 1] - A.bandStart[o];
        const int base = 3 * A.bandStart[o] + jj * bands;
        uint32_t run = 0;
        for (int k = 0; k < bands; k++) {
            const uint32_t c = s[base + k];
            s[base + k] = run;
            run += c;
        }
        tot[L] = run;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 1024) A.bandOffset[i] = s[i];
    if (threadIdx.x == 0) {
        uint32_t num[BF_SIFT_LEVELS];
        uint32_t featureNum = 0;
        for (int L = 0; L < BF_SIFT_LEVELS; L++) {
            A.counts->raw[L] = tot[L];
            num[L] = min(tot[L], A.fmax[L / 3]);
            featureNum += num[L];
        }
        int i = 0;
        while (i < BF_SIFT_LEVELS && featureNum - num[i] > A.featureCountThreshold) {
            featureNum -= num[i];
            num[i++] = 0;
        }
        for (int L = 0; L < BF_SIFT_LEVELS; L++) A.counts->list[L] = num[L];
    }
}

struct GatherArgs {
    const uint32_t* stage[BF_SIFT_LEVELS];
    const uint32_t* bandCount;
    const uint32_t* bandOffset;
    const Sift::Counts* counts;
    uint32_t* rawList;
    uint32_t* rawOri;
    int w[4], bandStart[5];
    uint32_t listOff[BF_SIFT_LEVELS + 1];
};

__global__ __launch_bounds__(256) void k_sift_gather(GatherArgs A) {
    const int b = blockIdx.x, jj = blockIdx.y;
    int o = 0;
    while (o < 3 && b >= A.bandStart[o + 1]) o++;
    const int band = b - A.bandStart[o], bands = A.bandStart[o + 1] - A.bandStart[o], L = o * 3 + jj;
    const int bi = 3 * A.bandStart[o] + jj * bands + band;
    const uint32_t cnt = A.bandCount[bi], off = A.bandOffset[bi], n = A.counts->list[L];  // n <= fmax of the level
    const uint32_t* stage = A.stage[L] + (size_t)band * Sift::kBandRows * A.w[o];
    for (uint32_t i = threadIdx.x; i < cnt; i += 256) {
        const uint32_t p = off + i;
        if (p < n) {
            A.rawList[A.listOff[L] + p] = stage[i];
            A.rawOri[A.listOff[L] + p] = 0xFFFFFFFFu;
        }
    }
}

// ---- orientation ----------------------------------------------------------------------------------
// ComputeDOG_Kernel's gradient (ProgramCU.cu:560-567) of Gaussian level g at an interior pixel: {magnitude, angle}
__device__ __forceinline__ float2 grad_at(const float* g, int w, int px, int py) {
    const int i = py * w + px;
    const float dx = g[i + 1] - g[i - 1], dy = g[i + w] - g[i - w];
    const float grd = 0.5f * sqrtf(dx * dx + dy * dy);
    return make_float2(grd, grd == 0.0f ? 0.0f : atan2f(dy, dx));
}

struct OriArgs {
    const float* g[4][6];
    const uint32_t* rawList;
    uint32_t* rawOri;
    const Sift::Counts* counts;
    int w[4], h[4];
    uint32_t listOff[BF_SIFT_LEVELS + 1];
    float sigma[3];
    uint32_t mask;  // levels whose keys can pass minKeyScale
};

// ComputeOrientation_Kernel (ProgramCU.cu:905-1142), one wave per key, lane = the reference's thread. Votes: every lane
// adds its samples (sample index lane, lane + 64, ...) into its own 36 bins in LDS, then bin b is the sum of the lanes'
// partial sums in ascending lane order.
__global__ __launch_bounds__(64) void k_sift_orient(OriArgs A) {
    __shared__ float vote[36 * 64];
    __shared__ float hist[2][36];
    const int L = blockIdx.y, lane = threadIdx.x;
    if (!((A.mask >> L) & 1u) || blockIdx.x >= A.counts->list[L]) return;
    const int o = L / 3, jj = L % 3, w = A.w[o], h = A.h[o];
    const float* g = A.g[o][jj + 1];
    const uint32_t cr = A.rawList[A.listOff[L] + blockIdx.x];
    const float kx = (float)(cr & 0xFFFFu) + 0.5f, ky = (float)(cr >> 16) + 0.5f, sigma = A.sigma[jj];
    const float gsigma = sigma * 1.5f;
    const float win = fabsf(sigma) * 1.5f * 2.0f;
    const float dist_threshold = (float)((double)(win * win) + 0.5);
    const float factor = -0.5f / (gsigma * gsigma);
    const float xmin = fmaxf(1.5f, floorf(kx - win) + 0.5f), ymin = fmaxf(1.5f, floorf(ky - win) + 0.5f);
    const float xmax = fminf((float)w - 1.5f, floorf(kx + win) + 0.5f), ymax = fminf((float)h - 1.5f, floorf(ky + win) + 0.5f);
    for (int b = 0; b < 36; b++) vote[b * 64 + lane] = 0.0f;
    uint32_t xlen = 0, num = 0;
    if (xmax >= xmin && ymax >= ymin) {
        xlen = (uint32_t)roundf(xmax - xmin + 1);
        num = (uint32_t)roundf(ymax - ymin + 1) * xlen;
    }
    for (uint32_t i = lane; i < num; i += 64) {
        const float x = (float)(i % xlen) + xmin, y = (float)(i / xlen) + ymin;
        const float dx = x - kx, dy = y - ky;
        const float sq_dist = dx * dx + dy * dy;
        if (sq_dist < dist_threshold) {
            const float2 got = grad_at(g, w, (int)x, (int)y);
            const float weight = got.x * expf(sq_dist * factor);
            int oidx = (int)floorf(got.y * 5.7295779513082320876798154814105f);
            if (oidx < 0) oidx += 36;
            vote[oidx * 64 + lane] += weight;
        }
    }
    __syncthreads();
    if (lane < 36) {
        float v = 0.0f;
        for (int l = 0; l < 64; l++) v += vote[lane * 64 + l];
        hist[0][lane] = v;
    }
    __syncthreads();
    const float one_third = (float)(1.0 / 3.0);
    int src = 0;
    for (int it = 0; it < 6; it++) {
        if (lane < 36) hist[src ^ 1][lane] = (hist[src][(lane + 35) % 36] + hist[src][lane] + hist[src][(lane + 1) % 36]) * one_third;
        __syncthreads();
        src ^= 1;
    }
    if (lane == 0) {
        const float* vt = hist[src];
        float max_vote = 0.0f;
        for (int b = 0; b < 36; b++) max_vote = fmaxf(max_vote, vt[b]);
        const float thr = max_vote * 0.8f;
        int c1 = -1, c2 = -1;  // the two largest peaks (the lower bin on an exact tie)
        for (int b = 0; b < 36; b++) {
            const float m = vt[(b + 35) % 36], c = vt[b], p = vt[(b + 1) % 36];
            if (c > thr && c > m && c > p) {
                if (c1 < 0 || c > vt[c1]) { c2 = c1; c1 = b; }
                else if (c2 < 0 || c > vt[c2]) c2 = b;
            }
        }
        uint32_t us1 = 65535u, us2 = 65535u;
        if (c1 >= 0) {
            const float m = vt[(c1 + 35) % 36], c = vt[c1], p = vt[(c1 + 1) % 36];
            const float rot = (float)c1 + 0.5f * ((p - m) / (2.0f * c - p - m)) + 0.5f;
            float fr = rot / 36.0f;
            if (fr < 0) fr += 1.0f;
            us1 = (uint32_t)(unsigned short)floorf(fr * 65535.0f);
        }
        if (c2 >= 0) {
            const float m = vt[(c2 + 35) % 36], c = vt[c2], p = vt[(c2 + 1) % 36];
            const float rot = (float)c2 + 0.5f * ((p - m) / (2.0f * c - p - m)) + 0.5f;
            float fr = rot / 36.0f;
            if (fr < 0) fr += 1.0f;
            us2 = (uint32_t)(unsigned short)floorf(fr * 65535.0f);
        }
        A.rawOri[A.listOff[L] + blockIdx.x] = (us2 << 16) | us1;
    }
}

// ---- reshape, limits, offsets ---------------------------------------------------------------------
struct ReshapeArgs {
    const uint32_t* rawList;
    const uint32_t* rawOri;
    Sift::Counts* counts;
    uint4* fin;
    uint32_t listOff[BF_SIFT_LEVELS + 1];
    uint32_t fmax[4];
    uint32_t mask, featureCountThreshold, maxKeys;
};

// final entries of a raw key (ReshapeFeatureList_Kernel, ProgramCU.cu:1994-2026)
__device__ __forceinline__ uint32_t ori_count(uint32_t packed) {
    const uint32_t us1 = packed & 0xFFFFu, us2 = packed >> 16;
    if (us1 == 65535u) return 0;
    return (us2 != 65535u && us2 != us1) ? 2u : 1u;
}

__global__ __launch_bounds__(1024) void k_sift_reshape(ReshapeArgs A) {
    __shared__ uint32_t tot[BF_SIFT_LEVELS], start[BF_SIFT_LEVELS], keep[BF_SIFT_LEVELS], wsum[16];
    const int tid = threadIdx.x;
    if (tid < BF_SIFT_LEVELS) tot[tid] = 0;
    __syncthreads();
    for (int L = 0; L < BF_SIFT_LEVELS; L++) {
        if (!((A.mask >> L) & 1u)) continue;
        const uint32_t n = A.counts->list[L];
        uint32_t local = 0;
        for (uint32_t i = tid; i < n; i += 1024) local += ori_count(A.rawOri[A.listOff[L] + i]);
        if (local) atomicAdd(&tot[L], local);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t featureNum = 0;
        for (int L = 0; L < BF_SIFT_LEVELS; L++) {
            tot[L] = min(tot[L], A.fmax[L / 3]);  // the final list of a level holds fmax entries too
            featureNum += tot[L];
        }
        int i = 0;  // LimitFeatureCount(1)
        while (i < BF_SIFT_LEVELS && featureNum - tot[i] > A.featureCountThreshold) {
            featureNum -= tot[i];
            tot[i++] = 0;
        }
        // the key cap (SiftPyramid::CreateGlobalKeyPointList :746-757 as intended): coarsest levels first
        uint32_t cur = 0;
        for (int L = BF_SIFT_LEVELS - 1; L >= 0; L--) {
            keep[L] = min(tot[L], A.maxKeys - cur);
            cur += keep[L];
        }
        uint32_t run = 0;
        for (int L = 0; L < BF_SIFT_LEVELS; L++) {
            start[L] = run;
            run += keep[L];
            A.counts->kept[L] = keep[L];
            A.counts->outStart[L] = start[L];
        }
        A.counts->nFinal = run;
        A.counts->flags = featureNum > A.maxKeys ? BF_SIFT_TRUNCATED : 0u;
    }
    __syncthreads();
    const float factor = (float)(2.0 * 3.14159265358979323846 / 65535.0);
    for (int L = 0; L < BF_SIFT_LEVELS; L++) {
        const uint32_t kp = keep[L];
        if (kp == 0) continue;
        const uint32_t n = A.counts->list[L];
        uint32_t running = 0;
        for (uint32_t base = 0; base < n && running < kp; base += 1024) {
            const uint32_t i = base + tid;
            uint32_t packed = 0xFFFFFFFFu, cr = 0;
            if (i < n) {
                packed = A.rawOri[A.listOff[L] + i];
                cr = A.rawList[A.listOff[L] + i];
            }
            const uint32_t c = ori_count(packed);
            uint32_t total;
            const uint32_t p = running + wg_exclusive_scan<16>(c, wsum, total);
            if (c >= 1 && p < kp) A.fin[start[L] + p] = make_uint4(cr, (uint32_t)L, __float_as_uint(factor * (float)(packed & 0xFFFFu)), 0u);
            if (c == 2 && p + 1 < kp) A.fin[start[L] + p + 1] = make_uint4(cr, (uint32_t)L, __float_as_uint(factor * (float)(packed >> 16)), 0u);
            running += total;
            __syncthreads();
        }
    }
}

// ---- descriptor -----------------------------------------------------------------------------------
struct DescArgs {
    const float* g[4][6];
    const uint4* fin;
    const Sift::Counts* counts;
    const float* depth;
    BFSiftKeyPoint* keys;
    uint8_t* descs;
    int w[4], h[4];
    int iw, ih, dw, dh;
    float sigma[3];
};

// ComputeDescriptor_Kernel (ProgramCU.cu:1178-1257) + NormalizeDescriptor_Kernel (:1339-1370) + ConvertDescriptorTo-
// UChar_Kernel (:2100-2107) + CreateGlobalKeyPointList_Kernel (:2049-2081), one workgroup per final key: 16 lanes per
// cell. Every lane adds its samples (sample index l, l + 16, ...) into 8 bins of its own in registers; bin b of a cell
// is then the sum of its 16 lanes' partial sums in ascending lane order. The norms are LDS trees of fixed shape.
__global__ __launch_bounds__(256) void k_sift_desc(DescArgs A) {
    __shared__ float part[256 * 8];
    __shared__ float des[128], sq[128];
    const uint32_t f = blockIdx.x;
    if (f >= A.counts->nFinal) return;
    const int tid = threadIdx.x;
    const uint4 e = A.fin[f];
    const int col = (int)(e.x & 0xFFFFu), row = (int)(e.x >> 16), L = (int)e.y, o = L / 3, jj = L % 3;
    const int w = A.w[o], h = A.h[o];
    const float* g = A.g[o][jj + 1];
    const float kx = (float)col + 0.5f, ky = (float)row + 0.5f, sigma = A.sigma[jj], ori = __uint_as_float(e.z);
    const int cell = tid >> 4, l16 = tid & 15, ix = cell & 3, iy = cell >> 2;
    const float rpi = (float)(4.0 / 3.14159265358979323846);
    const float spt = fabsf(sigma * 3.0f);
    float s, c;
    sincosf(ori, &s, &c);
    const float anglef = (double)ori > 3.14159265358979323846 ? (float)((double)ori - 2.0 * 3.14159265358979323846) : ori;
    const float cspt = c * spt, sspt = s * spt;
    const float crspt = c / spt, srspt = s / spt;
    const float ox = (float)ix - 1.5f, oy = (float)iy - 1.5f;
    const float ptx = cspt * ox - sspt * oy + kx;
    const float pty = cspt * oy + sspt * ox + ky;
    const float bsz = fabsf(cspt) + fabsf(sspt);
    const float xmin = fmaxf(1.5f, floorf(ptx - bsz) + 0.5f), ymin = fmaxf(1.5f, floorf(pty - bsz) + 0.5f);
    const float xmax = fminf((float)w - 1.5f, floorf(ptx + bsz) + 0.5f), ymax = fminf((float)h - 1.5f, floorf(pty + bsz) + 0.5f);
    uint32_t xlen = 0, size = 0;
    if (xmax >= xmin && ymax >= ymin) {
        xlen = (uint32_t)roundf(xmax - xmin + 1);
        size = (uint32_t)roundf(ymax - ymin + 1) * xlen;
    }
    float d[8];
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = 0.0f;
    for (uint32_t i = l16; i < size; i += 16) {
        const float x = (float)(i % xlen) + xmin, y = (float)(i / xlen) + ymin;
        const float dx = x - ptx, dy = y - pty;
        const float nx = crspt * dx + srspt * dy;
        const float ny = crspt * dy - srspt * dx;
        const float nxn = fabsf(nx), nyn = fabsf(ny);
        if (nxn < 1.0f && nyn < 1.0f) {
            const float2 cc = grad_at(g, w, (int)x, (int)y);
            const float dnx = nx + ox, dny = ny + oy;
            const float ww = expf(-0.125f * (dnx * dnx + dny * dny));
            const float wx = 1.0f - nxn, wy = 1.0f - nyn;
            const float weight = ww * wx * wy * cc.x;
            float theta = (anglef - cc.y) * rpi;
            if (theta < 0) theta += 8.0f;
            const float fo = floorf(theta);
            const int f0 = (int)fo & 7, f1 = ((int)fo + 1) & 7;  // theta == 8 wraps to bin 0 (the reference writes past des[7])
            const float a1 = (fo + 1.0f - theta) * weight, a2 = (theta - fo) * weight;
#pragma unroll
            for (int k = 0; k < 8; k++) d[k] += (k == f0) ? a1 : ((k == f1) ? a2 : 0.0f);
        }
    }
#pragma unroll
    for (int k = 0; k < 8; k++) part[tid * 8 + k] = d[k];
    __syncthreads();
    float v = 0.0f;
    if (tid < 128) {
        const int cl = tid >> 3, bin = tid & 7;  // element (iy * 4 + ix) * 8 + bin == tid
        for (int l = 0; l < 16; l++) v += part[(cl * 16 + l) * 8 + bin];
    }
    for (int pass = 0; pass < 2; pass++) {
        if (tid < 128) sq[tid] = v * v;
        __syncthreads();
        for (int st = 64; st > 0; st >>= 1) {
            if (tid < st) sq[tid] += sq[tid + st];
            __syncthreads();
        }
        const float norm = 1.0f / sqrtf(sq[0]);
        v = pass == 0 ? fminf(0.2f, v * norm) : v * norm;
        __syncthreads();
    }
    if (tid < 128) A.descs[(size_t)f * 128 + tid] = (unsigned char)(int)((double)(512.0f * v) + 0.5);
    if (tid == 0) {
        const float kls = (float)(1 << o);
        BFSiftKeyPoint kp;
        kp.x = kls * (kx - 0.5f) + 0.5f;
        kp.y = kls * (ky - 0.5f) + 0.5f;
        kp.scale = kls * sigma;
        const int ipx = (int)roundf(kp.x * (float)(A.dw - 1) / (float)(A.iw - 1));
        const int ipy = (int)roundf(kp.y * (float)(A.dh - 1) / (float)(A.ih - 1));
        kp.depth = A.depth[(size_t)min(max(ipy, 0), A.dh - 1) * A.dw + min(max(ipx, 0), A.dw - 1)];
        A.keys[f] = kp;
    }
}

}  // namespace

// ---- host -----------------------------------------------------------------------------------------
Sift::Sift(const SiftConfig& cfg, hipStream_t stream) : cfg_(cfg), stream_(stream) {
    make_sift_tables(tab_);
    for (uint32_t w : tab_.width)  // k_sift_pyramid instantiates exactly these tap counts
        BF_REQUIRE(w == 11 || w == 13 || w == 17 || w == 21 || w == 25, BF_ERR_INTERNAL, "sift filter width without a kernel");
    size_t gaussTotal = 0, stageTotal = 0;
    bandStart_[0] = 0;
    listOff_[0] = 0;
    for (uint32_t o = 0; o < kOctaves; o++) {
        w_[o] = cfg.width >> o;
        h_[o] = cfg.height >> o;
        int fmax = (int)((float)(w_[o] * h_[o]) * 0.005f);  // SiftPyramid::BuildPyramid :133-136
        fmax = fmax > 4096 ? 4096 : (fmax < 32 ? 32 : fmax);
        fmax_[o] = (uint32_t)fmax;
        bands_[o] = div_up(h_[o], kBandRows);
        bandStart_[o + 1] = bandStart_[o] + bands_[o];
        for (uint32_t l = 0; l < kGauss; l++) {
            gaussOff_[o][l] = gaussTotal;
            gaussTotal += (size_t)w_[o] * h_[o];
        }
        for (uint32_t j = 0; j < kKeyLevels; j++) {
            stageOff_[o * 3 + j] = stageTotal;
            stageTotal += (size_t)w_[o] * h_[o];
            listOff_[o * 3 + j + 1] = listOff_[o * 3 + j] + fmax_[o];
            // ReshapeFeatureList_Kernel's test, on the host: the level's sigma is a constant
            if (tab_.levelSigma[j] * (float)(1 << o) >= cfg.minKeyScale) orientMask_ |= 1u << (o * 3 + j);
        }
    }
    BF_REQUIRE(3 * bandStart_[kOctaves] <= kMaxBands, BF_ERR_INTERNAL, "sift band table");
    intensity_.alloc((size_t)cfg.width * cfg.height);
    gauss_.alloc(gaussTotal);
    stage_.alloc(stageTotal);
    bandCount_.alloc(3 * bandStart_[kOctaves]);
    bandOffset_.alloc(3 * bandStart_[kOctaves]);
    rawList_.alloc(listOff_[kLevels]);
    rawOri_.alloc(listOff_[kLevels]);
    final_.alloc(cfg.maxKeys);
    keys_.alloc(cfg.maxKeys);
    descs_.alloc((size_t)cfg.maxKeys * 128);
    counts_.alloc(1);
    BF_HIP(hipHostMalloc((void**)&hostCounts_, sizeof(Counts), hipHostMallocDefault));
    std::memset(hostCounts_, 0, sizeof(Counts));
    BF_HIP(hipMemsetAsync(counts_.p, 0, sizeof(Counts), stream_));
}

Sift::~Sift() {
    if (hostCounts_) (void)hipHostFree(hostCounts_);
}

void Sift::intensity(const uint8_t* color, uint32_t cw, uint32_t ch, float* out) {
    BF_REQUIRE(color, BF_ERR_ARG, "null colour image");
    BF_REQUIRE(cw >= 2 && ch >= 2 && cw <= 16384 && ch <= 16384, BF_ERR_ARG, "colour size");
    k_sift_intensity<<<div_up((size_t)cfg_.width * cfg_.height, 256), 256, 0, stream_>>>(
        reinterpret_cast<const uchar4*>(color), cw, ch, out ? out : intensity_.p, cfg_.width, cfg_.height);
    BF_LAUNCH_CHECK();
    if (!out) haveIntensity_ = true;
}

void Sift::detect(const float* intensity, const float* depth) {
    BF_REQUIRE(depth, BF_ERR_ARG, "null depth image");
    BF_REQUIRE(intensity || haveIntensity_, BF_ERR_STATE, "null intensity image and no bf_sift_intensity into the detector's buffer");
    const float* input = intensity ? intensity : intensity_.p;
    auto G = [&](uint32_t o, uint32_t l) { return gauss_.p + gaussOff_[o][l]; };
    // ---- pyramid (SiftPyramid::BuildPyramid :82-127): job (octave, level); octave o + 1 level 0 is every second pixel
    // of octave o level 3, so it starts beside octave o level 4
    auto job = [&](PyrJob& J, uint32_t o, uint32_t l) {
        J.dst = G(o, l);
        J.w = (int)w_[o];
        J.h = (int)h_[o];
        J.tilesX = (int)div_up(w_[o], FT);
        J.blocks = J.tilesX * (int)div_up(h_[o], FT);
        if (l == 0 && o > 0) {
            J.src = G(o - 1, 3);
            J.sw = (int)w_[o - 1];
            J.fw = 0;
        } else {
            J.src = l == 0 ? input : G(o, l - 1);
            J.sw = J.w;
            J.fw = (int)tab_.width[l];
            std::memcpy(J.k, tab_.k[l], sizeof(J.k));
        }
    };
    auto launch = [&](int o0, int l0, int o1, int l1) {
        PyrArgs a;
        std::memset(&a, 0, sizeof(a));
        job(a.job[0], (uint32_t)o0, (uint32_t)l0);
        if (o1 >= 0) job(a.job[1], (uint32_t)o1, (uint32_t)l1);
        k_sift_pyramid<<<a.job[0].blocks + a.job[1].blocks, 256, 0, stream_>>>(a);
        BF_LAUNCH_CHECK();
    };
    for (int l = 0; l < 4; l++) launch(0, l, -1, 0);
    for (int o = 0; o < 3; o++) {
        launch(o, 4, o + 1, 0);
        launch(o, 5, o + 1, 1);
        launch(o + 1, 2, -1, 0);
        launch(o + 1, 3, -1, 0);
    }
    launch(3, 4, -1, 0);
    launch(3, 5, -1, 0);

    // ---- keys, counts, raw lists
    KeyArgs ka{};
    GatherArgs ga{};
    OriArgs oa{};
    DescArgs da{};
    for (uint32_t o = 0; o < kOctaves; o++) {
        for (uint32_t l = 0; l < kGauss; l++) ka.g[o][l] = oa.g[o][l] = da.g[o][l] = G(o, l);
        ka.w[o] = ga.w[o] = oa.w[o] = da.w[o] = (int)w_[o];
        ka.h[o] = oa.h[o] = da.h[o] = (int)h_[o];
    }
    for (uint32_t L = 0; L < kLevels; L++) {
        ka.stage[L] = stage_.p + stageOff_[L];
        ga.stage[L] = stage_.p + stageOff_[L];
    }
    for (uint32_t o = 0; o <= kOctaves; o++) ka.bandStart[o] = ga.bandStart[o] = (int)bandStart_[o];
    ka.bandCount = bandCount_.p;
    ka.depth = depth;
    ka.iw = (int)cfg_.width; ka.ih = (int)cfg_.height; ka.dw = (int)cfg_.depthWidth; ka.dh = (int)cfg_.depthHeight;
    ka.dmin = cfg_.sensorDepthMin; ka.dmax = cfg_.sensorDepthMax;
    ka.thr = cfg_.dogThreshold;
    ka.edge = (cfg_.edgeThreshold + 1) * (cfg_.edgeThreshold + 1) / cfg_.edgeThreshold;  // ProgramCU::ComputeKEY :770
    const dim3 bandGrid(bandStart_[kOctaves], kKeyLevels);
    k_sift_keys<<<bandGrid, 256, 0, stream_>>>(ka);
    BF_LAUNCH_CHECK();
    ScanArgs sa{};
    sa.bandCount = bandCount_.p; sa.bandOffset = bandOffset_.p; sa.counts = counts_.p;
    for (uint32_t o = 0; o <= kOctaves; o++) sa.bandStart[o] = (int)bandStart_[o];
    for (uint32_t o = 0; o < kOctaves; o++) sa.fmax[o] = fmax_[o];
    sa.featureCountThreshold = cfg_.featureCountThreshold;
    k_sift_scan<<<1, 1024, 0, stream_>>>(sa);
    BF_LAUNCH_CHECK();
    ga.bandCount = bandCount_.p; ga.bandOffset = bandOffset_.p; ga.counts = counts_.p;
    ga.rawList = rawList_.p; ga.rawOri = rawOri_.p;
    std::memcpy(ga.listOff, listOff_, sizeof(ga.listOff));
    k_sift_gather<<<bandGrid, 256, 0, stream_>>>(ga);
    BF_LAUNCH_CHECK();

    // ---- orientations (SiftPyramid::GetFeatureOrientations :426-450)
    oa.rawList = rawList_.p; oa.rawOri = rawOri_.p; oa.counts = counts_.p;
    std::memcpy(oa.listOff, listOff_, sizeof(oa.listOff));
    std::memcpy(oa.sigma, tab_.levelSigma, sizeof(oa.sigma));
    oa.mask = orientMask_;
    k_sift_orient<<<dim3(fmax_[0], kLevels), 64, 0, stream_>>>(oa);
    BF_LAUNCH_CHECK();

    // ---- reshape + limits, then descriptors and key points
    ReshapeArgs ra{};
    ra.rawList = rawList_.p; ra.rawOri = rawOri_.p; ra.counts = counts_.p; ra.fin = final_.p;
    std::memcpy(ra.listOff, listOff_, sizeof(ra.listOff));
    for (uint32_t o = 0; o < kOctaves; o++) ra.fmax[o] = fmax_[o];
    ra.mask = orientMask_; ra.featureCountThreshold = cfg_.featureCountThreshold; ra.maxKeys = cfg_.maxKeys;
    k_sift_reshape<<<1, 1024, 0, stream_>>>(ra);
    BF_LAUNCH_CHECK();
    da.fin = final_.p; da.counts = counts_.p; da.depth = depth; da.keys = keys_.p; da.descs = descs_.p;
    da.iw = ka.iw; da.ih = ka.ih; da.dw = ka.dw; da.dh = ka.dh;
    std::memcpy(da.sigma, tab_.levelSigma, sizeof(da.sigma));
    k_sift_desc<<<cfg_.maxKeys, 256, 0, stream_>>>(da);
    BF_LAUNCH_CHECK();
    BF_HIP(hipMemcpyAsync(hostCounts_, counts_.p, sizeof(Counts), hipMemcpyDeviceToHost, stream_));
    detected_ = true;
}

void Sift::result(const BFSiftKeyPoint** keys, const uint8_t** descs, uint32_t* n, uint32_t* flags) {
    BF_REQUIRE(detected_, BF_ERR_STATE, "bf_sift_result before bf_sift_detect");
    BF_HIP(hipStreamSynchronize(stream_));
    if (keys) *keys = keys_.p;
    if (descs) *descs = descs_.p;
    if (n) *n = hostCounts_->nFinal;
    if (flags) *flags = hostCounts_->flags;
}

void Sift::levelCounts(uint32_t* raw, uint32_t* kept) {
    BF_REQUIRE(detected_, BF_ERR_STATE, "bf_sift_level_counts before bf_sift_detect");
    BF_HIP(hipStreamSynchronize(stream_));
    if (raw) std::memcpy(raw, hostCounts_->raw, sizeof(hostCounts_->raw));
    if (kept) std::memcpy(kept, hostCounts_->kept, sizeof(hostCounts_->kept));
}

void Sift::debugLevel(uint32_t octave, uint32_t level, float* host) {
    BF_REQUIRE(detected_, BF_ERR_STATE, "bf_sift_debug_level before bf_sift_detect");
    BF_REQUIRE(octave < kOctaves && level < kGauss && host, BF_ERR_ARG, "octave >= 4, level >= 6 or null output");
    BF_HIP(hipMemcpyAsync(host, gauss_.p + gaussOff_[octave][level], (size_t)w_[octave] * h_[octave] * sizeof(float),
                          hipMemcpyDeviceToHost, stream_));
    BF_HIP(hipStreamSynchronize(stream_));
}

void Sift::debugRawKeys(uint32_t level, int32_t* colRow, uint32_t* packed, uint32_t cap, uint32_t* n) {
    BF_REQUIRE(detected_, BF_ERR_STATE, "bf_sift_debug_raw_keys before bf_sift_detect");
    BF_REQUIRE(level < kLevels, BF_ERR_ARG, "levelIndex >= 12");
    BF_HIP(hipStreamSynchronize(stream_));
    const uint32_t cnt = hostCounts_->list[level], m = cnt < cap ? cnt : cap;
    if (n) *n = cnt;
    if (m == 0) return;
    std::vector<uint32_t> tmp(m);
    if (colRow) {
        BF_HIP(hipMemcpy(tmp.data(), rawList_.p + listOff_[level], m * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < m; i++) {
            colRow[2 * i] = (int32_t)(tmp[i] & 0xFFFFu);
            colRow[2 * i + 1] = (int32_t)(tmp[i] >> 16);
        }
    }
    if (packed) BF_HIP(hipMemcpy(packed, rawOri_.p + listOff_[level], m * sizeof(uint32_t), hipMemcpyDeviceToHost));
}

}  // namespace bf
