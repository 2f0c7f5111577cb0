// bundler.hip — the bundler: one handle from a frame to its submap's and the global EntryJ list. Restates (paths relative
// to FriedLiver/Source/) Bundler.cpp:91-394 in both roles, OnlineBundler.cpp:106-227 (getCurrentFrame, processInput,
// computeCurrentSiftTransform, prepareLocalSolve's swap) and :280-361 (processGlobal without the solves),
// OnlineBundler.cu:6-71 (computeSiftTransformCU) and CUDAImageUtil.cu:811-847 (gaussFilterIntensityDevice). The detector,
// the matcher with its filters, key fusing and the cache are the existing classes; the kernels here are the two the
// reference has no counterpart of in them.
//
// k_frame_close — ONE wave64, one launch per frame on the bundler's stream, in place of four host round trips
// (filterFrames' count read-back, AddCurrToResidualsCU's two, the transform read-back):
//   1. filterFrames (SIFTImageManager.cpp:551-575): the highest valid prev != cur in [start, n) with a filtered count > 0
//      (ballot per round of 64 images).
//   2. the exclusive scan of the filtered counts over prev ascending (wave.h's scan, rounds of 64 with a carry); the
//      bases go to the matcher's base array, the one k_add_residuals reads.
//   3. AddCurrToResidualsCU (SIFTImageManager.cu:610-687) at the device-resident end of the list, only when a frame
//      matched: pairs in ascending prev, matches in list order, key_point's arithmetic (match_dev.h), with the key-index
//      pairs. A list that would pass its capacity writes nothing and raises the record's overflow flag.
//   4. local role only, getSiftTransformCU_Kernel (OnlineBundler.cu:6-53): prev walks from cur - 1 down to the first
//      filtered count > 0; sift[f] = sift[idxPrevSiftKnown] * TransformsInv[prev]; the integrate transform by the three
//      cases on lastValidCompleteTransform. An invalid frame copies sift[f - 1] and gets -inf
//      (OnlineBundler.cpp:120-124). A 4 x 4 product is plain float32, one lane per element, the k-sum ascending from 0
//      (cuda_SimpleMatrixUtil.h operator*), under the build's -ffp-contract=off. getInverse() in the third case is the
//      RIGID inverse [R^T | -R^T t] with the translation's dot products in double, as k_filter's Tinv: mLib's own
//      float4x4::getInverse is not in the reference tree, and a sift pose is a product of rigid Kabsch transforms.
//   5. the record, into pinned host memory (lane 0 the words, lanes 0..15 the matrices), then a system-scope fence.
// No float atomics, no scratch (the matrices live in LDS, every index into a per-lane array is a constant).
// The retry launch (Bundler::tryRevalidation, Bundler.cpp:306-352) is the same kernel for a key frame in the middle of
// the global store: cur = idx, start = idx + 1, no chain. Every pass walks rounds of 64 images from `start`, lane l of a
// round owns prev = r0 + l in both, nothing below `start` is read (those counts belong to the current key frame's own
// match), and the records it appends are {imgIdx_i = prev > idx, imgIdx_j = idx}.
// k_gauss_intensity — one lane per pixel; window clipped at the borders; sum order m (x) outer, n (y) inner.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "bundler.h"
#include "match_dev.h"
#include "wave.h"

namespace bf {

namespace {

constexpr uint32_t FILT = BF_MAX_MATCHES_FILTERED;
constexpr uint32_t NONE = BF_BUNDLER_NO_FRAME;

struct CloseArgs {
    Matcher::CloseView v;
    uint32_t cur, start, n;
    BFEntryJ* corr;
    uint32_t* keyIdx;
    uint32_t* count;  // the list's device-resident length
    uint32_t cap;
    uint32_t chain;   // 1: local role, step 4 runs
    float* sift;
    float* integ;
    const float* complete;
    uint32_t lastValidComplete, frameAll;
    CloseRecord* rec;
    uint32_t seq;
};

// element `lane` (< 16) of a * b, row-major 4 x 4: s = 0, then += a[r][k] * b[k][c] for k = 0..3
__device__ __forceinline__ float mul_elem(const float* a, const float* b, uint32_t lane) {
    const uint32_t r = (lane >> 2) & 3, c = lane & 3;
    float s = 0.0f;
    s += a[4 * r + 0] * b[0 + c];
    s += a[4 * r + 1] * b[4 + c];
    s += a[4 * r + 2] * b[8 + c];
    s += a[4 * r + 3] * b[12 + c];
    return s;
}

// element `lane` (< 16) of the rigid inverse of t, k_filter's Tinv
__device__ __forceinline__ float rigid_inverse_elem(const float* t, uint32_t lane) {
    const uint32_t r = (lane >> 2) & 3, c = lane & 3;
    if (r == 3) return c == 3 ? 1.0f : 0.0f;
    if (c < 3) return t[4 * c + r];
    return (float)(-((double)t[r] * t[3] + (double)t[4 + r] * t[7] + (double)t[8 + r] * t[11]));
}

__global__ __launch_bounds__(64) void k_frame_close(CloseArgs A) {
    __shared__ uint32_t sWave[1];
    __shared__ float sA[16], sB[16], sC[16], sD[16];
    const uint32_t lane = threadIdx.x;
    const uint32_t listEnd = *A.count;

    // 1 + 2: filterFrames and the scan, a round of 64 images at a time
    uint32_t last = NONE, sum = 0;
    for (uint32_t r0 = A.start; r0 < A.n; r0 += 64) {
        const uint32_t prev = r0 + lane;
        const bool in = prev < A.n && prev != A.cur;
        const uint32_t c = in ? min(A.v.filtCount[prev], FILT) : 0u;
        const uint64_t m = __ballot(in && c > 0 && A.v.table[4 * prev + 2] != 0);
        if (m) last = r0 + 63u - (uint32_t)__builtin_clzll(m);  // rounds ascend: a later one overrides
        uint32_t tot;
        const uint32_t excl = wg_exclusive_scan<1>(c, sWave, tot);
        if (prev < A.n) A.v.base[prev] = sum + excl;
        sum += tot;
        __syncthreads();  // sWave is written again next round
    }
    const bool overflow = last != NONE && (uint64_t)listEnd + sum > A.cap;
    bool valid = last != NONE && !overflow;
    int i = -1;  // step 4's prev: from cur - 1 down to the first filtered count > 0
    if (A.chain && valid) {
        i = (int)A.cur - 1;
        while (i >= (int)A.start && A.v.filtCount[i] == 0) i--;  // wave-uniform; a count below start is another launch's
        if (i < (int)A.start) valid = false;  // cur is not the last image: no chain, as an unmatched frame
    }

    // 3: AddCurrToResidualsCU
    if (valid && sum) {
        float kinv[16];
#pragma unroll
        for (int k = 0; k < 16; k++) kinv[k] = A.v.kinv[k];
        for (uint32_t r0 = A.start; r0 < A.n; r0 += 64) {
            const uint32_t prev = r0 + lane;
            const bool in = prev < A.n && prev != A.cur;
            const uint32_t c = in ? min(A.v.filtCount[prev], FILT) : 0u;
            const uint32_t b = in ? A.v.base[prev] : 0u;  // this lane's own write of the first pass
            uint64_t m = __ballot(c > 0);
            while (m) {  // wave-uniform
                const uint32_t p = (uint32_t)__builtin_ctzll(m);
                m &= m - 1;
                const uint32_t cnt = __shfl(c, (int)p), at = listEnd + __shfl(b, (int)p) + lane, pp = r0 + p;
                if (lane < cnt) {
                    const uint2 ij = A.v.filtIdx[(size_t)pp * FILT + lane];
                    float pi[3], pj[3];
                    key_point(kinv, A.v.keys[ij.x], pi);
                    key_point(kinv, A.v.keys[ij.y], pj);
                    BFEntryJ e;
                    e.imgIdx_i = pp;
                    e.imgIdx_j = A.cur;
                    e.pos_i.x = pi[0]; e.pos_i.y = pi[1]; e.pos_i.z = pi[2];
                    e.pos_j.x = pj[0]; e.pos_j.y = pj[1]; e.pos_j.z = pj[2];
                    A.corr[at] = e;
                    A.keyIdx[2 * (size_t)at] = ij.x;
                    A.keyIdx[2 * (size_t)at + 1] = ij.y;
                }
            }
        }
    }
    const uint32_t added = valid ? sum : 0u;
    if (lane == 0) *A.count = listEnd + added;

    // 4: getSiftTransformCU_Kernel
    float siftE = 0.0f, integE = 0.0f;  // this lane's element of the two matrices (lanes 0..15)
    if (A.chain) {
        const size_t f = (size_t)A.frameAll;
        if (!valid) {
            if (lane < 16) {
                siftE = A.sift[16 * (f - 1) + lane];
                integE = -INFINITY;
            }
        } else {
            const uint32_t known = A.frameAll - (A.cur - (uint32_t)i), lv = A.lastValidComplete;
            if (lane < 16) {
                sA[lane] = A.sift[16 * (size_t)known + lane];
                sB[lane] = A.v.Tinv[16 * (size_t)i + lane];
            }
            __syncthreads();
            if (lane < 16) siftE = mul_elem(sA, sB, lane);
            if (lv == 0) {
                integE = siftE;
            } else if (known < lv) {
                if (lane < 16) sC[lane] = A.complete[16 * (size_t)known + lane];
                __syncthreads();
                if (lane < 16) integE = mul_elem(sC, sB, lane);
            } else {
                if (lane < 16) {
                    sC[lane] = A.sift[16 * (size_t)lv + lane];
                    sD[lane] = A.complete[16 * (size_t)lv + lane];
                }
                __syncthreads();
                const float inv = lane < 16 ? rigid_inverse_elem(sC, lane) : 0.0f;
                __syncthreads();
                if (lane < 16) sC[lane] = inv;  // sift[lv]^-1
                __syncthreads();
                const float off = lane < 16 ? mul_elem(sC, sA, lane) : 0.0f;  // offset
                __syncthreads();
                if (lane < 16) sC[lane] = off;
                __syncthreads();
                const float t1 = lane < 16 ? mul_elem(sD, sC, lane) : 0.0f;  // complete[lv] * offset
                __syncthreads();
                if (lane < 16) sC[lane] = t1;
                __syncthreads();
                if (lane < 16) integE = mul_elem(sC, sB, lane);
            }
        }
        if (lane < 16) {
            A.sift[16 * f + lane] = siftE;
            A.integ[16 * f + lane] = integE;
        }
    }

    // 5: the record
    if (lane < 16) {
        A.rec->sift[lane] = siftE;
        A.rec->integ[lane] = integE;
    }
    if (lane == 0) {
        A.rec->valid = valid ? 1u : 0u;
        A.rec->lastMatched = valid ? last : NONE;
        A.rec->added = valid ? added : 0u;
        A.rec->total = listEnd + (valid ? added : 0u);
        A.rec->flags = overflow ? Bundler::kOverflow : 0u;
        A.rec->seq = A.seq;
        A.rec->cur = A.cur;
        A.rec->start = A.start;
    }
    __threadfence_system();
}

// gaussFilterIntensityDevice (CUDAImageUtil.cu:811-847)
__global__ __launch_bounds__(256) void k_gauss_intensity(const float* in, float* out, int w, int h, GaussTable g) {
    const int x = (int)(blockIdx.x * 16 + (threadIdx.x & 15)), y = (int)(blockIdx.y * 16 + (threadIdx.x >> 4));
    if (x >= w || y >= h) return;
    const int r = g.radius, side = 2 * r + 1;
    float sum = 0.0f, sumWeight = 0.0f;
    for (int m = x - r; m <= x + r; m++)
        for (int n = y - r; n <= y + r; n++)
            if (m >= 0 && n >= 0 && m < w && n < h) {
                const float weight = g.w[(n - y + r) * side + (m - x + r)];
                sumWeight += weight;
                sum += weight * in[(size_t)n * w + m];
            }
    out[(size_t)y * w + x] = sumWeight > 0.0f ? sum / sumWeight : in[(size_t)y * w + x];
}

CacheConfig cache_config(const BFCacheOptions& o, uint32_t maxFrames) {
    CacheConfig c{};
    c.inputWidth = o.inputWidth; c.inputHeight = o.inputHeight;
    c.width = o.width; c.height = o.height; c.maxFrames = maxFrames;
    std::memcpy(c.inputIntrinsics, o.inputIntrinsics, 64);
    c.colorSigma = o.colorSigma; c.depthSigmaD = o.depthSigmaD; c.depthSigmaR = o.depthSigmaR;
    return c;
}

}  // namespace

GaussTable intensity_gauss_table(float sigmaD) {
    GaussTable g{};
    g.radius = (int)std::ceil(2.0 * (double)sigmaD);
    BF_REQUIRE(g.radius >= 1 && g.radius <= 7, BF_ERR_ARG, "intensitySigmaD out of range (0 < sigma <= 3.5)");
    const int side = 2 * g.radius + 1;
    for (int dy = -g.radius; dy <= g.radius; dy++)
        for (int dx = -g.radius; dx <= g.radius; dx++) {
            const float arg = -((float)(dx * dx + dy * dy) / (2.0f * sigmaD * sigmaD));
            g.w[(dy + g.radius) * side + (dx + g.radius)] = (float)std::exp((double)arg);
        }
    return g;
}

BundlerConfig make_bundler_config(const BFBundlerOptions* o) {
    BF_REQUIRE(o != nullptr, BF_ERR_ARG, "null bundler options");
    BF_REQUIRE(o->submapSize >= 1, BF_ERR_ARG, "bundler options: submapSize is 0");
    BF_REQUIRE(o->maxKeyframes >= 2, BF_ERR_ARG, "bundler options: maxKeyframes below 2");
    BF_REQUIRE((uint64_t)o->submapSize * o->maxKeyframes <= (1ull << 28) && o->submapSize < (1u << 20), BF_ERR_ARG,
               "bundler options: submapSize * maxKeyframes above 2^28");
    BundlerConfig c;
    c.submapSize = o->submapSize;
    c.maxKeyframes = o->maxKeyframes;
    const uint64_t S = o->submapSize, K = o->maxKeyframes;
    const uint64_t localCorr = o->maxLocalCorr ? o->maxLocalCorr : FILT * (S + 1) * S / 2;
    const uint64_t globalCorr = o->maxGlobalCorr ? o->maxGlobalCorr : FILT * K * (K - 1) / 2;
    BF_REQUIRE(localCorr <= (1ull << 28) && globalCorr <= (1ull << 28), BF_ERR_ARG, "bundler options: a list capacity above 2^28");
    c.maxLocalCorr = (uint32_t)localCorr;
    c.maxGlobalCorr = (uint32_t)globalCorr;
    c.sift = make_sift_config(&o->sift);
    BF_REQUIRE(o->local.maxKeysPerImage == 0 || c.sift.maxKeys <= o->local.maxKeysPerImage, BF_ERR_ARG,
               "bundler options: the detector's maxKeys above local.maxKeysPerImage");
    BFMatcherOptions ml = o->local, mg = o->global;
    BF_REQUIRE(ml.maxImages == 0 || ml.maxImages == o->submapSize + 1, BF_ERR_ARG, "bundler options: local.maxImages is submapSize + 1");
    BF_REQUIRE(mg.maxImages == 0 || mg.maxImages == o->maxKeyframes, BF_ERR_ARG, "bundler options: global.maxImages is maxKeyframes");
    BF_REQUIRE(ml.fuseMaxCorr == 0 || ml.fuseMaxCorr == c.maxLocalCorr, BF_ERR_ARG, "bundler options: local.fuseMaxCorr is maxLocalCorr");
    BF_REQUIRE(mg.fuseMaxCorr == 0, BF_ERR_ARG, "bundler options: global.fuseMaxCorr is 0 (nothing is fused from the global store)");
    ml.maxImages = o->submapSize + 1;
    mg.maxImages = o->maxKeyframes;
    ml.fuseMaxCorr = c.maxLocalCorr;
    c.local = make_matcher_config(&ml);
    c.global = make_matcher_config(&mg);
    c.verify = make_match_verify_config(&o->verify);
    BF_REQUIRE(o->cache.maxFrames == 0 || o->cache.maxFrames == o->submapSize + 1, BF_ERR_ARG,
               "bundler options: cache.maxFrames is set per cache (0 or submapSize + 1)");
    c.cache = cache_config(o->cache, o->submapSize + 1);
    check_cache_config(c.cache);
    for (int k = 0; k < 16; k++) BF_REQUIRE(std::isfinite(c.cache.inputIntrinsics[k]), BF_ERR_ARG, "bundler options: non-finite cache intrinsics");
    BF_REQUIRE(c.cache.inputWidth == c.sift.depthWidth && c.cache.inputHeight == c.sift.depthHeight, BF_ERR_ARG,
               "bundler options: the cache's input size is the detector's depth size");
    check_dense_frame_shape(c.cache.width, c.cache.height, c.cache.inputIntrinsics);
    for (int k = 0; k < 16; k++) {
        BF_REQUIRE(std::isfinite(o->colorIntrinsics[k]), BF_ERR_ARG, "bundler options: non-finite colorIntrinsics");
        c.K[k] = o->colorIntrinsics[k];
    }
    c.filterIntensity = o->filterIntensity != 0;
    c.intensitySigmaD = o->intensitySigmaD;
    if (c.filterIntensity) {
        BF_REQUIRE(std::isfinite(o->intensitySigmaD) && o->intensitySigmaD > 0.0f, BF_ERR_ARG,
                   "bundler options: filterIntensity with a non-positive or non-finite intensitySigmaD");
        (void)intensity_gauss_table(o->intensitySigmaD);
    }
    return c;
}

Bundler::Bundler(const BundlerConfig& cfg) : cfg_(cfg) {
    BF_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    try {
        const uint32_t S = cfg.submapSize, frames = S * cfg.maxKeyframes;
        sift_.reset(new Sift(cfg.sift, stream_));
        CacheConfig cl = cfg.cache, cg = cfg.cache;
        cl.maxFrames = S + 1;
        cg.maxFrames = cfg.maxKeyframes;
        for (int s = 0; s < 2; s++) {
            loc_[s].reset(new Matcher(cfg.local, stream_));
            cacheLoc_[s].reset(new Cache(cl, stream_));
        }
        glob_.reset(new Matcher(cfg.global, stream_));
        cacheGlob_.reset(new Cache(cg, stream_));
        cap_[0] = cap_[1] = cfg.maxLocalCorr;
        cap_[2] = cfg.maxGlobalCorr;
        for (int l = 0; l < 3; l++) {
            corr_[l].alloc(cap_[l] ? cap_[l] : 1);
            keyIdx_[l].alloc(2 * (size_t)(cap_[l] ? cap_[l] : 1));
        }
        counts_.alloc(3);
        for (int l = 0; l < 3; l++) {
            Cache& c = l < 2 ? *cacheLoc_[l] : *cacheGlob_;
            const uint32_t n = c.config().maxFrames;
            std::vector<BFCachedFrame> tab(n);
            for (uint32_t i = 0; i < n; i++) tab[i] = c.frame(i);
            frameTab_[l].alloc(n);
            BF_HIP(hipMemcpy(frameTab_[l].p, tab.data(), n * sizeof(BFCachedFrame), hipMemcpyHostToDevice));
            if (l < 2) hostFrames_[l] = tab;
        }
        for (int s = 0; s < 2; s++) dValid_[s].alloc(S + 1);
        siftTraj_.alloc(16 * (size_t)frames);
        integ_.alloc(16 * (size_t)frames);
        complete_.alloc(16 * (size_t)frames);
        const size_t px = (size_t)cfg.sift.width * cfg.sift.height;
        intensity_.alloc(px);
        if (cfg.filterIntensity) {
            intensityTmp_.alloc(px);
            gauss_ = intensity_gauss_table(cfg.intensitySigmaD);
        }
        // the record, then the two sets' valid flags (int32 [S + 1] each), in one pinned block
        BF_HIP(hipHostMalloc((void**)&rec_, sizeof(CloseRecord) + 2 * (size_t)(S + 1) * sizeof(int32_t), hipHostMallocCoherent));
        reset();
    } catch (...) {
        if (rec_) (void)hipHostFree(rec_);
        sift_.reset();
        for (int s = 0; s < 2; s++) {
            loc_[s].reset();
            cacheLoc_[s].reset();
        }
        glob_.reset();
        cacheGlob_.reset();
        (void)hipStreamDestroy(stream_);
        throw;
    }
}

Bundler::~Bundler() {
    (void)hipStreamSynchronize(stream_);
    if (rec_) (void)hipHostFree(rec_);
    sift_.reset();
    for (int s = 0; s < 2; s++) {
        loc_[s].reset();
        cacheLoc_[s].reset();
    }
    glob_.reset();
    cacheGlob_.reset();
    (void)hipStreamDestroy(stream_);
}

void Bundler::wait() {
    BF_HIP(hipStreamSynchronize(stream_));
    stats_.hostWaits++;
}

void Bundler::reset() {
    BF_HIP(hipStreamSynchronize(stream_));
    for (int s = 0; s < 2; s++) {
        loc_[s]->reset();
        cacheLoc_[s]->reset();
        free_[s] = true;
    }
    glob_->reset();
    cacheGlob_->reset();
    BF_HIP(hipMemsetAsync(counts_.p, 0, 3 * sizeof(uint32_t), stream_));
    BF_HIP(hipMemsetAsync(siftTraj_.p, 0, siftTraj_.bytes(), stream_));
    BF_HIP(hipMemsetAsync(integ_.p, 0, integ_.bytes(), stream_));
    BF_HIP(hipMemsetAsync(complete_.p, 0, complete_.bytes(), stream_));
    static const float id[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::memset(rec_, 0, sizeof(CloseRecord) + 2 * (size_t)(cfg_.submapSize + 1) * sizeof(int32_t));
    std::memcpy(rec_->sift, id, 64);  // staging for the two identities (OnlineBundler.cpp:66-71)
    BF_HIP(hipMemcpyAsync(siftTraj_.p, rec_->sift, 64, hipMemcpyHostToDevice, stream_));
    BF_HIP(hipMemcpyAsync(integ_.p, rec_->sift, 64, hipMemcpyHostToDevice, stream_));
    BF_HIP(hipStreamSynchronize(stream_));
    for (int s = 0; s < 2; s++) loc_[s]->streamDrained();
    glob_->streamDrained();
    total_[0] = total_[1] = total_[2] = 0;
    cur_ = 0;
    frame_ = 0;
    ended_ = false;
    lastValidComplete_ = 0;
    lastIntensity_ = nullptr;
    closed_ = -1;
    released_ = true;
    canReclose_ = false;
    prefix_.clear();
    retryList_.clear();  // retry_ itself is a setting and stays
    continueRetry_ = 0;
    keyframeValid_.clear();
    beginRetryReport();
    stats_ = BFBundlerStats{};
}

void Bundler::closeFrame(Matcher& m, uint32_t list, uint32_t cur, uint32_t start, bool chain, uint32_t frameAll) {
    BF_REQUIRE(!chain || start == 0, BF_ERR_INTERNAL, "the sift chain walks from frame 0: a local close starts at 0");
    CloseArgs A{};
    A.v = m.prepareClose(cur, start);
    A.cur = cur;
    A.start = start;  // 0 for a current frame, cur + 1 for a retry frame (Bundler.cpp:112)
    A.n = m.numImages();
    A.corr = corr_[list].p;
    A.keyIdx = keyIdx_[list].p;
    A.count = counts_.p + list;
    A.cap = cap_[list];
    A.chain = chain ? 1u : 0u;
    A.sift = siftTraj_.p;
    A.integ = integ_.p;
    A.complete = complete_.p;
    A.lastValidComplete = lastValidComplete_;
    A.frameAll = frameAll;
    A.rec = rec_;
    A.seq = ++seq_;
    k_frame_close<<<1, 64, 0, stream_>>>(A);
    BF_LAUNCH_CHECK();
    wait();
    m.streamDrained();
    BF_REQUIRE(rec_->seq == seq_, BF_ERR_INTERNAL, "the closing launch left no record");
    m.applyClose(cur, rec_->valid != 0);
    total_[list] = rec_->total;
}

void Bundler::fillFrame(BFBundlerFrame* out, uint32_t lf, bool closed) const {
    out->localFrame = lf;
    out->valid = rec_->valid;
    out->lastMatchedLocal = rec_->lastMatched;
    out->residualsAdded = rec_->added;
    out->residualsTotal = rec_->total;
    out->submapClosed = closed ? 1u : 0u;
    std::memcpy(out->siftPose, rec_->sift, 64);
    std::memcpy(out->integrateTransform, rec_->integ, 64);
}

void Bundler::processFrame(const uint8_t* color, uint32_t cw, uint32_t ch, const float* depthFilt, const float* depthRaw,
                           BFBundlerFrame* out) {
    BF_REQUIRE(color && depthFilt && depthRaw && out, BF_ERR_ARG, "process_frame: null argument");
    BF_REQUIRE(cw >= 2 && ch >= 2 && cw <= 16384 && ch <= 16384, BF_ERR_ARG, "process_frame: colour size");
    const uint32_t S = cfg_.submapSize, f = frame_;
    BF_REQUIRE(!ended_, BF_ERR_STATE, "process_frame: the sequence is over (end_sequence); reset starts a new one");
    BF_REQUIRE(f < S * cfg_.maxKeyframes, BF_ERR_CAPACITY, "process_frame: submapSize * maxKeyframes frames have been processed");
    const bool closes = f > 0 && f % S == 0;  // isLastLocalFrame
    BF_REQUIRE(!closes || free_[1 - cur_], BF_ERR_STATE,
               "process_frame: this frame closes a submap and the previous one waits for fuse_submap / invalid_submap");
    Matcher& M = *loc_[cur_];
    Cache& C = *cacheLoc_[cur_];
    canReclose_ = false;

    // getCurrentFrame + detectFeatures + storeCachedFrame
    sift_->intensity(color, cw, ch, intensity_.p);
    const float* input = intensity_.p;
    if (cfg_.filterIntensity) {
        const dim3 grid(div_up(cfg_.sift.width, 16), div_up(cfg_.sift.height, 16));
        k_gauss_intensity<<<grid, 256, 0, stream_>>>(intensity_.p, intensityTmp_.p, (int)cfg_.sift.width, (int)cfg_.sift.height, gauss_);
        BF_LAUNCH_CHECK();
        input = intensityTmp_.p;
    }
    lastIntensity_ = input;
    sift_->detect(input, depthFilt);
    C.storeFrame(depthRaw, color, cw, ch);
    stats_.frames++;
    const BFSiftKeyPoint* keys = nullptr;
    const uint8_t* descs = nullptr;
    uint32_t n = 0, flags = 0;
    sift_->result(&keys, &descs, &n, &flags);  // waits: the store's host table needs the count
    stats_.hostWaits++;
    M.streamDrained();
    const uint32_t lf = M.addImage(keys, descs, n);
    free_[cur_] = false;
    frame_ = f + 1;

    std::memset(out, 0, sizeof(*out));
    out->frame = f;
    out->submap = f == 0 ? 0 : (f - 1) / S;
    out->numKeys = n;
    out->siftFlags = flags;
    bool overflow = false;
    if (lf > 0) {
        // matchAndFilter (Bundler.cpp:103-221) up to filterFrames, then the closing launch
        M.match(lf, 0);
        M.filter(lf, 0);
        M.filterSurfaceArea(lf, 0, cfg_.verify);
        M.filterDenseVerify(lf, 0, frameTab_[cur_].p, S + 1, C.config().width, C.config().height, C.intrinsics(), cfg_.verify);
        lastBefore_ = total_[cur_];
        closeFrame(M, cur_, lf, 0, true, f);
        overflow = (rec_->flags & kOverflow) != 0;
        fillFrame(out, lf, closes);
    } else {  // the very first frame: both trajectories start at the identity (OnlineBundler.cpp:66-74)
        out->localFrame = 0;
        out->valid = 1;
        out->lastMatchedLocal = kNone;
        out->submapClosed = 0;
        for (int k = 0; k < 16; k += 5) out->siftPose[k] = out->integrateTransform[k] = 1.0f;
    }

    if (closes) {  // copyFrame into the other set, prepareLocalSolve's bookkeeping and the swap
        const uint32_t o = 1 - cur_;
        loc_[o]->copyImageFrom(M, lf);
        cacheLoc_[o]->copyFrameFrom(C, lf);
        free_[o] = false;
        recordClosed(lf + 1, out->submap);
        cur_ = o;
    } else {
        canReclose_ = lf > 0;
    }
    lastFrame_ = *out;
    BF_REQUIRE(!overflow, BF_ERR_CAPACITY, "process_frame: the frame's residuals would pass maxLocalCorr; none was appended");
}

void Bundler::recordClosed(uint32_t numFrames, uint32_t submap) {
    const uint32_t S = cfg_.submapSize;
    const Matcher& M = *loc_[cur_];
    closed_ = (int)cur_;
    released_ = false;
    closedFrames_ = numFrames;
    closedSubmap_ = submap;
    closedCorr_ = total_[cur_];
    closedValidImages_.resize(closedFrames_);
    closedValid_ = false;
    int32_t* hv = reinterpret_cast<int32_t*>(rec_ + 1) + (size_t)cur_ * (S + 1);
    for (uint32_t i = 0; i < closedFrames_; i++) {
        hv[i] = closedValidImages_[i] = M.valid(i);
        if (i > 0 && M.valid(i)) closedValid_ = true;  // Bundler::isValid
    }
    BF_HIP(hipMemcpyAsync(dValid_[cur_].p, hv, closedFrames_ * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
}

// processInput past the end (OnlineBundler.cpp:171-174): no local solve pending and the last frame not a boundary frame
// -> prepareLocalSolve(curFrame, true) (:134-165). Its "only the overlap frame" branch (:138-144) cannot be reached from
// there: a set of one image follows a boundary frame (or is frame 0 alone), which :171-173 exclude.
void Bundler::endSequence(BFBundlerEnd* out) {
    BF_REQUIRE(out != nullptr, BF_ERR_ARG, "end_sequence: null output");
    BF_REQUIRE(frame_ > 0, BF_ERR_STATE, "end_sequence: no frame has been processed");
    std::memset(out, 0, sizeof(*out));
    if (ended_) return;
    const uint32_t S = cfg_.submapSize, last = frame_ - 1, n = loc_[cur_]->numImages();
    const bool boundary = last > 0 && last % S == 0;  // isLastLocalFrame: that frame closed its submap itself
    if (n >= 2 && !boundary) {
        BF_REQUIRE(closed_ < 0 || released_, BF_ERR_STATE,
                   "end_sequence: this call closes a submap and the previous one waits for fuse_submap / invalid_submap");
        recordClosed(n, last / S);
        out->closed = 1;
        out->submap = closedSubmap_;
        out->numFrames = closedFrames_;
        out->numCorr = closedCorr_;
        out->isValid = closedValid_ ? 1u : 0u;
    }
    canReclose_ = false;
    ended_ = true;
}

void Bundler::debugReclose(BFBundlerFrame* out) {
    BF_REQUIRE(out != nullptr, BF_ERR_ARG, "debug_reclose: null output");
    BF_REQUIRE(canReclose_, BF_ERR_STATE, "debug_reclose: not right after a process_frame of a local frame > 0 inside a submap");
    Matcher& M = *loc_[cur_];
    BF_HIP(hipStreamSynchronize(stream_));
    rec_->total = lastBefore_;  // staging: the list's length before the frame
    BF_HIP(hipMemcpyAsync(counts_.p + cur_, &rec_->total, 4, hipMemcpyHostToDevice, stream_));
    BF_HIP(hipStreamSynchronize(stream_));
    total_[cur_] = lastBefore_;
    closeFrame(M, cur_, lastFrame_.localFrame, 0, true, lastFrame_.frame);
    const bool overflow = (rec_->flags & kOverflow) != 0;
    *out = lastFrame_;
    fillFrame(out, lastFrame_.localFrame, false);
    lastFrame_ = *out;
    BF_REQUIRE(!overflow, BF_ERR_CAPACITY, "debug_reclose: the frame's residuals would pass maxLocalCorr; none was appended");
}

void Bundler::setCompleteTrajectory(const float* T, uint32_t n, uint32_t lastValid) {
    BF_REQUIRE(n <= cfg_.submapSize * cfg_.maxKeyframes, BF_ERR_ARG, "set_complete_trajectory: n above submapSize * maxKeyframes");
    BF_REQUIRE(n == 0 || T != nullptr, BF_ERR_ARG, "set_complete_trajectory: null trajectory");
    BF_REQUIRE(lastValid < (n ? n : 1u), BF_ERR_ARG, "set_complete_trajectory: lastValidCompleteTransform >= n");
    if (n) BF_HIP(hipMemcpyAsync(complete_.p, T, 64 * (size_t)n, hipMemcpyDeviceToDevice, stream_));
    lastValidComplete_ = lastValid;
}

void Bundler::submap(BFBundlerSubmap* out) const {
    BF_REQUIRE(out != nullptr, BF_ERR_ARG, "submap: null output");
    BF_REQUIRE(closed_ >= 0, BF_ERR_STATE, "submap: no submap has closed");
    std::memset(out, 0, sizeof(*out));
    out->d_corr = corr_[closed_].p;
    out->d_keyIdx = keyIdx_[closed_].p;
    out->d_validImages = dValid_[closed_].p;
    out->validImages = closedValidImages_.data();
    out->cacheFrames = hostFrames_[closed_].data();
    out->d_cacheFrames = frameTab_[closed_].p;
    out->numCorr = closedCorr_;
    out->numFrames = closedFrames_;
    out->submap = closedSubmap_;
    out->isValid = closedValid_ ? 1u : 0u;
    out->released = released_ ? 1u : 0u;
}

void Bundler::fuseSubmap(const float* localTransforms, BFBundlerKeyframe* out) {
    BF_REQUIRE(out != nullptr, BF_ERR_ARG, "fuse_submap: null output");
    BF_REQUIRE(closed_ >= 0 && !released_, BF_ERR_STATE, "fuse_submap: no closed submap waits");
    BF_REQUIRE(localTransforms != nullptr, BF_ERR_ARG, "fuse_submap: null local transforms");
    BF_REQUIRE(cacheGlob_->numFrames() < cfg_.maxKeyframes, BF_ERR_CAPACITY, "fuse_submap: the global store is full");
    Matcher& L = *loc_[closed_];
    uint32_t idx = 0, nk = 0, nt = 0;
    // Bundler::fuseToGlobal (Bundler.cpp:388-394); returns after the read-back of its counts
    L.fuseToGlobal(*glob_, corr_[closed_].p, keyIdx_[closed_].p, closedCorr_, localTransforms, cfg_.K, &idx, &nk, &nt);
    stats_.hostWaits++;
    glob_->streamDrained();
    cacheGlob_->copyFrameFrom(*cacheLoc_[closed_], 0);
    stats_.keyframes++;
    // m_localTrajectoriesValid[curGlobalFrame] (OnlineBundler.cpp:321)
    keyframeValid_.resize(idx + 1);
    keyframeValid_[idx].assign(closedValidImages_.begin(), closedValidImages_.begin() + std::min(cfg_.submapSize, closedFrames_));
    beginRetryReport();
    std::memset(out, 0, sizeof(*out));
    out->keyframe = idx;
    out->numKeys = nk;
    out->numTracks = nt;
    out->valid = 1;
    out->lastMatchedGlobal = kNone;
    out->residualsTotal = total_[2];
    bool overflow = false, retryOverflow = false;
    if (glob_->numImages() > 1) {
        matchGlobal(idx, 0);
        closeFrame(*glob_, 2, idx, 0, false, 0);
        overflow = (rec_->flags & kOverflow) != 0;
        out->valid = rec_->valid;
        out->lastMatchedGlobal = rec_->lastMatched;
        out->residualsAdded = rec_->added;
        out->residualsTotal = rec_->total;
        out->globalTrackingLost = rec_->valid ? 0u : 1u;
        if (retry_) {  // Bundler.cpp:223-237
            if (rec_->valid) {
                addSeeds(idx, rec_->lastMatched);
                retryOverflow = tryRevalidation(false);  // one revalidation per key frame
            } else if (nk > 0) {
                retryList_.push_front(idx);
            }
        }
    }
    prefix_.resize(idx + 1, prefix_.empty() ? 0u : prefix_.back());
    prefix_[idx] = total_[2];
    endRetryReport();
    // done with local data (OnlineBundler.cpp:324)
    L.reset();
    cacheLoc_[closed_]->reset();
    BF_HIP(hipMemsetAsync(counts_.p + closed_, 0, sizeof(uint32_t), stream_));
    total_[closed_] = 0;
    free_[closed_] = true;
    released_ = true;
    BF_REQUIRE(!overflow, BF_ERR_CAPACITY, "fuse_submap: the key frame's residuals would pass maxGlobalCorr; none was appended");
    BF_REQUIRE(!retryOverflow, BF_ERR_CAPACITY, "fuse_submap: the retry candidate's residuals would pass maxGlobalCorr; none was appended");
}

// ---- retry: Bundler::tryRevalidation (Bundler.cpp:306-352), the list of SIFTImageManager.h:263-271 ------------------------
void Bundler::matchGlobal(uint32_t cur, uint32_t start) {
    Cache& G = *cacheGlob_;
    glob_->match(cur, start);
    glob_->filter(cur, start);
    glob_->filterSurfaceArea(cur, start, cfg_.verify);
    glob_->filterDenseVerify(cur, start, frameTab_[2].p, cfg_.maxKeyframes, G.config().width, G.config().height, G.intrinsics(), cfg_.verify);
}

void Bundler::beginRetryReport() {
    last_ = BFBundlerRetry{};
    last_.candidate = last_.revalidated = last_.lastMatchedGlobal = kNone;
}

void Bundler::endRetryReport() {
    last_.residualsTotal = total_[2];
    last_.listLength = (uint32_t)retryList_.size();
    last_.finished = continueRetry_ < 0 ? 1u : 0u;
}

void Bundler::pushSeed(uint32_t to, uint32_t from) {
    if (to >= cfg_.maxKeyframes || last_.numSeeds >= 5) return;  // d_trajectory has maxKeyframes poses
    last_.seeds[last_.numSeeds][0] = to;
    last_.seeds[last_.numSeeds][1] = from;
    last_.numSeeds++;
}

void Bundler::addSeeds(uint32_t cur, uint32_t lastMatched) {
    if (lastMatched + 1 == cur) return;  // re-initialize to a better location based off of the last match
    pushSeed(cur, lastMatched);
    pushSeed(cur + 1, lastMatched);
}

bool Bundler::revalidate(uint32_t idx, bool filters) {
    const uint32_t n = glob_->numImages();
    // an entry equal to the last key frame is a current frame: matched against the earlier images, once
    const uint32_t start = idx + 1 == n ? 0 : idx + 1;
    if (filters) matchGlobal(idx, start);
    closeFrame(*glob_, 2, idx, start, false, 0);
    last_.attempted = 1;
    last_.candidate = idx;
    if (rec_->valid) {
        last_.revalidated = idx;
        last_.lastMatchedGlobal = rec_->lastMatched;
        last_.residualsAdded = rec_->added;
        addSeeds(idx, rec_->lastMatched);
        pushSeed(idx, rec_->lastMatched);  // Bundler.cpp:330
    }
    return (rec_->flags & kOverflow) != 0;
}

bool Bundler::tryRevalidation(bool scanDone) {
    if (continueRetry_ < 0 || retryList_.empty()) return false;  // nothing to do
    const uint32_t idx = retryList_.front();
    retryList_.pop_front();
    if (scanDone) {
        if (continueRetry_ == 0) {
            continueRetry_ = idx;
        } else if (continueRetry_ == (int64_t)idx) {
            continueRetry_ = -1;  // looped around again: nothing more to do
            return false;
        }
    }
    const bool overflow = revalidate(idx, true);
    if (last_.revalidated != idx) retryList_.push_front(idx);
    return overflow;
}

void Bundler::setRetry(bool on) {
    BF_REQUIRE(glob_->numImages() == 0, BF_ERR_STATE, "set_retry: a key frame exists");
    retry_ = on;
}

void Bundler::retry(BFBundlerRetry* out) {
    BF_REQUIRE(out != nullptr, BF_ERR_ARG, "retry: null output");
    BF_REQUIRE(retry_, BF_ERR_STATE, "retry: retry is off (bf_retry_enable)");
    BF_REQUIRE(closed_ < 0 || released_, BF_ERR_STATE, "retry: a closed submap waits for fuse_submap / invalid_submap");
    beginRetryReport();
    const bool overflow = tryRevalidation(true);
    if (!prefix_.empty()) prefix_.back() = total_[2];
    endRetryReport();
    *out = last_;
    BF_REQUIRE(!overflow, BF_ERR_CAPACITY, "retry: the candidate's residuals would pass maxGlobalCorr; none was appended");
}

void Bundler::lastRetry(BFBundlerRetry* out) const {
    BF_REQUIRE(out != nullptr, BF_ERR_ARG, "last_retry: null output");
    *out = last_;
}

void Bundler::retryList(uint32_t* out, uint32_t cap, uint32_t* n) const {
    BF_REQUIRE(n != nullptr && (out != nullptr || cap == 0), BF_ERR_ARG, "retry_list: null output");
    *n = (uint32_t)retryList_.size();
    for (uint32_t k = 0; k < cap && k < retryList_.size(); k++) out[k] = retryList_[k];
}

void Bundler::applySeeds(float* dT, uint32_t numPoses) {
    BF_REQUIRE(dT != nullptr, BF_ERR_ARG, "apply_seeds: null trajectory");
    for (uint32_t k = 0; k < last_.numSeeds; k++)
        BF_REQUIRE(last_.seeds[k][0] < numPoses && last_.seeds[k][1] < numPoses, BF_ERR_ARG, "apply_seeds: a seed names a pose >= numPoses");
    for (uint32_t k = 0; k < last_.numSeeds; k++)
        BF_HIP(hipMemcpyAsync(dT + 16 * (size_t)last_.seeds[k][0], dT + 16 * (size_t)last_.seeds[k][1], 64, hipMemcpyDeviceToDevice, stream_));
}

void Bundler::keyframeFrames(uint32_t k, int32_t* valid, uint32_t* n) const {
    BF_REQUIRE(valid != nullptr && n != nullptr, BF_ERR_ARG, "keyframe_frames: null output");
    BF_REQUIRE(k < keyframeValid_.size(), BF_ERR_ARG, "keyframe_frames: k >= the number of key frames");
    *n = (uint32_t)keyframeValid_[k].size();
    for (uint32_t i = 0; i < *n; i++) valid[i] = keyframeValid_[k][i];
}

void Bundler::debugRetryClose(uint32_t idx, BFBundlerRetry* out) {
    BF_REQUIRE(out != nullptr, BF_ERR_ARG, "debug_retry_close: null output");
    const uint32_t n = glob_->numImages();
    BF_REQUIRE(idx < n, BF_ERR_ARG, "debug_retry_close: idx >= the number of key frames");
    BF_REQUIRE(retry_ && (closed_ < 0 || released_) && idx >= 1 && idx + 1 < n && glob_->valid(idx) == 0, BF_ERR_STATE,
               "debug_retry_close: retry on, no closed submap waiting, and idx an invalid key frame in [1, n - 1)");
    beginRetryReport();
    const bool overflow = revalidate(idx, false);
    if (last_.revalidated == idx)
        for (auto it = retryList_.begin(); it != retryList_.end(); ++it)
            if (*it == idx) {
                retryList_.erase(it);
                break;
            }
    prefix_.back() = total_[2];
    endRetryReport();
    *out = last_;
    BF_REQUIRE(!overflow, BF_ERR_CAPACITY, "debug_retry_close: the candidate's residuals would pass maxGlobalCorr; none was appended");
}

void Bundler::invalidSubmap() {
    BF_REQUIRE(closed_ >= 0 && !released_, BF_ERR_STATE, "invalid_submap: no closed submap waits");
    BF_REQUIRE(cacheGlob_->numFrames() < cfg_.maxKeyframes, BF_ERR_CAPACITY, "invalid_submap: the global store is full");
    // Bundler::addInvalidFrame (Bundler.cpp:362-368)
    cacheGlob_->increment();
    const uint32_t idx = glob_->addImage(nullptr, nullptr, 0);
    if (idx > 0) glob_->setValid(idx, 0);
    stats_.keyframes++;
    keyframeValid_.resize(idx + 1);  // no frames: the INVALIDATE branch records none (OnlineBundler.cpp:351-360)
    prefix_.resize(idx + 1, prefix_.empty() ? 0u : prefix_.back());
    prefix_[idx] = total_[2];
    loc_[closed_]->reset();
    cacheLoc_[closed_]->reset();
    BF_HIP(hipMemsetAsync(counts_.p + closed_, 0, sizeof(uint32_t), stream_));
    total_[closed_] = 0;
    free_[closed_] = true;
    released_ = true;
}

void Bundler::global(BFEntryJ** corr, const uint32_t** keyIdx, uint32_t* n, const uint32_t** prefix, uint32_t* numKeyframes) {
    // a key frame is only paired with earlier ones, so prefix[] ascends and ends at the list's length
    for (size_t k = 1; k < prefix_.size(); k++) BF_REQUIRE(prefix_[k - 1] <= prefix_[k], BF_ERR_INTERNAL, "global: the list is not ordered by max(i, j)");
    BF_REQUIRE(prefix_.empty() || prefix_.back() == total_[2], BF_ERR_INTERNAL, "global: prefix[] does not end at the list's length");
    if (corr) *corr = corr_[2].p;
    if (keyIdx) *keyIdx = keyIdx_[2].p;
    if (n) *n = total_[2];
    if (prefix) *prefix = prefix_.data();
    if (numKeyframes) *numKeyframes = (uint32_t)prefix_.size();
}

}  // namespace bf
