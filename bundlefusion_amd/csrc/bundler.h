// bundler.h — the bundler (bundler.hip): Bundler (Bundler.cpp:91-394) as the local and the global bundler, with the input
// half of OnlineBundler that drives it (getCurrentFrame, processInput up to prepareLocalSolve, processGlobal without the
// solves: OnlineBundler.cpp:106-227, 280-361). It owns one Sift, two local Matchers (m_local / m_optLocal) and one
// global Matcher, a Cache per matcher, and the device lists and trajectories; it adds two kernels of its own
// (k_frame_close, k_gauss_intensity) and copies none of the stages'. One stream, no device allocation after the ctor.
//
// Host wait budgets (counted in BFBundlerStats.hostWaits): processFrame <= 2 (the detector's key count; the closing
// launch's record), fuseSubmap <= 2 (the fuse's count read-back; the record) and <= 3 with a retry attempt (the
// candidate's record), retry <= 1, invalidSubmap 0, endSequence 0 (the valid flags' upload is stream-ordered; whoever reads
// the closed submap on another stream waits, as after a boundary frame).
//
// Retry (Bundler::tryRevalidation, Bundler.cpp:306-352; SIFTImageManager.h:263-271; off unless setRetry): a key frame with
// keys that matched no earlier one waits on a host deque, front in / front out; a key frame that matched pops one
// candidate idx and matches it against the LATER images (cur = idx, start = idx + 1), one more closing launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <deque>
#include <memory>
#include <vector>

#include "../../include/bf/bf.h"
#include "bf_runtime.h"
#include "cache.h"
#include "frames.h"
#include "match.h"
#include "sift.h"

namespace bf {

struct BundlerConfig {
    SiftConfig sift;
    MatcherConfig local, global;
    MatchVerifyConfig verify;
    CacheConfig cache;  // maxFrames is set per cache
    uint32_t submapSize = 0, maxKeyframes = 0, maxLocalCorr = 0, maxGlobalCorr = 0;
    float K[16] = {};
    bool filterIntensity = false;
    float intensitySigmaD = 0.0f;
};

// BFBundlerOptions -> config with the defaults filled in; every check of every stage; throws BF_ERR_ARG (host only)
BundlerConfig make_bundler_config(const BFBundlerOptions* o);

// gaussD (CUDAImageUtil.cu:20-23) per integer offset for k_gauss_intensity: exp taken in double and rounded to float, so
// the table does not depend on which float routine a C library ships (host only)
GaussTable intensity_gauss_table(float sigmaD);

// what k_frame_close leaves in pinned host memory
struct CloseRecord {
    uint32_t valid, lastMatched, added, total;
    uint32_t flags;  // 1: the list would pass its capacity, nothing was appended
    uint32_t seq;
    uint32_t cur, start;  // the launch's own image and first prev: a retry launch's record names its candidate
    float sift[16], integ[16];
};

class Bundler {
public:
    static constexpr uint32_t kNone = BF_BUNDLER_NO_FRAME;
    static constexpr uint32_t kOverflow = 1u;

    explicit Bundler(const BundlerConfig& cfg);
    ~Bundler();
    Bundler(const Bundler&) = delete;
    Bundler& operator=(const Bundler&) = delete;

    void reset();
    void processFrame(const uint8_t* color, uint32_t cw, uint32_t ch, const float* depthFilt, const float* depthRaw,
                      BFBundlerFrame* out);
    // processInput's past-the-end branch (OnlineBundler.cpp:171-174) -> prepareLocalSolve(curFrame, true) (:134-165): the
    // current local set closes where it stands, nothing is copied into the other set; processFrame is refused afterwards
    void endSequence(BFBundlerEnd* out);
    void setCompleteTrajectory(const float* T, uint32_t n, uint32_t lastValid);
    void submap(BFBundlerSubmap* out) const;
    void fuseSubmap(const float* localTransforms, BFBundlerKeyframe* out);
    void invalidSubmap();
    void global(BFEntryJ** corr, const uint32_t** keyIdx, uint32_t* n, const uint32_t** prefix, uint32_t* numKeyframes);
    void debugReclose(BFBundlerFrame* out);
    // retry
    void setRetry(bool on);
    void retry(BFBundlerRetry* out);  // the sequence-over attempt (OnlineBundler.cpp:287-296)
    void lastRetry(BFBundlerRetry* out) const;
    void retryList(uint32_t* out, uint32_t cap, uint32_t* n) const;
    void applySeeds(float* dT, uint32_t numPoses);
    void keyframeFrames(uint32_t k, int32_t* valid, uint32_t* n) const;
    void debugRetryClose(uint32_t idx, BFBundlerRetry* out);

    const BundlerConfig& config() const { return cfg_; }
    hipStream_t stream() const { return stream_; }
    Sift& sift() { return *sift_; }
    Matcher& matcher(uint32_t which) { return which == BF_BUNDLER_GLOBAL ? *glob_ : *loc_[which == BF_BUNDLER_LOCAL ? cur_ : 1 - cur_]; }
    Cache& cache(uint32_t which) { return which == BF_BUNDLER_GLOBAL ? *cacheGlob_ : *cacheLoc_[which == BF_BUNDLER_LOCAL ? cur_ : 1 - cur_]; }
    const float* intensity() const { return lastIntensity_; }
    const BFBundlerStats& stats() const { return stats_; }
    uint32_t numFrames() const { return frame_; }      // frames processed since create / reset
    bool retryEnabled() const { return retry_; }
    // the global cache's device table of BFCachedFrame [maxKeyframes]: key frame k's cache frame (the dense end solve's)
    const BFCachedFrame* globalCacheTable() const { return frameTab_[2].p; }

private:
    // prepareLocalSolve's bookkeeping for set cur_ as the closed submap: the valid flags from the matcher's host mirror,
    // uploaded on the stream
    void recordClosed(uint32_t numFrames, uint32_t submap);

    // one launch of k_frame_close for image `cur` of matcher m on list `list` (0 / 1 local, 2 global), then the wait
    // over prev in [start, n)
    void closeFrame(Matcher& m, uint32_t list, uint32_t cur, uint32_t start, bool chain, uint32_t frameAll);
    // Bundler::matchAndFilter up to filterFrames for image cur of the global store
    void matchGlobal(uint32_t cur, uint32_t start);
    // tryRevalidation's body for candidate idx: [the filter chain,] the closing launch, last_ and the seeds. The list
    // is the caller's. True: the launch reported an overflow.
    bool revalidate(uint32_t idx, bool filters);
    bool tryRevalidation(bool scanDone);  // pops, revalidates, pushes back on failure; true: overflow
    void addSeeds(uint32_t cur, uint32_t lastMatched);
    void pushSeed(uint32_t to, uint32_t from);
    void beginRetryReport();
    void endRetryReport();
    void fillFrame(BFBundlerFrame* out, uint32_t lf, bool closed) const;
    void wait();  // the stream, counted

    BundlerConfig cfg_;
    hipStream_t stream_ = nullptr;
    std::unique_ptr<Sift> sift_;
    std::unique_ptr<Matcher> loc_[2], glob_;
    std::unique_ptr<Cache> cacheLoc_[2], cacheGlob_;
    DevBuf<BFEntryJ> corr_[3];
    DevBuf<uint32_t> keyIdx_[3];
    DevBuf<uint32_t> counts_;            // device-resident list lengths {local 0, local 1, global}
    DevBuf<BFCachedFrame> frameTab_[3];  // device BFCachedFrame tables of the three caches
    std::vector<BFCachedFrame> hostFrames_[2];
    DevBuf<int32_t> dValid_[2];
    DevBuf<float> siftTraj_, integ_, complete_;  // [submapSize * maxKeyframes][16]
    DevBuf<float> intensity_, intensityTmp_;
    GaussTable gauss_{};
    CloseRecord* rec_ = nullptr;  // pinned, written by k_frame_close
    uint32_t cap_[3] = {};
    uint32_t total_[3] = {};      // host mirrors of counts_
    uint32_t cur_ = 0;            // which local set is m_local
    bool free_[2] = {true, true}; // the set is reset and empty
    uint32_t frame_ = 0;          // frames processed
    bool ended_ = false;          // endSequence was called: no more frames until reset
    uint32_t lastValidComplete_ = 0;
    uint32_t seq_ = 0;
    const float* lastIntensity_ = nullptr;
    // the last closed submap
    int closed_ = -1;  // its local set, -1: none yet
    bool released_ = true;
    uint32_t closedFrames_ = 0, closedSubmap_ = 0, closedCorr_ = 0;
    bool closedValid_ = false;
    std::vector<int32_t> closedValidImages_;
    // the last frame, for debugReclose
    BFBundlerFrame lastFrame_{};
    uint32_t lastBefore_ = 0;
    bool canReclose_ = false;
    std::vector<uint32_t> prefix_;
    // retry
    bool retry_ = false;
    std::deque<uint32_t> retryList_;     // m_imagesToRetry
    int64_t continueRetry_ = 0;          // m_continueRetry: 0 unset, > 0 the first candidate after the sequence ended, -1 done
    BFBundlerRetry last_{};              // what the last fuseSubmap / retry did
    std::vector<std::vector<int32_t>> keyframeValid_;  // m_localTrajectoriesValid
    BFBundlerStats stats_{};
};

}  // namespace bf
