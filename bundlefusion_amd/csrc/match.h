// match.h — the sparse matcher (match.hip): image store of key points + descriptors, descriptor matching on
// the int8 matrix cores, the Kabsch key-point match filter, the surface-area and dense-verify filters, filterFrames
// and the EntryJ producer. One handle per Bundler (local / global), everything queued on the handle's stream, no
// device allocation after the ctor.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/bf/bf.h"
#include "bf_runtime.h"

namespace bf {

struct MatcherConfig {
    uint32_t maxImages = 0, maxKeys = 0;
    float matchThresh = 0.7f, ratioMax = 0.8f;
    uint32_t minNumMatches = 5;
    float maxKabschRes2 = 0.0004f;
    float kinv[16] = {};
    uint32_t fuseMaxCorr = 0;  // records a fuseToGlobal FROM this matcher may take; 0: no fuse scratch, no fusing
};

// thresholds of the surface-area and dense-verify filters (zParametersBundlingDefault.txt / zParametersDefault.txt)
struct MatchVerifyConfig {
    float surfAreaPcaThresh = 0.032f;
    float projCorrDistThres = 0.15f, projCorrNormalThres = 0.97f;
    float verifySiftErrThresh = 0.075f, verifySiftCorrThresh = 0.02f;
    float sensorDepthMin = 0.1f, sensorDepthMax = 4.0f;
};

// BFMatcherOptions -> config with the defaults filled in; throws BF_ERR_ARG on invalid options (host only)
MatcherConfig make_matcher_config(const BFMatcherOptions* o);
// ... and BFMatchVerifyOptions (null: every default)
MatchVerifyConfig make_match_verify_config(const BFMatchVerifyOptions* o);
// W, H >= 1, W * H <= 2^20, finite intrinsics; throws BF_ERR_ARG (host only)
void check_dense_frame_shape(uint32_t W, uint32_t H, const float* intrinsics);

class Matcher {
public:
    static constexpr uint32_t kRaw = BF_MAX_MATCHES_RAW, kFilt = BF_MAX_MATCHES_FILTERED, kDbg = 32;
    static constexpr uint32_t kSlices = 16;  // row slices (workgroups) per pair of the dense-verify kernel

    Matcher(const MatcherConfig& cfg, hipStream_t stream);
    ~Matcher();
    void reset();
    uint32_t addImage(const BFSiftKeyPoint* keys, const uint8_t* descs, uint32_t n);
    uint32_t numImages() const { return (uint32_t)num_.size(); }
    uint32_t numKeys(uint32_t i) const { return num_[i]; }
    uint32_t keyOffset(uint32_t i) const { return off_[i]; }
    void setValid(uint32_t i, int v);
    int valid(uint32_t i) const { return valid_[i]; }
    const MatcherConfig& config() const { return cfg_; }

    void match(uint32_t cur, uint32_t start);
    void filter(uint32_t cur, uint32_t start);
    // both reject a pair of the last filter() by setting its filtered count to 0; host checks before any device work
    void filterSurfaceArea(uint32_t cur, uint32_t start, const MatchVerifyConfig& v);
    void filterDenseVerify(uint32_t cur, uint32_t start, const BFCachedFrame* frames, uint32_t nFrames, uint32_t W, uint32_t H,
                           const float* intrinsics, const MatchVerifyConfig& v);
    void checkFrames(uint32_t cur, uint32_t start) const;
    void checkDenseShape(uint32_t nFrames, uint32_t W, uint32_t H, const float* intrinsics) const;
    void verifyStats(uint32_t prev, float* area, float* sums);
    void debugSetFiltered(uint32_t prev, uint32_t count, const uint32_t* idx);
    uint32_t filterFrames(uint32_t cur, uint32_t start);
    uint32_t addToResiduals(uint32_t cur, uint32_t start, BFEntryJ* out, uint32_t* keyIdx, uint32_t cap, uint32_t* total);
    void rawMatches(uint32_t prev, uint32_t* count, uint32_t* idx, float* dist);
    void filteredMatches(uint32_t prev, uint32_t* count, uint32_t* idx, float* dist);
    void transforms(uint32_t prev, float* T, float* Tinv);
    void debugDots(uint32_t prev, uint32_t cur, const uint32_t* rows, uint32_t nRows, const uint32_t* cols, uint32_t nCols,
                   int32_t* dots, int32_t* rowStats);
    // match_fuse.h: this store's tracks become the next image of glob's store; queued on this matcher's stream, glob's
    // stream ordered behind it, returns after the read-back of the counts
    void fuseToGlobal(Matcher& glob, const BFEntryJ* corr, const uint32_t* keyIdx, uint32_t nCorr, const float* transforms,
                      const float* intrinsics, uint32_t* index, uint32_t* numKeys, uint32_t* numTracks);
    void fuseTracks(uint32_t* root, uint32_t* rank, uint8_t* good);
    void imageKeys(uint32_t image, BFSiftKeyPoint* keys, uint8_t* descs);

    // ---- what the bundler's closing launch (bundler.hip, k_frame_close) needs; none of it changes a member above ----
    // device views of the state filterFrames / addToResiduals / transforms read on the host
    struct CloseView {
        const BFSiftKeyPoint* keys;
        const uint32_t* filtCount;
        const uint2* filtIdx;
        const uint32_t* table;  // per image {offset, count, valid, 0}
        const float* Tinv;
        const float* kinv;      // intrinsicsInv, 16 floats
        uint32_t* base;         // [maxImages] EntryJ base per pair, the array k_add_residuals reads
    };
    // the argument checks of filterFrames, the image table brought up to date on the device, then the views
    CloseView prepareClose(uint32_t cur, uint32_t start);
    // filterFrames' host half once the closing launch has decided: valid_[cur] from its record
    void applyClose(uint32_t cur, bool valid) { setValid(cur, valid); }
    // The caller has just waited for this matcher's stream: no earlier table upload can still read the pinned table,
    // so the next upload skips its own wait. Without this call every upload waits, as before.
    void streamDrained() { tableInFlight_ = false; }
    // Bundler::copyFrame's sparse half: image `image` of src becomes this store's next image (device-to-device)
    uint32_t copyImageFrom(const Matcher& src, uint32_t image);
    hipStream_t stream() const { return stream_; }

private:
    uint32_t appendStored(uint32_t n);  // the bookkeeping of addImage for n keys already in place behind the last image
    void uploadTable();
    void launchMatch(uint32_t cur, uint32_t start, uint32_t pairs, bool debug, uint32_t nRows, uint32_t nCols);

    MatcherConfig cfg_;
    hipStream_t stream_;
    std::vector<uint32_t> num_, off_;
    std::vector<int> valid_;
    uint32_t totalKeys_ = 0;
    bool tableDirty_ = true;
    bool tableInFlight_ = true;  // an upload may still read hostTable_ (cleared only by streamDrained)
    DevBuf<BFSiftKeyPoint> keys_;  // [maxImages * maxKeys], linear
    DevBuf<uint8_t> descs_;        // [maxImages * maxKeys][128]
    DevBuf<int32_t> sums_;         // byte sum per descriptor
    DevBuf<uint32_t> table_;       // per image {offset, count, valid, 0}
    DevBuf<uint32_t> rawCount_, filtCount_;  // [maxImages]
    DevBuf<uint2> rawIdx_, filtIdx_;         // [maxImages][128] / [maxImages][25]
    DevBuf<float> rawDist_, filtDist_;
    DevBuf<float> T_, Tinv_;                 // [maxImages][16]
    DevBuf<uint32_t> base_;                  // [maxImages] EntryJ base per pair
    DevBuf<float> area_;                     // [maxImages][2] surface areas of the last filterSurfaceArea (NaN: skipped)
    DevBuf<float> denseSums_;                // [maxImages][6] {residual, weight, count} x direction (NaN: skipped)
    DevBuf<float> densePartial_;             // [maxImages][kSlices][6] per-workgroup sums
    DevBuf<uint32_t> dbgSel_;                // rows[32], cols[32]
    DevBuf<int32_t> dbgOut_;                 // dots[32 * 32], rowStats[3 * 32]
    uint32_t* hostTable_ = nullptr;          // pinned, 4 * maxImages
    uint32_t* hostCounts_ = nullptr;         // pinned, maxImages
    uint32_t* hostBase_ = nullptr;           // pinned, maxImages
    // key fusing (match_fuse.h), allocated when cfg.fuseMaxCorr > 0
    DevBuf<uint32_t> fuseCnt_, fuseOff_, fusePar_, fuseRoot_, fuseRank_;  // per key
    DevBuf<uint8_t> fuseGood_, fuseEdge_;                                 // per key, per record
    DevBuf<uint32_t> fuseAdj_, fuseAdjT_;                                 // per half-edge
    DevBuf<uint32_t> fuseComp_, fuseRep_, fuseOutRep_;                    // per component / fused key
    DevBuf<BFSiftKeyPoint> fuseCompKey_, fuseOutKey_;
    DevBuf<uint32_t> fuseCounts_;                                         // {tracks, keys stored, error bits, components}
    uint32_t* hostFuse_ = nullptr;                                        // pinned, 4
    hipEvent_t fuseDone_ = nullptr;
    uint32_t fuseKeys_ = 0;  // keys in use at the last fuse
    bool fuseRan_ = false;
};

}  // namespace bf
