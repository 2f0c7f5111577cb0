// sift.h — the SIFT detector (sift.hip): SiftGPU's DoG key points, orientations and 128-byte descriptors as
// BundleFusion configures it, from the float intensity + depth image to what Matcher::addImage takes. One handle per
// input stream, everything queued on the handle's stream with no host round trip, no device allocation after the ctor.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/bf/bf.h"
#include "bf_runtime.h"

namespace bf {

struct SiftConfig {
    uint32_t width = 0, height = 0, depthWidth = 0, depthHeight = 0;
    uint32_t maxKeys = 1024, featureCountThreshold = 150;
    float sensorDepthMin = 0.1f, sensorDepthMax = 4.0f, minKeyScale = 3.0f;
    float dogThreshold = 0.02f / 3.0f, edgeThreshold = 10.0f;
};

// BFSiftOptions -> config with the defaults filled in; throws BF_ERR_ARG on invalid options (host only)
SiftConfig make_sift_config(const BFSiftOptions* o);

// SiftParam::ParseSiftParam's filter tables and level sigmas (host only)
struct SiftTables {
    float k[6][BF_SIFT_MAX_FILTER];
    uint32_t width[6];
    float levelSigma[3];  // GetLevelSigma of the three key levels
};
void make_sift_tables(SiftTables& t);

class Sift {
public:
    static constexpr uint32_t kOctaves = 4, kGauss = 6, kKeyLevels = 3, kLevels = BF_SIFT_LEVELS;
    static constexpr uint32_t kBandRows = 4;  // rows per workgroup of the key pass (a band spans the image width)

    Sift(const SiftConfig& cfg, hipStream_t stream);
    ~Sift();
    const SiftConfig& config() const { return cfg_; }
    const SiftTables& tables() const { return tab_; }
    void intensity(const uint8_t* color, uint32_t cw, uint32_t ch, float* out);
    void detect(const float* intensity, const float* depth);
    void result(const BFSiftKeyPoint** keys, const uint8_t** descs, uint32_t* n, uint32_t* flags);
    void levelCounts(uint32_t* raw, uint32_t* kept);
    void debugLevel(uint32_t octave, uint32_t level, float* host);
    void debugRawKeys(uint32_t level, int32_t* colRow, uint32_t* packed, uint32_t cap, uint32_t* n);

    // device-side counters of one detect; mirrored to pinned host memory at the end of detect()
    struct Counts {
        uint32_t raw[kLevels];       // keys the key test found
        uint32_t list[kLevels];      // after the per-level cap and LimitFeatureCount(0): the raw lists' lengths
        uint32_t kept[kLevels];      // keys of the level in the output
        uint32_t outStart[kLevels];  // first output index of the level
        uint32_t nFinal, flags;
    };

private:
    SiftConfig cfg_;
    SiftTables tab_;
    hipStream_t stream_;
    uint32_t w_[kOctaves], h_[kOctaves], fmax_[kOctaves], bands_[kOctaves], bandStart_[kOctaves + 1];
    size_t gaussOff_[kOctaves][kGauss], stageOff_[kLevels];
    uint32_t listOff_[kLevels + 1];
    uint32_t orientMask_ = 0;  // levels whose keys can pass minKeyScale
    bool detected_ = false, haveIntensity_ = false;
    DevBuf<float> intensity_, gauss_;
    DevBuf<uint32_t> stage_;      // per level, per band: the band's keys (row << 16 | col) from pixel r0 * w on
    DevBuf<uint32_t> bandCount_, bandOffset_;  // [3 * bandStart_[4]] (level-major within an octave)
    DevBuf<uint32_t> rawList_, rawOri_;        // per level fmax entries: row << 16 | col, packed orientations
    DevBuf<uint4> final_;                      // [maxKeys] {row << 16 | col, level, orientation bits, 0}
    DevBuf<BFSiftKeyPoint> keys_;
    DevBuf<uint8_t> descs_;
    DevBuf<Counts> counts_;
    Counts* hostCounts_ = nullptr;  // pinned
};

}  // namespace bf
