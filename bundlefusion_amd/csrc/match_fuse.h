// match_fuse.h — key fusing: a solved submap's correspondences become the key points of its global image.
// Restates SIFTImageManager::fuseToGlobal / computeTracks / findTrack (SiftGPU/SIFTImageManager.cpp:367-476), which the
// reference runs on the host behind five device-to-host copies ("TODO GPU version of this??", OnlineBundler.cpp:308).
// Included by match.hip; DESIGN.md §3.5 has the semantics and the proof sketch of the search equivalence used here:
// the track of a component is the preorder of a depth-first search that STARTS AT THE FIRST NEIGHBOUR of the component's
// lowest key, neighbours taken in record order, and every key carries the good / bad flag of the edge that found it.
//
// k_fuse — ONE workgroup of 1024 lanes, every phase of the stage behind a workgroup barrier, no host step and no
// second launch in between: the problem is 11 x 1 024 keys and 1 375 records in the loop, so its time is launch
// latency and dependent loads, not bandwidth. All state is per-key / per-record scratch in global memory (L2
// resident), so it is correct for any store size and any record count up to fuseMaxCorr, only slower.
//   0  per key: degree 0, union-find parent = itself, root / rank = none
//   1  per record: skip invalid ones, flag malformed ones (never dereferenced), classify the edge good / bad
//      (MAX_TRACK_CORR_ERROR), count degrees (atomicAdd), unite the two keys. The union-find links the larger root
//      under the smaller one (atomicCAS on roots only), so a component's root is its lowest key whatever the order
//      of arrival; finds halve paths.
//   2  exclusive scan of the degrees -> list offsets
//   3  half-edge 2r (at x, towards y) and 2r + 1 (at y, towards x) of record r into their keys' lists at an atomic
//      slot ...
//   4  ... and every list sorted by half-edge id, which is record order (insertion sort, heap sort above 16); the
//      list of target keys; root of every key; the components numbered in ascending order of their lowest key (scan)
//   5  one lane per component: the search, with per-key parent and cursor arrays instead of a stack, so its depth is
//      unbounded (state is O(keys)). The lane adds T[image] * pos of every good entry in track order: no float
//      atomics, the sum has one order. mean, projection, the representative (first) entry's scale.
//   6  components that yielded a key compacted in component order (scan) -> the track order of the reference
//   7  more than the limit: rank by (depth, track order) by counting, the first `limit` kept, descriptors moving
//      with their keys (the reference sorts only the key points: DESIGN.md §3.5, third departure); otherwise track order.
//      Keys, descriptors and descriptor byte sums go straight behind the global store's last image.
// Every loop of the union-find and of the search is bounded by keys + 2 records + 2; running into the bound raises
// the internal-error bit instead of hanging.
#pragma once
#include <hip/hip_runtime.h>

#include "bf_math.h"
#include "match.h"
#include "wave.h"

namespace bf {
namespace {

constexpr uint32_t FUSE_WG = 1024;
constexpr uint32_t FUSE_NONE = 0xFFFFFFFFu;
constexpr uint32_t FUSE_BAD_RECORD = 1u, FUSE_INTERNAL = 2u;  // counts[2]
constexpr float FUSE_MAX_TRACK_CORR_ERROR = 0.03f;            // SIFTImageManager.cpp:380

struct FuseArgs {
    // the local store and the submap
    const BFSiftKeyPoint* keys;
    const uint8_t* descs;
    const int32_t* sums;
    const BFEntryJ* corr;
    const uint32_t* keyIdx;   // [2 * nCorr] {x, y}
    const float* transforms;  // [nImages][16]
    m4 K;
    uint32_t nKeys, nImages, nCorr;
    // scratch
    uint32_t *cnt, *off, *par, *root, *rank;  // per key (off: + 1)
    uint8_t* good;                            // per key
    uint8_t* eflag;                           // per record: 0 no edge, 1 good, 2 bad
    uint32_t *adj, *adjT;                     // per half-edge: id, target key
    uint32_t *comp, *rep;                     // per component: lowest key (later: destination), representative key
    BFSiftKeyPoint* ckey;                     // per component
    uint32_t* outRep;                         // per fused key, track order
    BFSiftKeyPoint* outKey;
    uint32_t compCap;
    uint32_t* counts;  // {fused keys before truncation, keys stored, error bits, components}
    // the global store, behind its last image
    BFSiftKeyPoint* gKeys;
    uint8_t* gDescs;
    int32_t* gSums;
    uint32_t gOff, limit;
};

__device__ __forceinline__ uint32_t fuse_ld(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void fuse_st(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// between two phases: what a lane wrote, atomically or not, is what every lane of the workgroup reads afterwards
__device__ __forceinline__ void fuse_sync() {
    __threadfence();
    __syncthreads();
    __threadfence();
}

// root of v; par[u] <= u throughout, so the walk ends. Halves the path.
__device__ uint32_t fuse_find(uint32_t* par, uint32_t v, uint32_t bound) {
    for (uint32_t it = 0; it < bound; it++) {
        const uint32_t p = fuse_ld(par + v);
        if (p == v) return v;
        const uint32_t g = fuse_ld(par + p);
        if (g == p) return p;
        fuse_st(par + v, g);
        v = g;
    }
    return v;
}

// false: ran into the bound
__device__ bool fuse_unite(uint32_t* par, uint32_t a, uint32_t b, uint32_t bound) {
    for (uint32_t it = 0; it < bound; it++) {
        a = fuse_find(par, a, bound);
        b = fuse_find(par, b, bound);
        if (a == b) return true;
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        if (atomicCAS(par + a, a, b) == a) return true;  // only a root is ever linked, and only below itself
    }
    return false;
}

__device__ void fuse_sift_down(uint32_t* a, uint32_t i, uint32_t n) {
    for (;;) {
        uint32_t c = 2 * i + 1;
        if (c >= n) return;
        if (c + 1 < n && a[c + 1] > a[c]) c++;
        if (a[i] >= a[c]) return;
        const uint32_t t = a[i];
        a[i] = a[c];
        a[c] = t;
        i = c;
    }
}

// ascending, in place, by one lane: lists are a handful of entries unless one key sits in very many records
__device__ void fuse_sort(uint32_t* a, uint32_t n) {
    if (n <= 16) {
        for (uint32_t i = 1; i < n; i++) {
            const uint32_t v = a[i];
            uint32_t j = i;
            for (; j > 0 && a[j - 1] > v; j--) a[j] = a[j - 1];
            a[j] = v;
        }
        return;
    }
    for (uint32_t i = n / 2; i-- > 0;) fuse_sift_down(a, i, n);
    for (uint32_t end = n - 1; end > 0; end--) {
        const uint32_t t = a[0];
        a[0] = a[end];
        a[end] = t;
        fuse_sift_down(a, 0, end);
    }
}

// a float as an unsigned integer of the same order (-0 counts as +0)
__device__ __forceinline__ uint32_t fuse_depth_order(float d) {
    const uint32_t u = __float_as_uint(d + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ f3 fuse_world(const FuseArgs& A, uint32_t img, const BFFloat3& p) {
    m4 T;
    const float* t = A.transforms + 16 * (size_t)img;
    for (int k = 0; k < 16; k++) T.e[k] = t[k];
    return xform(T, mk3(p.x, p.y, p.z));
}

__global__ __launch_bounds__(FUSE_WG) void k_fuse(FuseArgs A) {
    __shared__ uint32_t sScan[FUSE_WG / 64];  // every scan is followed by a fuse_sync() before the next one writes it
    const uint32_t tid = threadIdx.x, N = A.nKeys, C = A.nCorr;
    const uint32_t bound = N + 2 * C + 2;
    const uint32_t chunk = (N + FUSE_WG - 1) / FUSE_WG;  // consecutive keys per lane in the scans
    const uint32_t lo = min(tid * chunk, N), hi = min(lo + chunk, N);

    // 0
    for (uint32_t k = tid; k < N; k += FUSE_WG) {
        A.cnt[k] = 0;
        A.par[k] = k;
        A.root[k] = FUSE_NONE;
        A.rank[k] = FUSE_NONE;
        A.good[k] = 0;
    }
    if (tid == 0) A.counts[2] = 0;
    fuse_sync();

    // 1
    for (uint32_t r = tid; r < C; r += FUSE_WG) {
        const BFEntryJ e = A.corr[r];
        uint8_t f = 0;
        if (e.imgIdx_i != FUSE_NONE) {
            const uint32_t x = A.keyIdx[2 * (size_t)r], y = A.keyIdx[2 * (size_t)r + 1];
            if (x >= N || y >= N || e.imgIdx_i >= A.nImages || e.imgIdx_j >= A.nImages) {
                atomicOr(A.counts + 2, FUSE_BAD_RECORD);
            } else {
                const float err = length3(fuse_world(A, e.imgIdx_i, e.pos_i) - fuse_world(A, e.imgIdx_j, e.pos_j));
                f = err < FUSE_MAX_TRACK_CORR_ERROR ? 1 : 2;
                atomicAdd(A.cnt + x, 1u);
                atomicAdd(A.cnt + y, 1u);
                if (!fuse_unite(A.par, x, y, bound)) atomicOr(A.counts + 2, FUSE_INTERNAL);
            }
        }
        A.eflag[r] = f;
    }
    fuse_sync();

    // 2
    {
        uint32_t sum = 0;
        for (uint32_t k = lo; k < hi; k++) sum += fuse_ld(A.cnt + k);
        uint32_t total;
        uint32_t run = wg_exclusive_scan<FUSE_WG / 64>(sum, sScan, total);
        for (uint32_t k = lo; k < hi; k++) {
            const uint32_t d = fuse_ld(A.cnt + k);
            A.off[k] = run;
            fuse_st(A.cnt + k, 0);  // the fill cursor of phase 3
            run += d;
        }
        if (tid == 0) A.off[N] = total;
    }
    fuse_sync();

    // 3
    for (uint32_t r = tid; r < C; r += FUSE_WG) {
        if (!A.eflag[r]) continue;
        const uint32_t x = A.keyIdx[2 * (size_t)r], y = A.keyIdx[2 * (size_t)r + 1];
        A.adj[A.off[x] + atomicAdd(A.cnt + x, 1u)] = 2 * r;
        A.adj[A.off[y] + atomicAdd(A.cnt + y, 1u)] = 2 * r + 1;
    }
    fuse_sync();

    // 4: cnt[k] is the degree again, and from here the number of neighbours the search has not looked at yet
    for (uint32_t k = tid; k < N; k += FUSE_WG) {
        const uint32_t o = A.off[k], d = A.off[k + 1] - o;
        if (d == 0) continue;
        fuse_sort(A.adj + o, d);
        for (uint32_t s = o; s < o + d; s++) {
            const uint32_t h = A.adj[s];
            A.adjT[s] = (h >> 1) < C ? A.keyIdx[2 * (size_t)(h >> 1) + ((h & 1u) ^ 1u)] : FUSE_NONE;
        }
        A.root[k] = fuse_find(A.par, k, bound);
    }
    fuse_sync();
    uint32_t nComp;
    {
        uint32_t mine = 0;
        for (uint32_t k = lo; k < hi; k++) mine += A.root[k] == k;
        uint32_t at = wg_exclusive_scan<FUSE_WG / 64>(mine, sScan, nComp);
        for (uint32_t k = lo; k < hi; k++)
            if (A.root[k] == k) {
                if (at < A.compCap) A.comp[at] = k;
                at++;
            }
        if (nComp > A.compCap) {  // a component has a valid record of its own, so this cannot happen
            if (tid == 0) atomicOr(A.counts + 2, FUSE_INTERNAL);
            nComp = A.compCap;
        }
    }
    fuse_sync();

    // 5: par[] is the search's parent pointer from here
    for (uint32_t c = tid; c < nComp; c += FUSE_WG) {
        const uint32_t k = A.comp[c];
        const uint32_t first = A.adjT[A.off[k]];
        uint32_t placed = 0, nGood = 0;
        f3 sum = mk3(0.0f, 0.0f, 0.0f);
        // key o enters the track through half-edge h, found from key `from`
        auto discover = [&](uint32_t o, uint32_t h, uint32_t from) {
            const uint32_t r = h >> 1;
            const bool g = A.eflag[r] == 1;
            A.rank[o] = placed++;
            A.good[o] = g ? 1 : 0;
            A.par[o] = from;
            if (g) {
                const BFEntryJ e = A.corr[r];
                sum += (h & 1u) ? fuse_world(A, e.imgIdx_i, e.pos_i) : fuse_world(A, e.imgIdx_j, e.pos_j);
                nGood++;
            }
        };
        bool ok = first < N && (A.adj[A.off[k]] >> 1) < C;
        if (ok) {
            discover(first, A.adj[A.off[k]], FUSE_NONE);
            uint32_t cur = first;
            for (uint32_t it = 0;; it++) {  // a step takes one neighbour or returns to the parent: <= 2 C + keys steps
                if (it >= bound) {
                    ok = false;
                    break;
                }
                const uint32_t left = fuse_ld(A.cnt + cur);
                if (left == 0) {
                    cur = A.par[cur];
                    if (cur == FUSE_NONE) break;
                    continue;
                }
                const uint32_t s = A.off[cur + 1] - left;
                fuse_st(A.cnt + cur, left - 1);
                const uint32_t o = A.adjT[s], h = A.adj[s];
                if (o >= N || (h >> 1) >= C) {
                    ok = false;
                    break;
                }
                if (A.rank[o] == FUSE_NONE) {
                    discover(o, h, cur);
                    cur = o;
                }
            }
        }
        if (!ok) atomicOr(A.counts + 2, FUSE_INTERNAL);
        uint32_t rep = FUSE_NONE;
        if (ok && nGood > 0) {
            const f3 mean = sum / (float)nGood;  // cutil_math.h:908
            const f3 p = xform(A.K, mean);
            BFSiftKeyPoint key;
            key.x = p.x / p.z;
            key.y = p.y / p.z;
            key.scale = A.keys[first].scale;
            key.depth = p.z;
            A.ckey[c] = key;
            rep = first;
        }
        A.rep[c] = rep;
    }
    fuse_sync();

    // 6
    const uint32_t cchunk = (nComp + FUSE_WG - 1) / FUSE_WG;
    const uint32_t clo = min(tid * cchunk, nComp), chi = min(clo + cchunk, nComp);
    uint32_t nTracks;
    {
        uint32_t mine = 0;
        for (uint32_t c = clo; c < chi; c++) mine += A.rep[c] != FUSE_NONE;
        uint32_t at = wg_exclusive_scan<FUSE_WG / 64>(mine, sScan, nTracks);
        for (uint32_t c = clo; c < chi; c++)
            if (A.rep[c] != FUSE_NONE) {
                A.outKey[at] = A.ckey[c];
                A.outRep[at] = A.rep[c];
                at++;
            }
    }
    fuse_sync();

    // 7: comp[] is the destination of every fused key from here
    const uint32_t nOut = min(nTracks, A.limit);
    for (uint32_t i = tid; i < nTracks; i += FUSE_WG) {
        uint32_t dst = i;
        if (nTracks > A.limit) {
            const uint32_t di = fuse_depth_order(A.outKey[i].depth);
            dst = 0;
            for (uint32_t j = 0; j < nTracks; j++) {
                const uint32_t dj = fuse_depth_order(A.outKey[j].depth);
                dst += dj < di || (dj == di && j < i);
            }
        }
        if (dst < nOut) {
            A.gKeys[A.gOff + dst] = A.outKey[i];
            A.gSums[A.gOff + dst] = A.sums[A.outRep[i]];
        } else {
            dst = FUSE_NONE;
        }
        A.comp[i] = dst;
    }
    fuse_sync();
    for (uint32_t q = tid; q < 8 * nTracks; q += FUSE_WG) {  // 128 bytes = 8 x 16 per descriptor
        const uint32_t i = q >> 3, part = q & 7u, dst = A.comp[i];
        if (dst == FUSE_NONE) continue;
        const uint4* from = (const uint4*)(A.descs + (size_t)A.outRep[i] * 128);
        uint4* to = (uint4*)(A.gDescs + (size_t)(A.gOff + dst) * 128);
        to[part] = from[part];
    }
    if (tid == 0) {
        A.counts[0] = nTracks;
        A.counts[1] = nOut;
        A.counts[3] = nComp;
    }
}

}  // namespace

void Matcher::fuseToGlobal(Matcher& glob, const BFEntryJ* corr, const uint32_t* keyIdx, uint32_t nCorr, const float* transforms,
                           const float* intrinsics, uint32_t* index, uint32_t* numKeys, uint32_t* numTracks) {
    BF_REQUIRE(cfg_.fuseMaxCorr > 0, BF_ERR_ARG, "fuse_to_global: the local matcher was created with fuseMaxCorr = 0");
    BF_REQUIRE(&glob != this, BF_ERR_ARG, "fuse_to_global: global and local are the same matcher");
    BF_REQUIRE(nCorr <= cfg_.fuseMaxCorr, BF_ERR_ARG, "fuse_to_global: nCorr above fuseMaxCorr");
    BF_REQUIRE(nCorr == 0 || (corr && keyIdx && transforms), BF_ERR_ARG, "fuse_to_global: null records / key indices / transforms");
    BF_REQUIRE(intrinsics != nullptr, BF_ERR_ARG, "fuse_to_global: null intrinsics");
    for (int k = 0; k < 16; k++) BF_REQUIRE(std::isfinite(intrinsics[k]), BF_ERR_ARG, "fuse_to_global: non-finite intrinsics");
    BF_REQUIRE(glob.num_.size() < glob.cfg_.maxImages, BF_ERR_CAPACITY, "fuse_to_global: the global image store is full");
    FuseArgs A{};
    A.keys = keys_.p;
    A.descs = descs_.p;
    A.sums = sums_.p;
    A.corr = corr;
    A.keyIdx = keyIdx;
    A.transforms = transforms;
    for (int k = 0; k < 16; k++) A.K.e[k] = intrinsics[k];
    A.nKeys = totalKeys_;
    A.nImages = numImages();
    A.nCorr = nCorr;
    A.cnt = fuseCnt_.p;
    A.off = fuseOff_.p;
    A.par = fusePar_.p;
    A.root = fuseRoot_.p;
    A.rank = fuseRank_.p;
    A.good = fuseGood_.p;
    A.eflag = fuseEdge_.p;
    A.adj = fuseAdj_.p;
    A.adjT = fuseAdjT_.p;
    A.comp = fuseComp_.p;
    A.rep = fuseRep_.p;
    A.ckey = fuseCompKey_.p;
    A.outRep = fuseOutRep_.p;
    A.outKey = fuseOutKey_.p;
    A.compCap = (uint32_t)fuseComp_.n;
    A.counts = fuseCounts_.p;
    A.gKeys = glob.keys_.p;
    A.gDescs = glob.descs_.p;
    A.gSums = glob.sums_.p;
    A.gOff = glob.totalKeys_;
    // the reference cuts at its own m_maxKeyPointsPerImage; the image must fit the global store's row limit too
    A.limit = cfg_.maxKeys < glob.cfg_.maxKeys ? cfg_.maxKeys : glob.cfg_.maxKeys;
    k_fuse<<<1, FUSE_WG, 0, stream_>>>(A);
    BF_LAUNCH_CHECK();
    BF_HIP(hipMemcpyAsync(hostFuse_, fuseCounts_.p, 16, hipMemcpyDeviceToHost, stream_));
    BF_HIP(hipEventRecord(fuseDone_, stream_));
    BF_HIP(hipStreamWaitEvent(glob.stream_, fuseDone_, 0));
    BF_HIP(hipStreamSynchronize(stream_));
    fuseKeys_ = totalKeys_;
    fuseRan_ = true;
    BF_REQUIRE(!(hostFuse_[2] & FUSE_INTERNAL), BF_ERR_INTERNAL, "fuse_to_global: a search loop ran into its bound");
    BF_REQUIRE(!(hostFuse_[2] & FUSE_BAD_RECORD), BF_ERR_ARG,
               "fuse_to_global: a record's key index or image index is outside the local store");
    const uint32_t n = hostFuse_[1];
    BF_REQUIRE(n <= glob.cfg_.maxKeys, BF_ERR_CAPACITY, "fuse_to_global: more keys than the global store's maxKeysPerImage");
    const uint32_t at = glob.appendStored(n);
    if (index) *index = at;
    if (numKeys) *numKeys = n;
    if (numTracks) *numTracks = hostFuse_[0];
}

void Matcher::fuseTracks(uint32_t* root, uint32_t* rank, uint8_t* good) {
    BF_REQUIRE(fuseRan_, BF_ERR_STATE, "fuse_tracks: no fuse_to_global has run on this matcher");
    BF_HIP(hipStreamSynchronize(stream_));
    if (fuseKeys_ == 0) return;
    if (root) BF_HIP(hipMemcpy(root, fuseRoot_.p, 4 * (size_t)fuseKeys_, hipMemcpyDeviceToHost));
    if (rank) BF_HIP(hipMemcpy(rank, fuseRank_.p, 4 * (size_t)fuseKeys_, hipMemcpyDeviceToHost));
    if (good) BF_HIP(hipMemcpy(good, fuseGood_.p, (size_t)fuseKeys_, hipMemcpyDeviceToHost));
}

}  // namespace bf
