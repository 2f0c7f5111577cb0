// ba.hip — the bundle adjuster's translation unit: the host class Solver, the small pose and gate
// kernels, and the gfx950 kernels of the solve, which live in five headers that only this file includes
// (see ba.h for the device layout):
//   ba_dev.h      constants, the argument block BA, sums, hand-off primitives, the PCG step rule
//   ba_table.h    row table, pair table, the assembled pair blocks
//   ba_pcg.h      GN step setup; the PCG with one launch per iteration (matrix-free and pair mode),
//                 and in one workgroup (k_pcg_small)
//   ba_persist.h  the persistent PCG launch (one or four finisher workgroups), its timeout redo, k_gn_end
//   ba_dense.h    dense term, residual analysis, local verification
// Every PCG route must give the same bits; what they share is defined once, in ba_dev.h and ba_pcg.h.
//
// Reference: Source/Solver/SolverBundling.cu, SolverBundlingEquationsLie.h,
// SolverBundlingDenseUtil.h, LieDerivUtil.h (cited per kernel).
//
// The sparse term is rewritten around two identities of the reference's Lie Jacobian
// (evalLie_dAlpha/dBeta/dGamma, LieDerivUtil.h:231-242):
//   da*w.x + db*w.y + dc*w.z = w x P      and      (da.g, db.g, dc.g) = P x g
// so with P_s = T_self p_self and P_o = T_other p_other fixed for a GN iteration, one row entry of
// image v contributes   g = w[(pRot_v x P_s + pTrans_v) - (pRot_o x P_o + pTrans_o)],
//   Ap_rot(v) += P_s x g,   Ap_trans(v) += g
// (applyJDevice + applyJTDevice, SolverBundlingEquationsLie.h:154-228, with the +-1 sign of the
// row folded in). The PCG loop streams 32 B per row entry and gathers only the N-sized p vector.
#include "ba.h"
#include "lie.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

// the kernels by route, in dependency order (only this file includes them)
#include "ba_dev.h"
#include "ba_table.h"
#include "ba_pcg.h"
#include "ba_persist.h"
#include "ba_dense.h"

namespace bf {

namespace {

// ---- SBA.cu / SIFTImageManager.cu helpers ----
__global__ void k_m2p(const float* T, uint32_t n, float* rot, float* trans, const int* valid) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && valid[i]) {
        m4 M;
        for (int k = 0; k < 16; k++) M.e[k] = T[(size_t)i * 16 + k];
        f3 r, t;
        matrix_to_pose(M, r, t);
        rot[3 * i] = r.x; rot[3 * i + 1] = r.y; rot[3 * i + 2] = r.z;
        trans[3 * i] = t.x; trans[3 * i + 1] = t.y; trans[3 * i + 2] = t.z;
    }
}
__global__ void k_p2m(const float* rot, const float* trans, uint32_t n, float* T, const int* valid) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && valid[i]) {
        const m4 M = pose_to_matrix(mk3(rot[3 * i], rot[3 * i + 1], rot[3 * i + 2]), mk3(trans[3 * i], trans[3 * i + 1], trans[3 * i + 2]));
        for (int k = 0; k < 16; k++) T[(size_t)i * 16 + k] = M.e[k];
    }
}
__global__ void k_invalidate_pair(BFEntryJ* corr, uint32_t n, uint32_t i, uint32_t j) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n && corr[c].imgIdx_i == i && corr[c].imgIdx_j == j) { corr[c].imgIdx_i = BF_INVALID_IMAGE; corr[c].imgIdx_j = BF_INVALID_IMAGE; }
}
__global__ void k_check_frames(const int* numEntries, int* valid, uint32_t numImages, BFEntryJ* corr, uint32_t nCorr, int comprehensive) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < numImages && numEntries[t] == 0) valid[t] = 0;
    if (comprehensive) {
        for (uint32_t c = t; c < nCorr; c += gridDim.x * blockDim.x) {
            const BFEntryJ e = corr[c];
            if (corr_valid(e) && (numEntries[e.imgIdx_i] == 0 || numEntries[e.imgIdx_j] == 0)) {
                corr[c].imgIdx_i = BF_INVALID_IMAGE;
                corr[c].imgIdx_j = BF_INVALID_IMAGE;
            }
        }
    }
}

// initNextGlobalTransformCU (OnlineBundler.cu:112-140): keyframe s+1 = global[s] * local[last]; when the
// submap's gate is 0 (invalid local) Bundler::initializeNextTransformUnknown instead (Bundler.h:75-79,
// via addInvalidFrame, Bundler.cpp:362-368): keyframe s+1 = keyframe s
__global__ void k_seed_keyframe(const float* localRot, const float* localTrans, uint32_t last, float* rot, float* trans,
                                uint32_t s, const int* gate) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (gate && *gate == 0) {
        for (int k = 0; k < 3; k++) { rot[3 * (s + 1) + k] = rot[3 * s + k]; trans[3 * (s + 1) + k] = trans[3 * s + k]; }
        return;
    }
    const m4 G = pose_to_matrix(mk3(rot[3 * s], rot[3 * s + 1], rot[3 * s + 2]), mk3(trans[3 * s], trans[3 * s + 1], trans[3 * s + 2]));
    const m4 L = pose_to_matrix(mk3(localRot[3 * last], localRot[3 * last + 1], localRot[3 * last + 2]),
                                mk3(localTrans[3 * last], localTrans[3 * last + 1], localTrans[3 * last + 2]));
    f3 r, t;
    matrix_to_pose(mul44(G, L), r, t);
    rot[3 * (s + 1)] = r.x; rot[3 * (s + 1) + 1] = r.y; rot[3 * (s + 1) + 2] = r.z;
    trans[3 * (s + 1)] = t.x; trans[3 * (s + 1) + 1] = t.y; trans[3 * (s + 1) + 2] = t.z;
}
__global__ void k_set_gate(int* gate, const int* src) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *gate = src ? *src : 1;
}
// An invalidated local submap becomes an invalid global frame with no features
// (OnlineBundler.cpp:351-360: addInvalidFrame; :399-401: invalidateLastFrame): its keyframe is marked
// invalid and no correspondence of the global list may reference it (the reference's matcher finds
// none for a frame with 0 SIFT keys; here the list is an input, so its entries are invalidated)
__global__ void k_invalidate_local(const int* gate, uint32_t s, int* valid, BFEntryJ* corr, uint32_t n) {
    if (*gate != 0) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) valid[s] = 0;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x)
        if (corr[c].imgIdx_i == s || corr[c].imgIdx_j == s) { corr[c].imgIdx_i = BF_INVALID_IMAGE; corr[c].imgIdx_j = BF_INVALID_IMAGE; }
}

// SBA::removeMaxResidualCUDA (SBA.cpp:164-203) + getMaxResidual (CUDASolverBundling.cpp:429-452) on
// the device: pick the pair of the max residual when it exceeds the threshold and is not (0, <10)
__global__ void k_pick_maxres_pair(uint32_t* ctrl, const BFEntryJ* corr, float thresh) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint32_t pi = BF_INVALID_IMAGE, pj = BF_INVALID_IMAGE;
    const float mr = __uint_as_float(ctrl[K_MAXRES]);
    if (mr > thresh) {
        const BFEntryJ e = corr[ctrl[K_MAXIDX]];
        if (e.imgIdx_i != BF_INVALID_IMAGE && !(e.imgIdx_i == 0 && e.imgIdx_j < 10)) {
            pi = e.imgIdx_i;
            pj = e.imgIdx_j;
        }
    }
    ctrl[K_RM_I] = pi;
    ctrl[K_RM_J] = pj;
}
__global__ void k_invalidate_picked_pair(const uint32_t* ctrl, BFEntryJ* corr, uint32_t n) {
    const uint32_t i = ctrl[K_RM_I], j = ctrl[K_RM_J];
    if (i == BF_INVALID_IMAGE) return;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x)
        if (corr[c].imgIdx_i == i && corr[c].imgIdx_j == j) { corr[c].imgIdx_i = BF_INVALID_IMAGE; corr[c].imgIdx_j = BF_INVALID_IMAGE; }
}
// CheckForInvalidFramesSimpleCU (SIFTImageManager.cu:725-745), only after a removal
__global__ void k_check_frames_if_removed(const uint32_t* ctrl, const int* numEntries, int* valid, uint32_t numImages) {
    if (ctrl[K_RM_I] == BF_INVALID_IMAGE) return;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < numImages && numEntries[t] == 0) valid[t] = 0;
}

// one per device: orders the persistent PCG launches of all solvers on it (Solver::solve)
struct PersistGate {
    std::mutex mu;
    hipEvent_t ev = nullptr;
    hipStream_t stream = nullptr;
};
PersistGate& persist_gate() {
    static PersistGate gates[64];
    int dev = 0;
    BF_HIP(hipGetDevice(&dev));
    return gates[dev & 63];
}

}  // namespace

// zParametersBundlingDefault.txt defaults for every option left 0
SolverConfig make_solver_config(uint32_t maxImages, uint32_t maxCorr, const BFSolverOptions* o) {
    SolverConfig cfg{};
    cfg.maxImages = maxImages;
    cfg.maxCorr = maxCorr;
    cfg.denseDistThresh = (o && o->denseDistThresh > 0) ? o->denseDistThresh : 0.15f;
    cfg.denseNormalThresh = (o && o->denseNormalThresh > 0) ? o->denseNormalThresh : 0.97f;
    cfg.denseColorThresh = (o && o->denseColorThresh > 0) ? o->denseColorThresh : 0.1f;
    cfg.denseColorGradientMin = (o && o->denseColorGradientMin > 0) ? o->denseColorGradientMin : 0.005f;
    cfg.denseDepthMin = (o && o->denseDepthMin > 0) ? o->denseDepthMin : 0.5f;
    cfg.denseDepthMax = (o && o->denseDepthMax > 0) ? o->denseDepthMax : 4.0f;
    cfg.denseOverlapSubsample = (o && o->denseOverlapSubsample) ? o->denseOverlapSubsample : 4;
    cfg.verifyOptDistThresh = (o && o->verifyOptDistThresh > 0) ? o->verifyOptDistThresh : 0.02f;
    cfg.normalEquations = o ? o->normalEquations : 0;
    cfg.earlyOut = !(o && o->disableEarlyOut);
    cfg.pcgLaunch = o ? o->pcgLaunch : 0;
    cfg.pcgSpinLimitUs = o ? o->pcgSpinLimitUs : 0u;
    return cfg;
}

VerifyParams verify_params(const BFVerifyOptions* o) {
    VerifyParams p{};
    if (!o) return p;
    if (o->projCorrDistThresh > 0) p.distThresh = o->projCorrDistThresh;
    if (o->projCorrNormalThresh > 0) p.normalThresh = o->projCorrNormalThresh;
    if (o->verifyOptErrThresh > 0) p.errThresh = o->verifyOptErrThresh;
    if (o->verifyOptCorrThresh > 0) p.corrThresh = o->verifyOptCorrThresh;
    if (o->verifyOptPercentThresh > 0) p.percentThresh = o->verifyOptPercentThresh;
    if (o->sensorDepthMin > 0) p.depthMin = o->sensorDepthMin;
    if (o->sensorDepthMax > 0) p.depthMax = o->sensorDepthMax;
    p.always = o->always != 0;
    return p;
}

// ------------------------------------------------------------------------------------------------
Solver::Solver(const SolverConfig& cfg, hipStream_t stream) : cfg_(cfg), stream_(stream) {
    BF_REQUIRE(cfg.maxImages >= 2 && cfg.maxCorr >= 1, BF_ERR_ARG, "solver capacity");
    // maxCorrPerImage = clamp(maxRes / maxImages, 1000, 4000) (CUDASolverBundling.cpp:37)
    maxCorrPerImage_ = std::min(4000u, std::max(1000u, cfg.maxCorr / cfg.maxImages));
    maxPairs_ = cfg.maxImages * (cfg.maxImages - 1) / 2;
    const uint32_t N = cfg.maxImages;
    rowCount_.alloc(N + 1);
    rowStart_.alloc(N + 1);
    rowLen_.alloc(N + 1);
    BF_REQUIRE(cfg.maxImages <= 16384, BF_ERR_CAPACITY, "maxImages > 16384 (LDS row histograms)");
    maxTiles_ = div_up(cfg.maxCorr, TILE);  // tiles at <= 256 images; tileCnt_ holds any n x div_up(nCorr, tile_for(n))
    maxChunks_ = div_up(2 * (size_t)cfg.maxCorr, (size_t)CH) + N;
    tileCnt_.alloc((size_t)maxTiles_ * std::min(N, 256u) + (size_t)cfg.maxCorr + N + TILE + 1);
    rowChunk_.alloc(N + 1);
    chunkRow_.alloc(maxChunks_ + 1);
    chunkPart_.alloc(3 * (size_t)maxChunks_ + 3);
    rowTmp_.alloc(2 * (size_t)cfg.maxCorr + 1);
    rowIdx_.alloc(2 * (size_t)cfg.maxCorr + 1);
    entries_.alloc(4 * (size_t)cfg.maxCorr + 2);
    vec_.alloc((size_t)V_NUM * N * 8);
    img_.alloc(2 * (size_t)N);
    T_.alloc((size_t)N * 16);
    Tinv_.alloc((size_t)N * 16);
    ctrl_.alloc(K_CTRL_WORDS);
    sync_.alloc(SYNC_WORDS);
    part_.alloc(2 * 4096);
    partIdx_.alloc(2 * 4096);
    pairs_.alloc(maxPairs_);
    pairW_.alloc(maxPairs_);
    pairBlk_.alloc((size_t)maxPairs_ * 36);
    diag_.alloc((size_t)N * 36);
    jtr_.alloc((size_t)N * 6);
    pairFlag_.alloc((size_t)N * N);
    pairAcc_.alloc((size_t)maxPairs_ * 54);
    pairProd_.alloc((size_t)N * 8);
    imgPairs_.alloc((size_t)N * N);
    imgPairN_.alloc(N);
    // assembled normal equations: a pair has >= 1 correspondence, so pairs <= min(N(N-1)/2, maxCorr)
    maxPairsA_ = (uint32_t)std::min<size_t>((size_t)N * (N - 1) / 2, (size_t)cfg.maxCorr);
    rowSorted_.alloc(2 * (size_t)cfg.maxCorr + 1);
    rowOther_.alloc(2 * (size_t)cfg.maxCorr + 1);
    rowSeg_.alloc(2 * (size_t)cfg.maxCorr + 1);
    rowDeg_.alloc(N + 1);
    rowNA_.alloc(N + 1);
    pairStart_.alloc(N + 1);
    rowPairStart_.alloc(N + 1);
    pairA_.alloc(maxPairsA_ + 1);
    pairB_.alloc(maxPairsA_ + 1);
    pairCorr_.alloc(maxPairsA_ + 1);
    rowPair_.alloc(2 * (size_t)maxPairsA_ + 1);
    pstat_.alloc(((size_t)maxPairsA_ + 1) * PSTAT);
    dstat_.alloc((size_t)N * DSTAT);
    apPair_.alloc((size_t)N * 8);
    aGran_.alloc((size_t)N * 12);  // [2][N][6]: sparse Ap rows, then the dense off-diagonal products
    fxGran_.alloc(16);
    rzPart_.alloc(N);
    poseBak_.alloc((size_t)N * 6);
    int dev = 0;
    hipDeviceProp_t prop;
    BF_HIP(hipGetDevice(&dev));
    BF_HIP(hipGetDeviceProperties(&prop, dev));
    numCUs_ = prop.multiProcessorCount;
    int occP = 0, occP8 = 0;
    BF_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occP, k_pcg_persist<2>, WG, 0));
    BF_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occP8, k_pcg_persist<2, PP_NF>, WG, 0));
    persistCapacity_ = (unsigned)std::max(std::min(occP, occP8), 0) * (unsigned)numCUs_;
    BF_HIP(hipMemsetAsync(vec_.p, 0, vec_.bytes(), stream_));
    BF_HIP(hipMemsetAsync(ctrl_.p, 0, ctrl_.bytes(), stream_));
    BF_HIP(hipMemsetAsync(sync_.p, 0, sync_.bytes(), stream_));
    BF_HIP(hipMemsetAsync(aGran_.p, 0, aGran_.bytes(), stream_));  // tag 0 is never awaited
    BF_HIP(hipMemsetAsync(fxGran_.p, 0, fxGran_.bytes(), stream_));
    BF_HIP(hipMemsetAsync(imgPairN_.p, 0, imgPairN_.bytes(), stream_));
    BF_HIP(hipMemsetAsync(rowCount_.p, 0, rowCount_.bytes(), stream_));
}

void Solver::setShard(uint32_t count, uint32_t index, Comm* comm) {
    BF_REQUIRE(count >= 1 && index < count, BF_ERR_ARG, "shard index / count");
    BF_REQUIRE(!comm || (comm->size() == (int)count && comm->rank() == (int)index), BF_ERR_ARG,
               "communicator size / rank must equal the shard count / index");
    shardCount_ = count;
    shardIndex_ = index;
    comm_ = comm;
}

uint32_t Solver::exportPairs(double* stats, int* pairAB, uint32_t cap) {
    BF_HIP(hipStreamSynchronize(stream_));
    uint32_t np = 0;
    if (lastPairMode_) BF_HIP(hipMemcpy(&np, ctrl_.p + K_NPAIRS_A, 4, hipMemcpyDeviceToHost));
    const uint32_t n = std::min(np, cap);
    if (n && stats) BF_HIP(hipMemcpy(stats, pstat_.p, sizeof(double) * PSTAT * n, hipMemcpyDeviceToHost));
    if (n && pairAB) {
        std::vector<int> A(n), B(n);
        BF_HIP(hipMemcpy(A.data(), pairA_.p, 4 * n, hipMemcpyDeviceToHost));
        BF_HIP(hipMemcpy(B.data(), pairB_.p, 4 * n, hipMemcpyDeviceToHost));
        for (uint32_t k = 0; k < n; k++) { pairAB[2 * k] = A[k]; pairAB[2 * k + 1] = B[k]; }
    }
    return np;
}

// the kernels' argument block of one solve (pairMode and pairBound are solve()'s)
BA Solver::makeArgs(const SolveArgs& s) const {
    BA a{};
    a.corr = s.corr; a.nCorr = s.numCorr; a.valid = s.valid; a.N = s.numImages; a.maxN = cfg_.maxImages; a.cap = maxCorrPerImage_;
    a.rowCount = rowCount_.p; a.rowStart = rowStart_.p; a.rowLen = rowLen_.p; a.rowTmp = rowTmp_.p; a.rowIdx = rowIdx_.p;
    a.entries = entries_.p; a.entTail = 2u * cfg_.maxCorr + 1u; a.vec = vec_.p; a.img = img_.p; a.T = T_.p; a.Tinv = Tinv_.p; a.ctrl = ctrl_.p;
    a.part = part_.p; a.partIdx = partIdx_.p; a.rot = s.rot; a.trans = s.trans;
    a.pairs = pairs_.p; a.pairW = pairW_.p; a.pairBlk = pairBlk_.p; a.diag = diag_.p; a.jtr = jtr_.p;
    a.pairFlag = pairFlag_.p; a.pairAcc = pairAcc_.p; a.pairProd = pairProd_.p; a.imgPairs = imgPairs_.p; a.imgPairN = imgPairN_.p;
    a.maxPairs = s.numImages * (s.numImages - 1) / 2;
    a.tileCnt = tileCnt_.p; a.tile = tile_for(s.numImages); a.nTiles = div_up(s.numCorr, a.tile);
    a.rowChunk = rowChunk_.p; a.chunkRow = chunkRow_.p; a.chunkPart = chunkPart_.p; a.sync = sync_.p;
    a.cache = s.cache; a.cw = s.cacheW; a.ch = s.cacheH;
    a.fx = s.intrinsics[0]; a.fy = s.intrinsics[1]; a.mx = s.intrinsics[2]; a.my = s.intrinsics[3];
    a.distT = cfg_.denseDistThresh; a.normT = cfg_.denseNormalThresh; a.colT = cfg_.denseColorThresh;
    a.gradMin = cfg_.denseColorGradientMin; a.dmin = cfg_.denseDepthMin; a.dmax = cfg_.denseDepthMax;
    a.sub = cfg_.denseOverlapSubsample ? cfg_.denseOverlapSubsample : 4;
    a.verifyT = cfg_.verifyOptDistThresh;
    a.rowSorted = rowSorted_.p; a.rowOther = rowOther_.p; a.rowSeg = rowSeg_.p; a.rowDeg = rowDeg_.p; a.rowNA = rowNA_.p;
    a.pairStart = pairStart_.p; a.rowPairStart = rowPairStart_.p; a.pairA = pairA_.p; a.pairB = pairB_.p;
    a.pairCorr = pairCorr_.p; a.rowPair = rowPair_.p; a.pstat = pstat_.p; a.dstat = dstat_.p;
    a.apPair = apPair_.p; a.rzPart = rzPart_.p;
    a.aGran = aGran_.p;
    a.fxGran = fxGran_.p;
    a.shardCount = shardCount_; a.shardIndex = shardIndex_; a.pairBound = 0;
    a.earlyOut = cfg_.earlyOut ? 1u : 0u;
    a.poseBak = poseBak_.p;
    a.spinTicks = cfg_.pcgSpinLimitUs ? 100ull * cfg_.pcgSpinLimitUs : PP_SPIN_TICKS;
    return a;
}

// the dense term of a GN step: overlapping image pairs, then their normal-equation blocks and per-image lists
void Solver::buildDense(const BA& a, float wD, float wC) {
    k_dense_reset<<<64, WG, 0, stream_>>>(a);
    k_dense_overlap<<<dim3(a.N, a.N), 64, 0, stream_>>>(a);
    k_dense_compact<<<1, 256, 0, stream_>>>(a);
    k_dense_count<<<std::min(a.maxPairs, (uint32_t)numCUs_ * 8), WG, 0, stream_>>>(a);
    k_dense_build<<<std::min(a.maxPairs, (uint32_t)numCUs_ * 4), WG, 0, stream_>>>(a, wD, wC);
    k_dense_lists<<<a.N, 64, 0, stream_>>>(a);
    BF_LAUNCH_CHECK();
}

// The PCG loop of a pair-mode GN step. Returns the finisher form (image rows per thread, 2 or 8) of a
// persistent launch, with which k_gn_end redoes a timed-out step; 0 when there was no persistent launch.
int Solver::launchPairPcg(const BA& a, const SolveArgs& s, float wS, bool dense, unsigned pairRowGrid) {
    if (s.numImages <= (uint32_t)SMALL_N) {
        if (s.nLin) k_pcg_small<<<1, SMALL_WG, 0, stream_>>>(a, wS, (int)s.nLin);
        return 0;
    }
    // one launch for the GN step's PCG loop when its grid is co-resident: up to 513 images
    // (one finisher workgroup, rows in registers, dense term included) with room to spare; up
    // to 2 017 sparse-only (config 4's 2 001 keyframes) with PP_NF finisher workgroups within
    // the occupancy query's capacity (persistent launches are serialized per device, below)
    const bool smallN = s.numImages <= 2u * WG + 1u;
    const unsigned nF = smallN ? 1u : (unsigned)PP_NF;
    const unsigned nW = div_up(s.numImages - 1u, (unsigned)(WG / 64));
    unsigned persistGrid = nF + nW;
    if (persistGrid > PP_SHADOW) persistGrid += nF;  // the row-less workgroups on the finishers' CUs
    const bool small = smallN && persistGrid * 2u <= persistCapacity_;
    // the PP_NF finishers own rows 1 .. 2 * PP_NF * WG: beyond that no finisher would tag a row's p
    const bool wide = !smallN && !dense && s.numImages <= 2u * (unsigned)PP_NF * WG + 1u && persistGrid <= persistCapacity_;
    if (cfg_.pcgLaunch != 0 || s.nLin >= 255u || !(small || wide)) {  // one launch per PCG iteration
        if (smallN)
            for (uint32_t li = 0; li < s.nLin; li++) k_pcg_pairs<2><<<pairRowGrid, WG, 0, stream_>>>(a, wS, (int)li, (int)s.nLin);
        else
            for (uint32_t li = 0; li < s.nLin; li++) k_pcg_pairs<8><<<pairRowGrid, WG, 0, stream_>>>(a, wS, (int)li, (int)s.nLin);
        return 0;
    }
    if (!s.nLin) return 0;
    // ranks of a loopback group (one GPU) issue their persistent launches in rank order
    struct Turn {
        Comm* c;
        explicit Turn(Comm* x) : c(x) { if (c) c->orderedLaunchBegin(); }
        ~Turn() { if (c) c->orderedLaunchEnd(); }
    } turn(comm_ && comm_->size() > 1 ? comm_ : nullptr);
    // persistent launches of every solver on this device run one at a time: two
    // partly resident persistent grids could each wait on the other's workgroups
    PersistGate& pg = persist_gate();
    std::lock_guard<std::mutex> lk(pg.mu);
    // always wait, on the same stream too: a destroyed solver's stream handle may be
    // reused by a new solver whose launch must still follow the old one (cheap in order)
    if (pg.ev) BF_HIP(hipStreamWaitEvent(stream_, pg.ev, 0));
    // dispatch-stamped events (pcgClock): the launch's own device time, for the in-loop
    // time per PCG iteration beside the standalone one
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const bool timed = pcgClock_.enabled();
    if (timed) pcgClock_.slot(e0, e1);
    if (small)
        hipExtLaunchKernelGGL(k_pcg_persist<2>, dim3(persistGrid), dim3(WG), 0, stream_, e0, e1, 0, a, wS, (int)s.nLin, pcgEpoch_);
    else
        hipExtLaunchKernelGGL((k_pcg_persist<2, PP_NF>), dim3(persistGrid), dim3(WG), 0, stream_, e0, e1, 0, a, wS, (int)s.nLin,
                              pcgEpoch_);
    BF_LAUNCH_CHECK();
    if (timed) pcgClock_.commit();
    if (!pg.ev) BF_HIP(hipEventCreateWithFlags(&pg.ev, hipEventDisableTiming));
    BF_HIP(hipEventRecord(pg.ev, stream_));
    pg.stream = stream_;
    pcgEpoch_ = (pcgEpoch_ + 1) & 0xFFFFFFu;
    return smallN ? 2 : 8;
}

// CUDASolverBundling::solve (CUDASolverBundling.cpp:187-284) -> solveBundlingStub (SolverBundling.cu:1137-1220)
void Solver::solve(const SolveArgs& s) {
    BF_REQUIRE(s.numImages > 1 && s.numImages <= cfg_.maxImages, BF_ERR_ARG, "numImages out of range");
    BF_REQUIRE(s.numCorr <= cfg_.maxCorr, BF_ERR_CAPACITY, "numCorr exceeds solver capacity");
    BF_REQUIRE(s.nNonLin > 0 && s.wSparse, BF_ERR_ARG, "nNonLin / weights");
    BA a = makeArgs(s);
    // assembled normal equations unless the matrix-free path is forced
    const bool pairMode = cfg_.normalEquations != 1;
    BF_REQUIRE(pairMode || shardCount_ == 1, BF_ERR_ARG, "sharded solves use the assembled normal equations");
    a.pairMode = pairMode ? 1u : 0u;
    lastPairMode_ = pairMode;

    const unsigned corrGrid = std::max(1u, std::min(div_up(s.numCorr, WG), (unsigned)numCUs_ * 8));
    // chunk kernels: one wave per chunk of CH row entries, up to 16 waves per CU
    const size_t chunkBound = div_up(2 * (size_t)s.numCorr, (size_t)CH) + s.numImages;
    const unsigned rowGrid = std::max(1u, std::min(div_up(chunkBound, (size_t)(WG / 64)), (unsigned)numCUs_ * 4));
    const bool timed = solveClock_.enabled();
    if (timed) solveClock_.start(stream_);
    k_solve_begin<<<1, 64, 0, stream_>>>(ctrl_.p, s.gate);
    BF_LAUNCH_CHECK();
    if (s.rebuildJT) {
        const size_t lds = sizeof(int) * s.numImages;
        if (a.nTiles) k_tile_count<<<a.nTiles, 64, lds, stream_>>>(a);
        k_tile_scan<<<s.numImages, WG, 0, stream_>>>(a);
        k_scan<<<1, WG, 0, stream_>>>(a);
        if (a.nTiles) k_tile_fill<<<a.nTiles, 64, lds, stream_>>>(a);
        k_compact_rows<<<s.numImages, WG, 0, stream_>>>(a);
        k_chunks<<<1, WG, 0, stream_>>>(a);
        BF_LAUNCH_CHECK();
        pairTable_ = false;
    }
    uint32_t bound = 0;
    if (pairMode) {
        if (!pairTable_) {
            k_pair_sort<<<s.numImages, WG, 0, stream_>>>(a);
            k_pair_scan<<<1, WG, 0, stream_>>>(a);
            k_pair_fill<<<s.numImages, 64, 0, stream_>>>(a);
            k_pair_rows<<<s.numImages, 64, 0, stream_>>>(a);
            BF_LAUNCH_CHECK();
            pairTable_ = true;
            pairCountHost_ = 0;
        }
        if (comm_ && comm_->size() > 1) {
            // the all-reduce count must be known on the host: the caller's bound, or the pair count
            // read back once per table build
            if (s.pairBound) {
                bound = s.pairBound;
            } else {
                if (!pairCountHost_) {
                    BF_HIP(hipMemcpyAsync(&pairCountHost_, ctrl_.p + K_NPAIRS_A, 4, hipMemcpyDeviceToHost, stream_));
                    BF_HIP(hipStreamSynchronize(stream_));
                }
                bound = std::max(pairCountHost_, 1u);
            }
            BF_REQUIRE(bound <= maxPairsA_, BF_ERR_CAPACITY, "pair bound exceeds the solver's pair capacity");
            a.pairBound = bound;
        }
    }
    if (pairMode) k_pair_gather<<<(unsigned)numCUs_ * 4, WG, 0, stream_>>>(a);
    const unsigned pairRowGrid = std::max(1u, std::min(div_up(s.numImages, WG / 64), (unsigned)numCUs_ * 4));
    bool transformsDone = false;
    for (uint32_t it = 0; it < s.nNonLin; it++) {
        const float wS = s.wSparse[it];
        const float wD = s.wDenseDepth ? s.wDenseDepth[it] : 0.0f;
        const float wC = s.wDenseColor ? s.wDenseColor[it] : 0.0f;
        const bool dense = (wD > 0.0f || wC > 0.0f) && s.cache != nullptr;
        // the next sparse pair-mode step's transforms come from this step's k_gn_end
        const bool nextDense = it + 1 < s.nNonLin && s.cache != nullptr &&
                               ((s.wDenseDepth && s.wDenseDepth[it + 1] > 0.0f) || (s.wDenseColor && s.wDenseColor[it + 1] > 0.0f));
        const float nextW = (pairMode && it + 1 < s.nNonLin && !nextDense && s.wSparse[it + 1] > 0.0f) ? s.wSparse[it + 1] : 0.0f;
        if (!transformsDone) k_transforms<<<div_up(s.numImages, 64), 64, 0, stream_>>>(a, wS, dense ? 1 : 0, 1, 1);
        transformsDone = nextW > 0.0f;
        if (pairMode) {
            if (dense) buildDense(a, wD, wC);
            k_pair_stats<<<(unsigned)numCUs_ * 4, WG, 0, stream_>>>(a);
            BF_LAUNCH_CHECK();
            if (comm_ && comm_->size() > 1) comm_->allreduceSum(pstat_.p, (size_t)bound * PSTAT, stream_);
            k_pair_init<<<pairRowGrid, WG, 0, stream_>>>(a, wS);
            const int recoverRB = launchPairPcg(a, s, wS, dense, pairRowGrid);  // k_gn_end redoes a timed-out persistent step
            BF_LAUNCH_CHECK();
            if (recoverRB == 2) k_gn_end<2><<<1, WG, 0, stream_>>>(a, (int)it, (int)s.nNonLin, wS, (int)s.nLin, nextW);
            else if (recoverRB == 8) k_gn_end<8><<<1, WG, 0, stream_>>>(a, (int)it, (int)s.nNonLin, wS, (int)s.nLin, nextW);
            else k_gn_end<0><<<1, WG, 0, stream_>>>(a, (int)it, (int)s.nNonLin, wS, (int)s.nLin, nextW);
            BF_LAUNCH_CHECK();
            continue;
        }
        if (dense) buildDense(a, wD, wC);
        k_entries<<<rowGrid, WG, 0, stream_>>>(a);
        k_init<<<rowGrid, WG, 0, stream_>>>(a, wS);
        BF_LAUNCH_CHECK();
        for (uint32_t li = 0; li < s.nLin; li++) k_pcg<<<rowGrid, WG, 0, stream_>>>(a, wS, (int)li, (int)s.nLin);
        BF_LAUNCH_CHECK();
        k_gn_end<0><<<1, WG, 0, stream_>>>(a, (int)it, (int)s.nNonLin, wS, (int)s.nLin, 0.0f);
        BF_LAUNCH_CHECK();
        transformsDone = false;
    }
    if (s.findMaxResidual) {
        // T from the final poses (ctrl untouched), then computeMaxResidual with the weightSparse of
        // the last GN iteration that ran (CUDASolverBundling.cpp:313-427)
        k_transforms<<<div_up(s.numImages, 64), 64, 0, stream_>>>(a, 0.0f, 0, 0, 0);
        k_residuals<<<corrGrid, WG, 0, stream_>>>(a);
        BF_LAUNCH_CHECK();
    }
    if (timed) solveClock_.stop(stream_);
}

SolveResult Solver::result() {
    uint32_t c[K_COUNT];
    BF_HIP(hipMemcpyAsync(c, ctrl_.p, sizeof(c), hipMemcpyDeviceToHost, stream_));
    BF_HIP(hipStreamSynchronize(stream_));
    return decodeResult(c);
}

void Solver::resultAsync(uint32_t* pinnedCtrl) {
    BF_HIP(hipMemcpyAsync(pinnedCtrl, ctrl_.p, sizeof(uint32_t) * K_COUNT, hipMemcpyDeviceToHost, stream_));
}

void Solver::removeMaxResidualAsync(BFEntryJ* corr, uint32_t n, int* valid, uint32_t numImages, float thresh) {
    k_pick_maxres_pair<<<1, 64, 0, stream_>>>(ctrl_.p, corr, thresh);
    BF_LAUNCH_CHECK();
    if (n) k_invalidate_picked_pair<<<std::max(1u, std::min(div_up(n, 256), 1024u)), 256, 0, stream_>>>(ctrl_.p, corr, n);
    k_check_frames_if_removed<<<div_up(numImages, 64), 64, 0, stream_>>>(ctrl_.p, rowCount_.p, valid, numImages);
    BF_LAUNCH_CHECK();
}

SolveResult Solver::decodeResult(const uint32_t* c) {
    SolveResult r{};
    r.gnIterations = c[K_GN_ITERS];
    r.pcgIterations = c[K_PCG_ITERS];
    std::memcpy(&r.maxResidual, &c[K_MAXRES], 4);
    r.maxResidualIndex = (int32_t)c[K_MAXIDX];
    std::memcpy(&r.energy, &c[K_ENERGY], 4);
    r.highResidualCount = c[K_HIGHCOUNT];
    r.numDensePairs = c[K_NPAIRS];
    r.error = c[K_ERROR];
    r.removedI = c[K_RM_I];
    r.removedJ = c[K_RM_J];
    r.skipped = c[K_SKIPPED];
    r.verifyUsed = c[K_VERIFY_USED];
    r.verifyOk = c[K_VERIFY_OK];
    return r;
}

void Solver::verify(const VerifyParams& p) {
    BF_REQUIRE(p.numImages >= 1 && p.numImages <= cfg_.maxImages, BF_ERR_ARG, "verify: numImages out of range");
    BF_REQUIRE(p.cache && p.T && p.valid, BF_ERR_ARG, "verify: trajectory, valid flags and cache frames are required");
    VerifyArgs v{};
    v.T = p.T; v.valid = p.valid; v.N = p.numImages; v.cache = p.cache; v.W = p.cacheW; v.H = p.cacheH;
    for (int k = 0; k < 16; k++) v.K[k] = 0.0f;  // mat4f intrinsics of the cache (CUDACache.cpp:20-24)
    v.K[0] = p.intrinsics[0]; v.K[2] = p.intrinsics[2];
    v.K[5] = p.intrinsics[1]; v.K[6] = p.intrinsics[3];
    v.K[10] = 1.0f; v.K[15] = 1.0f;
    v.distT = p.distThresh; v.normT = p.normalThresh; v.errT = p.errThresh; v.corrT = p.corrThresh;
    v.dmin = p.depthMin; v.dmax = p.depthMax; v.percentT = p.percentThresh;
    v.nCorr = p.numCorr; v.always = p.always ? 1u : 0u; v.ctrl = ctrl_.p; v.stats = p.pairStats;
    k_verify_begin<<<1, 64, 0, stream_>>>(v);
    if (p.numImages >= 2) k_verify_pairs<<<p.numImages * p.numImages, WG, 0, stream_>>>(v);
    BF_LAUNCH_CHECK();
}

const int* Solver::verifyFlag() const { return reinterpret_cast<const int*>(ctrl_.p + K_VERIFY_OK); }

void seed_keyframe(const float* localRot, const float* localTrans, uint32_t last, float* rot, float* trans, uint32_t s,
                   hipStream_t st, const int* gate) {
    k_seed_keyframe<<<1, 64, 0, st>>>(localRot, localTrans, last, rot, trans, s, gate);
    BF_LAUNCH_CHECK();
}
void set_gate(int* gate, const int* src, hipStream_t st) {
    k_set_gate<<<1, 64, 0, st>>>(gate, src);
    BF_LAUNCH_CHECK();
}
void invalidate_local(const int* gate, uint32_t s, int* valid, BFEntryJ* corr, uint32_t n, hipStream_t st) {
    k_invalidate_local<<<std::max(1u, std::min(div_up(n, 256), 1024u)), 256, 0, st>>>(gate, s, valid, corr, n);
    BF_LAUNCH_CHECK();
}

void matrices_to_poses(const float* T, uint32_t n, float* rot, float* trans, const int* valid, hipStream_t s) {
    if (!n) return;
    k_m2p<<<div_up(n, 64), 64, 0, s>>>(T, n, rot, trans, valid);
    BF_LAUNCH_CHECK();
}
void poses_to_matrices(const float* rot, const float* trans, uint32_t n, float* T, const int* valid, hipStream_t s) {
    if (!n) return;
    k_p2m<<<div_up(n, 64), 64, 0, s>>>(rot, trans, n, T, valid);
    BF_LAUNCH_CHECK();
}
void invalidate_image_pair(BFEntryJ* corr, uint32_t n, uint32_t i, uint32_t j, hipStream_t s) {
    if (!n) return;
    k_invalidate_pair<<<div_up(n, 128), 128, 0, s>>>(corr, n, i, j);
    BF_LAUNCH_CHECK();
}
void check_invalid_frames(const int* numEntries, int* valid, uint32_t numImages, BFEntryJ* corr, uint32_t nCorr,
                          bool comprehensive, hipStream_t s) {
    const uint32_t n = std::max(numImages, comprehensive ? nCorr : 0u);
    k_check_frames<<<std::max(1u, std::min(div_up(n, 256), 4096u)), 256, 0, s>>>(numEntries, valid, numImages, corr, nCorr,
                                                                                  comprehensive ? 1 : 0);
    BF_LAUNCH_CHECK();
}

}  // namespace bf
