// ba_dev.h — what every route of the bundle adjuster's kernels shares (included by ba.hip's route headers only).
// Launches no kernel. Holds the constants, the kernels' argument block (struct BA) and control words, the
// vector-field loads / stores, the fixed-order DPP wave and block sums, the write-through (sc1) hand-off
// primitives with the last-workgroup elections and the SYNC_* layout, the block scan, and the one definition
// of the PCG step that the PCG routes share (pcg_alpha / pcg_beta / pcg_last, pcg_iter_end).
// Relies on ba.h (Solver's constants, BFEntryJ; through it bf_math.h: f3, m4) and brings in lie.h, the
// 4x4 and pose maths every route uses (xf, pose_to_matrix, lie_update).
#pragma once
#include "ba.h"
#include "lie.h"
#include "wave.h"

namespace bf {
namespace {

constexpr float FLOAT_EPSILON = 0.000001f;  // Source/SolverUtil.h:9
constexpr int WG = 256;
static_assert(Solver::kSmallPersistImages == 2 * WG + 1, "the small persistent route (one finisher, 2 rows per thread)");
constexpr uint32_t TILE = 256;  // correspondences per table-build tile, per 256 images (a.tile)
// tile size for n images: the [n][nTiles] count matrix stays ~nCorr entries at any image count (a
// fixed 256 made it 8 x nCorr at 2 001 images: 955 us of strided count writes per solve)
__host__ __device__ constexpr uint32_t tile_for(uint32_t n) { return TILE * (n > 256u ? (n + 255u) / 256u : 1u); }
constexpr int CH = 512;        // row entries per chunk: the work unit of one wave in the GN/PCG kernels
constexpr int CPL = CH / 64;   // chunk entries per lane

enum VecField { V_DELTA = 0, V_R, V_Z, V_P, V_AP, V_M, V_NUM };
enum CtrlWord {
    K_TICKET = 0, K_PCG_DONE, K_GN_DONE, K_GN_ITERS, K_PCG_ITERS, K_RDOTZ, K_NPAIRS, K_LAST_W,
    K_MAXRES, K_MAXIDX, K_ENERGY, K_HIGHCOUNT, K_ERROR, K_USE_DENSE, K_RM_I, K_RM_J,
    K_SKIPPED,      // the solve's gate was 0: nothing ran (an invalidated local submap's global solve)
    K_VERIFY_USED,  // useVerification said yes: the dense pair check ran
    K_VERIFY_OK,    // VerifyTrajectoryCU's d_validOpt (1 unless a pair failed)
    K_COUNT,
    K_NCHUNK = K_COUNT, K_NPAIRS_A,
    K_PCG_ITERS0,  // K_PCG_ITERS before the GN step's PCG (k_pair_init): the timeout recovery (pcg_recover) restarts from it
    K_CTRL_WORDS = 32  // words past K_COUNT are solver-internal (not part of the result)
};
static_assert(K_COUNT == Solver::kResultWords, "result words");

struct BA {
    BFEntryJ* corr;
    uint32_t nCorr;
    const int* valid;
    uint32_t N, maxN, cap;
    int *rowCount, *rowStart, *rowLen, *rowTmp, *rowIdx;
    int* tileCnt;  // [N][nTiles]
    uint32_t nTiles, tile;
    int *rowChunk, *chunkRow;  // chunks of row v: [rowChunk[v], rowChunk[v+1]); chunk -> row
    float4* chunkPart;         // [chunk][3] per-chunk partial sums
    uint32_t* sync;            // last_block_sharded: 8 shard counters + top counter (+ flag words), 64 B apart
    float4* entries;
    float* vec;
    float* img;
    float* T;
    float* Tinv;
    uint32_t* ctrl;
    float* part;
    int* partIdx;
    float* rot;
    float* trans;
    uint2* pairs;
    float* pairW;
    float* pairBlk;
    float* diag;
    float* jtr;
    // dense term in a fixed order (no float atomics, so two solves of one problem agree bit for bit):
    uint32_t* pairFlag;  // [N][N] overlap flag of (i, j), i < j (k_dense_overlap)
    float* pairAcc;      // [maxPairs][54] a pair's J_i^T J_i | J_j^T J_j upper triangles (21 + 21), J_i^T r | J_j^T r
    float* pairProd;     // [N][8] per PCG iteration: image v's dense off-diagonal Ap rows [trans | rot]
    uint32_t* imgPairs;  // [N][N] pairs of image v in pair order: k << 1 | (v is the pair's j)
    uint32_t* imgPairN;  // [N]
    uint32_t maxPairs;
    const BFCachedFrame* cache;
    uint32_t cw, ch;
    float fx, fy, mx, my;
    float distT, normT, colT, gradMin, dmin, dmax, verifyT;
    uint32_t sub;
    // assembled normal equations (pair mode)
    int *rowSorted, *rowOther, *rowSeg, *rowDeg, *rowNA, *pairStart, *rowPairStart, *pairA, *pairB;
    int2 *pairCorr, *rowPair;
    uint32_t entTail;  // float4 offset of k_pair_gather's float2 tail in entries (2 maxCorr + 1)
    double *pstat, *dstat;
    float *apPair, *rzPart;
    uint2* aGran;  // [2][maxN][6] {value bits, tag}: k_pcg_persist's Ap hand-off
    uint2* fxGran; // [2][8] {block partial, tag}: the four-workgroup finisher's p.Ap / r.z partials
    uint32_t pairMode, shardCount, shardIndex, pairBound;
    uint32_t earlyOut;  // ENABLE_EARLY_OUT (SolverBundling.cu:7): PCG |p.Ap| < 5e-7 and GN max|delta| < 0.005 exits
    float* poseBak;     // [maxN][6] rot | trans at the GN step's start (k_pair_init), for the timeout recovery (pcg_recover)
    unsigned long long spinTicks;  // bound of every k_pcg_persist wait (s_memrealtime ticks, 100 MHz)
};

__device__ __forceinline__ float* vptr(const BA& a, int field, uint32_t v) { return a.vec + ((size_t)field * a.maxN + v) * 8; }
__device__ __forceinline__ void vload(const BA& a, int field, uint32_t v, f3& r, f3& t) {
    const float4* p = reinterpret_cast<const float4*>(vptr(a, field, v));
    float4 x = p[0], y = p[1];
    r = mk3(x.x, x.y, x.z);
    t = mk3(y.x, y.y, y.z);
}
__device__ __forceinline__ void vstore(const BA& a, int field, uint32_t v, f3 r, f3 t) {
    float4* p = reinterpret_cast<float4*>(vptr(a, field, v));
    p[0] = make_float4(r.x, r.y, r.z, 0.0f);
    p[1] = make_float4(t.x, t.y, t.z, 0.0f);
}
// Fixed-order wave sums (all 64 lanes active): adjacent lanes, quads, half rows and rows through DPP
// (after each step every lane of the group holds the same value, so the mirrors pair groups exactly as
// an xor butterfly would), then the four row sums as (r0 + r1) + (r2 + r3), read into scalars. Every
// lane returns the same value; no LDS round trips.
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true)); }
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_mov_dpp((int)(uint32_t)b, CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp((int)(uint32_t)(b >> 32), CTRL, 0xF, 0xF, true);
    return __longlong_as_double(((long long)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ float wave_sum(float v) {
    v += dpp_f<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp_f<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dpp_f<0x141>(v);  // row_half_mirror
    v += dpp_f<0x140>(v);  // row_mirror
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return (r0 + r1) + (r2 + r3);
}
__device__ __forceinline__ double readlane_d(double v, int l) {
    const long long b = __double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | lo);
}
__device__ __forceinline__ double wave_sum_d(double v) {  // wave_sum's order in fp64
    v += dpp_d<0xB1>(v);
    v += dpp_d<0x4E>(v);
    v += dpp_d<0x141>(v);
    v += dpp_d<0x140>(v);
    return (readlane_d(v, 0) + readlane_d(v, 16)) + (readlane_d(v, 32) + readlane_d(v, 48));
}
__device__ __forceinline__ float ctrlf(const uint32_t* c, int k) { return __uint_as_float(c[k]); }
__device__ __forceinline__ m4 loadm4(const float* p) {
    m4 m;
    const float4* q = reinterpret_cast<const float4*>(p);
    for (int r = 0; r < 4; r++) {
        float4 v = q[r];
        m.e[r * 4 + 0] = v.x; m.e[r * 4 + 1] = v.y; m.e[r * 4 + 2] = v.z; m.e[r * 4 + 3] = v.w;
    }
    return m;
}
__device__ __forceinline__ bool corr_valid(const BFEntryJ& e) { return e.imgIdx_i != BF_INVALID_IMAGE; }

// In-launch hand-offs (MI355X_MICROARCH.md §inter-workgroup visibility, "valid forms" row 1): the
// producer stores its payload write-through (sc1: 8-B agent-scope atomic stores to global memory),
// drains its stores (s_waitcnt vmcnt(0)) and then adds to an agent-scope counter; the adder that
// draws the last ticket reads the payload with sc1 loads (which bypass this CU's L1). No release or
// acquire fence is needed, so the hand-off costs no L2 write-back per wave.
typedef __attribute__((address_space(1))) uint64_t gu64;
typedef __attribute__((address_space(1))) uint32_t gu32;
__device__ __forceinline__ void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void st_wt(float4* p, float4 v) {
    gu64* q = (gu64*)(p);
    __hip_atomic_store(q, ((uint64_t)__float_as_uint(v.y) << 32) | __float_as_uint(v.x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(q + 1, ((uint64_t)__float_as_uint(v.w) << 32) | __float_as_uint(v.z), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float4 ld_wt(const float4* p) {
    gu64* q = (gu64*)(p);
    const uint64_t a = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t b = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return make_float4(__uint_as_float((uint32_t)a), __uint_as_float((uint32_t)(a >> 32)), __uint_as_float((uint32_t)b),
                       __uint_as_float((uint32_t)(b >> 32)));
}
__device__ __forceinline__ void st_wt(uint32_t* p, uint32_t v) { __hip_atomic_store((gu32*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t ld_wt(const uint32_t* p) { return __hip_atomic_load((gu32*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_wt(float* p, float v) { st_wt(reinterpret_cast<uint32_t*>(p), __float_as_uint(v)); }
// k_pcg_persist's flag word: {count, alpha bits} as one 8-B store / load (the workers get alpha with
// the flag instead of one more dependent load after it)
__device__ __forceinline__ void st_wt64(uint32_t* p, uint32_t lo, uint32_t hi) {
    __hip_atomic_store((gu64*)p, ((uint64_t)hi << 32) | lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t ld_wt64(const uint32_t* p) { return __hip_atomic_load((gu64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float ld_wtf(const float* p) { return __uint_as_float(ld_wt(reinterpret_cast<const uint32_t*>(p))); }
__device__ __forceinline__ uint32_t ticket_add(uint32_t* p) {
    return __hip_atomic_fetch_add((gu32*)p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Data-tagged granules for k_pcg_persist's Ap hand-off (MI355X_MICROARCH.md's handoff-1to1 row): one
// 8-B {value, tag} per float, written by ONE 8-B agent-scope atomic store and read by 8-B agent-scope
// atomic loads, so a granule is never torn and its tag says which iteration wrote it; the consumer
// polls the granules themselves (no drain, no arrival counter). Tags are epoch * 256 + iteration + 1:
// the epoch counts persistent launches on this solver, so no granule of an earlier launch matches.
// (Moving p to the workers the same way — 500 waves polling their partners' granules — ran 2x
// slower than the polled flag: the polls' load traffic swamps the hand-off.)
__device__ __forceinline__ void gran_store(uint2* g, float v, uint32_t tag) {
    __hip_atomic_store((gu64*)g, ((uint64_t)tag << 32) | __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t gran_load(const uint2* g) {
    return __hip_atomic_load((gu64*)g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// vector fields through write-through (WT) or plain accesses
template <bool WT>
__device__ __forceinline__ void vload_t(const BA& a, int field, uint32_t v, f3& r, f3& t) {
    if (WT) {
        const float4* p = reinterpret_cast<const float4*>(vptr(a, field, v));
        const float4 x = ld_wt(p), y = ld_wt(p + 1);
        r = mk3(x.x, x.y, x.z);
        t = mk3(y.x, y.y, y.z);
    } else {
        vload(a, field, v, r, t);
    }
}
template <bool WT>
__device__ __forceinline__ void vstore_t(const BA& a, int field, uint32_t v, f3 r, f3 t) {
    if (WT) {
        float4* p = reinterpret_cast<float4*>(vptr(a, field, v));
        st_wt(p, make_float4(r.x, r.y, r.z, 0.0f));
        st_wt(p + 1, make_float4(t.x, t.y, t.z, 0.0f));
    } else {
        vstore(a, field, v, r, t);
    }
}

// "Last workgroup" hand-off: every wave drains its write-through stores, one lane takes a ticket;
// the workgroup holding the last ticket continues (and reads the hand-off with ld_wt).
__device__ bool last_block(uint32_t* ticket) {
    __shared__ int isLast;
    drain_stores();
    __syncthreads();
    if (threadIdx.x == 0) isLast = (ticket_add(ticket) == gridDim.x * gridDim.y - 1) ? 1 : 0;
    __syncthreads();
    return isLast != 0;
}

// Two-level arrival for grid-wide hand-offs with many workgroups (MI355X_MICROARCH.md: one counter
// with hundreds of arrivers serialises at ~11 ns per atomic): workgroups are split into 8 shards by
// blockIdx % 8 (the dispatcher's round-robin XCD: a placement guess for speed only, correctness does
// not depend on it); a shard's last arriver adds to the top counter. Counters grow monotonically
// within a launch, so round `epoch` (1-based) completes at epoch * arrivers.
constexpr int SYNC_LINE = 16;  // words per 64-B line
constexpr int SYNC_TOP = 8 * SYNC_LINE, SYNC_ALPHA = 17 * SYNC_LINE;  // alpha: 256 words
// k_pcg_persist's flag in PP_NFLAG replicas 256 B apart (one per 64-word stride): 500 workgroups polling
// one word took 5.9 us from the finisher's store to the last of them seeing it (1.0 at 126)
constexpr int PP_NFLAG = 16, PP_FLAG_STRIDE = 64;
constexpr int SYNC_FLAGR = SYNC_ALPHA + 256;
constexpr int SYNC_WORDS = SYNC_FLAGR + PP_NFLAG * PP_FLAG_STRIDE + SYNC_LINE;
__device__ bool last_block_sharded(uint32_t* sync, uint32_t epoch) {
    __shared__ int isLast;
    drain_stores();
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t G = gridDim.x, sh = blockIdx.x & 7u;
        const uint32_t ns = (G + 7u - sh) / 8u, nShards = G < 8u ? G : 8u;
        int last = 0;
        if (ticket_add(&sync[sh * SYNC_LINE]) == epoch * ns - 1u) last = ticket_add(&sync[SYNC_TOP]) == epoch * nShards - 1u;
        isLast = last;
    }
    __syncthreads();
    return isLast != 0;
}

// deterministic block reduction of one float per thread: fixed butterfly per wave, then the wave
// sums in wave order
__device__ float block_sum(float v, float* sh) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = 0.0f;
    for (uint32_t w = 0; w < (blockDim.x >> 6); w++) r += sh[w];
    __syncthreads();
    return r;
}

// one workgroup of WG threads: exclusive scan of in[0, n) -> out[0, n), out[n] = total (sh: WG ints)
__device__ void block_exclusive_scan(const int* in, int* out, uint32_t n, int* sh) {
    int carry = 0;
    for (uint32_t base = 0; base < n; base += WG) {
        const uint32_t v = base + threadIdx.x;
        const int c = v < n ? in[v] : 0;
        sh[threadIdx.x] = c;
        __syncthreads();
        for (int off = 1; off < WG; off <<= 1) {
            const int x = (int)threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
            __syncthreads();
            sh[threadIdx.x] += x;
            __syncthreads();
        }
        if (v < n) out[v] = carry + sh[threadIdx.x] - c;
        carry += sh[WG - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[n] = carry;
    __syncthreads();
}

// ---- the PCG step, defined once for every route (PCGIteration, SolverBundling.cu:1024-1108) -----
// The routes (k_pcg, k_pcg_pairs, both k_pcg_persist finishers, pcg_recover, k_pcg_small) must agree bit
// for bit, so the scalars of an iteration come from here: the step size alpha of Kernel1b
// (SolverBundling.cu:959), beta of Kernel3 (:997), and the exit test: the last of nLin iterations, or the
// ENABLE_EARLY_OUT test of the host loop on p.Ap (:1089-1092).
// Two things stay written out where they are used, because a shared helper changed the register allocation
// of the kernels around them: pcg_last's test in pcg_finish_regs and pcg_finisher (ba_pcg.h), and the Lie
// update of a pose on the exiting iteration (lie_update on a.rot / a.trans) in every route.
__device__ __forceinline__ float pcg_alpha(float rz, float pAp) { return (pAp > FLOAT_EPSILON) ? rz / pAp : 0.0f; }
__device__ __forceinline__ float pcg_beta(float rzNew, float rz) { return (rz > FLOAT_EPSILON) ? rzNew / rz : 0.0f; }
__device__ __forceinline__ bool pcg_last(const BA& a, int it, int nLin, float pAp) {
    return (it == nLin - 1) || (a.earlyOut && fabsf(pAp) < 5e-7f);
}
// What one thread of the finisher leaves behind an iteration of the per-launch routes (k_pcg, k_pcg_pairs):
// the new r.z, one more iteration, the loop's end, and last_block's ticket at 0 for the launches that follow.
// pcg_recover's iterations have no ticket to clear and keep their own three stores. `last` by reference:
// k_pcg_pairs<8> gets it from a call through memory, and a copy changed that kernel's registers.
__device__ __forceinline__ void pcg_iter_end(const BA& a, float rDotzNew, const bool& last) {
    a.ctrl[K_RDOTZ] = __float_as_uint(rDotzNew);
    a.ctrl[K_PCG_ITERS]++;
    if (last) a.ctrl[K_PCG_DONE] = 1;
    a.ctrl[K_TICKET] = 0;
}

}  // namespace
}  // namespace bf
