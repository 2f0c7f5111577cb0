// match.hip — the sparse matcher: descriptor matching, the Kabsch, surface-area and dense-verify filters, to EntryJ.
// Restates the matching side of SIFTImageManager + SiftMatchCU + Bundler::matchAndFilter (paths relative to
// FriedLiver/Source/):
//   Bundler.cpp:103-249, SiftGPU/ProgramCU.cu:1634-1936 (MultiplyDescriptor / RowMatch / ColMatch),
//   SiftGPU/SIFTImageManager.cu:59-607, 610-687, SiftGPU/SIFTImageManager.cpp:44-83, 551-575,
//   SiftGPU/cuda_kabsch.h:73-229, 281-502, SiftGPU/cuda_surfaceArea.h, SiftGPU/cuda_SVD.h:17-213,
//   SiftGPU/cuda_EigenValue.h:56-85.
// The DoG detector / descriptor is sift.hip, tryRevalidation is the bundler's (bundler.hip); fuseToGlobal is
// match_fuse.h, included at the end.
//
// k_match — one workgroup (4 waves) per image pair (prev, cur), every pair of a call in one launch. The reference
// writes the num1 x num2 int32 dot matrix to memory and reduces it with two more kernels per pair; here it never
// leaves the registers:
//   * dot[a][b] = sum_k prev[a][k] * cur[b][k] on v_mfma_i32_32x32x32_i8. The instruction is signed and the
//     descriptors are unsigned bytes, so it is fed d - 128 (d ^ 0x80) and the exact unsigned dot is restored with
//     sum ab = sum (a-128)(b-128) + 128 (sum a + sum b) - 128 * 16384 from per-descriptor byte sums (all int32).
//     Both operands of a k-step are 16 contiguous bytes of a descriptor at the same offset, so the k order inside
//     the instruction cancels; the row / column maps are A: row = lane & 31, B: col = lane & 31,
//     D: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
//   * cur's descriptors sit in LDS in chunks of 512 columns (64 KB, 16-byte units XOR-swizzled by column); a wave
//     owns the 32-row strips w, w + 4, ... of prev (A fragments in 16 VGPRs from global memory) and walks the
//     chunk's column tiles.
//   * best / second best / argument per ROW: per lane over its column of every tile, then a butterfly over the 32
//     lanes of a strip half, merged into an LDS row table (a strip's rows belong to one wave). Per COLUMN: per
//     lane over its 16 rows into a per-wave, per-lane-half LDS table, merged over the 8 tables after each chunk.
//     Ties go to the lowest index and the second best then equals the best (RowMatch_Kernel's strict >).
//   * acceptance, mutual check, and the raw list ordered by (dot descending, cur key ascending), first 128 kept:
//     the one deliberate departure from the reference, which appends in race order (atomicAdd) before its sort
//     and keeps an arbitrary 128 of more; the count written is the true number of mutual matches.
// k_filter — one wave per pair, lane 0 runs filterKeyPointMatches' greedy loop (the reference runs it on one
// thread too); Kabsch's 3x3 SVD and the covariance eigenvalues use a double-precision Jacobi iteration.
// k_surface_area — one wave per pair, lanes 0..31 as the reference's warp; k_dense_verify + k_dense_decide — row slices x
// pairs, sums in a fixed order (the comments at the kernels).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/bf/bf.h"
#include "bf_math.h"
#include "bf_runtime.h"
#include "match.h"
#include "match_dev.h"
#include "wave.h"

namespace bf {

namespace {

constexpr int MATCH_WG = 256;
constexpr uint32_t MAXK = BF_MATCH_MAX_KEYS_PER_IMAGE;  // rows / columns of one pair
constexpr uint32_t CHUNK = 512;                         // columns of cur resident in LDS
constexpr uint32_t RAW = BF_MAX_MATCHES_RAW, FILT = BF_MAX_MATCHES_FILTERED;
constexpr uint32_t DBG_MAX = Matcher::kDbg;
// LDS (ints): descriptors, per-wave column tables, column table, row table, scratch
constexpr uint32_t LDS_DESC = CHUNK * 32, LDS_COLW = 3 * 4 * 2 * CHUNK, LDS_COL = 3 * MAXK, LDS_ROW = 3 * MAXK, LDS_MISC = 8;
constexpr size_t MATCH_LDS_BYTES = 4 * (size_t)(LDS_DESC + LDS_COLW + LDS_COL + LDS_ROW + LDS_MISC);
static_assert(MATCH_LDS_BYTES <= 160 * 1024, "k_match's LDS exceeds a gfx950 workgroup's 160 KB");

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

struct MatchArgs {
    const uint8_t* descs;
    const int32_t* sums;
    const uint32_t* table;  // per image {offset, count, valid, 0}
    uint32_t cur, start;
    float thresh, ratio;
    uint32_t* rawCount;
    uint2* rawIdx;
    float* rawDist;
    const uint32_t* dbgSel;  // rows[32], cols[32]
    int32_t* dbgOut;         // dots[32 * 32], rowStats[3 * 32]
    uint32_t dbgRows, dbgCols;
};

// (best, next, arg) <- merged with (b2, n2, a2): ties on best go to the lower index, next = best then
__device__ __forceinline__ void merge3(int& b, int& n, int& a, int b2, int n2, int a2) {
    const bool second = b2 > b || (b2 == b && (uint32_t)a2 < (uint32_t)a);
    const int lo = min(b, b2);
    n = max(lo, max(n, n2));
    b = max(b, b2);
    a = second ? a2 : a;
}

__device__ __forceinline__ float match_dist(int dot) {
    return acosf(fminf((float)dot * 0.000003814697265625f, 1.0f));  // 2^-18 (RowMatch_Kernel, ProgramCU.cu:1824)
}

__device__ __forceinline__ v4i flip128(int4 v) {
    v4i r;
    r.x = v.x ^ (int)0x80808080;
    r.y = v.y ^ (int)0x80808080;
    r.z = v.z ^ (int)0x80808080;
    r.w = v.w ^ (int)0x80808080;
    return r;
}

template <bool DBG>
__global__ __launch_bounds__(MATCH_WG) void k_match(MatchArgs A) {
    extern __shared__ int4 smem4[];
    v4i* sDesc = (v4i*)smem4;
    int* sColW = (int*)smem4 + LDS_DESC;
    int* sCol = sColW + LDS_COLW;
    int* sRow = sCol + LDS_COL;
    uint32_t* sMisc = (uint32_t*)(sRow + LDS_ROW);  // the scan's wave totals

    const uint32_t prev = A.start + blockIdx.x;
    if (prev == A.cur) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t l31 = lane & 31, h = lane >> 5;
    const uint32_t prevOff = A.table[4 * prev], nPrev = A.table[4 * prev + 1], prevValid = A.table[4 * prev + 2];
    const uint32_t curOff = A.table[4 * A.cur], nCur = A.table[4 * A.cur + 1];
    uint2* oIdx = A.rawIdx + (size_t)prev * RAW;
    float* oDist = A.rawDist + (size_t)prev * RAW;
    if (!prevValid || nPrev == 0 || nCur == 0 || nPrev > MAXK || nCur > MAXK) {  // workgroup-uniform
        if (tid < RAW) {
            oIdx[tid] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
            oDist[tid] = 999.0f;
        }
        if (tid == 0) A.rawCount[prev] = 0;
        return;
    }

    for (uint32_t k = tid; k < MAXK; k += MATCH_WG) {
        sRow[k] = 0;
        sRow[MAXK + k] = 0;
        sRow[2 * MAXK + k] = -1;
    }
    const uint32_t nRowTiles = (nPrev + 31) / 32;
    const int4* gPrev = (const int4*)A.descs + (size_t)prevOff * 8;
    const int4* gCur = (const int4*)A.descs + (size_t)curOff * 8;
    const int32_t* sumPrev = A.sums + prevOff;
    const int32_t* sumCur = A.sums + curOff;

    for (uint32_t c0 = 0; c0 < nCur; c0 += CHUNK) {
        const uint32_t chunkCols = min(CHUNK, ((nCur - c0) + 31u) & ~31u);
        const uint32_t nColTiles = chunkCols / 32;
        __syncthreads();  // the previous chunk's tables are merged, its descriptors no longer read
        for (uint32_t u = tid; u < chunkCols * 8; u += MATCH_WG) {
            const uint32_t cl = u >> 3, p = u & 7, col = c0 + cl;
            v4i v = {0, 0, 0, 0};
            if (col < nCur) v = flip128(gCur[(size_t)col * 8 + p]);
            sDesc[cl * 8 + (p ^ (cl & 7))] = v;
        }
        for (uint32_t k = lane; k < 2 * CHUNK; k += 64) {  // this wave's two column tables
            sColW[(0 * 4 + wave) * 2 * CHUNK + k] = 0;
            sColW[(1 * 4 + wave) * 2 * CHUNK + k] = 0;
            sColW[(2 * 4 + wave) * 2 * CHUNK + k] = -1;
        }
        __syncthreads();

        for (uint32_t rs = wave; rs < nRowTiles; rs += 4) {
            // A fragments: row rs * 32 + (lane & 31), bytes [32 s + 16 h, + 16) of k-step s
            const uint32_t arow = rs * 32 + l31;
            v4i a[4];
#pragma unroll
            for (int s = 0; s < 4; s++) {
                a[s] = v4i{0, 0, 0, 0};
                if (arow < nPrev) a[s] = flip128(gPrev[(size_t)arow * 8 + 2 * s + h]);
            }
            // this lane's 16 rows of the accumulator tile
            int rterm[16], rb[16], rn[16], ra[16];
            uint32_t rmask = 0;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const uint32_t row = rs * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                const bool ok = row < nPrev;
                rterm[i] = ok ? 128 * sumPrev[row] : 0;
                rmask |= ok ? (1u << i) : 0u;
                rb[i] = 0;
                rn[i] = 0;
                ra[i] = -1;
            }
            for (uint32_t ct = 0; ct < nColTiles; ct++) {
                const uint32_t cl = ct * 32 + l31, col = c0 + cl;
                v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int s = 0; s < 4; s++) {
                    const v4i b = sDesc[cl * 8 + ((2 * s + h) ^ (cl & 7))];
                    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], b, acc, 0, 0, 0);
                }
                const bool colOk = col < nCur;
                const int cterm = colOk ? 128 * sumCur[col] - 128 * 16384 : 0;
                const uint32_t ci = (wave * 2 + h) * CHUNK + cl;
                int cb = sColW[ci], cn = sColW[4 * 2 * CHUNK + ci], ca = sColW[2 * 4 * 2 * CHUNK + ci];
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const int row = (int)(rs * 32 + (i & 3) + 8 * (i >> 2) + 4 * h);
                    int v = acc[i] + rterm[i] + cterm;
                    v = (colOk && ((rmask >> i) & 1u)) ? v : 0;  // a padded row / column never beats the initial 0
                    if constexpr (DBG) {
                        for (uint32_t r = 0; r < A.dbgRows; r++)
                            for (uint32_t c = 0; c < A.dbgCols; c++)
                                if (A.dbgSel[r] == (uint32_t)row && A.dbgSel[DBG_MAX + c] == col) A.dbgOut[r * A.dbgCols + c] = v;
                    }
                    // row statistics (columns arrive in ascending order: strict > keeps the lowest index)
                    const bool tr = v > rb[i];
                    rn[i] = tr ? rb[i] : max(rn[i], v);
                    ra[i] = tr ? (int)col : ra[i];
                    rb[i] = tr ? v : rb[i];
                    // column statistics (rows arrive in ascending order)
                    const bool tc = v > cb;
                    cn = tc ? cb : max(cn, v);
                    ca = tc ? row : ca;
                    cb = tc ? v : cb;
                }
                sColW[ci] = cb;
                sColW[4 * 2 * CHUNK + ci] = cn;
                sColW[2 * 4 * 2 * CHUNK + ci] = ca;
            }
            // rows: butterfly over the 32 lanes (columns) of this half, then into the row table
#pragma unroll
            for (int step = 1; step < 32; step <<= 1) {
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const int b2 = __shfl_xor(rb[i], step), n2 = __shfl_xor(rn[i], step), a2 = __shfl_xor(ra[i], step);
                    merge3(rb[i], rn[i], ra[i], b2, n2, a2);
                }
            }
#pragma unroll
            for (int i = 0; i < 16; i++) {
                if (l31 == (uint32_t)i) {
                    const uint32_t row = rs * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;  // < MAXK
                    int b = sRow[row], n = sRow[MAXK + row], ar = sRow[2 * MAXK + row];  // earlier chunks: lower columns
                    merge3(b, n, ar, rb[i], rn[i], ra[i]);
                    sRow[row] = b;
                    sRow[MAXK + row] = n;
                    sRow[2 * MAXK + row] = ar;
                }
            }
        }
        __syncthreads();
        // columns of this chunk: merge the 4 waves x 2 halves
        for (uint32_t cl = tid; cl < chunkCols; cl += MATCH_WG) {
            int b = 0, n = 0, ar = -1;
            for (uint32_t t = 0; t < 8; t++) {
                const uint32_t ci = t * CHUNK + cl;
                merge3(b, n, ar, sColW[ci], sColW[4 * 2 * CHUNK + ci], sColW[2 * 4 * 2 * CHUNK + ci]);
            }
            sCol[c0 + cl] = b;
            sCol[MAXK + c0 + cl] = n;
            sCol[2 * MAXK + c0 + cl] = ar;
        }
    }
    __syncthreads();

    if constexpr (DBG) {
        if (tid < A.dbgRows) {
            const uint32_t row = A.dbgSel[tid];
            for (int k = 0; k < 3; k++) A.dbgOut[DBG_MAX * DBG_MAX + 3 * tid + k] = row < MAXK ? sRow[k * MAXK + row] : 0;
        }
    }

    // acceptance per row (GetRowMatch): result index or -1, and the row's distance
    int* rowRes = sColW;                        // [MAXK]
    float* rowDist = (float*)(sColW + MAXK);    // [MAXK]
    for (uint32_t r = tid; r < nPrev; r += MATCH_WG) {
        const float dist = match_dist(sRow[r]), distn = match_dist(sRow[MAXK + r]);
        rowRes[r] = (dist < A.thresh && dist < distn * A.ratio) ? sRow[2 * MAXK + r] : -1;
        rowDist[r] = dist;
    }
    __syncthreads();

    // mutual matches in column order (GetColMatch): thread t owns columns 4 t .. 4 t + 3
    int* mDot = (int*)sDesc;                 // [MAXK]
    int* mA = mDot + MAXK;
    int* mB = mA + MAXK;
    float* mDist = (float*)(mB + MAXK);
    int fa[4];
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t b = 4 * tid + j;
        fa[j] = -1;
        if (b < nCur) {
            const float dist = match_dist(sCol[b]), distn = match_dist(sCol[MAXK + b]);
            const int f1 = (dist < A.thresh && dist < distn * A.ratio) ? sCol[2 * MAXK + b] : -1;
            if (f1 >= 0 && rowRes[f1] == (int)b) {
                fa[j] = f1;
                mine++;
            }
        }
    }
    uint32_t total;
    uint32_t at = wg_exclusive_scan<MATCH_WG / 64>(mine, sMisc, total);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (fa[j] >= 0) {
            mDot[at] = sRow[fa[j]];
            mA[at] = fa[j];
            mB[at] = (int)(4 * tid + j);
            mDist[at] = rowDist[fa[j]];
            at++;
        }
    }
    __syncthreads();
    // order: dot descending, then cur key ascending (the list is in cur key order); keep the first 128
    for (uint32_t j = tid; j < total; j += MATCH_WG) {
        const int d = mDot[j];
        uint32_t rank = 0;
        for (uint32_t k = 0; k < total; k++) rank += (mDot[k] > d || (mDot[k] == d && k < j)) ? 1u : 0u;
        if (rank < RAW) {
            oIdx[rank] = make_uint2(prevOff + (uint32_t)mA[j], curOff + (uint32_t)mB[j]);
            oDist[rank] = mDist[j];
        }
    }
    if (tid < RAW && tid >= total) {
        oIdx[tid] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        oDist[tid] = 999.0f;
    }
    if (tid == 0) A.rawCount[prev] = total;
}

// byte sum of every descriptor of an image
__global__ void k_desc_sums(const uint8_t* descs, int32_t* sums, uint32_t first, uint32_t n) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint4* d = (const uint4*)(descs + (size_t)(first + k) * 128);
    uint32_t s = 0;
    for (int i = 0; i < 8; i++) {
        const uint4 v = d[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        for (int j = 0; j < 4; j++) s += (w[j] & 0xFF) + ((w[j] >> 8) & 0xFF) + ((w[j] >> 16) & 0xFF) + (w[j] >> 24);
    }
    sums[first + k] = (int32_t)s;
}

// ---- FilterKeyPointMatchesCU ------------------------------------------------------------------------------
struct FilterArgs {
    const BFSiftKeyPoint* keys;
    const uint32_t* rawCount;
    const uint2* rawIdx;
    const float* rawDist;
    uint32_t* filtCount;
    uint2* filtIdx;
    float* filtDist;
    float* T;
    float* Tinv;
    float kinv[16];
    uint32_t cur, start, minNumMatches;
    float maxRes2;
};

// xform3 / key_point (a key's camera-space point): match_dev.h

// cyclic Jacobi on a symmetric 3x3: a -> diagonal (eigenvalues), V's columns the eigenvectors
__device__ void jacobi3(double a[3][3], double V[3][3]) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 12; sweep++) {
        const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
        if (off == 0.0) break;
#pragma unroll
        for (int pq = 0; pq < 3; pq++) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            if (a[p][q] == 0.0) continue;
            const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double akp = a[k][p], akq = a[k][q];
                a[k][p] = c * akp - s * akq;
                a[k][q] = s * akp + c * akq;
            }
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double apk = a[p][k], aqk = a[q][k];
                a[p][k] = c * apk - s * aqk;
                a[q][k] = s * apk + c * aqk;
            }
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double vkp = V[k][p], vkq = V[k][q];
                V[k][p] = c * vkp - s * vkq;
                V[k][q] = s * vkp + c * vkq;
            }
        }
    }
}

// largest / second eigenvalue of the covariance of n points (covarianceSVD, cuda_kabsch.h:213-229)
__device__ double cov_ratio(const float* pts, uint32_t n) {
    double m[3] = {0, 0, 0};
    for (uint32_t i = 0; i < n; i++)
        for (int r = 0; r < 3; r++) m[r] += (double)pts[3 * i + r];
    for (int r = 0; r < 3; r++) m[r] /= (double)n;
    double C[3][3] = {};
    for (uint32_t i = 0; i < n; i++) {
        const double d[3] = {pts[3 * i] - m[0], pts[3 * i + 1] - m[1], pts[3 * i + 2] - m[2]};
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) C[r][c] += d[r] * d[c];
    }
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) C[r][c] /= (double)n;
    double V[3][3];
    jacobi3(C, V);
    double e0 = C[0][0], e1 = C[1][1], e2 = C[2][2], t;
    if (e0 < e1) { t = e0; e0 = e1; e1 = t; }
    if (e1 < e2) { t = e1; e1 = e2; e2 = t; }
    if (e0 < e1) { t = e0; e0 = e1; e1 = t; }
    return e0 / e1;
}

// kabsch (cuda_kabsch.h:73-211): rigid transform src -> tgt; *c1 = largest / second singular value of the
// cross-covariance. The reflection case flips the direction of the smallest singular value.
__device__ void kabsch(const float* src, const float* tgt, uint32_t n, float* T, double* c1) {
    double p0[3] = {0, 0, 0}, q0[3] = {0, 0, 0};
    for (uint32_t i = 0; i < n; i++)
        for (int r = 0; r < 3; r++) {
            p0[r] += (double)src[3 * i + r];
            q0[r] += (double)tgt[3 * i + r];
        }
    for (int r = 0; r < 3; r++) {
        p0[r] /= (double)n;
        q0[r] /= (double)n;
    }
    double H[3][3] = {};
    for (uint32_t i = 0; i < n; i++) {
        const double dp[3] = {src[3 * i] - p0[0], src[3 * i + 1] - p0[1], src[3 * i + 2] - p0[2]};
        const double dq[3] = {tgt[3 * i] - q0[0], tgt[3 * i + 1] - q0[1], tgt[3 * i + 2] - q0[2]};
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) H[r][c] += dp[r] * dq[c];
    }
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) H[r][c] /= (double)n;
    // H = U S W^T: W from the eigenvectors of H^T H, U = H W / S
    double M[3][3], W[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) M[i][j] = H[0][i] * H[0][j] + H[1][i] * H[1][j] + H[2][i] * H[2][j];
    jacobi3(M, W);
    double ev[3] = {M[0][0], M[1][1], M[2][2]};
    int o0 = 0, o1 = 1, o2 = 2, ti;
    if (ev[o0] < ev[o1]) { ti = o0; o0 = o1; o1 = ti; }
    if (ev[o1] < ev[o2]) { ti = o1; o1 = o2; o2 = ti; }
    if (ev[o0] < ev[o1]) { ti = o0; o0 = o1; o1 = ti; }
    double w1[3], w2[3], w3[3], u1[3], u2[3], u3[3];
    for (int r = 0; r < 3; r++) {
        w1[r] = o0 == 0 ? W[r][0] : (o0 == 1 ? W[r][1] : W[r][2]);
        w2[r] = o1 == 0 ? W[r][0] : (o1 == 1 ? W[r][1] : W[r][2]);
    }
    const double l1 = o0 == 0 ? ev[0] : (o0 == 1 ? ev[1] : ev[2]), l2 = o1 == 0 ? ev[0] : (o1 == 1 ? ev[1] : ev[2]);
    *c1 = sqrt(fmax(l1, 0.0)) / sqrt(fmax(l2, 0.0));
    for (int r = 0; r < 3; r++) {
        u1[r] = H[r][0] * w1[0] + H[r][1] * w1[1] + H[r][2] * w1[2];
        u2[r] = H[r][0] * w2[0] + H[r][1] * w2[1] + H[r][2] * w2[2];
    }
    double n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
    if (n1 > 0.0) {
        for (int r = 0; r < 3; r++) u1[r] /= n1;
    } else {
        u1[0] = 1.0; u1[1] = 0.0; u1[2] = 0.0;
    }
    double d12 = u2[0] * u1[0] + u2[1] * u1[1] + u2[2] * u1[2];
    for (int r = 0; r < 3; r++) u2[r] -= d12 * u1[r];
    double n2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
    if (n2 > 1e-150) {
        for (int r = 0; r < 3; r++) u2[r] /= n2;
    } else {  // rank <= 1 (rejected by the condition test): any unit vector orthogonal to u1
        const int m = fabs(u1[0]) <= fabs(u1[1]) ? (fabs(u1[0]) <= fabs(u1[2]) ? 0 : 2) : (fabs(u1[1]) <= fabs(u1[2]) ? 1 : 2);
        double e[3] = {m == 0 ? 1.0 : 0.0, m == 1 ? 1.0 : 0.0, m == 2 ? 1.0 : 0.0};
        d12 = e[0] * u1[0] + e[1] * u1[1] + e[2] * u1[2];
        for (int r = 0; r < 3; r++) u2[r] = e[r] - d12 * u1[r];
        n2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
        for (int r = 0; r < 3; r++) u2[r] /= n2;
    }
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1]; u3[1] = u1[2] * u2[0] - u1[0] * u2[2]; u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    w3[0] = w1[1] * w2[2] - w1[2] * w2[1]; w3[1] = w1[2] * w2[0] - w1[0] * w2[2]; w3[2] = w1[0] * w2[1] - w1[1] * w2[0];
    double R[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) R[r][c] = w1[r] * u1[c] + w2[r] * u2[c] + w3[r] * u3[c];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T[4 * r + c] = (float)R[r][c];
        T[4 * r + 3] = (float)(q0[r] - (R[r][0] * p0[0] + R[r][1] * p0[1] + R[r][2] * p0[2]));
    }
    T[12] = 0.0f; T[13] = 0.0f; T[14] = 0.0f; T[15] = 1.0f;
}

struct FilterLds {
    uint2 idx[RAW];
    float dist[RAW];
    float src[3 * FILT], tgt[3 * FILT], res[FILT];
};

// ComputeReprojection (cuda_kabsch.h:380-412)
__device__ bool compute_reprojection(FilterLds& L, uint32_t n, float* T) {
    double c1;
    kabsch(L.src, L.tgt, n, T, &c1);
    for (uint32_t i = 0; i < n; i++) {
        float p[3];
        xform3(T, L.src[3 * i], L.src[3 * i + 1], L.src[3 * i + 2], p);
        const float dx = p[0] - L.tgt[3 * i], dy = p[1] - L.tgt[3 * i + 1], dz = p[2] - L.tgt[3 * i + 2];
        L.res[i] = dx * dx + dy * dy + dz * dz;
    }
    // sortKabschResiduals: exchange sort, points / indices / distances along
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t j = i; j < n; j++)
            if (L.res[i] > L.res[j]) {
                float t = L.res[i]; L.res[i] = L.res[j]; L.res[j] = t;
                for (int r = 0; r < 3; r++) {
                    t = L.src[3 * i + r]; L.src[3 * i + r] = L.src[3 * j + r]; L.src[3 * j + r] = t;
                    t = L.tgt[3 * i + r]; L.tgt[3 * i + r] = L.tgt[3 * j + r]; L.tgt[3 * j + r] = t;
                }
                const uint2 ti = L.idx[i]; L.idx[i] = L.idx[j]; L.idx[j] = ti;
                t = L.dist[i]; L.dist[i] = L.dist[j]; L.dist[j] = t;
            }
    const double cp = cov_ratio(L.src, n), cq = cov_ratio(L.tgt, n);
    if (isnan(c1) || isnan(cp) || isnan(cq) || fabs(c1) > 100.0 || fabs(cp) > 100.0 || fabs(cq) > 100.0) return false;
    return true;
}

// filterKeyPointMatches (cuda_kabsch.h:422-502) on the raw list in L (sorted by distance); returns the kept count
__device__ uint32_t filter_matches(FilterLds& L, const BFSiftKeyPoint* keys, uint32_t numRaw, float* T, const float* kinv,
                                   uint32_t minNumMatches, float maxRes) {
    uint32_t idx = 0, cur = 0;
    float curMaxResidual = 100.0f;
    bool validTransform = false;
    for (int k = 0; k < 16; k++) T[k] = (k % 5 == 0) ? 1.0f : 0.0f;
    while (true) {
        if (idx == numRaw || cur >= FILT) {
            if (cur < minNumMatches || curMaxResidual >= maxRes || !validTransform) cur = 0;
            break;
        }
        // addMatch (cuda_kabsch.h:281-295): 5-pixel rejection against the kept matches in either image
        const uint2 add = L.idx[idx];
        bool ok = true;
        {
            const BFSiftKeyPoint ai = keys[add.x], aj = keys[add.y];
            for (uint32_t i = 0; i < cur && ok; i++) {
                const BFSiftKeyPoint ki = keys[L.idx[i].x], kj = keys[L.idx[i].y];
                const float dix = ai.x - ki.x, diy = ai.y - ki.y, djx = aj.x - kj.x, djy = aj.y - kj.y;
                if (sqrtf(dix * dix + diy * diy) <= 5.0f || sqrtf(djx * djx + djy * djy) <= 5.0f) ok = false;
            }
        }
        if (ok) {
            L.idx[cur] = add;
            L.dist[cur] = L.dist[idx];
            cur++;
            if (cur >= 3) {
                for (uint32_t i = 0; i < cur; i++) {
                    key_point(kinv, keys[L.idx[i].x], &L.src[3 * i]);
                    key_point(kinv, keys[L.idx[i].y], &L.tgt[3 * i]);
                }
                validTransform = compute_reprojection(L, cur, T);
                const bool b = validTransform;
                float prevT[16];
                for (int k = 0; k < 16; k++) prevT[k] = T[k];
                curMaxResidual = L.res[cur - 1];
                if (curMaxResidual > maxRes) {  // some bad matches: remove the largest until below
                    float lastRes = -1.0f;
                    const int startIdx = (int)cur - 1;
                    for (int i = startIdx; i >= 3; i--) {
                        lastRes = L.res[i];
                        cur--;
                        validTransform = compute_reprojection(L, cur, T);
                        curMaxResidual = L.res[cur - 1];
                        if (cur == 3 && (curMaxResidual > maxRes || (b && !validTransform))) {
                            cur++;  // removing made it worse: restore
                            curMaxResidual = lastRes;
                            validTransform = b;
                            for (int k = 0; k < 16; k++) T[k] = prevT[k];
                            break;
                        }
                        if (curMaxResidual < maxRes) break;
                    }
                }
            }
        }
        idx++;
    }
    return cur;
}

__global__ __launch_bounds__(64) void k_filter(FilterArgs A) {
    __shared__ FilterLds L;
    __shared__ uint32_t sKept;
    __shared__ float sT[16];
    const uint32_t prev = A.start + blockIdx.x;
    if (prev == A.cur) return;
    const uint32_t tid = threadIdx.x;
    const uint32_t numRaw = min(RAW, A.rawCount[prev]);
    for (uint32_t k = tid; k < RAW; k += 64) {
        L.idx[k] = k < numRaw ? A.rawIdx[(size_t)prev * RAW + k] : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        L.dist[k] = k < numRaw ? A.rawDist[(size_t)prev * RAW + k] : 999.0f;
    }
    __syncthreads();
    if (tid == 0) {
        float T[16];
        for (int k = 0; k < 16; k++) T[k] = (k % 5 == 0) ? 1.0f : 0.0f;
        sKept = numRaw ? filter_matches(L, A.keys, numRaw, T, A.kinv, A.minNumMatches, A.maxRes2) : 0u;
        for (int k = 0; k < 16; k++) sT[k] = T[k];
    }
    __syncthreads();
    const uint32_t kept = sKept;
    if (tid == 0) A.filtCount[prev] = kept;
    if (tid < FILT) {
        A.filtIdx[(size_t)prev * FILT + tid] = tid < kept ? L.idx[tid] : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        A.filtDist[(size_t)prev * FILT + tid] = tid < kept ? L.dist[tid] : 999.0f;
    }
    if (tid < 16) A.T[16 * (size_t)prev + tid] = sT[tid];
    if (tid < 16) {  // rigid inverse [R^T | -R^T t]
        const uint32_t r = tid >> 2, c = tid & 3;
        float v;
        if (r == 3) {
            v = c == 3 ? 1.0f : 0.0f;
        } else if (c < 3) {
            v = sT[4 * c + r];
        } else {
            v = (float)(-((double)sT[r] * sT[3] + (double)sT[4 + r] * sT[7] + (double)sT[8 + r] * sT[11]));
        }
        A.Tinv[16 * (size_t)prev + tid] = v;
    }
}

// ---- AddCurrToResidualsCU ---------------------------------------------------------------------------------
__global__ __launch_bounds__(32) void k_add_residuals(const BFSiftKeyPoint* keys, const uint32_t* filtCount, const uint2* filtIdx,
                                                      const uint32_t* base, uint32_t cur, uint32_t start, BFEntryJ* out,
                                                      uint32_t* keyIdx, uint32_t cap, const float* kinvDev) {
    const uint32_t prev = start + blockIdx.x;
    if (prev == cur) return;
    const uint32_t n = filtCount[prev], t = threadIdx.x, at = base[prev] + t;
    if (t >= n || at >= cap) return;
    const uint2 ij = filtIdx[(size_t)prev * FILT + t];
    float kinv[16];
    for (int k = 0; k < 16; k++) kinv[k] = kinvDev[k];
    float pi[3], pj[3];
    key_point(kinv, keys[ij.x], pi);
    key_point(kinv, keys[ij.y], pj);
    BFEntryJ e;
    e.imgIdx_i = prev;
    e.imgIdx_j = cur;
    e.pos_i.x = pi[0]; e.pos_i.y = pi[1]; e.pos_i.z = pi[2];
    e.pos_j.x = pj[0]; e.pos_j.y = pj[1]; e.pos_j.z = pj[2];
    out[at] = e;
    if (keyIdx) {
        keyIdx[2 * (size_t)at] = ij.x;
        keyIdx[2 * (size_t)at + 1] = ij.y;
    }
}

// ---- FilterMatchesBySurfaceAreaCU (SIFTImageManager.cu:318-389, cuda_surfaceArea.h) ------------------------------
// The reference's block is one 32-thread warp, thread t owns match t; here lanes 0..31 of the wave play that warp
// (lanes 32..63 carry the neutral element), so every sum / min / max is the reference's __shfl_down tree; lane 0's
// result goes to the whole wave, which keeps control flow uniform.
__device__ __forceinline__ float tree_sum32(float v) {
    for (int off = 16; off > 0; off >>= 1) v += __shfl_down(v, off, 32);
    return __shfl(v, 0);
}
__device__ __forceinline__ float tree_min32(float v) {
    for (int off = 16; off > 0; off >>= 1) v = fminf(v, __shfl_down(v, off, 32));
    return __shfl(v, 0);
}
__device__ __forceinline__ float tree_max32(float v) {
    for (int off = 16; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off, 32));
    return __shfl(v, 0);
}

// MYEIGEN::jacobi<3> (cuda_SVD.h:138-213), float32: the Numerical-Recipes cyclic sweep (0,1), (0,2), (1,2), threshold
// 0.2 sm / 9 in sweeps 1-3, at most 50 sweeps. a: upper triangle used; d: eigenvalues; v: rotations accumulated in
// its COLUMNS. False when 50 sweeps do not converge.
__device__ bool jacobi3f(float a[3][3], float d[3], float v[3][3]) {
    float b[3], z[3];
    for (int ip = 0; ip < 3; ip++) {
        for (int iq = 0; iq < 3; iq++) v[ip][iq] = 0.0f;
        v[ip][ip] = 1.0f;
    }
    for (int ip = 0; ip < 3; ip++) {
        b[ip] = d[ip] = a[ip][ip];
        z[ip] = 0.0f;
    }
    for (int i = 1; i <= 50; i++) {
        const float sm = (fabsf(a[0][1]) + fabsf(a[0][2])) + fabsf(a[1][2]);
        if (sm == 0.0f) return true;
        const float tresh = i < 4 ? 0.2f * sm / 9.0f : 0.0f;
#pragma unroll
        for (int pq = 0; pq < 3; pq++) {
            const int ip = pq == 2 ? 1 : 0, iq = pq == 0 ? 1 : 2;
            const float g = 100.0f * fabsf(a[ip][iq]);
            if (i > 4 && fabsf(d[ip]) + g == fabsf(d[ip]) && fabsf(d[iq]) + g == fabsf(d[iq])) {
                a[ip][iq] = 0.0f;
            } else if (fabsf(a[ip][iq]) > tresh) {
                float h = d[iq] - d[ip], t;
                if (fabsf(h) + g == fabsf(h)) {
                    t = a[ip][iq] / h;
                } else {
                    const float theta = 0.5f * h / a[ip][iq];
                    t = 1.0f / (fabsf(theta) + sqrtf(1.0f + theta * theta));
                    if (theta < 0.0f) t = -t;
                }
                const float c = 1.0f / sqrtf(1.0f + t * t), s = t * c, tau = s / (1.0f + c);
                h = t * a[ip][iq];
                z[ip] -= h;
                z[iq] += h;
                d[ip] -= h;
                d[iq] += h;
                a[ip][iq] = 0.0f;
                // ROTATE(a, i, j, k, l): g = a[i][j], h = a[k][l]; a[i][j] = g - s (h + g tau); a[k][l] = h + s (g - h tau)
                const int j = 3 - ip - iq;  // the one remaining index of a 3x3
                {
                    float* x = j < ip ? &a[j][ip] : &a[ip][j];
                    float* y = j < iq ? &a[j][iq] : &a[iq][j];
                    const float gg = *x, hh = *y;
                    *x = gg - s * (hh + gg * tau);
                    *y = hh + s * (gg - hh * tau);
                }
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const float gg = v[k][ip], hh = v[k][iq];
                    v[k][ip] = gg - s * (hh + gg * tau);
                    v[k][iq] = hh + s * (gg - hh * tau);
                }
            }
        }
        for (int ip = 0; ip < 3; ip++) {
            b[ip] += z[ip];
            d[ip] = b[ip];
            z[ip] = 0.0f;
        }
    }
    return false;
}

// MYEIGEN::eigenSystem (cuda_SVD.h:69-125): ev[i] = ROW i of the rotation matrix (:95-100), although jacobi leaves
// the eigenvectors in its columns; then a selection sort by |eigenvalue| descending that moves those rows along.
// Restated as the reference computes it: s_surfAreaPcaThresh was tuned against this.
__device__ bool eigen_system3(const float V[3][3], float ev[3][3]) {
    float a[3][3], d[3], v[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) a[i][j] = V[j][i];
    if (!jacobi3f(a, d, v)) return false;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) ev[i][j] = v[i][j];
    for (int i = 0; i < 3; i++) {
        float curMax = 0.0f;
        int at = -1;
        for (int j = i; j < 3; j++)
            if (fabsf(d[j]) > curMax) {
                curMax = fabsf(d[j]);
                at = j;
            }
        if (at != i && at != -1) {
            float t = d[i]; d[i] = d[at]; d[at] = t;
            for (int j = 0; j < 3; j++) {
                t = ev[i][j]; ev[i][j] = ev[at][j]; ev[at][j] = t;
            }
        }
    }
    return true;
}

// area of one side of a pair (which = 0 prev, 1 cur); every lane returns the same value
__device__ float surface_area_side(const BFSiftKeyPoint* keys, const uint2* idx, uint32_t n, const float* kinv, uint32_t which,
                                   uint32_t lane) {
    const bool mine = lane < n;
    float pt[3] = {0.0f, 0.0f, 0.0f};
    if (mine) {
        const uint2 ij = idx[lane];
        key_point(kinv, keys[which ? ij.y : ij.x], pt);
    }
    // computeKeyPointMatchesCovariance
    float mean[3], V[3][3];
    for (int r = 0; r < 3; r++) mean[r] = tree_sum32(pt[r]) / (float)n;
    const float dl[3] = {pt[0] - mean[0], pt[1] - mean[1], pt[2] - mean[2]};
    for (int r = 0; r < 3; r++)
        for (int c = r; c < 3; c++) V[r][c] = V[c][r] = tree_sum32(mine ? dl[r] * dl[c] : 0.0f) / (float)n;
    float ev[3][3];
    if (!eigen_system3(V, ev)) return 0.0f;
    // projectKeysToPlane: onto the plane through the mean orthogonal to ev[2], in the (ev[0], ev[1]) frame
    float px = 0.0f, py = 0.0f;
    if (mine) {
        const float k = (ev[2][0] * dl[0] + ev[2][1] * dl[1]) + ev[2][2] * dl[2];
        const float s[3] = {(pt[0] - k * ev[2][0]) - mean[0], (pt[1] - k * ev[2][1]) - mean[1], (pt[2] - k * ev[2][2]) - mean[2]};
        px = (s[0] * ev[0][0] + s[1] * ev[0][1]) + s[2] * ev[0][2];
        py = (s[0] * ev[1][0] + s[1] * ev[1][1]) + s[2] * ev[1][2];
    }
    // computeAreaOrientedBoundingBox2: computeCovariance2d, computeEigenValues / computeEigenVector (2x2)
    const float mx = tree_sum32(px) / (float)n, my = tree_sum32(py) / (float)n;
    const float ex = px - mx, ey = py - my;
    const float cxx = tree_sum32(mine ? ex * ex : 0.0f) / (float)n, cxy = tree_sum32(mine ? ex * ey : 0.0f) / (float)n,
                cyy = tree_sum32(mine ? ey * ey : 0.0f) / (float)n;
    const float disc = 0.5f * sqrtf((cxx - cyy) * (cxx - cyy) + 4.0f * cxy * cxy);
    const float lam[2] = {(cxx + cyy) / 2.0f + disc, (cxx + cyy) / 2.0f - disc};
    float ax[2][2];
    for (int k = 0; k < 2; k++) {
        float vx = -cxy, vy = cxx - lam[k];
        const float mag = sqrtf(vx * vx + vy * vy);
        vx /= mag;
        vy /= mag;
        const float inv = 1.0f / sqrtf(vx * vx + vy * vy);  // normalize(): v * rsqrtf(dot(v, v))
        ax[k][0] = vx * inv;
        ax[k][1] = vy * inv;
    }
    const float qx = ax[0][0] * px + ax[0][1] * py, qy = ax[1][0] * px + ax[1][1] * py;
    const float minX = tree_min32(mine ? qx : 3.402823466e+38f), minY = tree_min32(mine ? qy : 3.402823466e+38f);
    const float maxX = tree_max32(mine ? qx : -3.402823466e+38f), maxY = tree_max32(mine ? qy : -3.402823466e+38f);
    const float extX = maxX - minX, extY = maxY - minY;
    if (extX < 0.00001f || extY < 0.00001f) return 0.0f;
    return extX * extY;
}

__global__ __launch_bounds__(64) void k_surface_area(const BFSiftKeyPoint* keys, uint32_t* filtCount, const uint2* filtIdx,
                                                     const uint32_t* table, const float* kinvDev, float* area, uint32_t cur,
                                                     uint32_t start, float areaThresh) {
    const uint32_t prev = start + blockIdx.x;
    if (prev == cur) return;
    const uint32_t n = min(filtCount[prev], FILT);
    if (n == 0) return;
    if (!table[4 * prev + 2]) return;
    float kinv[16];
    for (int k = 0; k < 16; k++) kinv[k] = kinvDev[k];
    const uint32_t lane = threadIdx.x;
    const uint2* idx = filtIdx + (size_t)prev * FILT;
    const float a0 = surface_area_side(keys, idx, n, kinv, 0, lane);
    const float a1 = surface_area_side(keys, idx, n, kinv, 1, lane);
    if (lane == 0) {
        area[2 * (size_t)prev] = a0;
        area[2 * (size_t)prev + 1] = a1;
        if (a0 < areaThresh && a1 < areaThresh) filtCount[prev] = 0;
    }
}

// ---- FilterMatchesByDenseVerifyCU (SIFTImageManager.cu:417-607) ----------------------------------------------
// The reference runs one block of W x ceil(H / 32) threads per pair, which caps W ceil(H / 32) at 1 024 and leaves a
// local matcher's <= 10 pairs on 10 CUs. Here a pair's rows are cut into DV_SLICES slices, one 256-thread workgroup
// each (grid = slices x pairs); a thread takes pixels t, t + 256, ... of its slice, both directions of a pixel as the
// reference's thread does, two pixels at a time so that four gathers are in flight before the first is used. Sums:
// per thread in pixel order, per direction; the __shfl_down tree per wave; waves 0..3; k_dense_decide then adds the
// slices 0, 1, ... in order. The reference adds warp sums with shared-memory float atomics in race order: this
// fixed order is the stage's one deliberate departure, results are bit-deterministic.
constexpr uint32_t DV_SLICES = Matcher::kSlices, DV_WG = 256, DV_UNROLL = 2;

struct DenseArgs {
    const BFCachedFrame* frames;
    uint32_t* filtCount;
    const float* T;
    const float* Tinv;
    const uint32_t* table;
    float* partial;  // [maxImages][DV_SLICES][6]
    float* sums;     // [maxImages][6]
    uint32_t cur, start, n, W, H, rowsPerSlice, nSlices;
    float K[16];
    float distT, normT, errT, corrT, dmin, dmax;
};

struct DenseProbe {
    float4 pT;
    float nx, ny, nz;
    uint32_t t;  // target pixel (0 when !ok: any frame has pixel 0)
    bool ok;
};

// computeProjError up to the bounds test (SIFTImageManager.cu:433-451)
__device__ __forceinline__ DenseProbe dense_probe(const DenseArgs& A, const float* tr, float4 pIn, float4 nIn, float dIn, bool live) {
    DenseProbe P;
    P.t = 0;
    P.ok = false;
    nIn.w = 0.0f;
    P.pT = make_float4(tr[0] * pIn.x + tr[1] * pIn.y + tr[2] * pIn.z + tr[3] * pIn.w, tr[4] * pIn.x + tr[5] * pIn.y + tr[6] * pIn.z + tr[7] * pIn.w,
                       tr[8] * pIn.x + tr[9] * pIn.y + tr[10] * pIn.z + tr[11] * pIn.w,
                       tr[12] * pIn.x + tr[13] * pIn.y + tr[14] * pIn.z + tr[15] * pIn.w);
    P.nx = tr[0] * nIn.x + tr[1] * nIn.y + tr[2] * nIn.z + tr[3] * nIn.w;
    P.ny = tr[4] * nIn.x + tr[5] * nIn.y + tr[6] * nIn.z + tr[7] * nIn.w;
    P.nz = tr[8] * nIn.x + tr[9] * nIn.y + tr[10] * nIn.z + tr[11] * nIn.w;
    if (!(live && pIn.x != -INFINITY && nIn.x != -INFINITY && dIn >= A.dmin && dIn <= A.dmax)) return P;
    const float* K = A.K;
    const float qx = K[0] * P.pT.x + K[1] * P.pT.y + K[2] * P.pT.z + K[3] * 1.0f;
    const float qy = K[4] * P.pT.x + K[5] * P.pT.y + K[6] * P.pT.z + K[7] * 1.0f;
    const float qz = K[8] * P.pT.x + K[9] * P.pT.y + K[10] * P.pT.z + K[11] * 1.0f;
    const int sx = f2i(roundf(qx / qz)), sy = f2i(roundf(qy / qz));
    if (!(sx >= 0 && sy >= 0 && sx < (int)A.W && sy < (int)A.H)) return P;  // the gather below is inside the image
    P.t = (uint32_t)sy * A.W + (uint32_t)sx;
    P.ok = true;
    return P;
}

// ... and from the gathered target on (:452-486): (residual, weight, 1) is added to s[0..2]
__device__ __forceinline__ void dense_accept(const DenseArgs& A, const DenseProbe& P, float4 pTg, float4 nTg, float tgtDepth, float* s) {
    if (!(P.ok && pTg.x != -INFINITY && nTg.x != -INFINITY)) return;
    const float dx = P.pT.x - pTg.x, dy = P.pT.y - pTg.y, dz = P.pT.z - pTg.z, dw = P.pT.w - pTg.w;
    const float d = sqrtf(dx * dx + dy * dy + dz * dz + dw * dw);  // length(float4)
    const float dN = P.nx * nTg.x + P.ny * nTg.y + P.nz * nTg.z;
    if (!(tgtDepth >= A.dmin && tgtDepth <= A.dmax)) return;
    const bool bad = (tgtDepth != -INFINITY && P.pT.z < tgtDepth) && d > A.distT;  // known bad match
    if (!((dN >= A.normT && d <= A.distT) || bad)) return;
    const float camZ = (P.pT.z - A.dmin) / (A.dmax - A.dmin);
    const float w = fmaxf(0.0f, 0.5f * ((1.0f - d / A.distT) + (1.0f - camZ)));
    s[0] += d;
    s[1] += w;
    s[2] += 1.0f;
}

__global__ __launch_bounds__(DV_WG) void k_dense_verify(DenseArgs A) {
    __shared__ float sh[6][DV_WG / 64];
    const uint32_t prev = A.start + blockIdx.y, slice = blockIdx.x;
    if (prev == A.cur) return;
    if (A.filtCount[prev] == 0) return;
    if (!A.table[4 * prev + 2]) return;
    const uint32_t tid = threadIdx.x;
    const uint32_t row0 = slice * A.rowsPerSlice, row1 = min(A.H, row0 + A.rowsPerSlice);  // row0 < H: nSlices slices
    const uint32_t first = row0 * A.W, npix = (row1 - row0) * A.W;
    float T[16], Ti[16];
    for (int k = 0; k < 16; k++) {
        T[k] = A.T[16 * (size_t)prev + k];
        Ti[k] = A.Tinv[16 * (size_t)prev + k];
    }
    const BFCachedFrame fp = A.frames[prev], fc = A.frames[A.cur];
    if (!fp.depth || !fp.campos || !fp.normals || !fc.depth || !fc.campos || !fc.normals) {  // no frame: no correspondence
        if (tid < 6) A.partial[((size_t)prev * DV_SLICES + slice) * 6 + tid] = 0.0f;
        return;
    }
    const float4* pos[2] = {(const float4*)fp.campos, (const float4*)fc.campos};
    const float4* nrm[2] = {(const float4*)fp.normals, (const float4*)fc.normals};
    const float* dep[2] = {fp.depth, fc.depth};
    float s[2][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
    for (uint32_t p0 = tid; p0 < npix; p0 += DV_WG * DV_UNROLL) {
        DenseProbe P[DV_UNROLL][2];
#pragma unroll
        for (uint32_t u = 0; u < DV_UNROLL; u++) {
            const uint32_t p = p0 + u * DV_WG;
            const bool live = p < npix;
            const uint32_t idx = first + (live ? p : 0u);
#pragma unroll
            for (int dir = 0; dir < 2; dir++)  // 0: prev's pixel into cur by T; 1: cur's pixel into prev by Tinv
                P[u][dir] = dense_probe(A, dir ? Ti : T, pos[dir][idx], nrm[dir][idx], dep[dir][idx], live);
        }
        float4 gp[DV_UNROLL][2], gn[DV_UNROLL][2];
        float gd[DV_UNROLL][2];
#pragma unroll
        for (uint32_t u = 0; u < DV_UNROLL; u++)
#pragma unroll
            for (int dir = 0; dir < 2; dir++) {
                const uint32_t t = P[u][dir].t;
                gp[u][dir] = pos[1 - dir][t];
                gn[u][dir] = nrm[1 - dir][t];
                gd[u][dir] = dep[1 - dir][t];
            }
#pragma unroll
        for (uint32_t u = 0; u < DV_UNROLL; u++)
#pragma unroll
            for (int dir = 0; dir < 2; dir++) dense_accept(A, P[u][dir], gp[u][dir], gn[u][dir], gd[u][dir], s[dir]);
    }
    float v[6] = {s[0][0], s[0][1], s[0][2], s[1][0], s[1][1], s[1][2]};
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int q = 0; q < 6; q++) v[q] += __shfl_down(v[q], off);
    if ((tid & 63) == 0)
        for (int q = 0; q < 6; q++) sh[q][tid >> 6] = v[q];
    __syncthreads();
    if (tid < 6) A.partial[((size_t)prev * DV_SLICES + slice) * 6 + tid] = ((sh[tid][0] + sh[tid][1]) + sh[tid][2]) + sh[tid][3];
}

// one thread per pair: slices in order, then the reference's verdict (SIFTImageManager.cu:572-584)
__global__ __launch_bounds__(64) void k_dense_decide(DenseArgs A) {
    const uint32_t prev = A.start + blockIdx.x * 64 + threadIdx.x;
    if (prev >= A.n || prev == A.cur) return;
    if (A.filtCount[prev] == 0) return;
    if (!A.table[4 * prev + 2]) return;
    float s[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t sl = 0; sl < A.nSlices; sl++)
        for (int q = 0; q < 6; q++) s[q] += A.partial[((size_t)prev * DV_SLICES + sl) * 6 + q];
    for (int q = 0; q < 6; q++) A.sums[6 * (size_t)prev + q] = s[q];
    const float err = (s[0] + s[3]) / (s[1] + s[4]);
    const float corr = 0.5f * (s[2] + s[5]) / (float)(A.W * A.H);
    if (corr < A.corrT || err > A.errT || isnan(err)) A.filtCount[prev] = 0;
}

}  // namespace

MatcherConfig make_matcher_config(const BFMatcherOptions* o) {
    BF_REQUIRE(o != nullptr, BF_ERR_ARG, "null matcher options");
    BF_REQUIRE(o->maxImages > 0 && o->maxKeysPerImage > 0, BF_ERR_ARG, "matcher capacity: maxImages / maxKeysPerImage are 0");
    BF_REQUIRE(o->maxKeysPerImage <= BF_MATCH_MAX_KEYS_PER_IMAGE, BF_ERR_ARG, "maxKeysPerImage above 1024");
    BF_REQUIRE((uint64_t)o->maxImages * o->maxKeysPerImage <= (1ull << 28), BF_ERR_ARG, "matcher capacity too large");
    BF_REQUIRE(std::isfinite(o->matchThresh) && std::isfinite(o->ratioMax) && std::isfinite(o->maxKabschRes2) &&
                   o->matchThresh >= 0.0f && o->ratioMax >= 0.0f && o->maxKabschRes2 >= 0.0f,
               BF_ERR_ARG, "matcher options: non-finite or negative threshold");
    MatcherConfig c;
    c.maxImages = o->maxImages;
    c.maxKeys = o->maxKeysPerImage;
    c.matchThresh = o->matchThresh > 0.0f ? o->matchThresh : 0.7f;
    c.ratioMax = o->ratioMax > 0.0f ? o->ratioMax : 0.8f;
    c.minNumMatches = o->minNumMatches ? o->minNumMatches : 5u;
    c.maxKabschRes2 = o->maxKabschRes2 > 0.0f ? o->maxKabschRes2 : 0.0004f;
    bool any = false;
    for (int k = 0; k < 16; k++) {
        BF_REQUIRE(std::isfinite(o->intrinsicsInv[k]), BF_ERR_ARG, "matcher options: non-finite intrinsicsInv");
        any = any || o->intrinsicsInv[k] != 0.0f;
        c.kinv[k] = o->intrinsicsInv[k];
    }
    if (!any)
        for (int k = 0; k < 16; k++) c.kinv[k] = (k % 5 == 0) ? 1.0f : 0.0f;
    BF_REQUIRE(o->fuseMaxCorr <= (1u << 28), BF_ERR_ARG, "fuseMaxCorr above 2^28");
    c.fuseMaxCorr = o->fuseMaxCorr;
    return c;
}

Matcher::Matcher(const MatcherConfig& cfg, hipStream_t stream) : cfg_(cfg), stream_(stream) {
    const size_t keys = (size_t)cfg.maxImages * cfg.maxKeys, n = cfg.maxImages;
    keys_.alloc(keys);
    descs_.alloc(keys * 128);
    sums_.alloc(keys);
    table_.alloc(4 * n);
    rawCount_.alloc(n);
    filtCount_.alloc(n);
    rawIdx_.alloc(n * kRaw);
    rawDist_.alloc(n * kRaw);
    filtIdx_.alloc(n * kFilt);
    filtDist_.alloc(n * kFilt);
    T_.alloc(16 * n);
    Tinv_.alloc(16 * n);
    base_.alloc(n + 16);  // + intrinsicsInv (16 floats) behind the bases
    dbgSel_.alloc(2 * kDbg);
    dbgOut_.alloc(kDbg * kDbg + 3 * kDbg);
    area_.alloc(2 * n);
    denseSums_.alloc(6 * n);
    densePartial_.alloc(6 * n * kSlices);
    BF_HIP(hipHostMalloc((void**)&hostTable_, 4 * n * sizeof(uint32_t), hipHostMallocDefault));
    BF_HIP(hipHostMalloc((void**)&hostCounts_, n * sizeof(uint32_t), hipHostMallocDefault));
    BF_HIP(hipHostMalloc((void**)&hostBase_, (n + 16) * sizeof(uint32_t), hipHostMallocDefault));
    if (cfg.fuseMaxCorr) {
        const size_t rec = cfg.fuseMaxCorr, comps = keys < rec ? keys : rec;  // a component holds a record of its own
        fuseCnt_.alloc(keys);
        fuseOff_.alloc(keys + 1);
        fusePar_.alloc(keys);
        fuseRoot_.alloc(keys);
        fuseRank_.alloc(keys);
        fuseGood_.alloc(keys);
        fuseEdge_.alloc(rec);
        fuseAdj_.alloc(2 * rec);
        fuseAdjT_.alloc(2 * rec);
        fuseComp_.alloc(comps);
        fuseRep_.alloc(comps);
        fuseOutRep_.alloc(comps);
        fuseCompKey_.alloc(comps);
        fuseOutKey_.alloc(comps);
        fuseCounts_.alloc(4);
        BF_HIP(hipHostMalloc((void**)&hostFuse_, 4 * sizeof(uint32_t), hipHostMallocDefault));
        BF_HIP(hipEventCreateWithFlags(&fuseDone_, hipEventDisableTiming));
    }
    BF_HIP(hipFuncSetAttribute((const void*)k_match<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MATCH_LDS_BYTES));
    BF_HIP(hipFuncSetAttribute((const void*)k_match<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MATCH_LDS_BYTES));
    std::memcpy(hostBase_ + n, cfg_.kinv, 64);
    BF_HIP(hipMemcpyAsync(base_.p + n, hostBase_ + n, 64, hipMemcpyHostToDevice, stream_));
    reset();
}

Matcher::~Matcher() {
    if (hostTable_) (void)hipHostFree(hostTable_);
    if (hostCounts_) (void)hipHostFree(hostCounts_);
    if (hostBase_) (void)hipHostFree(hostBase_);
    if (hostFuse_) (void)hipHostFree(hostFuse_);
    if (fuseDone_) (void)hipEventDestroy(fuseDone_);
}

void Matcher::reset() {
    num_.clear();
    off_.clear();
    valid_.clear();
    totalKeys_ = 0;
    tableDirty_ = true;
    fuseRan_ = false;
    const size_t n = cfg_.maxImages;
    BF_HIP(hipMemsetAsync(rawCount_.p, 0, n * 4, stream_));
    BF_HIP(hipMemsetAsync(filtCount_.p, 0, n * 4, stream_));
    BF_HIP(hipMemsetAsync(rawIdx_.p, 0xFF, rawIdx_.bytes(), stream_));
    BF_HIP(hipMemsetAsync(filtIdx_.p, 0xFF, filtIdx_.bytes(), stream_));
    BF_HIP(hipMemsetAsync(rawDist_.p, 0, rawDist_.bytes(), stream_));
    BF_HIP(hipMemsetAsync(filtDist_.p, 0, filtDist_.bytes(), stream_));
    BF_HIP(hipMemsetAsync(T_.p, 0, T_.bytes(), stream_));
    BF_HIP(hipMemsetAsync(Tinv_.p, 0, Tinv_.bytes(), stream_));
    BF_HIP(hipMemsetAsync(area_.p, 0xFF, area_.bytes(), stream_));  // NaN: no stage has looked at the pair
    BF_HIP(hipMemsetAsync(denseSums_.p, 0xFF, denseSums_.bytes(), stream_));
}

uint32_t Matcher::addImage(const BFSiftKeyPoint* keys, const uint8_t* descs, uint32_t n) {
    BF_REQUIRE(n <= cfg_.maxKeys, BF_ERR_ARG, "more keys than maxKeysPerImage");
    BF_REQUIRE(n == 0 || (keys && descs), BF_ERR_ARG, "null keys / descriptors");
    BF_REQUIRE(num_.size() < cfg_.maxImages, BF_ERR_CAPACITY, "matcher image store is full");
    if (n) {
        BF_HIP(hipMemcpyAsync(keys_.p + totalKeys_, keys, (size_t)n * sizeof(BFSiftKeyPoint), hipMemcpyDeviceToDevice, stream_));
        BF_HIP(hipMemcpyAsync(descs_.p + (size_t)totalKeys_ * 128, descs, (size_t)n * 128, hipMemcpyDeviceToDevice, stream_));
        k_desc_sums<<<div_up(n, 128), 128, 0, stream_>>>(descs_.p, sums_.p, totalKeys_, n);
        BF_LAUNCH_CHECK();
    }
    return appendStored(n);
}

uint32_t Matcher::appendStored(uint32_t n) {
    const uint32_t index = (uint32_t)num_.size();
    num_.push_back(n);
    off_.push_back(totalKeys_);
    valid_.push_back(index == 0 ? 1 : 0);  // image 0 starts valid; filterFrames decides the others
    totalKeys_ += n;
    tableDirty_ = true;
    return index;
}

void Matcher::setValid(uint32_t i, int v) {
    valid_[i] = v ? 1 : 0;
    tableDirty_ = true;
}

void Matcher::uploadTable() {
    if (!tableDirty_) return;
    if (tableInFlight_) BF_HIP(hipStreamSynchronize(stream_));  // an earlier upload may still read the pinned table
    tableInFlight_ = true;
    const uint32_t n = numImages();
    for (uint32_t i = 0; i < n; i++) {
        hostTable_[4 * i] = off_[i];
        hostTable_[4 * i + 1] = num_[i];
        hostTable_[4 * i + 2] = (uint32_t)valid_[i];
        hostTable_[4 * i + 3] = 0;
    }
    if (n) BF_HIP(hipMemcpyAsync(table_.p, hostTable_, 16 * (size_t)n, hipMemcpyHostToDevice, stream_));
    tableDirty_ = false;
}

void Matcher::launchMatch(uint32_t cur, uint32_t start, uint32_t pairs, bool debug, uint32_t nRows, uint32_t nCols) {
    MatchArgs A{};
    A.descs = descs_.p;
    A.sums = sums_.p;
    A.table = table_.p;
    A.cur = cur;
    A.start = start;
    A.thresh = cfg_.matchThresh;
    A.ratio = cfg_.ratioMax;
    A.rawCount = rawCount_.p;
    A.rawIdx = rawIdx_.p;
    A.rawDist = rawDist_.p;
    A.dbgSel = dbgSel_.p;
    A.dbgOut = dbgOut_.p;
    A.dbgRows = nRows;
    A.dbgCols = nCols;
    if (debug)
        k_match<true><<<pairs, MATCH_WG, MATCH_LDS_BYTES, stream_>>>(A);
    else
        k_match<false><<<pairs, MATCH_WG, MATCH_LDS_BYTES, stream_>>>(A);
    BF_LAUNCH_CHECK();
}

void Matcher::match(uint32_t cur, uint32_t start) {
    const uint32_t n = numImages();
    BF_REQUIRE(cur < n, BF_ERR_ARG, "curFrame >= numImages");
    BF_REQUIRE(start <= n, BF_ERR_ARG, "startFrame > numImages");
    if (start == n) return;
    uploadTable();
    launchMatch(cur, start, n - start, false, 0, 0);
}

void Matcher::filter(uint32_t cur, uint32_t start) {
    const uint32_t n = numImages();
    BF_REQUIRE(cur < n, BF_ERR_ARG, "curFrame >= numImages");
    BF_REQUIRE(start <= n, BF_ERR_ARG, "startFrame > numImages");
    if (start == n) return;
    FilterArgs A{};
    A.keys = keys_.p;
    A.rawCount = rawCount_.p;
    A.rawIdx = rawIdx_.p;
    A.rawDist = rawDist_.p;
    A.filtCount = filtCount_.p;
    A.filtIdx = filtIdx_.p;
    A.filtDist = filtDist_.p;
    A.T = T_.p;
    A.Tinv = Tinv_.p;
    for (int k = 0; k < 16; k++) A.kinv[k] = cfg_.kinv[k];
    A.cur = cur;
    A.start = start;
    A.minNumMatches = cfg_.minNumMatches;
    A.maxRes2 = cfg_.maxKabschRes2;
    k_filter<<<n - start, 64, 0, stream_>>>(A);
    BF_LAUNCH_CHECK();
}

uint32_t Matcher::filterFrames(uint32_t cur, uint32_t start) {
    const uint32_t n = numImages();
    BF_REQUIRE(cur < n, BF_ERR_ARG, "curFrame >= numImages");
    BF_REQUIRE(start <= n, BF_ERR_ARG, "startFrame > numImages");
    uint32_t last = 0xFFFFFFFFu;
    if (start < n) {
        BF_HIP(hipMemcpyAsync(hostCounts_, filtCount_.p + start, 4 * (size_t)(n - start), hipMemcpyDeviceToHost, stream_));
        BF_HIP(hipStreamSynchronize(stream_));
        for (int i = (int)n - 1; i >= (int)start; i--)
            if (valid_[i] != 0 && hostCounts_[i - start] > 0 && (uint32_t)i != cur) {
                last = (uint32_t)i;
                break;
            }
    }
    setValid(cur, last != 0xFFFFFFFFu);
    return last;
}

uint32_t Matcher::addToResiduals(uint32_t cur, uint32_t start, BFEntryJ* out, uint32_t* keyIdx, uint32_t cap, uint32_t* total) {
    const uint32_t n = numImages();
    BF_REQUIRE(cur < n, BF_ERR_ARG, "curFrame >= numImages");
    BF_REQUIRE(start <= n, BF_ERR_ARG, "startFrame > numImages");
    BF_REQUIRE(out != nullptr || cap == 0, BF_ERR_ARG, "null output");
    if (total) *total = 0;
    if (start == n) return 0;
    BF_HIP(hipMemcpyAsync(hostCounts_, filtCount_.p + start, 4 * (size_t)(n - start), hipMemcpyDeviceToHost, stream_));
    BF_HIP(hipStreamSynchronize(stream_));
    uint32_t sum = 0;
    for (uint32_t i = start; i < n; i++) {
        hostBase_[i] = sum;
        if (i != cur) sum += hostCounts_[i - start];
    }
    if (total) *total = sum;
    if (sum && cap) {
        BF_HIP(hipMemcpyAsync(base_.p + start, hostBase_ + start, 4 * (size_t)(n - start), hipMemcpyHostToDevice, stream_));
        k_add_residuals<<<n - start, 32, 0, stream_>>>(keys_.p, filtCount_.p, filtIdx_.p, base_.p, cur, start, out, keyIdx, cap,
                                                      (const float*)(base_.p + cfg_.maxImages));
        BF_LAUNCH_CHECK();
        BF_HIP(hipStreamSynchronize(stream_));
    }
    return sum < cap ? sum : cap;
}

Matcher::CloseView Matcher::prepareClose(uint32_t cur, uint32_t start) {
    checkFrames(cur, start);
    uploadTable();
    return CloseView{keys_.p, filtCount_.p, filtIdx_.p, table_.p, Tinv_.p, (const float*)(base_.p + cfg_.maxImages), base_.p};
}

uint32_t Matcher::copyImageFrom(const Matcher& src, uint32_t image) {
    BF_REQUIRE(&src != this, BF_ERR_ARG, "copyImageFrom: source and destination are the same matcher");
    BF_REQUIRE(image < src.numImages(), BF_ERR_ARG, "copyImageFrom: image >= the source's numImages");
    const size_t at = src.off_[image];
    return addImage(src.keys_.p + at, src.descs_.p + at * 128, src.num_[image]);
}

MatchVerifyConfig make_match_verify_config(const BFMatchVerifyOptions* o) {
    MatchVerifyConfig c;
    if (!o) return c;
    const float v[7] = {o->surfAreaPcaThresh, o->projCorrDistThres, o->projCorrNormalThres, o->verifySiftErrThresh,
                        o->verifySiftCorrThresh, o->sensorDepthMin, o->sensorDepthMax};
    for (float x : v) BF_REQUIRE(std::isfinite(x) && x >= 0.0f, BF_ERR_ARG, "match verify options: non-finite or negative threshold");
    if (o->surfAreaPcaThresh > 0.0f) c.surfAreaPcaThresh = o->surfAreaPcaThresh;
    if (o->projCorrDistThres > 0.0f) c.projCorrDistThres = o->projCorrDistThres;
    if (o->projCorrNormalThres > 0.0f) c.projCorrNormalThres = o->projCorrNormalThres;
    if (o->verifySiftErrThresh > 0.0f) c.verifySiftErrThresh = o->verifySiftErrThresh;
    if (o->verifySiftCorrThresh > 0.0f) c.verifySiftCorrThresh = o->verifySiftCorrThresh;
    if (o->sensorDepthMin > 0.0f) c.sensorDepthMin = o->sensorDepthMin;
    if (o->sensorDepthMax > 0.0f) c.sensorDepthMax = o->sensorDepthMax;
    BF_REQUIRE(c.sensorDepthMax > c.sensorDepthMin, BF_ERR_ARG, "match verify options: sensorDepthMax <= sensorDepthMin");
    return c;
}

void Matcher::checkFrames(uint32_t cur, uint32_t start) const {
    const uint32_t n = numImages();
    BF_REQUIRE(cur < n, BF_ERR_ARG, "curFrame >= numImages");
    BF_REQUIRE(start <= n, BF_ERR_ARG, "startFrame > numImages");
}

void check_dense_frame_shape(uint32_t W, uint32_t H, const float* intrinsics) {
    BF_REQUIRE(W >= 1 && H >= 1 && (uint64_t)W * H <= (1ull << 20), BF_ERR_ARG, "cache frame size: W, H >= 1 and W * H <= 2^20");
    BF_REQUIRE(intrinsics != nullptr, BF_ERR_ARG, "null intrinsics");
    for (int k = 0; k < 16; k++) BF_REQUIRE(std::isfinite(intrinsics[k]), BF_ERR_ARG, "non-finite cache intrinsics");
}

void Matcher::checkDenseShape(uint32_t nFrames, uint32_t W, uint32_t H, const float* intrinsics) const {
    check_dense_frame_shape(W, H, intrinsics);
    BF_REQUIRE(nFrames >= numImages(), BF_ERR_ARG, "nFrames below the matcher's image count");
}

void Matcher::filterSurfaceArea(uint32_t cur, uint32_t start, const MatchVerifyConfig& v) {
    checkFrames(cur, start);
    const uint32_t n = numImages();
    BF_HIP(hipMemsetAsync(area_.p, 0xFF, area_.bytes(), stream_));
    if (start == n) return;
    uploadTable();
    k_surface_area<<<n - start, 64, 0, stream_>>>(keys_.p, filtCount_.p, filtIdx_.p, table_.p, (const float*)(base_.p + cfg_.maxImages),
                                                  area_.p, cur, start, v.surfAreaPcaThresh);
    BF_LAUNCH_CHECK();
}

void Matcher::filterDenseVerify(uint32_t cur, uint32_t start, const BFCachedFrame* frames, uint32_t nFrames, uint32_t W, uint32_t H,
                                const float* intrinsics, const MatchVerifyConfig& v) {
    checkFrames(cur, start);
    checkDenseShape(nFrames, W, H, intrinsics);
    BF_REQUIRE(frames != nullptr, BF_ERR_ARG, "null cache frames");
    const uint32_t n = numImages();
    BF_HIP(hipMemsetAsync(denseSums_.p, 0xFF, denseSums_.bytes(), stream_));
    if (start == n) return;
    uploadTable();
    DenseArgs A{};
    A.frames = frames;
    A.filtCount = filtCount_.p;
    A.T = T_.p;
    A.Tinv = Tinv_.p;
    A.table = table_.p;
    A.partial = densePartial_.p;
    A.sums = denseSums_.p;
    A.cur = cur;
    A.start = start;
    A.n = n;
    A.W = W;
    A.H = H;
    A.rowsPerSlice = div_up(H, DV_SLICES);
    A.nSlices = div_up(H, A.rowsPerSlice);  // <= DV_SLICES, every slice has a row
    for (int k = 0; k < 16; k++) A.K[k] = intrinsics[k];
    A.distT = v.projCorrDistThres;
    A.normT = v.projCorrNormalThres;
    A.errT = v.verifySiftErrThresh;
    A.corrT = v.verifySiftCorrThresh;
    A.dmin = v.sensorDepthMin;
    A.dmax = v.sensorDepthMax;
    k_dense_verify<<<dim3(A.nSlices, n - start), DV_WG, 0, stream_>>>(A);
    BF_LAUNCH_CHECK();
    k_dense_decide<<<div_up(n - start, 64u), 64, 0, stream_>>>(A);
    BF_LAUNCH_CHECK();
}

void Matcher::verifyStats(uint32_t prev, float* area, float* sums) {
    BF_REQUIRE(prev < numImages(), BF_ERR_ARG, "prev >= numImages");
    BF_HIP(hipStreamSynchronize(stream_));
    if (area) BF_HIP(hipMemcpy(area, area_.p + 2 * (size_t)prev, 8, hipMemcpyDeviceToHost));
    if (sums) BF_HIP(hipMemcpy(sums, denseSums_.p + 6 * (size_t)prev, 24, hipMemcpyDeviceToHost));
}

void Matcher::debugSetFiltered(uint32_t prev, uint32_t count, const uint32_t* idx) {
    BF_REQUIRE(prev < numImages(), BF_ERR_ARG, "prev >= numImages");
    BF_REQUIRE(count <= kFilt && (idx || count == 0), BF_ERR_ARG, "at most 25 filtered matches");
    for (uint32_t k = 0; k < 2 * count; k++) BF_REQUIRE(idx[k] < totalKeys_, BF_ERR_ARG, "key index >= the store's key count");
    uint32_t list[2 * kFilt];
    for (uint32_t k = 0; k < 2 * kFilt; k++) list[k] = k < 2 * count ? idx[k] : 0xFFFFFFFFu;
    BF_HIP(hipStreamSynchronize(stream_));
    BF_HIP(hipMemcpy(filtIdx_.p + (size_t)prev * kFilt, list, sizeof(list), hipMemcpyHostToDevice));
    BF_HIP(hipMemcpy(filtCount_.p + prev, &count, 4, hipMemcpyHostToDevice));
}

void Matcher::rawMatches(uint32_t prev, uint32_t* count, uint32_t* idx, float* dist) {
    BF_REQUIRE(prev < numImages(), BF_ERR_ARG, "prev >= numImages");
    BF_HIP(hipStreamSynchronize(stream_));
    if (count) BF_HIP(hipMemcpy(count, rawCount_.p + prev, 4, hipMemcpyDeviceToHost));
    if (idx) BF_HIP(hipMemcpy(idx, rawIdx_.p + (size_t)prev * kRaw, 8 * kRaw, hipMemcpyDeviceToHost));
    if (dist) BF_HIP(hipMemcpy(dist, rawDist_.p + (size_t)prev * kRaw, 4 * kRaw, hipMemcpyDeviceToHost));
}

void Matcher::filteredMatches(uint32_t prev, uint32_t* count, uint32_t* idx, float* dist) {
    BF_REQUIRE(prev < numImages(), BF_ERR_ARG, "prev >= numImages");
    BF_HIP(hipStreamSynchronize(stream_));
    if (count) BF_HIP(hipMemcpy(count, filtCount_.p + prev, 4, hipMemcpyDeviceToHost));
    if (idx) BF_HIP(hipMemcpy(idx, filtIdx_.p + (size_t)prev * kFilt, 8 * kFilt, hipMemcpyDeviceToHost));
    if (dist) BF_HIP(hipMemcpy(dist, filtDist_.p + (size_t)prev * kFilt, 4 * kFilt, hipMemcpyDeviceToHost));
}

void Matcher::imageKeys(uint32_t image, BFSiftKeyPoint* keys, uint8_t* descs) {
    BF_REQUIRE(image < numImages(), BF_ERR_ARG, "image >= numImages");
    BF_HIP(hipStreamSynchronize(stream_));
    const size_t n = num_[image], at = off_[image];
    if (n == 0) return;
    if (keys) BF_HIP(hipMemcpy(keys, keys_.p + at, n * sizeof(BFSiftKeyPoint), hipMemcpyDeviceToHost));
    if (descs) BF_HIP(hipMemcpy(descs, descs_.p + at * 128, n * 128, hipMemcpyDeviceToHost));
}

void Matcher::transforms(uint32_t prev, float* T, float* Tinv) {
    BF_REQUIRE(prev < numImages(), BF_ERR_ARG, "prev >= numImages");
    BF_HIP(hipStreamSynchronize(stream_));
    if (T) BF_HIP(hipMemcpy(T, T_.p + 16 * (size_t)prev, 64, hipMemcpyDeviceToHost));
    if (Tinv) BF_HIP(hipMemcpy(Tinv, Tinv_.p + 16 * (size_t)prev, 64, hipMemcpyDeviceToHost));
}

void Matcher::debugDots(uint32_t prev, uint32_t cur, const uint32_t* rows, uint32_t nRows, const uint32_t* cols, uint32_t nCols,
                        int32_t* dots, int32_t* rowStats) {
    const uint32_t n = numImages();
    BF_REQUIRE(prev < n && cur < n && prev != cur, BF_ERR_ARG, "prev / curFrame out of range or equal");
    BF_REQUIRE(nRows <= kDbg && nCols <= kDbg && (rows || nRows == 0) && (cols || nCols == 0), BF_ERR_ARG,
               "at most 32 rows and 32 columns");
    for (uint32_t r = 0; r < nRows; r++) BF_REQUIRE(rows[r] < num_[prev], BF_ERR_ARG, "row >= prev's key count");
    for (uint32_t c = 0; c < nCols; c++) BF_REQUIRE(cols[c] < num_[cur], BF_ERR_ARG, "column >= curFrame's key count");
    uploadTable();
    uint32_t sel[2 * kDbg] = {};
    for (uint32_t r = 0; r < nRows; r++) sel[r] = rows[r];
    for (uint32_t c = 0; c < nCols; c++) sel[kDbg + c] = cols[c];
    BF_HIP(hipMemcpyAsync(dbgSel_.p, sel, sizeof(sel), hipMemcpyHostToDevice, stream_));  // pageable: staged before it returns
    BF_HIP(hipMemsetAsync(dbgOut_.p, 0, dbgOut_.bytes(), stream_));
    launchMatch(cur, prev, 1, true, nRows, nCols);
    BF_HIP(hipStreamSynchronize(stream_));
    if (dots && nRows * nCols) BF_HIP(hipMemcpy(dots, dbgOut_.p, 4 * (size_t)nRows * nCols, hipMemcpyDeviceToHost));
    if (rowStats && nRows) BF_HIP(hipMemcpy(rowStats, dbgOut_.p + kDbg * kDbg, 12 * (size_t)nRows, hipMemcpyDeviceToHost));
}

}  // namespace bf

#include "match_fuse.h"
