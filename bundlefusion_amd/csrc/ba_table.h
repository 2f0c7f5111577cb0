// ba_table.h — the tables a solve is built on, and the assembled (pair mode) normal-equation blocks.
// Row table (per rebuildJT): k_tile_count, k_tile_scan, k_scan, k_tile_fill, k_compact_rows, k_chunks.
// Pair table (per row table): k_pair_sort, k_pair_scan, k_pair_fill, k_pair_rows; k_pair_gather per solve and
// k_pair_stats per GN iteration. chunk_range, pair_block_apply and diag_apply are what the PCG routes
// (ba_pcg.h, ba_persist.h) apply these tables with. Relies on ba_dev.h only.
#pragma once
#include "ba_dev.h"

namespace bf {
namespace {

// ---- correspondence table (BuildVariablesToCorrespondencesTableDevice, SolverBundling.cu:1226-1248) ----
// The reference appends (image -> correspondence) pairs with atomics and drops an append once the row
// holds maxCorrPerImage entries. The deterministic replay here is a stable counting sort: rows list
// their correspondences in ascending index order (the serial order of that loop), an entry ranked
// >= cap in either of its rows invalidates the correspondence. Three passes over tiles of TILE
// consecutive correspondences: per-tile row histograms, a per-row scan over tiles, and a placement
// pass that ranks each entry inside its tile with wave ballots (no global atomics, no row sort).
__device__ __forceinline__ bool corr_rows(const BA& a, uint32_t c, uint32_t& i, uint32_t& j) {
    const uint2 ij = *reinterpret_cast<const uint2*>(&a.corr[c].imgIdx_i);
    i = ij.x; j = ij.y;
    return i != BF_INVALID_IMAGE && i < a.N && j < a.N;
}
__global__ __launch_bounds__(64) void k_tile_count(BA a) {
    extern __shared__ int hist[];  // [N]
    const uint32_t t = blockIdx.x;
    for (uint32_t r = threadIdx.x; r < a.N; r += 64) hist[r] = 0;
    __syncthreads();
    const uint32_t c1 = min((t + 1) * a.tile, a.nCorr);
    for (uint32_t c = t * a.tile + threadIdx.x; c < c1; c += 64) {
        uint32_t i, j;
        if (!corr_rows(a, c, i, j)) continue;
        atomicAdd(&hist[i], 1);
        atomicAdd(&hist[j], 1);
    }
    __syncthreads();
    for (uint32_t r = threadIdx.x; r < a.N; r += 64) a.tileCnt[(size_t)r * a.nTiles + t] = hist[r];
}
// one workgroup per row: exclusive scan of the row's tile counts (in place), rowCount = total
__global__ __launch_bounds__(WG) void k_tile_scan(BA a) {
    __shared__ int sh[WG];
    const uint32_t r = blockIdx.x;
    int* cnt = a.tileCnt + (size_t)r * a.nTiles;
    int carry = 0;
    for (uint32_t base = 0; base < a.nTiles; base += WG) {
        const uint32_t t = base + threadIdx.x;
        const int c = t < a.nTiles ? cnt[t] : 0;
        sh[threadIdx.x] = c;
        __syncthreads();
        for (int off = 1; off < WG; off <<= 1) {
            const int x = (int)threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
            __syncthreads();
            sh[threadIdx.x] += x;
            __syncthreads();
        }
        if (t < a.nTiles) cnt[t] = carry + sh[threadIdx.x] - c;
        carry += sh[WG - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.rowCount[r] = carry;
}
__global__ void k_scan(BA a) {  // one workgroup: exclusive scan of rowCount -> rowStart
    __shared__ int sh[WG];
    int carry = 0;
    for (uint32_t base = 0; base < a.N; base += WG) {
        const uint32_t v = base + threadIdx.x;
        const int c = v < a.N ? a.rowCount[v] : 0;
        sh[threadIdx.x] = c;
        __syncthreads();
        for (int off = 1; off < WG; off <<= 1) {
            int t = (int)threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
            __syncthreads();
            sh[threadIdx.x] += t;
            __syncthreads();
        }
        if (v < a.N) a.rowStart[v] = carry + sh[threadIdx.x] - c;
        carry += sh[WG - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.rowStart[a.N] = carry;
}
// placement: one wave per tile, 64 correspondences per step. Each distinct row key of the step is
// resolved in one ballot round: an entry's slot = row start + the row's tile offset + entries of
// that row placed earlier in this tile + lower lanes of this step holding the same row (an i entry
// precedes the j entry of the same correspondence).
__global__ __launch_bounds__(64) void k_tile_fill(BA a) {
    extern __shared__ int run[];  // [N] entries placed so far in this tile, per row
    const uint32_t t = blockIdx.x, lane = threadIdx.x;
    for (uint32_t r = lane; r < a.N; r += 64) run[r] = 0;
    __syncthreads();
    const uint64_t lower = lanes_below(lane);
    const uint32_t c1 = min((t + 1) * a.tile, a.nCorr);
    for (uint32_t c0 = t * a.tile; c0 < c1; c0 += 64) {
        const uint32_t c = c0 + lane;
        uint32_t i = BF_INVALID_IMAGE, j = BF_INVALID_IMAGE;
        const bool ok = c < c1 && corr_rows(a, c, i, j);
        uint64_t pendI = __ballot(ok), pendJ = pendI;
        int posI = -1, posJ = -1;
        while (pendI | pendJ) {
            const int src = pendI ? __ffsll((unsigned long long)pendI) - 1 : __ffsll((unsigned long long)pendJ) - 1;
            const uint32_t key = __shfl(pendI ? i : j, src);
            const bool hi = ok && i == key, hj = ok && j == key;
            const uint64_t mi = __ballot(hi), mj = __ballot(hj);
            const int base = a.rowStart[key] + a.tileCnt[(size_t)key * a.nTiles + t] + run[key];
            const int below = __popcll(mi & lower) + __popcll(mj & lower);
            if (hi) posI = base + below;
            if (hj) posJ = base + below + (hi ? 1 : 0);
            __syncthreads();
            if (lane == 0) run[key] += __popcll(mi) + __popcll(mj);
            __syncthreads();
            pendI &= ~mi;
            pendJ &= ~mj;
        }
        if (ok) {
            a.rowTmp[posI] = (int)c;
            a.rowTmp[posJ] = (int)c;
            // setInvalid (SolverBundling.cu:1241-1245) for an entry past the per-image cap
            if (posI - a.rowStart[i] >= (int)a.cap || posJ - a.rowStart[j] >= (int)a.cap) {
                a.corr[c].imgIdx_i = BF_INVALID_IMAGE;
                a.corr[c].imgIdx_j = BF_INVALID_IMAGE;
            }
        }
    }
}
// keep the entries that survived the cap (stable), rowLen = kept count
__global__ __launch_bounds__(WG) void k_compact_rows(BA a) {
    __shared__ uint32_t cnt[WG / 64];
    const uint32_t v = blockIdx.x;
    if (v >= a.N) return;
    const int n = min(a.rowCount[v], (int)a.cap), s0 = a.rowStart[v];
    uint32_t base = 0;  // the same in every lane
    for (int k0 = 0; k0 < n; k0 += WG) {
        const int k = k0 + threadIdx.x;
        bool keep = false;
        int c = 0;
        if (k < n) { c = a.rowTmp[s0 + k]; keep = corr_valid(a.corr[c]); }
        uint32_t kept;
        const uint32_t off = base + wg_compact_offset<WG / 64>(keep, cnt, kept);
        if (keep) a.rowIdx[s0 + off] = c;
        base += kept;
        __syncthreads();
    }
    if (threadIdx.x == 0) a.rowLen[v] = (int)base;
}

// chunk table: row v (v >= 1; image 0 is fixed) is cut into ceil(rowLen / CH) chunks of CH entries
__global__ void k_chunks(BA a) {  // one workgroup
    __shared__ int sh[WG];
    int carry = 0;
    for (uint32_t base = 0; base < a.N; base += WG) {
        const uint32_t v = base + threadIdx.x;
        const int c = (v >= 1 && v < a.N) ? (a.rowLen[v] + CH - 1) / CH : 0;
        sh[threadIdx.x] = c;
        __syncthreads();
        for (int off = 1; off < WG; off <<= 1) {
            const int x = (int)threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
            __syncthreads();
            sh[threadIdx.x] += x;
            __syncthreads();
        }
        const int s = carry + sh[threadIdx.x] - c;
        if (v < a.N) {
            a.rowChunk[v] = s;
            for (int q = 0; q < c; q++) a.chunkRow[s + q] = (int)v;
        }
        carry += sh[WG - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        a.rowChunk[a.N] = carry;
        a.ctrl[K_NCHUNK] = (uint32_t)carry;
    }
}
__device__ __forceinline__ void chunk_range(const BA& a, uint32_t c, uint32_t& v, int& k0, int& k1) {
    v = (uint32_t)a.chunkRow[c];
    const int s0 = a.rowStart[v];
    k0 = s0 + ((int)c - a.rowChunk[v]) * CH;
    k1 = min(s0 + a.rowLen[v], k0 + CH);
}

// ---- assembled normal equations (pair mode) ---------------------------------------------------
// The reference applies J^T J matrix-free: every PCG iteration streams all correspondences
// (applyJDevice / applyJTDevice, SolverBundlingEquationsLie.h:154-228). For a sparse-only solve the
// same operator is a sum over image pairs of 6x6 blocks, and with A_v = [-[P_v]x | I] (P_v = T_v p_v,
// the world point of a correspondence in image v) every block is fixed by a few sums over the pair's
// correspondences (a < b, P_a / P_b the two world points):
//   M = sum P_b P_a^T (9), s_a = sum P_a, s_b = sum P_b, n, Q_a = sum P_a P_a^T, Q_b = sum P_b P_b^T (6 each)
//   sum A_a^T A_b = [[tr(M) I - M, [s_a]x], [-[s_b]x, n I]]          (off-diagonal, row a)
//   sum A_v^T A_v = [[tr(Q) I - Q, [s]x], [-[s]x, n I]]              (diagonal, summed over v's pairs)
//   sum A_v^T r  = (-/+ (sum P_a x P_b), s_v - s_u)                     (J^T F, r = P_v - P_u)
// The statistics are accumulated in fp64 (products of fp32 points are exact in fp64), so the
// blocks keep the cancellation D_v p_v - sum_u B_vu p_u accurate. A PCG iteration then reads 128 B
// per (row, pair) entry instead of 64 B per (row, correspondence) entry. Pair p is built by shard
// p % shardCount; every other shard writes zeros, so the RCCL sum over shards reproduces the
// single-GPU statistics bit for bit (x + 0 = x), and the replicated PCG that follows is identical on
// every GPU (one all-reduce per GN iteration).
constexpr int PSTAT = 28;        // doubles per pair: M[9] s_a[3] s_b[3] n Q_a[6] Q_b[6]
constexpr int DSTAT = 10;        // doubles per image: Q[6] s[3] n
constexpr uint32_t SORT_MAX = 4096;  // >= maxCorrPerImage (4000)
constexpr uint32_t ROW_POS_BITS = 12;
constexpr uint32_t PAIR_A_FLAG = 0x80000000u;

// per row v: the row's entries ordered by (other image, position) — position order is ascending
// correspondence index — with the row's distinct partners counted (rowDeg) and those above v (rowNA)
__global__ __launch_bounds__(WG) void k_pair_sort(BA a) {
    __shared__ uint32_t key[SORT_MAX];
    __shared__ int shd[WG / 64], sha[WG / 64];
    const uint32_t v = blockIdx.x;
    const int n = a.rowLen[v], s0 = a.rowStart[v];
    uint32_t P = 1;
    while (P < (uint32_t)n) P <<= 1;
    for (uint32_t t = threadIdx.x; t < P; t += WG) {
        uint32_t k = 0xFFFFFFFFu;
        if ((int)t < n) {
            const int c = a.rowIdx[s0 + t];
            const uint2 ij = *reinterpret_cast<const uint2*>(&a.corr[c].imgIdx_i);
            const uint32_t u = (ij.x == v) ? ij.y : ij.x;
            k = (u << ROW_POS_BITS) | t;
        }
        key[t] = k;
    }
    __syncthreads();
    for (uint32_t size = 2; size <= P; size <<= 1) {  // bitonic sort, ascending
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t t = threadIdx.x; t < P / 2; t += WG) {
                const uint32_t i = 2 * t - (t & (stride - 1)), j = i + stride;
                const uint32_t x = key[i], y = key[j];
                if ((x > y) == ((i & size) == 0)) { key[i] = y; key[j] = x; }
            }
            __syncthreads();
        }
    }
    int deg = 0, na = 0;
    for (uint32_t t = threadIdx.x; t < (uint32_t)n; t += WG) {
        const uint32_t k = key[t], u = k >> ROW_POS_BITS;
        a.rowSorted[s0 + t] = a.rowIdx[s0 + (k & ((1u << ROW_POS_BITS) - 1))];
        a.rowOther[s0 + t] = (int)u;
        const bool head = (t == 0 || (key[t - 1] >> ROW_POS_BITS) != u) && u != v;  // self pairs are skipped
        int len = 0;
        if (head) {  // run length of partner u, from the sorted keys in LDS
            uint32_t e = t + 1;
            while (e < (uint32_t)n && (key[e] >> ROW_POS_BITS) == u) e++;
            len = (int)(e - t);
        }
        a.rowSeg[s0 + t] = len;
        deg += head ? 1 : 0;
        na += (head && u > v) ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) { deg += __shfl_xor(deg, off); na += __shfl_xor(na, off); }
    if ((threadIdx.x & 63) == 0) { shd[threadIdx.x >> 6] = deg; sha[threadIdx.x >> 6] = na; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int d = 0, m = 0;
        for (int w = 0; w < WG / 64; w++) { d += shd[w]; m += sha[w]; }
        a.rowDeg[v] = d;
        a.rowNA[v] = m;
    }
}
// one workgroup: exclusive scans rowNA -> pairStart (pairs (a, b > a) numbered in (a, b) order) and
// rowDeg -> rowPairStart (each row's incident pairs)
__global__ void k_pair_scan(BA a) {
    __shared__ int sh[WG];
    block_exclusive_scan(a.rowNA, a.pairStart, a.N, sh);
    block_exclusive_scan(a.rowDeg, a.rowPairStart, a.N, sh);
    if (threadIdx.x == 0) a.ctrl[K_NPAIRS_A] = (uint32_t)a.pairStart[a.N];
}
// one wave per row: segments (runs of one partner u) of the sorted row. Row a numbers its pairs with
// u > a and records their correspondence runs; the row entries of pairs with u < a are filled by
// k_pair_rows once every pair has its number.
template <bool OWN>
__device__ void pair_segments(const BA& a, uint32_t v) {
    const uint32_t lane = lane_id();
    const int n = a.rowLen[v], s0 = a.rowStart[v];
    int seg = 0, segA = 0;
    for (int base = 0; base < n; base += 64) {
        const int t = base + (int)lane;
        const int u = t < n ? a.rowOther[s0 + t] : -1;
        const int prev = (t > 0 && t < n) ? a.rowOther[s0 + t - 1] : -1;
        const bool head = t < n && u != prev && u != (int)v;
        const uint64_t mh = __ballot(head), ma = __ballot(head && u > (int)v);
        const int rank = seg + __popcll(mh & lanes_below(lane));
        if (head) {
            if (OWN && u > (int)v) {
                const int p = a.pairStart[v] + segA + __popcll(ma & lanes_below(lane));
                a.pairA[p] = (int)v;
                a.pairB[p] = u;
                a.pairCorr[p] = make_int2(s0 + t, a.rowSeg[s0 + t]);
                a.rowPair[a.rowPairStart[v] + rank] = make_int2(p, (int)((uint32_t)u | PAIR_A_FLAG));
            } else if (!OWN && u < (int)v) {  // pair (u, v): binary search v in u's partner list
                int lo = a.pairStart[u], hi = a.pairStart[u + 1] - 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (a.pairB[mid] < (int)v) lo = mid + 1; else hi = mid;
                }
                a.rowPair[a.rowPairStart[v] + rank] = make_int2(lo, u);
            }
        }
        seg += __popcll(mh);
        segA += __popcll(ma);
    }
}
__global__ __launch_bounds__(64) void k_pair_fill(BA a) { pair_segments<true>(a, blockIdx.x); }
__global__ __launch_bounds__(64) void k_pair_rows(BA a) { pair_segments<false>(a, blockIdx.x); }

// once per solve (pair mode): each pair's correspondence points, oriented (a, b), copied into the
// pair's run order — k_pair_stats then streams them contiguously on every GN iteration instead of
// gathering 48-B EntryJ records through rowSorted three times (the entries buffer is free in pair mode)
__global__ __launch_bounds__(WG) void k_pair_gather(BA a) {
    if (a.ctrl[K_GN_DONE]) return;
    const uint32_t lane = lane_id();
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
    const uint32_t np = a.ctrl[K_NPAIRS_A];
    float2* tail = reinterpret_cast<float2*>(a.entries + a.entTail);
    for (uint32_t p = wave; p < np; p += nw) {
        if (p % a.shardCount != a.shardIndex) continue;
        const uint32_t pa = (uint32_t)a.pairA[p];
        const int2 run = a.pairCorr[p];
        for (int k = (int)lane; k < run.y; k += 64) {
            const BFEntryJ e = a.corr[a.rowSorted[run.x + k]];
            const bool aIsI = e.imgIdx_i == pa;
            const f3 pA = aIsI ? mk3(e.pos_i.x, e.pos_i.y, e.pos_i.z) : mk3(e.pos_j.x, e.pos_j.y, e.pos_j.z);
            const f3 pB = aIsI ? mk3(e.pos_j.x, e.pos_j.y, e.pos_j.z) : mk3(e.pos_i.x, e.pos_i.y, e.pos_i.z);
            a.entries[run.x + k] = make_float4(pA.x, pA.y, pA.z, pB.x);
            tail[run.x + k] = make_float2(pB.y, pB.z);
        }
    }
}

// per GN iteration: the sufficient statistics of every pair of this shard (one wave per pair,
// lanes over its correspondences in ascending index order, fixed butterfly); pairs of other shards
// and slots in [nPairs, pairBound) are written as zeros
__global__ __launch_bounds__(WG) void k_pair_stats(BA a) {
    if (a.ctrl[K_GN_DONE]) return;
    const uint32_t lane = lane_id();
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
    const uint32_t np = a.ctrl[K_NPAIRS_A];
    const uint32_t bound = a.pairBound > np ? a.pairBound : np;
    if (a.pairBound && np > a.pairBound && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&a.ctrl[K_ERROR], 4u);
    for (uint32_t p = wave; p < bound; p += nw) {
        double* out = a.pstat + (size_t)p * PSTAT;
        if (p >= np || p % a.shardCount != a.shardIndex) {
            if (lane < PSTAT) out[lane] = 0.0;
            continue;
        }
        const uint32_t pa = (uint32_t)a.pairA[p], pb = (uint32_t)a.pairB[p];
        const int2 run = a.pairCorr[p];
        const m4 Ta = loadm4(a.T + (size_t)pa * 16), Tb = loadm4(a.T + (size_t)pb * 16);
        double M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, sa[3] = {0, 0, 0}, sb[3] = {0, 0, 0}, cnt = 0.0;
        double qa[6] = {0, 0, 0, 0, 0, 0}, qb[6] = {0, 0, 0, 0, 0, 0};
        const float2* tail = reinterpret_cast<const float2*>(a.entries + a.entTail);
        for (int k = (int)lane; k < run.y; k += 64) {
            const float4 x = a.entries[run.x + k];  // k_pair_gather's copy, contiguous per pair
            const float2 y = tail[run.x + k];
            const f3 pA = mk3(x.x, x.y, x.z), pB = mk3(x.w, y.x, y.y);
            const f3 A3 = xf(Ta, pA), B3 = xf(Tb, pB);  // the world points of k_entries
            const double A[3] = {A3.x, A3.y, A3.z}, B[3] = {B3.x, B3.y, B3.z};
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int c = 0; c < 3; c++) M[r * 3 + c] += B[r] * A[c];
                sa[r] += A[r];
                sb[r] += B[r];
            }
            qa[0] += A[0] * A[0]; qa[1] += A[0] * A[1]; qa[2] += A[0] * A[2];
            qa[3] += A[1] * A[1]; qa[4] += A[1] * A[2]; qa[5] += A[2] * A[2];
            qb[0] += B[0] * B[0]; qb[1] += B[0] * B[1]; qb[2] += B[0] * B[2];
            qb[3] += B[1] * B[1]; qb[4] += B[1] * B[2]; qb[5] += B[2] * B[2];
            cnt += 1.0;
        }
        double s[PSTAT];
#pragma unroll
        for (int q = 0; q < 9; q++) s[q] = M[q];
#pragma unroll
        for (int q = 0; q < 3; q++) { s[9 + q] = sa[q]; s[12 + q] = sb[q]; }
        s[15] = cnt;
#pragma unroll
        for (int q = 0; q < 6; q++) { s[16 + q] = qa[q]; s[22 + q] = qb[q]; }
#pragma unroll
        for (int q = 0; q < PSTAT; q++) s[q] = wave_sum_d(s[q]) + 0.0;  // + 0.0: no -0 (exact shard sums)
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < PSTAT; q += 2) *reinterpret_cast<double2*>(out + q) = make_double2(s[q], s[q + 1]);
        }
    }
}

// B_vu p_u for the row entry (pair p, orientation): rot = tr(M) w - M w + s_v x t, trans = -s_u x w + n t,
// with M = sum P_u P_v^T (the pair's M for v = a, its transpose for v = b)
__device__ __forceinline__ void pair_block_apply(const double* st, bool vIsA, const double w[3], const double t[3],
                                                 double o[6]) {
    double M[9];
#pragma unroll
    for (int q = 0; q < 9; q++) M[q] = st[q];
    const double* sv = vIsA ? st + 9 : st + 12;
    const double* su = vIsA ? st + 12 : st + 9;
    const double n = st[15];
    const double tr = M[0] + M[4] + M[8];
    double Mw[3];
#pragma unroll
    for (int r = 0; r < 3; r++)
        Mw[r] = vIsA ? (M[r * 3] * w[0] + M[r * 3 + 1] * w[1] + M[r * 3 + 2] * w[2])
                     : (M[r] * w[0] + M[3 + r] * w[1] + M[6 + r] * w[2]);
    o[0] = tr * w[0] - Mw[0] + (sv[1] * t[2] - sv[2] * t[1]);
    o[1] = tr * w[1] - Mw[1] + (sv[2] * t[0] - sv[0] * t[2]);
    o[2] = tr * w[2] - Mw[2] + (sv[0] * t[1] - sv[1] * t[0]);
    o[3] = -(su[1] * w[2] - su[2] * w[1]) + n * t[0];
    o[4] = -(su[2] * w[0] - su[0] * w[2]) + n * t[1];
    o[5] = -(su[0] * w[1] - su[1] * w[0]) + n * t[2];
}
// D_v p_v from the image statistics Q (xx xy xz yy yz zz), s, n
__device__ __forceinline__ void diag_apply(const double* d, const double w[3], const double t[3], double o[6]) {
    const double Q[9] = {d[0], d[1], d[2], d[1], d[3], d[4], d[2], d[4], d[5]};
    const double* s = d + 6;
    const double n = d[9], tr = d[0] + d[3] + d[5];
#pragma unroll
    for (int r = 0; r < 3; r++) o[r] = tr * w[r] - (Q[r * 3] * w[0] + Q[r * 3 + 1] * w[1] + Q[r * 3 + 2] * w[2]);
    o[0] += s[1] * t[2] - s[2] * t[1];
    o[1] += s[2] * t[0] - s[0] * t[2];
    o[2] += s[0] * t[1] - s[1] * t[0];
    o[3] = -(s[1] * w[2] - s[2] * w[1]) + n * t[0];
    o[4] = -(s[2] * w[0] - s[0] * w[2]) + n * t[1];
    o[5] = -(s[0] * w[1] - s[1] * w[0]) + n * t[2];
}

}  // namespace
}  // namespace bf
