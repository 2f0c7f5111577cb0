// ba_pcg.h — a GN step's setup and the PCG routes with a kernel boundary per iteration, or one workgroup.
// Kernels: k_transforms, then matrix-free k_entries, k_init, k_pcg (one launch per iteration); pair mode
// k_pair_init, then k_pcg_pairs<2|8> (one launch per iteration) or k_pcg_small (N <= 64, one workgroup,
// every iteration). pcg_finisher / pcg_finish_regs, pair_init_row, pair_init_finish, pair_row_ap and
// pcg_dense_offdiag are shared with ba_persist.h, whose results must equal these routes' bit for bit.
// Relies on ba_dev.h (the PCG step rule, hand-offs, sums) and ba_table.h (chunk_range, pair blocks).
#pragma once
#include "ba_dev.h"
#include "ba_table.h"

namespace bf {
namespace {

// ---- per GN iteration -------------------------------------------------------------------------
// convertLiePosesToMatricesCU (SolverBundling.cu:1114-1121); also resets the PCG state of this
// GN iteration. gated: no-op once the GN loop converged on the device.
__device__ __forceinline__ void transforms_rows(const BA& a, uint32_t first, uint32_t stride) {
    for (uint32_t v = first; v < a.N; v += stride) {
        const m4 T = pose_to_matrix(mk3(a.rot[3 * v], a.rot[3 * v + 1], a.rot[3 * v + 2]),
                                    mk3(a.trans[3 * v], a.trans[3 * v + 1], a.trans[3 * v + 2]));
        const m4 Ti = inverse44(T);
        float4* t = reinterpret_cast<float4*>(a.T + (size_t)v * 16);
        float4* ti = reinterpret_cast<float4*>(a.Tinv + (size_t)v * 16);
        for (int r = 0; r < 4; r++) {
            t[r] = make_float4(T.e[r * 4], T.e[r * 4 + 1], T.e[r * 4 + 2], T.e[r * 4 + 3]);
            ti[r] = make_float4(Ti.e[r * 4], Ti.e[r * 4 + 1], Ti.e[r * 4 + 2], Ti.e[r * 4 + 3]);
        }
    }
}
__global__ void k_transforms(BA a, float wSparse, int useDense, int gated, int setState) {
    if (gated && a.ctrl[K_GN_DONE]) return;
    transforms_rows(a, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
    if (setState && blockIdx.x == 0 && threadIdx.x == 0) {
        a.ctrl[K_PCG_DONE] = 0;
        a.ctrl[K_TICKET] = 0;
        a.ctrl[K_LAST_W] = __float_as_uint(wSparse);
        a.ctrl[K_USE_DENSE] = (uint32_t)useDense;
    }
}

// chunk partials are handed to the finishing workgroup write-through (see last_block)
__device__ __forceinline__ void put_part(const BA& a, uint32_t c, int f, f3 s) {
    st_wt(a.chunkPart + (size_t)c * 3 + f, make_float4(s.x, s.y, s.z, 0.0f));
}
// PCGInit per row: r = -Jtr, Jacobi preconditioner, p = M r; returns r.z
__device__ float init_row_cnt(const BA& a, uint32_t v, f3 rr, f3 rt, f3 pr, float cnt, float wSparse, int useDense) {
    f3 resR = mk3(-wSparse * rr.x, -wSparse * rr.y, -wSparse * rr.z);
    f3 resT = mk3(-wSparse * rt.x, -wSparse * rt.y, -wSparse * rt.z);
    if (useDense) {
        const float* j = a.jtr + (size_t)v * 6;
        resR = resR - mk3(j[3], j[4], j[5]);
        resT = resT - mk3(j[0], j[1], j[2]);
    }
    auto inv = [](float x) { return x > FLOAT_EPSILON ? 1.0f / x : 1.0f; };
    const f3 mR = mk3(inv(pr.x), inv(pr.y), inv(pr.z));
    const f3 mT = mk3(inv(cnt), inv(cnt), inv(cnt));
    const f3 pR = mul3(mR, resR), pT = mul3(mT, resT);
    vstore(a, V_M, v, mR, mT);
    vstore(a, V_R, v, resR, resT);
    vstore(a, V_P, v, pR, pT);
    vstore(a, V_DELTA, v, mk3(0, 0, 0), mk3(0, 0, 0));
    return dot3(resR, pR) + dot3(resT, pT);
}
__device__ float init_row(const BA& a, uint32_t v, f3 rr, f3 rt, f3 pr, float wSparse, int useDense) {
    return init_row_cnt(a, v, rr, rt, pr, (float)a.rowLen[v], wSparse, useDense);
}

// world points of every row entry for this GN iteration: {T_self p_self, other}, {T_other p_other}
__global__ __launch_bounds__(WG) void k_entries(BA a) {
    if (a.ctrl[K_GN_DONE]) return;
    const uint32_t lane = lane_id();
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
    const uint32_t nch = a.ctrl[K_NCHUNK];
    for (uint32_t c = wave; c < nch; c += nw) {
        uint32_t v;
        int k0, k1;
        chunk_range(a, c, v, k0, k1);
        const m4 Tv = loadm4(a.T + (size_t)v * 16);
        int idx[CPL];
#pragma unroll
        for (int u = 0; u < CPL; u++) idx[u] = a.rowIdx[min(k0 + (int)lane + 64 * u, k1 - 1)];
        BFEntryJ ev[CPL];
#pragma unroll
        for (int u = 0; u < CPL; u++) ev[u] = a.corr[idx[u]];
#pragma unroll
        for (int u = 0; u < CPL; u++) {
            const int k = k0 + (int)lane + 64 * u;
            if (k >= k1) break;
            const BFEntryJ e = ev[u];
            const bool isI = (e.imgIdx_i == v);
            const uint32_t other = isI ? e.imgIdx_j : e.imgIdx_i;
            const f3 ps = isI ? mk3(e.pos_i.x, e.pos_i.y, e.pos_i.z) : mk3(e.pos_j.x, e.pos_j.y, e.pos_j.z);
            const f3 po = isI ? mk3(e.pos_j.x, e.pos_j.y, e.pos_j.z) : mk3(e.pos_i.x, e.pos_i.y, e.pos_i.z);
            const f3 Ps = xf(Tv, ps);
            const f3 Po = xf(loadm4(a.T + (size_t)other * 16), po);
            a.entries[2 * k] = make_float4(Ps.x, Ps.y, Ps.z, __uint_as_float(other));
            a.entries[2 * k + 1] = make_float4(Po.x, Po.y, Po.z, 0.0f);
        }
    }
}

// evalMinusJTFDevice (SolverBundlingEquationsLie.h:63-148) + PCGInit_Kernel1/2 (SolverBundling.cu:755-794).
// Every wave reduces one chunk; the last workgroup sums each row's chunk partials (chunk order),
// initialises the row and sums r.z.
__global__ __launch_bounds__(WG) void k_init(BA a, float wSparse) {
    __shared__ float sh[WG];
    if (a.ctrl[K_GN_DONE]) return;
    const uint32_t lane = lane_id();
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
    const uint32_t nch = a.ctrl[K_NCHUNK];
    const int useDense = (int)a.ctrl[K_USE_DENSE];
    for (uint32_t c = wave; c < nch; c += nw) {
        uint32_t v;
        int k0, k1;
        chunk_range(a, c, v, k0, k1);
        float rr[3] = {0, 0, 0}, rt[3] = {0, 0, 0}, pr[3] = {0, 0, 0};
        float4 A[CPL], B[CPL];
#pragma unroll
        for (int u = 0; u < CPL; u++) {
            const int k = min(k0 + (int)lane + 64 * u, k1 - 1);
            A[u] = a.entries[2 * k];
            B[u] = a.entries[2 * k + 1];
        }
#pragma unroll
        for (int u = 0; u < CPL; u++) {
            f3 Ps = mk3(A[u].x, A[u].y, A[u].z), Po = mk3(B[u].x, B[u].y, B[u].z);
            if (k0 + (int)lane + 64 * u >= k1) { Ps = mk3(0, 0, 0); Po = Ps; }
            const f3 r = Ps - Po;         // sign * (T_i p_i - T_j p_j)
            const f3 cr = cross3(Ps, r);  // (dot(da,r), dot(db,r), dot(dc,r)) of P_s
            rr[0] += cr.x; rr[1] += cr.y; rr[2] += cr.z;
            rt[0] += r.x; rt[1] += r.y; rt[2] += r.z;
            pr[0] += Ps.z * Ps.z + Ps.y * Ps.y;  // |dAlpha|^2
            pr[1] += Ps.z * Ps.z + Ps.x * Ps.x;  // |dBeta|^2
            pr[2] += Ps.y * Ps.y + Ps.x * Ps.x;  // |dGamma|^2
        }
        for (int q = 0; q < 3; q++) { rr[q] = wave_sum(rr[q]); rt[q] = wave_sum(rt[q]); pr[q] = wave_sum(pr[q]); }
        if (lane == 0) {
            put_part(a, c, 0, mk3(rr[0], rr[1], rr[2]));
            put_part(a, c, 1, mk3(rt[0], rt[1], rt[2]));
            put_part(a, c, 2, mk3(pr[0], pr[1], pr[2]));
        }
    }
    if (!last_block(&a.ctrl[K_TICKET])) return;
    float s = 0.0f;
    for (uint32_t v = 1 + threadIdx.x; v < a.N; v += blockDim.x) {
        f3 sR = mk3(0, 0, 0), sT = sR, sP = sR;
        for (int c = a.rowChunk[v]; c < a.rowChunk[v + 1]; c++) {
            const float4 x = ld_wt(a.chunkPart + (size_t)c * 3), y = ld_wt(a.chunkPart + (size_t)c * 3 + 1),
                         z = ld_wt(a.chunkPart + (size_t)c * 3 + 2);
            sR = sR + mk3(x.x, x.y, x.z);
            sT = sT + mk3(y.x, y.y, y.z);
            sP = sP + mk3(z.x, z.y, z.z);
        }
        s += init_row(a, v, sR, sT, sP, wSparse, useDense);
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0) {
        a.ctrl[K_RDOTZ] = __float_as_uint(s);
        a.ctrl[K_TICKET] = 0;
        for (int w = 0; w < SYNC_WORDS; w += SYNC_LINE) a.sync[w] = 0;  // the PCG launches' arrival counters
        vstore(a, V_P, 0, mk3(0, 0, 0), mk3(0, 0, 0));  // image 0 is fixed: its p stays 0
    }
}

// sparse JtJp partial of every chunk (one wave per chunk), handed over write-through
template <bool WT>
__device__ __forceinline__ void pcg_sparse_chunks(const BA& a, float wSparse, uint32_t wave, uint32_t nw, uint32_t nch) {
    const uint32_t lane = lane_id();
    for (uint32_t c = wave; c < nch; c += nw) {
        uint32_t v;
        int k0, k1;
        chunk_range(a, c, v, k0, k1);
        f3 pRv, pTv;
        vload_t<WT>(a, V_P, v, pRv, pTv);
        float ar[3] = {0, 0, 0}, at[3] = {0, 0, 0};
        // all CH/64 entries of this lane are loaded before any is used (clamped indices, masked
        // sums: no per-entry branch), so a chunk costs one HBM round trip plus one L2 gather
        float4 A[CPL], B[CPL];
#pragma unroll
        for (int u = 0; u < CPL; u++) {
            const int k = min(k0 + (int)lane + 64 * u, k1 - 1);
            A[u] = a.entries[2 * k];
            B[u] = a.entries[2 * k + 1];
        }
#pragma unroll
        for (int u = 0; u < CPL; u++) {
            const f3 Ps = mk3(A[u].x, A[u].y, A[u].z), Po = mk3(B[u].x, B[u].y, B[u].z);
            const uint32_t o = __float_as_uint(A[u].w);
            f3 pRo, pTo;
            vload_t<WT>(a, V_P, o, pRo, pTo);
            f3 g = (cross3(pRv, Ps) + pTv - (cross3(pRo, Po) + pTo)) * wSparse;
            f3 cr = cross3(Ps, g);
            if (k0 + (int)lane + 64 * u >= k1) { g = mk3(0, 0, 0); cr = g; }
            ar[0] += cr.x; ar[1] += cr.y; ar[2] += cr.z;
            at[0] += g.x; at[1] += g.y; at[2] += g.z;
        }
        for (int q = 0; q < 3; q++) { ar[q] = wave_sum(ar[q]); at[q] = wave_sum(at[q]); }
        if (lane == 0) { put_part(a, c, 0, mk3(ar[0], ar[1], ar[2])); put_part(a, c, 1, mk3(at[0], at[1], at[2])); }
    }
}

// Ap of row v for the finisher: the sparse part handed over by the row's last chunk wave, plus the
// dense diagonal block and the dense off-diagonal atomics (reset for the next iteration)
__device__ __forceinline__ void pcg_ap(const BA& a, uint32_t v, uint32_t nch, int useDense, f3 pR, f3 pT, f3& aR, f3& aT) {
    aR = mk3(0, 0, 0);
    aT = mk3(0, 0, 0);
    if (a.pairMode) {  // assembled normal equations: sparse Ap of the row, handed over by its wave
        const float4* q = reinterpret_cast<const float4*>(a.apPair + (size_t)v * 8);
        const float4 x = ld_wt(q), y = ld_wt(q + 1);
        aR = mk3(x.x, x.y, x.z);
        aT = mk3(y.x, y.y, y.z);
    } else if (nch) {  // sparse part: the row's chunk partials, in chunk order
        const int c1 = a.rowChunk[v + 1];
#pragma unroll 4
        for (int c = a.rowChunk[v]; c < c1; c++) {
            const float4 x = ld_wt(a.chunkPart + (size_t)c * 3), y = ld_wt(a.chunkPart + (size_t)c * 3 + 1);
            aR = aR + mk3(x.x, x.y, x.z);
            aT = aT + mk3(y.x, y.y, y.z);
        }
    }
    if (useDense) {  // diagonal block [trans | rot] x [pTrans | pRot]
        const float* D = a.diag + (size_t)v * 36;
        const float pv[6] = {pT.x, pT.y, pT.z, pR.x, pR.y, pR.z};
        float o6[6];
        for (int r = 0; r < 6; r++) {
            float s = 0.0f;
            for (int c = 0; c < 6; c++) s += D[r * 6 + c] * pv[c];
            o6[r] = s;
        }
        aT = aT + mk3(o6[0], o6[1], o6[2]);
        aR = aR + mk3(o6[3], o6[4], o6[5]);
        // off-diagonal blocks: the row's sum over its pairs of this launch (pcg_dense_offdiag, write-through)
        const float* pp = a.pairProd + (size_t)v * 8;
        aT = aT + mk3(ld_wtf(pp), ld_wtf(pp + 1), ld_wtf(pp + 2));
        aR = aR + mk3(ld_wtf(pp + 3), ld_wtf(pp + 4), ld_wtf(pp + 5));
    }
}

// PCG finisher with each thread's R rows held in registers: all loads issue up front, then the
// two block reductions, then the stores (z and Ap never go to memory). Same arithmetic as the
// multi-pass form below.
// R = 8 (514..2 049 images): the two dot products are summed as FIN_GROUPS block sums of two rows per
// thread each (rows q = 2g, 2g + 1), added in group order: the order of k_pcg_persist's four-workgroup
// finisher (pcg_persist_finisher_x4), so the persistent and the per-launch solves agree bit for bit
constexpr int FIN_GROUPS = 4;
template <int R>
__device__ __forceinline__ float grouped_sum(const float* e, float* sh) {
    if (R != 8) return block_sum(e[0], sh);
    float t = 0.0f;
#pragma unroll
    for (int g = 0; g < FIN_GROUPS; g++) t += block_sum(e[g], sh);
    return t;
}
template <int R, bool WT>
__device__ float pcg_finish_regs(const BA& a, float* sh, uint32_t nch, int useDense, int iter, int nLin, bool& lastOut) {
    f3 pR[R], pT[R], aR[R], aT[R], dR[R], dT[R], rR[R], rT[R], mR[R], mT[R];
    constexpr int NG = R == 8 ? FIN_GROUPS : 1;
    float d[NG];
#pragma unroll
    for (int g = 0; g < NG; g++) d[g] = 0.0f;
#pragma unroll
    for (int q = 0; q < R; q++) {
        const uint32_t v = 1 + threadIdx.x + q * WG;
        if (v < a.N) {
            vload_t<WT>(a, V_P, v, pR[q], pT[q]);
            vload_t<WT>(a, V_DELTA, v, dR[q], dT[q]);
            vload_t<WT>(a, V_R, v, rR[q], rT[q]);
            vload_t<WT>(a, V_M, v, mR[q], mT[q]);
            pcg_ap(a, v, nch, useDense, pR[q], pT[q], aR[q], aT[q]);
            d[NG > 1 ? q / 2 : 0] += dot3(pR[q], aR[q]) + dot3(pT[q], aT[q]);
        }
    }
    const float pAp = grouped_sum<R>(d, sh);
    const float rDotzOld = WT ? __uint_as_float(ld_wt(&a.ctrl[K_RDOTZ])) : ctrlf(a.ctrl, K_RDOTZ);
    const float alpha = pcg_alpha(rDotzOld, pAp);
    float b[NG];
#pragma unroll
    for (int g = 0; g < NG; g++) b[g] = 0.0f;
#pragma unroll
    for (int q = 0; q < R; q++) {
        if (1 + threadIdx.x + q * WG < a.N) {
            dR[q] = dR[q] + alpha * pR[q];
            dT[q] = dT[q] + alpha * pT[q];
            rR[q] = rR[q] - alpha * aR[q];
            rT[q] = rT[q] - alpha * aT[q];
            mR[q] = mul3(mR[q], rR[q]);  // z
            mT[q] = mul3(mT[q], rT[q]);
            b[NG > 1 ? q / 2 : 0] += dot3(mR[q], rR[q]) + dot3(mT[q], rT[q]);
        }
    }
    const float rDotzNew = grouped_sum<R>(b, sh);
    // pcg_last's test, written out: the call moved this finisher's register allocation
    const bool last = (iter == nLin - 1) || (a.earlyOut && fabsf(pAp) < 5e-7f);
    const float beta = pcg_beta(rDotzNew, rDotzOld);
#pragma unroll
    for (int q = 0; q < R; q++) {
        const uint32_t v = 1 + threadIdx.x + q * WG;
        if (v < a.N) {
            vstore_t<WT>(a, V_DELTA, v, dR[q], dT[q]);
            vstore_t<WT>(a, V_R, v, rR[q], rT[q]);
            vstore_t<WT>(a, V_P, v, mR[q] + beta * pR[q], mT[q] + beta * pT[q]);
            if (last) {  // computeLieUpdate (LieDerivUtil.h:301-307)
                f3 nr, nt;
                lie_update(dR[q], dT[q], mk3(a.rot[3 * v], a.rot[3 * v + 1], a.rot[3 * v + 2]),
                           mk3(a.trans[3 * v], a.trans[3 * v + 1], a.trans[3 * v + 2]), nr, nt);
                a.rot[3 * v] = nr.x; a.rot[3 * v + 1] = nr.y; a.rot[3 * v + 2] = nr.z;
                a.trans[3 * v] = nt.x; a.trans[3 * v + 1] = nt.y; a.trans[3 * v + 2] = nt.z;
            }
        }
    }
    lastOut = last;
    return rDotzNew;
}

// dense off-diagonal blocks, per image v (one wave each): Σ over v's pairs, in pair order, of B p_i
// (v = the pair's j) or B^T p_j (v = its i), [trans | rot] rows. Lanes form 10 groups of 6 (one lane
// per output row); group g takes the list entries g, g + 10, ...; the groups' partial sums are then
// added in group order, so the sum is the same on every run. Stored write-through for the finisher.
// granTag != 0 (k_pcg_persist): the products go out as Ap granules of that tag
template <bool WT>
__device__ void pcg_dense_offdiag_row(const BA& a, uint32_t v, uint32_t granTag = 0) {
    const uint32_t lane = lane_id();
    const uint32_t grp = lane / 6, row = lane % 6;
    const uint32_t* L = a.imgPairs + (size_t)v * a.maxN;
    const uint32_t nL = a.imgPairN[v];
    float o = 0.0f;
    if (grp < 10) {
        for (uint32_t q = grp; q < nL; q += 10) {
            const uint32_t e = L[q], k = e >> 1;
            const uint2 pr = a.pairs[k];
            const float* Bk = a.pairBlk + (size_t)k * 36;  // rows: image pr.y, columns: image pr.x
            f3 r, t;
            vload_t<WT>(a, V_P, (e & 1u) ? pr.x : pr.y, r, t);
            const float pv[6] = {t.x, t.y, t.z, r.x, r.y, r.z};
            float s = 0.0f;
            if (e & 1u) { for (int c = 0; c < 6; c++) s += Bk[row * 6 + c] * pv[c]; }
            else { for (int rr = 0; rr < 6; rr++) s += Bk[rr * 6 + row] * pv[rr]; }
            if ((e & 1u) ? pr.x > 0 : pr.y > 0) o += s;  // p_0 = 0 (image 0 fixed)
        }
    }
    float tot = 0.0f;
    for (uint32_t g = 0; g < 10; g++) tot += __shfl(o, (int)(g * 6 + row));
    if (lane < 6) {
        if (granTag) gran_store(a.aGran + ((size_t)a.maxN + v) * 6 + lane, tot, granTag);  // k_pcg_persist
        else st_wt(reinterpret_cast<uint32_t*>(a.pairProd) + (size_t)v * 8 + lane, __float_as_uint(tot));
    }
}
__device__ void pcg_dense_offdiag(const BA& a, uint32_t wave, uint32_t nw) {
    for (uint32_t v = 1 + wave; v < a.N; v += nw) pcg_dense_offdiag_row<false>(a, v);
}

// PCG finisher (one workgroup): Kernel1b, Kernel2, the host early-out test, Kernel3
template <int RB = 2>
__device__ void pcg_finisher(const BA& a, float* sh, uint32_t nch, int useDense, int iter, int nLin, float& rDotzNew,
                             bool& last) {
    if (a.N <= RB * WG + 1) {
        rDotzNew = pcg_finish_regs<RB, false>(a, sh, nch, useDense, iter, nLin, last);
    } else {
        float d = 0.0f;
        for (uint32_t v = 1 + threadIdx.x; v < a.N; v += blockDim.x) {
            f3 pR, pT, aR, aT;
            vload(a, V_P, v, pR, pT);
            pcg_ap(a, v, nch, useDense, pR, pT, aR, aT);
            vstore(a, V_AP, v, aR, aT);
            d += dot3(pR, aR) + dot3(pT, aT);
        }
        const float pAp = block_sum(d, sh);
        const float rDotzOld = ctrlf(a.ctrl, K_RDOTZ);
        const float alpha = pcg_alpha(rDotzOld, pAp);
        float b = 0.0f;
        for (uint32_t v = 1 + threadIdx.x; v < a.N; v += blockDim.x) {
            f3 dR, dT, pR, pT, rR, rT, aR, aT, mR, mT;
            vload(a, V_DELTA, v, dR, dT);
            vload(a, V_P, v, pR, pT);
            vload(a, V_R, v, rR, rT);
            vload(a, V_AP, v, aR, aT);
            vload(a, V_M, v, mR, mT);
            dR = dR + alpha * pR;
            dT = dT + alpha * pT;
            rR = rR - alpha * aR;
            rT = rT - alpha * aT;
            const f3 zR = mul3(mR, rR), zT = mul3(mT, rT);
            vstore(a, V_DELTA, v, dR, dT);
            vstore(a, V_R, v, rR, rT);
            vstore(a, V_Z, v, zR, zT);
            b += dot3(zR, rR) + dot3(zT, rT);
        }
        const float rDotzNew_ = block_sum(b, sh);
        const bool last_ = (iter == nLin - 1) || (a.earlyOut && fabsf(pAp) < 5e-7f);  // pcg_last, as above
        const float beta = pcg_beta(rDotzNew_, rDotzOld);
        for (uint32_t v = 1 + threadIdx.x; v < a.N; v += blockDim.x) {
            f3 zR, zT, pR, pT;
            vload(a, V_Z, v, zR, zT);
            vload(a, V_P, v, pR, pT);
            vstore(a, V_P, v, zR + beta * pR, zT + beta * pT);
            if (last_) {  // computeLieUpdate (LieDerivUtil.h:301-307)
                f3 dR, dT;
                vload(a, V_DELTA, v, dR, dT);
                f3 nr, nt;
                lie_update(dR, dT, mk3(a.rot[3 * v], a.rot[3 * v + 1], a.rot[3 * v + 2]),
                           mk3(a.trans[3 * v], a.trans[3 * v + 1], a.trans[3 * v + 2]), nr, nt);
                a.rot[3 * v] = nr.x; a.rot[3 * v + 1] = nr.y; a.rot[3 * v + 2] = nr.z;
                a.trans[3 * v] = nt.x; a.trans[3 * v + 1] = nt.y; a.trans[3 * v + 2] = nt.z;
            }
        }
        rDotzNew = rDotzNew_;
        last = last_;
    }
}

// One PCG iteration (PCGIteration, SolverBundling.cu:1024-1108) in one launch: every wave
// computes the sparse JtJp partial of its chunks; waves also apply the dense off-diagonal pair
// blocks. The last workgroup then sums each row's partials in chunk order, adds the dense diagonal
// block, does the global dot products and the alpha / beta updates (Kernel1b, Kernel2, Kernel3) and
// the Lie update on the exiting iteration.
__global__ __launch_bounds__(WG) void k_pcg(BA a, float wSparse, int iter, int nLin) {
    __shared__ float sh[WG];
    if (a.ctrl[K_GN_DONE] || a.ctrl[K_PCG_DONE]) return;
    const uint32_t lane = lane_id();  // unused; without it the prologue's instructions come out in another order
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
    const int useDense = (int)a.ctrl[K_USE_DENSE];
    const uint32_t nch = (wSparse > 0.0f) ? a.ctrl[K_NCHUNK] : 0u;
    pcg_sparse_chunks<false>(a, wSparse, wave, nw, nch);
    if (useDense) pcg_dense_offdiag(a, wave, nw);
    if (!last_block_sharded(a.sync, 1u)) return;
    if (threadIdx.x < 9) a.sync[threadIdx.x * SYNC_LINE] = 0;  // counters of the next launch
    // ---- finisher (one workgroup): Kernel1b, Kernel2, host early-out test, Kernel3 ----
    float rDotzNew;
    bool last;
    pcg_finisher(a, sh, nch, useDense, iter, nLin, rDotzNew, last);
    if (threadIdx.x == 0) pcg_iter_end(a, rDotzNew, last);
}

// Pair mode, per GN iteration after the exchange: one wave per image row v >= 1 sums its incident
// pairs (in partner order) into D_v (the diagonal block statistics), J^T F and the Jacobi
// preconditioner, then initialises the row as PCGInit does (evalMinusJTFDevice + PCGInit_Kernel1,
// SolverBundlingEquationsLie.h:63-148, SolverBundling.cu:755-794); the last workgroup sums r.z.
// Row v (one wave); lane 0 also keeps the row's pose as it was before the GN step (a.poseBak, the
// state pcg_recover restarts from)
__device__ void pair_init_row(const BA& a, float wSparse, uint32_t v, bool backup) {
    const uint32_t lane = lane_id();
    {
        const int e0 = a.rowPairStart[v], e1 = a.rowPairStart[v + 1];
        double d[DSTAT + 6];
#pragma unroll
        for (int q = 0; q < DSTAT + 6; q++) d[q] = 0.0;
        for (int k = e0 + (int)lane; k < e1; k += 64) {
            const int2 rp = a.rowPair[k];
            const bool vIsA = ((uint32_t)rp.y & PAIR_A_FLAG) != 0;
            const double* st = a.pstat + (size_t)rp.x * PSTAT;
            const double* qv = st + (vIsA ? 16 : 22);
            const double* sv = st + (vIsA ? 9 : 12);
            const double* su = st + (vIsA ? 12 : 9);
#pragma unroll
            for (int q = 0; q < 6; q++) d[q] += qv[q];
#pragma unroll
            for (int q = 0; q < 3; q++) d[6 + q] += sv[q];
            d[9] += st[15];
            // sum P_v x (P_v - P_u) = -/+ sum P_a x P_b, the antisymmetric part of M = sum P_b P_a^T
            const double sg = vIsA ? -1.0 : 1.0;
            d[10] += sg * (st[7] - st[5]);
            d[11] += sg * (st[2] - st[6]);
            d[12] += sg * (st[3] - st[1]);
#pragma unroll
            for (int q = 0; q < 3; q++) d[13 + q] += sv[q] - su[q];
        }
#pragma unroll
        for (int q = 0; q < DSTAT + 6; q++) d[q] = wave_sum_d(d[q]);
        if (lane == 0) {
            double* ds = a.dstat + (size_t)v * DSTAT;
#pragma unroll
            for (int q = 0; q < DSTAT; q += 2) *reinterpret_cast<double2*>(ds + q) = make_double2(d[q], d[q + 1]);
            const f3 rr = mk3((float)d[10], (float)d[11], (float)d[12]);
            const f3 rt = mk3((float)d[13], (float)d[14], (float)d[15]);
            // |dAlpha|^2, |dBeta|^2, |dGamma|^2 summed: (Qyy + Qzz, Qxx + Qzz, Qxx + Qyy)
            const f3 pr = mk3((float)(d[3] + d[5]), (float)(d[0] + d[5]), (float)(d[0] + d[3]));
            st_wt(&a.rzPart[v], init_row_cnt(a, v, rr, rt, pr, (float)d[9], wSparse, (int)a.ctrl[K_USE_DENSE]));
        }
        if (backup && lane < 6) a.poseBak[(size_t)v * 6 + lane] = lane < 3 ? a.rot[3 * v + lane] : a.trans[3 * v + lane - 3];
    }
}
// r.z summed over the rows by one workgroup (k_pair_init's last), PCG counters reset, p_0 = 0
__device__ void pair_init_finish(const BA& a, float* sh) {
    float s = 0.0f;
    for (uint32_t v = 1 + threadIdx.x; v < a.N; v += blockDim.x) s += ld_wtf(&a.rzPart[v]);
    s = block_sum(s, sh);
    if (threadIdx.x == 0) {
        a.ctrl[K_RDOTZ] = __float_as_uint(s);
        a.ctrl[K_TICKET] = 0;
        for (int w = 0; w < SYNC_WORDS; w += SYNC_LINE) a.sync[w] = 0;
        vstore(a, V_P, 0, mk3(0, 0, 0), mk3(0, 0, 0));  // image 0 is fixed: its p stays 0
    }
}
__global__ __launch_bounds__(WG) void k_pair_init(BA a, float wSparse) {
    __shared__ float sh[WG];
    if (a.ctrl[K_GN_DONE]) return;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t v = 1 + wave; v < a.N; v += nw) pair_init_row(a, wSparse, v, true);
    if (!last_block(&a.ctrl[K_TICKET])) return;
    if (threadIdx.x == 0) a.ctrl[K_PCG_ITERS0] = a.ctrl[K_PCG_ITERS];
    pair_init_finish(a, sh);
}

// Ap of row v (one wave), handed to the finisher write-through: k_pcg_pairs and pcg_recover
__device__ void pair_row_ap(const BA& a, float wSparse, uint32_t v) {
    const uint32_t lane = lane_id();
    const int e0 = a.rowPairStart[v], e1 = a.rowPairStart[v + 1];
    // the row's own p and image statistics, loaded beside the pair loop (lane 0 uses them)
    f3 pvR, pvT;
    vload(a, V_P, v, pvR, pvT);
    double dst[DSTAT];
#pragma unroll
    for (int q = 0; q < DSTAT; q++) dst[q] = a.dstat[(size_t)v * DSTAT + q];
    double o[6] = {0, 0, 0, 0, 0, 0};
    // two entries per lane per round (k and k + 64), every load of both issued before either is
    // used: one round of dependent loads (entry, then partner p + pair statistics) per 128 entries;
    // each lane still adds its entries in ascending k, so the sums equal the one-entry loop's
    for (int kb = e0; kb < e1; kb += 128) {
        const int k0 = kb + (int)lane, k1 = k0 + 64;
        const int2 rp0 = a.rowPair[min(k0, e1 - 1)], rp1 = a.rowPair[min(k1, e1 - 1)];
        const uint32_t u0 = (uint32_t)rp0.y & ~PAIR_A_FLAG, u1 = (uint32_t)rp1.y & ~PAIR_A_FLAG;
        f3 pr0, pt0, pr1, pt1;
        vload(a, V_P, u0, pr0, pt0);
        vload(a, V_P, u1, pr1, pt1);
        double st0[16], st1[16];
#pragma unroll
        for (int q = 0; q < 16; q += 2) {
            const double2 x0 = *reinterpret_cast<const double2*>(a.pstat + (size_t)rp0.x * PSTAT + q);
            const double2 x1 = *reinterpret_cast<const double2*>(a.pstat + (size_t)rp1.x * PSTAT + q);
            st0[q] = x0.x; st0[q + 1] = x0.y;
            st1[q] = x1.x; st1[q + 1] = x1.y;
        }
        if (k0 < e1 && u0 != 0) {  // p_0 = 0 (image 0 fixed)
            const double w[3] = {pr0.x, pr0.y, pr0.z}, t[3] = {pt0.x, pt0.y, pt0.z};
            double b[6];
            pair_block_apply(st0, ((uint32_t)rp0.y & PAIR_A_FLAG) != 0, w, t, b);
#pragma unroll
            for (int q = 0; q < 6; q++) o[q] += b[q];
        }
        if (k1 < e1 && u1 != 0) {
            const double w[3] = {pr1.x, pr1.y, pr1.z}, t[3] = {pt1.x, pt1.y, pt1.z};
            double b[6];
            pair_block_apply(st1, ((uint32_t)rp1.y & PAIR_A_FLAG) != 0, w, t, b);
#pragma unroll
            for (int q = 0; q < 6; q++) o[q] += b[q];
        }
    }
#pragma unroll
    for (int q = 0; q < 6; q++) o[q] = wave_sum_d(o[q]);
    if (lane == 0) {
        const f3 pr = pvR, pt = pvT;
        const double w[3] = {pr.x, pr.y, pr.z}, t[3] = {pt.x, pt.y, pt.z};
        double dp[6];
        diag_apply(dst, w, t, dp);
        const double ws = wSparse;
        float4* q = reinterpret_cast<float4*>(a.apPair + (size_t)v * 8);
        st_wt(q, make_float4((float)(ws * (dp[0] - o[0])), (float)(ws * (dp[1] - o[1])), (float)(ws * (dp[2] - o[2])), 0.0f));
        st_wt(q + 1, make_float4((float)(ws * (dp[3] - o[3])), (float)(ws * (dp[4] - o[4])), (float)(ws * (dp[5] - o[5])), 0.0f));
    }
}

// Pair mode PCG iteration: one wave per row v >= 1, Ap_v = w (D_v p_v - sum_u B_vu p_u) in fp64 over
// the row's pairs (the same operator as applyJ / applyJT; no second w, SolverBundlingEquationsLie.h:
// 154-228), handed to the finisher write-through; then the finisher of k_pcg.
// RB: image rows per finisher thread held in registers (2: up to 513 images; 8: up to 2 049, the
// host picks it from the solve's image count; beyond, the finisher's multi-pass form)
template <int RB>
__global__ __launch_bounds__(WG) void k_pcg_pairs(BA a, float wSparse, int iter, int nLin) {
    __shared__ float sh[WG];
    if (a.ctrl[K_GN_DONE] || a.ctrl[K_PCG_DONE]) return;
    const uint32_t lane = lane_id();  // unused; without it the prologue's instructions come out in another order
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t v = 1 + wave; v < a.N; v += nw) pair_row_ap(a, wSparse, v);
    const int useDense = (int)a.ctrl[K_USE_DENSE];
    if (useDense) pcg_dense_offdiag(a, wave, nw);
    if (!last_block_sharded(a.sync, 1u)) return;
    if (threadIdx.x < 9) a.sync[threadIdx.x * SYNC_LINE] = 0;  // counters of the next launch
    float rDotzNew;
    bool last;
    pcg_finisher<RB>(a, sh, 0u, useDense, iter, nLin, rDotzNew, last);
    if (threadIdx.x == 0) pcg_iter_end(a, rDotzNew, last);
}

// Small solves (N <= 64 images: the 11-frame local submaps, early global solves): every PCG
// iteration of the GN step in ONE workgroup. p lives in LDS; each wave applies the assembled
// operator to its rows (sparse pair blocks in fp64, dense blocks of BuildDenseSystem in fp32: the
// diagonal block and the off-diagonal pair blocks, with the [trans | rot] order of the dense system,
// SolverBundlingDenseUtil.h:371-411); wave 0 holds one row per lane for the vector updates and the
// two dot products (PCGIteration Kernel1b/2/3, SolverBundling.cu:930-1022) with fixed butterflies.
// No grid-wide hand-off and no launch per iteration.
constexpr int SMALL_N = 64;
constexpr int SMALL_WG = 1024;
__global__ __launch_bounds__(SMALL_WG) void k_pcg_small(BA a, float wSparse, int nLin) {
    __shared__ float sP[SMALL_N][6], sAp[SMALL_N][6];
    // wave 0's per-row vectors live in LDS between iterations: held in registers by every wave of the 16, one
    // of them was spilled and reloaded from scratch each iteration
    __shared__ f3 sV[SMALL_N][6];  // dR, dT, rR, rT, mR, mT
    __shared__ int sLast;
    if (a.ctrl[K_GN_DONE] || a.ctrl[K_PCG_DONE]) return;
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6, nw = SMALL_WG / 64;
    const int useDense = (int)a.ctrl[K_USE_DENSE];
    const uint32_t npD = useDense ? a.ctrl[K_NPAIRS] : 0u;
    // wave 0, lane v: row v's vectors (row 0 and rows >= N stay zero)
    const bool own = wave == 0 && lane >= 1 && lane < a.N;
    if (wave == 0) {
        f3 dR = mk3(0, 0, 0), dT = dR, rR = dR, rT = dR, mR = dR, mT = dR, pR = dR, pT = dR;
        if (own) {
            vload(a, V_DELTA, lane, dR, dT);
            vload(a, V_R, lane, rR, rT);
            vload(a, V_M, lane, mR, mT);
            vload(a, V_P, lane, pR, pT);
        }
        sV[lane][0] = dR; sV[lane][1] = dT; sV[lane][2] = rR; sV[lane][3] = rT; sV[lane][4] = mR; sV[lane][5] = mT;
        if (lane < a.N) {
            sP[lane][0] = pR.x; sP[lane][1] = pR.y; sP[lane][2] = pR.z;
            sP[lane][3] = pT.x; sP[lane][4] = pT.y; sP[lane][5] = pT.z;
        }
    }
    float rz = ctrlf(a.ctrl, K_RDOTZ);
    int iters = 0;
    __syncthreads();
    for (int iter = 0; iter < nLin; iter++) {
        for (uint32_t v = 1 + wave; v < a.N; v += nw) {
            double o[6] = {0, 0, 0, 0, 0, 0};
            const int e0 = a.rowPairStart[v], e1 = a.rowPairStart[v + 1];
            for (int k = e0 + (int)lane; k < e1; k += 64) {
                const int2 rp = a.rowPair[k];
                const uint32_t u = (uint32_t)rp.y & ~PAIR_A_FLAG;
                if (u == 0) continue;
                const double w[3] = {sP[u][0], sP[u][1], sP[u][2]}, t[3] = {sP[u][3], sP[u][4], sP[u][5]};
                double b[6];
                pair_block_apply(a.pstat + (size_t)rp.x * PSTAT, ((uint32_t)rp.y & PAIR_A_FLAG) != 0, w, t, b);
#pragma unroll
                for (int q = 0; q < 6; q++) o[q] += b[q];
            }
            float od[6] = {0, 0, 0, 0, 0, 0};  // dense part, [trans | rot] rows
            for (uint32_t k = lane; k < npD; k += 64) {
                if (a.pairW[k] == 0.0f) continue;
                const uint2 pr = a.pairs[k];
                const float* Bk = a.pairBlk + (size_t)k * 36;  // rows: image pr.y, columns: image pr.x
                if (pr.y == v && pr.x > 0) {
                    const float pv[6] = {sP[pr.x][3], sP[pr.x][4], sP[pr.x][5], sP[pr.x][0], sP[pr.x][1], sP[pr.x][2]};
                    for (int r = 0; r < 6; r++) {
                        float s = 0.0f;
                        for (int c = 0; c < 6; c++) s += Bk[r * 6 + c] * pv[c];
                        od[r] += s;
                    }
                } else if (pr.x == v && pr.y > 0) {
                    const float pv[6] = {sP[pr.y][3], sP[pr.y][4], sP[pr.y][5], sP[pr.y][0], sP[pr.y][1], sP[pr.y][2]};
                    for (int c = 0; c < 6; c++) {
                        float s = 0.0f;
                        for (int r = 0; r < 6; r++) s += Bk[r * 6 + c] * pv[r];
                        od[c] += s;
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 6; q++) o[q] = wave_sum_d(o[q]);
            if (useDense) {
#pragma unroll
                for (int q = 0; q < 6; q++) od[q] = wave_sum(od[q]);
            }
            if (lane == 0) {
                const double w[3] = {sP[v][0], sP[v][1], sP[v][2]}, t[3] = {sP[v][3], sP[v][4], sP[v][5]};
                double dp[6];
                diag_apply(a.dstat + (size_t)v * DSTAT, w, t, dp);
                const double ws = wSparse;
                float ap[6];
#pragma unroll
                for (int q = 0; q < 6; q++) ap[q] = (float)(ws * (dp[q] - o[q]));
                if (useDense) {
                    const float* D = a.diag + (size_t)v * 36;
                    const float pv[6] = {sP[v][3], sP[v][4], sP[v][5], sP[v][0], sP[v][1], sP[v][2]};
                    float o6[6];
                    for (int r = 0; r < 6; r++) {
                        float s = 0.0f;
                        for (int c = 0; c < 6; c++) s += D[r * 6 + c] * pv[c];
                        o6[r] = s;
                    }
                    for (int q = 0; q < 3; q++) {
                        ap[3 + q] += o6[q] + od[q];      // trans
                        ap[q] += o6[3 + q] + od[3 + q];  // rot
                    }
                }
#pragma unroll
                for (int q = 0; q < 6; q++) sAp[v][q] = ap[q];
            }
        }
        __syncthreads();
        if (wave == 0) {
            const f3 aR = own ? mk3(sAp[lane][0], sAp[lane][1], sAp[lane][2]) : mk3(0, 0, 0);
            const f3 aT = own ? mk3(sAp[lane][3], sAp[lane][4], sAp[lane][5]) : mk3(0, 0, 0);
            f3 pR = own ? mk3(sP[lane][0], sP[lane][1], sP[lane][2]) : mk3(0, 0, 0);
            f3 pT = own ? mk3(sP[lane][3], sP[lane][4], sP[lane][5]) : mk3(0, 0, 0);
            f3 dR = sV[lane][0], dT = sV[lane][1], rR = sV[lane][2], rT = sV[lane][3];
            const f3 mR = sV[lane][4], mT = sV[lane][5];
            const float pAp = wave_sum(dot3(pR, aR) + dot3(pT, aT));
            const float alpha = pcg_alpha(rz, pAp);
            dR = dR + alpha * pR;
            dT = dT + alpha * pT;
            rR = rR - alpha * aR;
            rT = rT - alpha * aT;
            const f3 zR = mul3(mR, rR), zT = mul3(mT, rT);
            const float rzNew = wave_sum(dot3(zR, rR) + dot3(zT, rT));
            const bool last = pcg_last(a, iter, nLin, pAp);
            const float beta = pcg_beta(rzNew, rz);
            if (own) {
                pR = zR + beta * pR;
                pT = zT + beta * pT;
                sP[lane][0] = pR.x; sP[lane][1] = pR.y; sP[lane][2] = pR.z;
                sP[lane][3] = pT.x; sP[lane][4] = pT.y; sP[lane][5] = pT.z;
            }
            sV[lane][0] = dR; sV[lane][1] = dT; sV[lane][2] = rR; sV[lane][3] = rT;
            rz = rzNew;
            if (lane == 0) sLast = last ? 1 : 0;
        }
        iters++;
        __syncthreads();
        if (sLast) break;
    }
    if (own) {
        const f3 dR = sV[lane][0], dT = sV[lane][1];
        vstore(a, V_DELTA, lane, dR, dT);
        vstore(a, V_R, lane, sV[lane][2], sV[lane][3]);
        vstore(a, V_P, lane, mk3(sP[lane][0], sP[lane][1], sP[lane][2]), mk3(sP[lane][3], sP[lane][4], sP[lane][5]));
        // computeLieUpdate (LieDerivUtil.h:301-307) on the exiting iteration
        f3 nr, nt;
        lie_update(dR, dT, mk3(a.rot[3 * lane], a.rot[3 * lane + 1], a.rot[3 * lane + 2]),
                   mk3(a.trans[3 * lane], a.trans[3 * lane + 1], a.trans[3 * lane + 2]), nr, nt);
        a.rot[3 * lane] = nr.x; a.rot[3 * lane + 1] = nr.y; a.rot[3 * lane + 2] = nr.z;
        a.trans[3 * lane] = nt.x; a.trans[3 * lane + 1] = nt.y; a.trans[3 * lane + 2] = nt.z;
    }
    if (threadIdx.x == 0) {
        a.ctrl[K_RDOTZ] = __float_as_uint(rz);
        a.ctrl[K_PCG_ITERS] += (uint32_t)iters;
        a.ctrl[K_PCG_DONE] = 1;
    }
}

}  // namespace
}  // namespace bf
