// ba_dense.h — the dense (depth / colour) term, the residual analysis and the local-submap verification.
// Kernels: k_dense_reset, k_dense_overlap, k_dense_compact, k_dense_count, k_dense_build, k_dense_lists
// (Solver::buildDense, per dense GN step); k_residuals (after a solve with findMaxResidual);
// k_solve_begin (first launch of every solve: resets the result words k_residuals and the verification
// write); k_verify_begin, k_verify_pairs (Solver::verify). Relies on ba_dev.h only.
#pragma once
#include "ba_dev.h"

namespace bf {
namespace {

// ---- dense term (BuildDenseSystem, SolverBundling.cu:308-471) ----------------------------------
__device__ __forceinline__ f3 d2c(const BA& a, int x, int y, float depth) {  // CUDACameraUtil.h:15-19
    const float xx = ((float)x - a.mx) / a.fx, yy = ((float)y - a.my) / a.fy;
    return mk3(depth * xx, depth * yy, depth);
}
__device__ __forceinline__ void bilinear(const BA& a, float x, float y, const float* img, int comp, float* out) {
    const int W = (int)a.cw, H = (int)a.ch;
    const int px = (int)floorf(x), py = (int)floorf(y);
    const float alpha = x - (float)px, beta = y - (float)py;
    float s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0}, w0 = 0, w1 = 0;
    const int qx[4] = {px, px + 1, px, px + 1}, qy[4] = {py, py, py + 1, py + 1};
    const float wt[4] = {1.0f - alpha, alpha, 1.0f - alpha, alpha};
    for (int t = 0; t < 4; t++) {
        if ((unsigned)qx[t] < (unsigned)W && (unsigned)qy[t] < (unsigned)H) {
            const float* v = img + ((size_t)qy[t] * W + qx[t]) * comp;
            if (v[0] != -INFINITY) {
                float* s = t < 2 ? s0 : s1;
                for (int k = 0; k < comp; k++) s[k] += wt[t] * v[k];
                if (t < 2) w0 += wt[t]; else w1 += wt[t];
            }
        }
    }
    float ss[4] = {0, 0, 0, 0}, ww = 0;
    if (w0 > 0.0f) { for (int k = 0; k < comp; k++) ss[k] += (1.0f - beta) * (s0[k] / w0); ww += (1.0f - beta); }
    if (w1 > 0.0f) { for (int k = 0; k < comp; k++) ss[k] += beta * (s1[k] / w1); ww += beta; }
    for (int k = 0; k < comp; k++) out[k] = (ww > 0.0f) ? ss[k] / ww : -INFINITY;
}

__global__ void k_dense_reset(BA a) {
    if (a.ctrl[K_GN_DONE]) return;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < a.N * a.N; k += gridDim.x * blockDim.x) a.pairFlag[k] = 0u;
}

// FindImageImageCorr_Kernel<true> (SolverBundling.cu:29-79), one wave per (i, j), i < j
__global__ void k_dense_overlap(BA a) {
    if (a.ctrl[K_GN_DONE]) return;
    const uint32_t i = blockIdx.x, j = blockIdx.y;
    if (i >= j || j >= a.N) return;
    if (a.valid[i] == 0 || a.valid[j] == 0) return;
    const m4 t = mul44(loadm4(a.Tinv + (size_t)i * 16), loadm4(a.T + (size_t)j * 16));
    // computeAngleDiff (SolverBundlingDenseUtil.h:416-424)
    const f3 x1 = normalize3(mk3(1.0f, 1.0f, 1.0f));
    const f3 v1 = mul3v(rot_of(t), x1);
    if (!(fabsf(acosf(fmaxf(-1.0f, fminf(dot3(x1, v1), 1.0f)))) < 0.52f)) return;
    const uint32_t W = a.cw, H = a.ch, subW = W / a.sub;
    const float* tgt = a.cache[i].depth;
    const float* src = a.cache[j].depth;
    int found = 0;
    for (uint32_t tid = threadIdx.x; tid < 512; tid += blockDim.x) {
        const uint32_t x = (tid % subW) * a.sub, y = (tid / subW) * a.sub, idx = y * W + x;
        if (idx >= W * H) continue;
        const f3 cj = d2c(a, (int)x, (int)y, src[idx]);  // findDenseCorr depth-only (:22-42)
        if (!(cj.z > a.dmin && cj.z < a.dmax)) continue;
        const f3 s2t = xf(t, cj);
        const float u = s2t.x * a.fx / s2t.z + a.mx, vv = s2t.y * a.fy / s2t.z + a.my;
        const int tx = (int)roundf(u), ty = (int)roundf(vv);
        if (!(tx >= 0 && ty >= 0 && tx < (int)W && ty < (int)H)) continue;
        const f3 ct = d2c(a, tx, ty, tgt[ty * W + tx]);
        if (!(ct.z > a.dmin && ct.z < a.dmax)) continue;
        if (length3(s2t - ct) <= a.distT) found++;
    }
    for (int off = 32; off > 0; off >>= 1) found += __shfl_xor(found, off);
    if (threadIdx.x == 0 && found > 10) a.pairFlag[(size_t)i * a.N + j] = 1u;
}

// The overlapping pairs in (i, j) order (the reference appends them at atomic offsets): one workgroup
// compacts the flag matrix with wave ballots; K_NPAIRS = all pairs found, the first maxPairs are kept.
__global__ __launch_bounds__(256) void k_dense_compact(BA a) {
    __shared__ uint32_t sCnt[4];
    if (a.ctrl[K_GN_DONE]) return;
    const uint32_t NN = a.N * a.N;
    uint32_t base = 0;  // the same in every lane
    for (uint32_t b0 = 0; b0 < NN; b0 += 256) {
        const uint32_t idx = b0 + threadIdx.x;
        const bool f = idx < NN && a.pairFlag[idx] != 0u;
        uint32_t found;
        const uint32_t off = base + wg_compact_offset<4>(f, sCnt, found);
        if (f && off < a.maxPairs) a.pairs[off] = make_uint2(idx / a.N, idx % a.N);
        base += found;
        __syncthreads();
    }
    if (threadIdx.x == 0) a.ctrl[K_NPAIRS] = base;
}

// FindDenseCorrespondences_Kernel (:92-160, uchar4-normal variant :152-184) + WeightDenseCorrespondences (:162-180)
__global__ void k_dense_count(BA a) {
    if (a.ctrl[K_GN_DONE]) return;
    const uint32_t np = min(a.ctrl[K_NPAIRS], a.maxPairs);
    for (uint32_t k = blockIdx.x; k < np; k += gridDim.x) {
        const uint2 pr = a.pairs[k];
        const m4 t = mul44(loadm4(a.Tinv + (size_t)pr.x * 16), loadm4(a.T + (size_t)pr.y * 16));
        const m3 R = rot_of(t);
        const BFCachedFrame fi = a.cache[pr.x], fj = a.cache[pr.y];
        const uint32_t W = a.cw, H = a.ch;
        int count = 0;
        for (uint32_t idx = threadIdx.x; idx < W * H; idx += blockDim.x) {
            const int x = (int)(idx % W), y = (int)(idx / W);
            const f3 cj = d2c(a, x, y, fj.depth[idx]);
            if (!(cj.z > a.dmin && cj.z < a.dmax)) continue;
            const uint32_t nj = reinterpret_cast<const uint32_t*>(fj.normalsU8)[idx];
            if (nj == 0) continue;
            f3 nrmj = mk3((float)(nj & 0xFF), (float)((nj >> 8) & 0xFF), (float)((nj >> 16) & 0xFF)) / 255.0f * 2.0f - mk3(1.0f, 1.0f, 1.0f);
            nrmj = mul3v(R, nrmj);
            const f3 s2t = xf(t, cj);
            const float u = s2t.x * a.fx / s2t.z + a.mx, vv = s2t.y * a.fy / s2t.z + a.my;
            const int tx = (int)roundf(u), ty = (int)roundf(vv);
            if (!(tx >= 0 && ty >= 0 && tx < (int)W && ty < (int)H)) continue;
            const f3 ct = d2c(a, tx, ty, fi.depth[ty * W + tx]);
            if (!(ct.z > a.dmin && ct.z < a.dmax)) continue;
            const uint32_t ni = reinterpret_cast<const uint32_t*>(fi.normalsU8)[ty * W + tx];
            if (ni == 0) continue;
            const f3 nrmi = mk3((float)(ni & 0xFF), (float)((ni >> 8) & 0xFF), (float)((ni >> 16) & 0xFF)) / 255.0f * 2.0f - mk3(1.0f, 1.0f, 1.0f);
            if (dot3(nrmj, nrmi) >= a.normT && length3(s2t - ct) <= a.distT) count++;
        }
        for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off);
        __shared__ int wc[WG / 64];
        if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = count;
        __syncthreads();
        if (threadIdx.x == 0) {
            int tot = 0;
            for (uint32_t q = 0; q < blockDim.x / 64; q++) tot += wc[q];
            float x = (float)tot;
            if (x > 0) x = (x < 800) ? 0.0f : 1.0f / fminf(logf(x), 9.0f);
            a.pairW[k] = x;
        }
        __syncthreads();
    }
}

// BuildDenseSystem_Kernel<depth, color> (:182-306): one workgroup per overlapping pair; every
// thread accumulates its pixels' 6x6 outer products (addToLocalSystem, DenseUtil.h:229-288) in
// registers, then one workgroup reduction and one set of global adds per pair.
__global__ __launch_bounds__(WG) void k_dense_build(BA a, float wDepth, float wColor) {
    __shared__ float red[WG / 64][90];
    if (a.ctrl[K_GN_DONE]) return;
    const uint32_t np = min(a.ctrl[K_NPAIRS], a.maxPairs);
    const bool useDepth = wDepth > 0.0f;
    const bool useColor = !useDepth || wColor > 0.0f;
    for (uint32_t k = blockIdx.x; k < np; k += gridDim.x) {
        const float pw = a.pairW[k];
        if (pw == 0.0f) continue;  // uniform per workgroup
        const uint2 pr = a.pairs[k];
        const uint32_t i = pr.x, j = pr.y;
        const m4 Ti = loadm4(a.T + (size_t)i * 16), Tj = loadm4(a.T + (size_t)j * 16);
        const m4 Tiinv = loadm4(a.Tinv + (size_t)i * 16), Tjinv = loadm4(a.Tinv + (size_t)j * 16);
        const m4 t = mul44(Tiinv, Tj);
        const BFCachedFrame fi = a.cache[i], fj = a.cache[j];
        float acc[90];  // [0,21) ii upper, [21,42) jj upper, [42,78) ij (row b of i . col c of j), [78,84) jtr_i, [84,90) jtr_j
#pragma unroll
        for (int q = 0; q < 90; q++) acc[q] = 0.0f;
        const uint32_t W = a.cw, H = a.ch;
        for (uint32_t src = threadIdx.x; src < W * H; src += blockDim.x) {
            // findDenseCorr with camera positions + float4 normals (DenseUtil.h:79-113)
            const float4 cp = reinterpret_cast<const float4*>(fj.campos)[src];
            if (!(cp.z > a.dmin && cp.z < a.dmax)) continue;
            const f3 cps = mk3(cp.x, cp.y, cp.z);
            const float4 nj = reinterpret_cast<const float4*>(fj.normals)[src];
            if (nj.x == -INFINITY) continue;
            const f3 nrmj = mk3(t.e[0] * nj.x + t.e[1] * nj.y + t.e[2] * nj.z + t.e[3] * nj.w,
                                t.e[4] * nj.x + t.e[5] * nj.y + t.e[6] * nj.z + t.e[7] * nj.w,
                                t.e[8] * nj.x + t.e[9] * nj.y + t.e[10] * nj.z + t.e[11] * nj.w);
            const float nrmjw = t.e[12] * nj.x + t.e[13] * nj.y + t.e[14] * nj.z + t.e[15] * nj.w;
            const f3 s2t = xf(t, cps);
            const float u = s2t.x * a.fx / s2t.z + a.mx, vv = s2t.y * a.fy / s2t.z + a.my;
            const int tx = (int)roundf(u), ty = (int)roundf(vv);
            if (!(tx >= 0 && ty >= 0 && tx < (int)W && ty < (int)H)) continue;
            float ci[4], ni[4];
            bilinear(a, u, vv, fi.campos, 4, ci);
            if (!(ci[2] > a.dmin && ci[2] < a.dmax)) continue;
            bilinear(a, u, vv, fi.normals, 4, ni);
            if (ni[0] == -INFINITY) continue;
            const f3 cpt = mk3(ci[0], ci[1], ci[2]), nT = mk3(ni[0], ni[1], ni[2]);
            const float dn = nrmj.x * ni[0] + nrmj.y * ni[1] + nrmj.z * ni[2] + nrmjw * ni[3];
            if (!(dn >= a.normT && length3(s2t - cpt) <= a.distT)) continue;
            // rows of the two terms; accumulate J^T W J and J^T W r (every loop over acc unrolled: with a
            // run-time index the 90 accumulators lived in scratch, one memory round trip per update)
#pragma unroll
            for (int term = 0; term < 2; term++) {
                float Ji[6] = {0, 0, 0, 0, 0, 0}, Jj[6] = {0, 0, 0, 0, 0, 0};
                float res = 0.0f, w = 0.0f;
                if (term == 0) {
                    if (!useDepth) continue;
                    res = dot3(cpt - s2t, nT);
                    w = wDepth * pw * powf(fmaxf(0.0f, 1.0f - cpt.z / 2.0f), 2.5f);
                    if (i > 0) { const m36 J = deriv_i(Tjinv, Ti, cps); for (int c = 0; c < 6; c++) Ji[c] = -dot3(mk3(J.e[c], J.e[6 + c], J.e[12 + c]), nT); }
                    if (j > 0) { const m36 J = deriv_j(Tiinv, Tj, cps); for (int c = 0; c < 6; c++) Jj[c] = -dot3(mk3(J.e[c], J.e[6 + c], J.e[12 + c]), nT); }
                } else {
                    if (!useColor) continue;
                    float dI[2], It;
                    bilinear(a, u, vv, fi.intensityDeriv, 2, dI);
                    bilinear(a, u, vv, fi.intensity, 1, &It);
                    res = It - fj.intensity[src];
                    if (!(dI[0] != -INFINITY && fabsf(res) < a.colT && sqrtf(dI[0] * dI[0] + dI[1] * dI[1]) > a.gradMin)) continue;
                    const float wSq = s2t.z * s2t.z;
                    const float d00 = a.fx / s2t.z, d11 = a.fy / s2t.z, d02 = -a.fx * s2t.x / wSq, d12 = -a.fy * s2t.y / wSq;
                    if (i > 0) {
                        const m36 J = deriv_i(Tjinv, Ti, cps);
                        for (int c = 0; c < 6; c++) Ji[c] = dI[0] * (d00 * J.e[c] + 0.0f * J.e[6 + c] + d02 * J.e[12 + c]) + dI[1] * (0.0f * J.e[c] + d11 * J.e[6 + c] + d12 * J.e[12 + c]);
                    }
                    if (j > 0) {
                        const m36 J = deriv_j(Tiinv, Tj, cps);
                        for (int c = 0; c < 6; c++) Jj[c] = dI[0] * (d00 * J.e[c] + 0.0f * J.e[6 + c] + d02 * J.e[12 + c]) + dI[1] * (0.0f * J.e[c] + d11 * J.e[6 + c] + d12 * J.e[12 + c]);
                    }
                    w = wColor * pw * fmaxf(0.0f, 1.0f - fabsf(res) / (1.15f * a.colT));
                }
#pragma unroll
                for (int r = 0; r < 6; r++)
#pragma unroll
                    for (int c = r; c < 6; c++) {
                        const int q = r * 6 - r * (r - 1) / 2 + (c - r);  // row-major upper triangle
                        acc[q] += Ji[r] * Ji[c] * w;
                        acc[21 + q] += Jj[r] * Jj[c] * w;
                    }
#pragma unroll
                for (int r = 0; r < 6; r++)
#pragma unroll
                    for (int c = 0; c < 6; c++) acc[42 + r * 6 + c] += Ji[r] * Jj[c] * w;
#pragma unroll
                for (int r = 0; r < 6; r++) { acc[78 + r] += Ji[r] * res * w; acc[84 + r] += Jj[r] * res * w; }
            }
        }
#pragma unroll
        for (int q = 0; q < 90; q++) {
            const float s = wave_sum(acc[q]);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = s;
        }
        __syncthreads();
        if (threadIdx.x < 90) {
            float s = 0.0f;
            for (uint32_t wv = 0; wv < blockDim.x / 64; wv++) s += red[wv][threadIdx.x];
            const int q = threadIdx.x;
            if (q < 42) {  // diagonal-block upper triangles of images i (q < 21) and j: summed per image by k_dense_lists
                a.pairAcc[(size_t)k * 54 + q] = s;
            } else if (q < 78) {  // B(row j-index c, col i-index r) = (J_i^T W J_j)^T
                const int r = (q - 42) / 6, c = (q - 42) % 6;
                a.pairBlk[(size_t)k * 36 + c * 6 + r] = s;
            } else {  // J_i^T r (q < 84), J_j^T r
                a.pairAcc[(size_t)k * 54 + 42 + (q - 78)] = s;
            }
        }
        __syncthreads();
    }
}

// Per image v (one wave): its pairs in pair order (pairW != 0), and its dense diagonal block and J^T r
// summed over them in that order (the reference adds them with float atomics in arrival order).
__global__ __launch_bounds__(64) void k_dense_lists(BA a) {
    if (a.ctrl[K_GN_DONE]) return;
    const uint32_t v = blockIdx.x, lane = lane_id();
    const uint32_t np = min(a.ctrl[K_NPAIRS], a.maxPairs);
    uint32_t* L = a.imgPairs + (size_t)v * a.maxN;
    uint32_t n = 0;
    float s = 0.0f;  // lane < 21: upper-triangle entry of the diagonal block, 21..26: J^T r
    for (uint32_t b0 = 0; b0 < np; b0 += 64) {
        const uint32_t k = b0 + lane;
        uint32_t e = 0;
        bool in = false;
        if (k < np && a.pairW[k] != 0.0f) {
            const uint2 pr = a.pairs[k];
            in = pr.x == v || pr.y == v;
            e = (k << 1) | (pr.y == v ? 1u : 0u);
        }
        const unsigned long long m = __ballot(in);
        if (in) L[n + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = e;
        n += (uint32_t)__popcll(m);
        for (unsigned long long mm = m; mm; mm &= mm - 1ull) {  // this chunk's pairs of v, ascending
            const uint32_t ek = (uint32_t)__shfl((int)e, (int)__builtin_ctzll(mm));
            const float* acc = a.pairAcc + (size_t)(ek >> 1) * 54;
            if (lane < 21) s += acc[((ek & 1u) ? 21 : 0) + lane];
            else if (lane < 27) s += acc[42 + ((ek & 1u) ? 6 : 0) + (lane - 21)];
        }
    }
    if (lane == 0) a.imgPairN[v] = n;
    if (lane < 21) {
        int r = 0, c = 0, t2 = 0;
        for (r = 0; r < 6; r++) { if ((int)lane < t2 + (6 - r)) { c = r + ((int)lane - t2); break; } t2 += 6 - r; }
        a.diag[(size_t)v * 36 + r * 6 + c] = s;
        a.diag[(size_t)v * 36 + c * 6 + r] = s;
    } else if (lane < 27) {
        a.jtr[(size_t)v * 6 + (lane - 21)] = s;
    }
}

// ---- residual analysis (EvalMaxResidual :511-564, EvalResidual :570-614, CountHighResiduals :657-687) ----
__global__ __launch_bounds__(WG) void k_residuals(BA a) {
    __shared__ float shv[WG];
    __shared__ int shi[WG];
    __shared__ float she[WG];
    __shared__ int shc[WG];
    if (a.ctrl[K_SKIPPED]) return;  // gated-off solve: no residual analysis, hence no removal
    const float w = ctrlf(a.ctrl, K_LAST_W);
    float best = 0.0f, e = 0.0f;
    int bi = 0x7FFFFFFF, cnt = 0;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < a.nCorr; c += gridDim.x * blockDim.x) {
        const BFEntryJ x = a.corr[c];
        if (!corr_valid(x)) continue;
        const f3 r = xf(loadm4(a.T + (size_t)x.imgIdx_i * 16), mk3(x.pos_i.x, x.pos_i.y, x.pos_i.z)) -
                     xf(loadm4(a.T + (size_t)x.imgIdx_j * 16), mk3(x.pos_j.x, x.pos_j.y, x.pos_j.z));
        const f3 ar = mk3(fabsf(r.x), fabsf(r.y), fabsf(r.z)) * w;
        const float m = fmaxf(ar.z, fmaxf(ar.x, ar.y));  // evalAbsMaxResidualDevice (EquationsLie.h:27-40)
        if (m > best || (m == best && (int)c < bi)) { best = m; bi = (int)c; }
        e += w * dot3(r, r);                              // evalFDevice (:42-57)
        if (m > a.verifyT) cnt++;
    }
    shv[threadIdx.x] = best; shi[threadIdx.x] = bi; she[threadIdx.x] = e; shc[threadIdx.x] = cnt;
    __syncthreads();
    for (int s = WG / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const float v2 = shv[threadIdx.x + s];
            const int i2 = shi[threadIdx.x + s];
            if (v2 > shv[threadIdx.x] || (v2 == shv[threadIdx.x] && i2 < shi[threadIdx.x])) { shv[threadIdx.x] = v2; shi[threadIdx.x] = i2; }
            she[threadIdx.x] += she[threadIdx.x + s];
            shc[threadIdx.x] += shc[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        st_wt(&a.part[blockIdx.x * 2], shv[0]);
        st_wt(&a.part[blockIdx.x * 2 + 1], she[0]);
        st_wt(reinterpret_cast<uint32_t*>(&a.partIdx[blockIdx.x * 2]), (uint32_t)shi[0]);
        st_wt(reinterpret_cast<uint32_t*>(&a.partIdx[blockIdx.x * 2 + 1]), (uint32_t)shc[0]);
    }
    if (!last_block(&a.ctrl[K_TICKET])) return;
    // all threads fold the per-workgroup partials, then one fixed tree (deterministic)
    float mv = 0.0f, en = 0.0f;
    int mi = 0x7FFFFFFF, hc = 0;
    for (uint32_t b = threadIdx.x; b < gridDim.x; b += blockDim.x) {
        const float v2 = ld_wtf(&a.part[b * 2]);
        const int i2 = (int)ld_wt(reinterpret_cast<const uint32_t*>(&a.partIdx[b * 2]));
        if (v2 > mv || (v2 == mv && i2 < mi)) { mv = v2; mi = i2; }
        en += ld_wtf(&a.part[b * 2 + 1]);
        hc += (int)ld_wt(reinterpret_cast<const uint32_t*>(&a.partIdx[b * 2 + 1]));
    }
    shv[threadIdx.x] = mv; shi[threadIdx.x] = mi; she[threadIdx.x] = en; shc[threadIdx.x] = hc;
    __syncthreads();
    for (int s = WG / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const float v2 = shv[threadIdx.x + s];
            const int i2 = shi[threadIdx.x + s];
            if (v2 > shv[threadIdx.x] || (v2 == shv[threadIdx.x] && i2 < shi[threadIdx.x])) { shv[threadIdx.x] = v2; shi[threadIdx.x] = i2; }
            she[threadIdx.x] += she[threadIdx.x + s];
            shc[threadIdx.x] += shc[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        mv = shv[0]; mi = shi[0]; en = she[0]; hc = shc[0];
        if (!(w > 0.0f) || mi == 0x7FFFFFFF) { mv = 0.0f; mi = 0; }
        a.ctrl[K_MAXRES] = __float_as_uint(mv);
        a.ctrl[K_MAXIDX] = (uint32_t)mi;
        a.ctrl[K_ENERGY] = __float_as_uint(en);
        a.ctrl[K_HIGHCOUNT] = (uint32_t)hc;
        a.ctrl[K_TICKET] = 0;
    }
}

__global__ void k_solve_begin(uint32_t* ctrl, const int* gate) {
    const uint32_t off = (gate && *gate == 0) ? 1u : 0u;
    const uint32_t t = threadIdx.x;
    if (t < K_COUNT)  // the error word too: every solve reports its own
        ctrl[t] = (t == K_RM_I || t == K_RM_J) ? BF_INVALID_IMAGE : (t == K_GN_DONE || t == K_SKIPPED) ? off : 0u;
}

// ---- local-submap verification (SBA.cpp:106-109 -> CUDASolverBundling::useVerification,
// CUDASolverBundling.cpp:454-476 -> Bundler::optimize, Bundler.cpp:259-274) ----------------------
struct VerifyArgs {
    const float* T;
    const int* valid;
    uint32_t N;
    const BFCachedFrame* cache;
    uint32_t W, H;
    float K[16];  // cache intrinsics as the reference's float4x4 (MatrixConversion::toCUDA(getIntrinsics()))
    float distT, normT, errT, corrT, dmin, dmax, percentT;
    uint32_t nCorr, always;
    uint32_t* ctrl;
    float* stats;
};
// useVerification: the pair check runs when the solve left >= 5 % of its correspondences with a
// max-norm residual above verifyOptDistThresh (K_HIGHCOUNT, counted by k_residuals)
__global__ void k_verify_begin(VerifyArgs v) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const bool used = v.always || ((float)v.ctrl[K_HIGHCOUNT] / (float)v.nCorr >= v.percentT);
    v.ctrl[K_VERIFY_USED] = used ? 1u : 0u;
    v.ctrl[K_VERIFY_OK] = 1u;
}
__device__ __forceinline__ float4 m4x4(const m4& m, float4 p) {  // float4x4 * float4 (cuda_SimpleMatrixUtil.h:925-933)
    const float* e = m.e;
    return make_float4(e[0] * p.x + e[1] * p.y + e[2] * p.z + e[3] * p.w, e[4] * p.x + e[5] * p.y + e[6] * p.z + e[7] * p.w,
                       e[8] * p.x + e[9] * p.y + e[10] * p.z + e[11] * p.w, e[12] * p.x + e[13] * p.y + e[14] * p.z + e[15] * p.w);
}
// computeProjError, CUDACACHE_FLOAT_NORMALS branch (SIFTImageManager.cu:418-487; CUDACacheUtil.h:7-8
// defines both normal formats, the float one is the branch compiled): {residual, weight, 1} of input
// pixel idx carried by `tr` into the model frame, or 0
__device__ f3 proj_error(const VerifyArgs& v, uint32_t idx, const m4& tr, const BFCachedFrame& in, const BFCachedFrame& model) {
    const float4 pIn = reinterpret_cast<const float4*>(in.campos)[idx];
    float4 nIn = reinterpret_cast<const float4*>(in.normals)[idx];
    nIn.w = 0.0f;
    const float dIn = in.depth[idx];
    if (!(pIn.x != -INFINITY && nIn.x != -INFINITY && dIn >= v.dmin && dIn <= v.dmax)) return mk3(0, 0, 0);
    const float4 pT = m4x4(tr, pIn), nT = m4x4(tr, nIn);
    const float* K = v.K;
    const f3 q = mk3(K[0] * pT.x + K[1] * pT.y + K[2] * pT.z + K[3] * 1.0f, K[4] * pT.x + K[5] * pT.y + K[6] * pT.z + K[7] * 1.0f,
                     K[8] * pT.x + K[9] * pT.y + K[10] * pT.z + K[11] * 1.0f);
    const int sx = f2i(roundf(q.x / q.z)), sy = f2i(roundf(q.y / q.z));
    if (!(sx >= 0 && sy >= 0 && sx < (int)v.W && sy < (int)v.H)) return mk3(0, 0, 0);
    const uint32_t t = (uint32_t)sy * v.W + (uint32_t)sx;
    const float4 pTg = reinterpret_cast<const float4*>(model.campos)[t];
    const float4 nTg = reinterpret_cast<const float4*>(model.normals)[t];
    if (!(pTg.x != -INFINITY && nTg.x != -INFINITY)) return mk3(0, 0, 0);
    const float dx = pT.x - pTg.x, dy = pT.y - pTg.y, dz = pT.z - pTg.z, dw = pT.w - pTg.w;
    const float d = sqrtf(dx * dx + dy * dy + dz * dz + dw * dw);  // length(float4)
    const float dN = nT.x * nTg.x + nT.y * nTg.y + nT.z * nTg.z;
    const float tgtDepth = model.depth[t];
    if (!(tgtDepth >= v.dmin && tgtDepth <= v.dmax)) return mk3(0, 0, 0);
    const bool bad = (tgtDepth != -INFINITY && pT.z < tgtDepth) && d > v.distT;  // known bad match
    if (!((dN >= v.normT && d <= v.distT) || bad)) return mk3(0, 0, 0);
    const float camZ = (pT.z - v.dmin) / (v.dmax - v.dmin);
    const float w = fmaxf(0.0f, 0.5f * ((1.0f - d / v.distT) + (1.0f - camZ)));
    return mk3(d, w, 1.0f);
}
// VerifyTrajectoryCU_Kernel (SIFTImageManager.cu:1036-1127): one workgroup per image pair i < j,
// both directions of every cache pixel. Sums per thread in pixel order (t, t + 256, ...), then a fixed
// tree per wave and the 4 waves in order (the reference's warp sums + shared float atomics have no
// fixed order; the oracle restates this one).
__global__ __launch_bounds__(WG) void k_verify_pairs(VerifyArgs v) {
    __shared__ float sh[3][WG / 64];
    if (!v.ctrl[K_VERIFY_USED]) return;
    const uint32_t i = blockIdx.x / v.N, j = blockIdx.x % v.N;
    if (i >= j) return;
    if (v.valid[i] == 0 || v.valid[j] == 0) return;
    const m4 tr = mul44(inverse44(loadm4(v.T + (size_t)j * 16)), loadm4(v.T + (size_t)i * 16));
    const m4 trInv = inverse44(tr);
    const BFCachedFrame in = v.cache[i], model = v.cache[j];
    float sr = 0.0f, sw = 0.0f, sn = 0.0f;
    for (uint32_t idx = threadIdx.x; idx < v.W * v.H; idx += WG) {
        const f3 a = proj_error(v, idx, tr, in, model);
        const f3 b = proj_error(v, idx, trInv, model, in);
        sr += a.x + b.x;
        sw += a.y + b.y;
        sn += a.z + b.z;
    }
    for (int off = 32; off > 0; off >>= 1) {
        sr += __shfl_down(sr, off);
        sw += __shfl_down(sw, off);
        sn += __shfl_down(sn, off);
    }
    if ((threadIdx.x & 63) == 0) {
        sh[0][threadIdx.x >> 6] = sr;
        sh[1][threadIdx.x >> 6] = sw;
        sh[2][threadIdx.x >> 6] = sn;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float s[3];
    for (int q = 0; q < 3; q++) s[q] = ((sh[q][0] + sh[q][1]) + sh[q][2]) + sh[q][3];
    if (v.stats)
        for (int q = 0; q < 3; q++) v.stats[((size_t)i * v.N + j) * 3 + q] = s[q];
    const float err = s[0] / s[1];
    const float corr = 0.5f * s[2] / (float)(v.W * v.H);
    if (corr < v.corrT || err > v.errT || isnan(err)) v.ctrl[K_VERIFY_OK] = 0u;  // every failing pair writes 0
}

}  // namespace
}  // namespace bf
