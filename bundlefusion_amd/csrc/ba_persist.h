// ba_persist.h — pair mode, every PCG iteration of a GN step in ONE launch, and the end of a GN step.
// Kernels: k_pcg_persist<2> (one finisher workgroup, pcg_persist_finisher), k_pcg_persist<2, PP_NF> (four,
// pcg_persist_finisher_x4), and k_gn_end<0|2|8>, which first redoes a timed-out persistent step in one
// workgroup (pcg_recover). Holds the bounded waits, the tagged granule and p hand-offs and their protocol.
// Relies on ba_dev.h (the PCG step rule, gran_store / gran_load, sums), ba_table.h (pair blocks) and
// ba_pcg.h (pair_init_row, pair_init_finish, pair_row_ap, pcg_dense_offdiag[_row], pcg_finisher,
// transforms_rows): the per-iteration routes whose results this one must equal bit for bit.
#pragma once
#include "ba_dev.h"
#include "ba_pcg.h"
#include "ba_table.h"

namespace bf {
namespace {

__device__ __forceinline__ unsigned long long rtc() { return __builtin_amdgcn_s_memrealtime(); }  // 100 MHz
constexpr unsigned long long PP_SPIN_TICKS = 200000000ull;  // 2 s at 100 MHz (BFSolverOptions.pcgSpinLimitUs = 0)
__device__ __forceinline__ bool pp_timed_out(unsigned long long t0, unsigned long long lim) { return rtc() - t0 > lim; }
// Waits until the granules g[i][0..5] (i < NR) all carry `tag`: every load of every row in flight at
// once, and all of them reloaded after a short sleep while any is stale (no per-granule branches, so
// the loaded values do not multiply into merge copies). Every pointer must be valid and written with
// this tag (a lane without a row of its own polls a row that is). Returns 1, or -1 on timeout.
template <int NR>
__device__ __forceinline__ int gran_rows(const uint2* const* g, uint32_t tag, float out[][6], unsigned long long t0,
                                         unsigned long long lim) {
    uint64_t x[NR][6];
    for (;;) {
#pragma unroll
        for (int r = 0; r < NR; r++)
#pragma unroll
            for (int q = 0; q < 6; q++) x[r][q] = gran_load(g[r] + q);
        bool all = true;
#pragma unroll
        for (int r = 0; r < NR; r++)
#pragma unroll
            for (int q = 0; q < 6; q++) all = all && (uint32_t)(x[r][q] >> 32) == tag;
        if (all) break;
        if (pp_timed_out(t0, lim)) return -1;
        __builtin_amdgcn_s_sleep(1);
    }
#pragma unroll
    for (int r = 0; r < NR; r++)
#pragma unroll
        for (int q = 0; q < 6; q++) out[r][q] = __uint_as_float((uint32_t)x[r][q]);
    return 1;
}

// Pair mode, all PCG iterations of one GN step in ONE launch (64 < N <= 2 WG + 1 images): the
// same arithmetic as k_pcg_pairs<2> + pcg_finish_regs<2> (bit-identical results), without a launch
// per iteration. Workgroup 0 is the finisher: its threads keep their rows' delta, r, M and p in
// registers across iterations. Workgroups 1.. are workers, one wave per image row, each holding its
// row's first PP_CPL x 64 pair entries and their pair statistics in registers across iterations.
// Per iteration the workers gather the partners' p (sc1 loads), apply the pair blocks in fp64 in the
// order of k_pcg_pairs, hand Ap_v over write-through (sc1, drained) and add to their shard's arrival
// counter; the finisher polls the 8 shards, runs Kernel1b / 2 / 3 (SolverBundling.cu:930-1022), stores
// p write-through (drained) and publishes the iteration on a flag word the workers poll: two hand-offs
// per iteration of MI355X_MICROARCH.md's first valid form, instead of a kernel boundary plus a
// last-workgroup election and two reloads of every vector. Every wait is bounded (2 s of s_memrealtime):
// a timeout sets result error bit 3 and releases every workgroup. The grid must be co-resident: the
// host launches it only when the occupancy query admits it with room to spare.
constexpr int kPcgPrio = 2;               // k_pcg_persist's wave priority
constexpr int PP_CPL = 3;                 // cached entries per lane: rows up to 192 partner pairs stay in registers
constexpr uint32_t PP_SHADOW = 256;       // the workgroup without rows (see the workers)
constexpr int PP_OV = 4;                  // further entries per lane whose pair refs stay in registers (rows up to 448)
constexpr uint32_t PP_DONE = 0x80000000u; // flag bit: the PCG loop ended (last iteration or timeout)
constexpr uint32_t PP_ERR_TIMEOUT = 8u;   // K_ERROR bit 3 (BF_SOLVE_ERR_PCG_TIMEOUT)
constexpr uint32_t PP_RECOVERED = 16u;    // K_ERROR bit 4 (BF_SOLVE_PCG_RECOVERED): pcg_recover redid the step

// The finisher workgroup of k_pcg_persist: R image rows per thread (R = 2: up to 513 images, every
// vector in registers; R = 8: up to 2 049, p and r in registers, the preconditioner M in LDS (sM,
// [6][8 WG] floats), delta read and written in memory by the thread that owns the row and z recomputed
// from M r: the same operations in the same order, so the result matches the per-launch finisher's bit
// for bit; the kernel stays within 256 VGPRs, i.e. two workgroups per CU for a 501-workgroup grid). The
// dense term is taken by R = 2 only (the host routes larger dense steps to one launch per iteration).
// The workers' gathers of p: two 16-B buffer loads per row with the sc1 (agent-coherent) cache policy
// — the policy of the agent-scope atomic loads in vload_t<true>, at half the L2 requests (four 8-B
// atomics per row). The finisher publishes p with 16-B write-through (sc1) stores, [r | tag][t | tag] (the
// MI355X_MICROARCH.md hand-off table: 16-B sc1 stores ~ plain, 8-B ones 2.7x the time per byte).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t p_rsrc(const BA& a) {
    return __builtin_amdgcn_make_buffer_rsrc(a.vec + (size_t)V_P * a.maxN * 8, (short)0, (int)(a.maxN * 32u), 0x00020000);
}

// The p hand-off of sparse solves, without the finisher's drain and barrier: each 16-B half carries its
// iteration's tag in the pad word (16-B sc1 halves are observed untorn, MI355X_MICROARCH.md R2), the
// flag only says when to start gathering, and a worker re-gathers a half whose tag is stale (standalone
// K = 500 GN iteration 1.016 / 1.050 -> 1.008 / 1.003 ms, A/B pairs). The dense solves keep the drained
// form (p complete, drained, then flagged, before any gather; tags not checked): their off-diagonal
// products gather p untagged.
__device__ __forceinline__ void pstore_tag(__amdgpu_buffer_rsrc_t rs, uint32_t u, f3 r, f3 t, uint32_t tag) {
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    const u4 x = {__float_as_uint(r.x), __float_as_uint(r.y), __float_as_uint(r.z), tag};
    const u4 y = {__float_as_uint(t.x), __float_as_uint(t.y), __float_as_uint(t.z), tag};
    __builtin_amdgcn_raw_buffer_store_b128(x, rs, u * 32u, 0, 16);  // 16: sc1
    __builtin_amdgcn_raw_buffer_store_b128(y, rs, u * 32u + 16u, 0, 16);
}
// gathers p of row u; true when both halves carry `tag`
__device__ __forceinline__ bool pload_tag(__amdgpu_buffer_rsrc_t rs, uint32_t u, f3& r, f3& t, uint32_t tag) {
    const auto x = __builtin_amdgcn_raw_buffer_load_b128(rs, u * 32u, 0, 16);  // 16: sc1
    const auto y = __builtin_amdgcn_raw_buffer_load_b128(rs, u * 32u + 16u, 0, 16);
    r = mk3(__uint_as_float(x[0]), __uint_as_float(x[1]), __uint_as_float(x[2]));
    t = mk3(__uint_as_float(y[0]), __uint_as_float(y[1]), __uint_as_float(y[2]));
    return x[3] == tag && y[3] == tag;
}
// pload_tag until the tag matches (check = false: p of an earlier launch, no tag); a timeout sets the
// error bit and leaves the last values
__device__ __forceinline__ void pload_wait(const BA& a, __amdgpu_buffer_rsrc_t rs, uint32_t u, f3& r, f3& t, uint32_t tag, bool check,
                                           unsigned long long t0) {
    while (!pload_tag(rs, u, r, t, tag) && check) {
        if (pp_timed_out(t0, a.spinTicks)) { atomicOr(&a.ctrl[K_ERROR], PP_ERR_TIMEOUT); break; }
        __builtin_amdgcn_s_sleep(1);
    }
}
// Row q of this finisher thread, opaque to the compiler at every use: otherwise the addresses of all
// R rows in all five vectors are hoisted out of the PCG loop and held in registers (R = 8: ~100 VGPRs).
__device__ __forceinline__ uint32_t fin_row(int q) {
    uint32_t v = 1 + threadIdx.x + q * WG;
    asm volatile("" : "+v"(v));
    return v;
}
template <int R>
__device__ void pcg_persist_finisher(const BA& a, float* sh, float* sM, int useDense, int nLin, uint32_t tagBase,
                                     uint32_t* flag, unsigned long long t0) {
    constexpr bool REGS = R <= 2;
    constexpr int SMR = R * WG;  // sM row stride (R > 2)
    f3 pR[R], pT[R], rR[R], rT[R];
    f3 mR[REGS ? R : 1], mT[REGS ? R : 1];
#pragma unroll
    for (int q = 0; q < R; q++) {
        const uint32_t v = fin_row(q);
        if (v < a.N) {
            vload(a, V_P, v, pR[q], pT[q]);
            vload(a, V_R, v, rR[q], rT[q]);
            if (REGS) {
                vload(a, V_M, v, mR[REGS ? q : 0], mT[REGS ? q : 0]);
            } else {
                f3 mr, mt;
                vload(a, V_M, v, mr, mt);
                const int i = (int)threadIdx.x + q * WG;
                sM[i] = mr.x; sM[SMR + i] = mr.y; sM[2 * SMR + i] = mr.z;
                sM[3 * SMR + i] = mt.x; sM[4 * SMR + i] = mt.y; sM[5 * SMR + i] = mt.z;
            }
        }
    }
    // M of row q (registers, or this thread's own LDS slots)
    auto getM = [&](int q, f3& mr, f3& mt) {
        if (REGS) { mr = mR[REGS ? q : 0]; mt = mT[REGS ? q : 0]; }
        else {
            const int i = (int)threadIdx.x + q * WG;
            mr = mk3(sM[i], sM[SMR + i], sM[2 * SMR + i]);
            mt = mk3(sM[3 * SMR + i], sM[4 * SMR + i], sM[5 * SMR + i]);
        }
    };
    float rz = ctrlf(a.ctrl, K_RDOTZ);
    const __amdgpu_buffer_rsrc_t prs = p_rsrc(a);
    int it = 0;
    bool last = false;
    float lastAlpha = 0.0f;
    for (;; it++) {
        // the rows' Ap granules (sparse part, then the dense off-diagonal products), all polled at once
        constexpr int NG = REGS ? 2 * R : R;
        const uint2* g[NG];
#pragma unroll
        for (int q = 0; q < R; q++) {
            const uint32_t v = fin_row(q);
            const uint32_t vv = v < a.N ? v : 1u;  // image 1's granules: written every iteration (N >= 2)
            g[q] = a.aGran + (size_t)vv * 6;
            if (REGS) g[(R + q) % NG] = useDense ? a.aGran + ((size_t)a.maxN + vv) * 6 : g[q];
        }
        float x[NG][6];
        int ok;
        if (REGS && useDense) ok = gran_rows<NG>(g, tagBase + (uint32_t)it + 1u, x, t0, a.spinTicks);
        else if (REGS) ok = gran_rows<R>(g, tagBase + (uint32_t)it + 1u, x, t0, a.spinTicks);  // no dense granules to poll
        else {  // R = 8: two halves of four rows (half the in-flight registers)
            constexpr int H = NG / 2 > 0 ? NG / 2 : 1;
            ok = gran_rows<H>(g, tagBase + (uint32_t)it + 1u, x, t0, a.spinTicks);
            if (ok > 0) ok = gran_rows<H>(g + H, tagBase + (uint32_t)it + 1u, x + H, t0, a.spinTicks);
        }
        float d = 0.0f;
#pragma unroll
        for (int q = 0; q < R; q++) {
            const uint32_t v = fin_row(q);
            if (v < a.N) {  // pcg_ap's order of additions; x[q] becomes Ap of the row
                f3 aR = mk3(x[q][0], x[q][1], x[q][2]), aT = mk3(x[q][3], x[q][4], x[q][5]);
                if (REGS && useDense) {  // diagonal block [trans | rot] x [pTrans | pRot], then the off-diagonal products
                    const float* D = a.diag + (size_t)v * 36;
                    const float pv[6] = {pT[q].x, pT[q].y, pT[q].z, pR[q].x, pR[q].y, pR[q].z};
                    float o6[6];
                    for (int r = 0; r < 6; r++) {
                        float sm = 0.0f;
                        for (int c = 0; c < 6; c++) sm += D[r * 6 + c] * pv[c];
                        o6[r] = sm;
                    }
                    aT = aT + mk3(o6[0], o6[1], o6[2]);
                    aR = aR + mk3(o6[3], o6[4], o6[5]);
                    aT = aT + mk3(x[(R + q) % NG][0], x[(R + q) % NG][1], x[(R + q) % NG][2]);
                    aR = aR + mk3(x[(R + q) % NG][3], x[(R + q) % NG][4], x[(R + q) % NG][5]);
                }
                x[q][0] = aR.x; x[q][1] = aR.y; x[q][2] = aR.z;
                x[q][3] = aT.x; x[q][4] = aT.y; x[q][5] = aT.z;
                d += dot3(pR[q], aR) + dot3(pT[q], aT);
            }
        }
        // pAp and the timeout vote in one reduction (block_sum's order; the vote rides in the same pass)
        float pAp;
        {
            const float wsum = wave_sum(d);
            const bool wok = __all(ok > 0);
            if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = wsum; sh[WG / 64 + (threadIdx.x >> 6)] = wok ? 1.0f : 0.0f; }
            __syncthreads();
            float r = 0.0f;
            bool all = true;
            for (uint32_t w = 0; w < WG / 64; w++) { r += sh[w]; all = all && sh[WG / 64 + w] != 0.0f; }
            // no trailing barrier: sh[0, 8) is rewritten next iteration, after every wave passed the rz barrier
            if (!all) break;  // timeout: released below
            pAp = r;
        }
        const float alpha = pcg_alpha(rz, pAp);
        // delta += alpha p is the workers' (each on its own row, from the p it gathered): alpha goes out
        // in the flag word
        lastAlpha = alpha;
        float b = 0.0f;
#pragma unroll
        for (int q = 0; q < R; q++) {
            const uint32_t v = fin_row(q);
            if (v < a.N) {
                const f3 aR = mk3(x[q][0], x[q][1], x[q][2]), aT = mk3(x[q][3], x[q][4], x[q][5]);
                f3 mr, mt;
                getM(q, mr, mt);
                rR[q] = rR[q] - alpha * aR;
                rT[q] = rT[q] - alpha * aT;
                const f3 zR = mul3(mr, rR[q]), zT = mul3(mt, rT[q]);
                b += dot3(zR, rR[q]) + dot3(zT, rT[q]);
            }
        }
        float rzNew;
        {   // block_sum's order in sh[16, 20): its next writer is behind the next iteration's pAp barrier
            const float wsum = wave_sum(b);
            if ((threadIdx.x & 63) == 0) sh[2 * (WG / 64) + (threadIdx.x >> 6)] = wsum;
            __syncthreads();
            float r = 0.0f;
            for (uint32_t w = 0; w < WG / 64; w++) r += sh[2 * (WG / 64) + w];
            rzNew = r;
        }
        last = pcg_last(a, it, nLin, pAp);
        const float beta = pcg_beta(rzNew, rz);
#pragma unroll
        for (int q = 0; q < R; q++) {
            const uint32_t v = fin_row(q);
            if (v < a.N) {
                f3 mr, mt;
                getM(q, mr, mt);
                const f3 zR = mul3(mr, rR[q]), zT = mul3(mt, rT[q]);
                pR[q] = zR + beta * pR[q];
                pT[q] = zT + beta * pT[q];
                if (!last) pstore_tag(prs, v, pR[q], pT[q], tagBase + (uint32_t)it + 2u);  // iteration it + 1's p
            }
        }
        rz = rzNew;
        if (last) break;
        // p is read by ~N x 92 gathers: published write-through, drained, then one flag word
        // (p as polled granules ran 20 % slower: the workers' polls swamp the hand-off)
        if (useDense) {  // (the dense products gather p untagged: drained hand-off)
            drain_stores();
            __syncthreads();
        }
        if (threadIdx.x < PP_NFLAG) st_wt64(flag + threadIdx.x * PP_FLAG_STRIDE, (uint32_t)(it + 1), __float_as_uint(lastAlpha));  // one instruction
    }
    // final state (later launches read it plainly across the kernel boundary); delta and the Lie
    // update are the workers'
#pragma unroll
    for (int q = 0; q < R; q++) {
        const uint32_t v = fin_row(q);
        if (v < a.N) {
            vstore(a, V_R, v, rR[q], rT[q]);
            vstore(a, V_P, v, pR[q], pT[q]);
        }
    }
    if (threadIdx.x == 0) {
        if (!last) atomicOr(&a.ctrl[K_ERROR], PP_ERR_TIMEOUT);
        a.ctrl[K_RDOTZ] = __float_as_uint(rz);
        a.ctrl[K_PCG_ITERS] += (uint32_t)(it + (last ? 1 : 0));
        a.ctrl[K_PCG_DONE] = 1;
    }
    if (threadIdx.x < 64) {  // wave 0: the final flag carries the last iteration's alpha (valid when last)
        drain_stores();
        if (threadIdx.x < PP_NFLAG)
            st_wt64(flag + threadIdx.x * PP_FLAG_STRIDE, PP_DONE | (uint32_t)(it + (last ? 1 : 0)), __float_as_uint(lastAlpha));
    }
}

// The finisher of wide sparse solves (514..2 017 images) as PP_NF workgroups instead of one with 8 rows per
// thread (whose serial per-row work and polls were 8 of the 11.7 us of a K = 2 001 iteration,
// profiles/r8h_pcg_phase_timing.txt): workgroup g owns rows 1 + t + (2g + q) WG, q = 0, 1, in registers (the
// R = 2 form), and the two dot products go through a hand-off: each workgroup publishes its block partial
// as a tagged granule, every workgroup adds the PP_NF partials in workgroup order (the grouped order of
// pcg_finish_regs<8>, so the result equals the per-launch solve's bit for bit). Workgroup 0 sets the
// flag (p halves carry their iteration's tag; workers re-gather a stale one) and the control words.
constexpr int PP_NF = FIN_GROUPS;
// the rows the wide finishers own, 1 .. 2 PP_NF WG: the host's wide-route bound on numImages (Solver::solve)
static_assert(2 * PP_NF * WG + 1 == 2049, "wide persistent finishers cover rows 1..2048");
constexpr int SH_FX = 64;  // the finisher's LDS slots of the exchanged totals
__device__ __forceinline__ float fx_exchange(const BA& a, float* sh, int kind, uint32_t g, float S, uint32_t tag,
                                             unsigned long long t0, bool& ok) {
    if (threadIdx.x == 0) gran_store(a.fxGran + kind * 8 + g, S, tag);
    if (threadIdx.x < 64) {
        const uint32_t l = threadIdx.x;
        uint64_t x = 0;
        bool got = l >= (uint32_t)PP_NF;
        for (;;) {
            if (!got) {
                x = gran_load(a.fxGran + kind * 8 + l);
                got = (uint32_t)(x >> 32) == tag;
            }
            if (__all(got)) break;
            if (pp_timed_out(t0, a.spinTicks)) break;
            __builtin_amdgcn_s_sleep(1);
        }
        const bool all = __all(got);
        float tot = 0.0f;
#pragma unroll
        for (int k = 0; k < PP_NF; k++) tot += __shfl(__uint_as_float((uint32_t)x), k);  // workgroup order
        if (l == 0) {
            sh[SH_FX + 2 * kind] = tot;
            sh[SH_FX + 2 * kind + 1] = all ? 1.0f : 0.0f;
        }
    }
    __syncthreads();
    ok = sh[SH_FX + 2 * kind + 1] != 0.0f;
    return sh[SH_FX + 2 * kind];
}
__device__ __forceinline__ uint32_t fin_row_g(int q, uint32_t g) {
    uint32_t v = 1 + threadIdx.x + (2 * g + (uint32_t)q) * WG;
    asm volatile("" : "+v"(v));
    return v;
}
__device__ void pcg_persist_finisher_x4(const BA& a, float* sh, int nLin, uint32_t tagBase, uint32_t* flag, unsigned long long t0,
                                        uint32_t g) {
    constexpr int R = 2;
    f3 pR[R], pT[R], rR[R], rT[R], mR[R], mT[R];
#pragma unroll
    for (int q = 0; q < R; q++) {
        const uint32_t v = fin_row_g(q, g);
        if (v < a.N) {
            vload(a, V_P, v, pR[q], pT[q]);
            vload(a, V_R, v, rR[q], rT[q]);
            vload(a, V_M, v, mR[q], mT[q]);
        }
    }
    float rz = ctrlf(a.ctrl, K_RDOTZ);
    const __amdgpu_buffer_rsrc_t prs = p_rsrc(a);
    int it = 0;
    bool last = false;
    float lastAlpha = 0.0f;
    for (;; it++) {
        const uint32_t tag = tagBase + (uint32_t)it + 1u;
        const uint2* gp[R];
#pragma unroll
        for (int q = 0; q < R; q++) {
            const uint32_t v = fin_row_g(q, g);
            gp[q] = a.aGran + (size_t)(v < a.N ? v : 1u) * 6;  // image 1's granules: written every iteration
        }
        float x[R][6];
        const int got = gran_rows<R>(gp, tag, x, t0, a.spinTicks);
        float d = 0.0f;
#pragma unroll
        for (int q = 0; q < R; q++)
            if (fin_row_g(q, g) < a.N) d += dot3(pR[q], mk3(x[q][0], x[q][1], x[q][2])) + dot3(pT[q], mk3(x[q][3], x[q][4], x[q][5]));
        float S;
        bool all = true;
        {   // block_sum's order, with the timeout vote in the same pass
            const float wsum = wave_sum(d);
            const bool wok = __all(got > 0);
            if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = wsum; sh[WG / 64 + (threadIdx.x >> 6)] = wok ? 1.0f : 0.0f; }
            __syncthreads();
            S = 0.0f;
            for (uint32_t w = 0; w < WG / 64; w++) { S += sh[w]; all = all && sh[WG / 64 + w] != 0.0f; }
        }
        if (!all) break;
        bool ok;
        const float pAp = fx_exchange(a, sh, 0, g, S, tag, t0, ok);
        if (!ok) break;
        const float alpha = pcg_alpha(rz, pAp);
        lastAlpha = alpha;
        float b = 0.0f;
#pragma unroll
        for (int q = 0; q < R; q++) {
            if (fin_row_g(q, g) < a.N) {
                rR[q] = rR[q] - alpha * mk3(x[q][0], x[q][1], x[q][2]);
                rT[q] = rT[q] - alpha * mk3(x[q][3], x[q][4], x[q][5]);
                const f3 zR = mul3(mR[q], rR[q]), zT = mul3(mT[q], rT[q]);
                b += dot3(zR, rR[q]) + dot3(zT, rT[q]);
            }
        }
        float S2;
        {
            const float wsum = wave_sum(b);
            if ((threadIdx.x & 63) == 0) sh[2 * (WG / 64) + (threadIdx.x >> 6)] = wsum;
            __syncthreads();
            S2 = 0.0f;
            for (uint32_t w = 0; w < WG / 64; w++) S2 += sh[2 * (WG / 64) + w];
        }
        const float rzNew = fx_exchange(a, sh, 1, g, S2, tag, t0, ok);
        if (!ok) break;
        last = pcg_last(a, it, nLin, pAp);
        const float beta = pcg_beta(rzNew, rz);
#pragma unroll
        for (int q = 0; q < R; q++) {
            const uint32_t v = fin_row_g(q, g);
            if (v < a.N) {
                const f3 zR = mul3(mR[q], rR[q]), zT = mul3(mT[q], rT[q]);
                pR[q] = zR + beta * pR[q];
                pT[q] = zT + beta * pT[q];
                if (!last) pstore_tag(prs, v, pR[q], pT[q], tagBase + (uint32_t)it + 2u);  // iteration it + 1's p
            }
        }
        rz = rzNew;
        if (last) break;
        // the flag only says when to start gathering: the p halves of the other finishers' rows carry
        // their tag, and a worker re-gathers a stale one
        if (g == 0 && threadIdx.x < PP_NFLAG) st_wt64(flag + threadIdx.x * PP_FLAG_STRIDE, (uint32_t)(it + 1), __float_as_uint(lastAlpha));
    }
#pragma unroll
    for (int q = 0; q < R; q++) {
        const uint32_t v = fin_row_g(q, g);
        if (v < a.N) {
            vstore(a, V_R, v, rR[q], rT[q]);
            vstore(a, V_P, v, pR[q], pT[q]);
        }
    }
    if (threadIdx.x == 0) {
        if (!last) atomicOr(&a.ctrl[K_ERROR], PP_ERR_TIMEOUT);
        if (g == 0) {
            a.ctrl[K_RDOTZ] = __float_as_uint(rz);
            a.ctrl[K_PCG_ITERS] += (uint32_t)(it + (last ? 1 : 0));
            a.ctrl[K_PCG_DONE] = 1;
        }
    }
    if (g == 0 && threadIdx.x < 64) {
        drain_stores();
        if (threadIdx.x < PP_NFLAG)
            st_wt64(flag + threadIdx.x * PP_FLAG_STRIDE, PP_DONE | (uint32_t)(it + (last ? 1 : 0)), __float_as_uint(lastAlpha));
    }
}

// NF finisher workgroups: 1 (the R-rows-per-thread finisher) or PP_NF (pcg_persist_finisher_x4, R = 2)
template <int R, int NF = 1>
__global__ __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(2))) void k_pcg_persist(BA a, float wSparse, int nLin, uint32_t epoch) {
    __shared__ float sh[WG];
    __shared__ float sM[R > 2 ? 6 * R * WG : 1];  // the R = 8 finisher's preconditioner (48 KB)
    __shared__ double sD[WG / 64][DSTAT];          // each worker wave's image statistics
    if (a.ctrl[K_GN_DONE] || a.ctrl[K_PCG_DONE]) return;  // uniform over the grid (set by earlier launches)
    const uint32_t lane = lane_id();
    // above the voxel pass's waves on the same CU (its op steps run at 1): an iteration's critical path is
    // this kernel's compute between hand-offs, and its waits sleep (s_sleep), so the raise costs the voxel
    // pass little: in-loop time per PCG iteration 7.67 -> 6.43 us (1.46x -> 1.23x standalone), frame rate
    // 1 576 -> 1 587 at the driver workload (profiles/r11_prio_ab.txt)
    __builtin_amdgcn_s_setprio(kPcgPrio);
    const int useDense = (int)a.ctrl[K_USE_DENSE];
    const unsigned long long t0 = rtc();
    uint32_t* flag = &a.sync[SYNC_FLAGR];
    const uint32_t tagBase = epoch << 8;  // iteration it's Ap granules carry tagBase + it + 1
    if (blockIdx.x < NF) {
        if (NF == 1) pcg_persist_finisher<R>(a, sh, sM, useDense, nLin, tagBase, flag, t0);
        else pcg_persist_finisher_x4(a, sh, nLin, tagBase, flag, t0, blockIdx.x);
        return;
    }
    const uint32_t* myFlag = flag + ((blockIdx.x * (WG / 64) + (threadIdx.x >> 6)) % PP_NFLAG) * PP_FLAG_STRIDE;
    // ---- workers: one wave per row ----
    // Workgroup PP_SHADOW is dispatched onto the finisher's CU (256 CUs, round-robin) and holds no rows:
    // there, the finisher's granule polls held its rows' gathers up 2.4x (8 us of the 3.4 us others took)
    // (the NF workgroups dispatched onto the finishers' CUs hold none)
    const bool shadow = blockIdx.x >= PP_SHADOW && blockIdx.x < PP_SHADOW + NF;
    const uint32_t wb = blockIdx.x - NF - (blockIdx.x >= PP_SHADOW + NF ? NF : 0);
    const uint32_t v = 1 + wb * (WG / 64) + (threadIdx.x >> 6);
    const bool hasRow = !shadow && v < a.N;
    f3 dlR = mk3(0, 0, 0), dlT = dlR, pvR = dlR, pvT = dlR;  // the row's delta (every lane), the p it gathered
    int e0 = 0, e1 = 0;
    int2 rp[PP_CPL], rq[PP_OV];
    double st[PP_CPL][16];
    double* dst = sD[threadIdx.x >> 6];
    if (hasRow) {
        e0 = a.rowPairStart[v];
        e1 = a.rowPairStart[v + 1];
#pragma unroll
        for (int c = 0; c < PP_CPL; c++) {
            const int k = e0 + (int)lane + 64 * c;
            rp[c] = k < e1 ? a.rowPair[k] : make_int2(0, (int)v);  // idle lanes gather the wave's own row, not one hot row 0
        }
#pragma unroll
        for (int c = 0; c < PP_OV; c++) {
            const int k = e0 + (int)lane + 64 * (PP_CPL + c);
            rq[c] = k < e1 ? a.rowPair[k] : make_int2(0, (int)v);
        }
#pragma unroll
        for (int c = 0; c < PP_CPL; c++) {
            const bool ok = e0 + (int)lane + 64 * c < e1;
#pragma unroll
            for (int q = 0; q < 16; q += 2) {
                const double2 x = ok ? *reinterpret_cast<const double2*>(a.pstat + (size_t)rp[c].x * PSTAT + q) : make_double2(0.0, 0.0);
                st[c][q] = x.x;
                st[c][q + 1] = x.y;
            }
        }
        if (lane < DSTAT) dst[lane] = a.dstat[(size_t)v * DSTAT + lane];
        vload(a, V_DELTA, v, dlR, dlT);
    }
    __syncthreads();
    if (!hasRow) return;  // the row-less waves (the shadow workgroup, rows past N) have nothing to wait for
    const __amdgpu_buffer_rsrc_t prs = p_rsrc(a);
    for (uint32_t it = 0;; it++) {
        if (hasRow) {
            // p of iteration it (the previous launch's, or the finisher's write-through stores)
            f3 pr[PP_CPL], pt[PP_CPL];
            const uint32_t tag = tagBase + it + 1u;
            {   // every gather in flight at once, then all of them again while any is stale (rows u = 0,
                // whose p is never written, and p of an earlier launch, it = 0, carry no tag)
                const bool chk = it > 0 && !useDense;
                for (;;) {
                    bool ok = pload_tag(prs, v, pvR, pvT, tag) || !chk;
#pragma unroll
                    for (int c = 0; c < PP_CPL; c++) {
                        const uint32_t u = (uint32_t)rp[c].y & ~PAIR_A_FLAG;
                        ok = (pload_tag(prs, u, pr[c], pt[c], tag) || !chk || u == 0) && ok;
                    }
                    if (ok) break;
                    if (pp_timed_out(t0, a.spinTicks)) { atomicOr(&a.ctrl[K_ERROR], PP_ERR_TIMEOUT); break; }
                    __builtin_amdgcn_s_sleep(1);
                }
            }
            double o[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int c = 0; c < PP_CPL; c++) {
                const uint32_t u = (uint32_t)rp[c].y & ~PAIR_A_FLAG;
                if (e0 + (int)lane + 64 * c < e1 && u != 0) {  // p_0 = 0 (image 0 fixed)
                    const double w[3] = {pr[c].x, pr[c].y, pr[c].z}, t[3] = {pt[c].x, pt[c].y, pt[c].z};
                    double bb[6];
                    pair_block_apply(st[c], ((uint32_t)rp[c].y & PAIR_A_FLAG) != 0, w, t, bb);
#pragma unroll
                    for (int q = 0; q < 6; q++) o[q] += bb[q];
                }
            }
            // entries beyond the cached ones (rows with more than PP_CPL x 64 partners): the next PP_OV
            // per lane with their pair refs in registers (one dependent load round fewer), then from memory
#pragma unroll
            for (int c = 0; c < PP_OV; c++) {
                if (e0 + (int)lane + 64 * (PP_CPL + c) >= e1) break;
                const uint32_t u = (uint32_t)rq[c].y & ~PAIR_A_FLAG;
                if (u == 0) continue;
                f3 qr, qt;
                pload_wait(a, prs, u, qr, qt, tag, it > 0 && !useDense, t0);
                const double w[3] = {qr.x, qr.y, qr.z}, t[3] = {qt.x, qt.y, qt.z};
                double bb[6];
                // the pair's statistics address formed here, each iteration: hoisted out of the loop it was spilled
                // (255 VGPRs) and reloaded from scratch every iteration
                int px = rq[c].x;
                asm volatile("" : "+v"(px));
                pair_block_apply(a.pstat + (size_t)px * PSTAT, ((uint32_t)rq[c].y & PAIR_A_FLAG) != 0, w, t, bb);
#pragma unroll
                for (int q = 0; q < 6; q++) o[q] += bb[q];
            }
            for (int k = e0 + (int)lane + 64 * (PP_CPL + PP_OV); k < e1; k += 64) {
                const int2 r2 = a.rowPair[k];
                const uint32_t u = (uint32_t)r2.y & ~PAIR_A_FLAG;
                if (u == 0) continue;
                f3 qr, qt;
                pload_wait(a, prs, u, qr, qt, tag, it > 0 && !useDense, t0);
                const double w[3] = {qr.x, qr.y, qr.z}, t[3] = {qt.x, qt.y, qt.z};
                double bb[6];
                pair_block_apply(a.pstat + (size_t)r2.x * PSTAT, ((uint32_t)r2.y & PAIR_A_FLAG) != 0, w, t, bb);
#pragma unroll
                for (int q = 0; q < 6; q++) o[q] += bb[q];
            }
#pragma unroll
            for (int q = 0; q < 6; q++) o[q] = wave_sum_d(o[q]);
            if (lane < 6) {  // Ap_v = w (D_v p_v - sum_u B_vu p_u): one granule per lane, [rot | trans]
                const double w[3] = {pvR.x, pvR.y, pvR.z}, t[3] = {pvT.x, pvT.y, pvT.z};
                double dp[6];
                diag_apply(dst, w, t, dp);
                const double ws = wSparse;
                float y = 0.0f;
#pragma unroll
                for (int q = 0; q < 6; q++)
                    if ((int)lane == q) y = (float)(ws * (dp[q] - o[q]));
                gran_store(a.aGran + (size_t)v * 6 + lane, y, tag);
            }
            if (useDense) pcg_dense_offdiag_row<true>(a, v, tag);
        }
        // every wave polls its own flag replica (no workgroup barrier per iteration): one load per poll
        uint32_t f, fa = 0;
        for (;;) {
            const uint64_t fw = ld_wt64(myFlag);
            f = __builtin_amdgcn_readfirstlane((uint32_t)fw);
            fa = __builtin_amdgcn_readfirstlane((uint32_t)(fw >> 32));
            if ((f & PP_DONE) || f >= it + 1) break;
            if (pp_timed_out(t0, a.spinTicks)) { f = PP_DONE; break; }
            __builtin_amdgcn_s_sleep(1);
        }
        // alpha of this iteration, in the flag word (PP_DONE carries how many iterations ran: the
        // flag seen here is exactly iteration it's, as the finisher's next one needs this row's Ap)
        const bool haveAlpha = !(f & PP_DONE) || (f & ~PP_DONE) > it;
        if (hasRow && haveAlpha) {  // delta += alpha p (the finisher's order of operations)
            const float alpha = __uint_as_float(fa);
            dlR = dlR + alpha * pvR;
            dlT = dlT + alpha * pvT;
        }
        if (f & PP_DONE) {
            if (hasRow && lane == 0) {
                vstore(a, V_DELTA, v, dlR, dlT);
                if (haveAlpha && (f & PP_DONE)) {  // the PCG loop ended normally: computeLieUpdate (LieDerivUtil.h:301-307)
                    f3 nr, nt;
                    lie_update(dlR, dlT, mk3(a.rot[3 * v], a.rot[3 * v + 1], a.rot[3 * v + 2]),
                               mk3(a.trans[3 * v], a.trans[3 * v + 1], a.trans[3 * v + 2]), nr, nt);
                    a.rot[3 * v] = nr.x; a.rot[3 * v + 1] = nr.y; a.rot[3 * v + 2] = nr.z;
                    a.trans[3 * v] = nt.x; a.trans[3 * v + 1] = nt.y; a.trans[3 * v + 2] = nt.z;
                }
            }
            return;
        }
    }
}

// Inside the k_gn_end that follows every k_pcg_persist launch (one workgroup; a uniform test of the
// error word unless the launch timed out): a persistent launch that timed out (a hand-off never arrived, e.g. the grid was not
// co-resident) redoes the GN step's PCG here, from the state k_pair_init left: the poses it saved are
// restored (the timed-out launch may have applied a partial Lie update), the rows are initialised
// again, and every PCG iteration runs as k_pcg_pairs<RB> + its finisher would, in one workgroup (the
// row order of the per-row work does not enter any sum, and the finisher is the same code), so the
// step's result is bit-identical to BFSolverOptions.pcgLaunch = 1. Bit 3 of the result's error word is
// then cleared and bit 4 set: the solve's result is valid and says that it took this path.
template <int RB>
__device__ __forceinline__ void pcg_recover(const BA& a, float* sh, float wSparse, int nLin) {
    const uint32_t wave = threadIdx.x >> 6, nw = WG / 64;
    for (uint32_t v = 1 + threadIdx.x; v < a.N; v += WG) {
        const float* b = a.poseBak + (size_t)v * 6;
        a.rot[3 * v] = b[0]; a.rot[3 * v + 1] = b[1]; a.rot[3 * v + 2] = b[2];
        a.trans[3 * v] = b[3]; a.trans[3 * v + 1] = b[4]; a.trans[3 * v + 2] = b[5];
    }
    __syncthreads();
    for (uint32_t v = 1 + wave; v < a.N; v += nw) pair_init_row(a, wSparse, v, false);
    __syncthreads();
    pair_init_finish(a, sh);
    if (threadIdx.x == 0) {
        a.ctrl[K_PCG_DONE] = 0;
        a.ctrl[K_PCG_ITERS] = a.ctrl[K_PCG_ITERS0];
    }
    __syncthreads();
    const int useDense = (int)a.ctrl[K_USE_DENSE];
    for (int iter = 0; iter < nLin; iter++) {
        for (uint32_t v = 1 + wave; v < a.N; v += nw) pair_row_ap(a, wSparse, v);
        if (useDense) pcg_dense_offdiag(a, wave, nw);
        __syncthreads();
        float rDotzNew;
        bool last;
        pcg_finisher<RB>(a, sh, 0u, useDense, iter, nLin, rDotzNew, last);
        if (threadIdx.x == 0) {
            a.ctrl[K_RDOTZ] = __float_as_uint(rDotzNew);
            a.ctrl[K_PCG_ITERS]++;
            if (last) a.ctrl[K_PCG_DONE] = 1;
        }
        __syncthreads();
        if (last) break;  // uniform: from block sums
    }
    if (threadIdx.x == 0) a.ctrl[K_ERROR] = (a.ctrl[K_ERROR] & ~PP_ERR_TIMEOUT) | PP_RECOVERED;
}

// EvalGNConvergence (SolverBundling.cu:694-749) + the early-out test of solveBundlingStub (:1204-1210).
// After a persistent PCG launch (recoverRB = its finisher's rows per thread) it first redoes a GN step
// whose launch timed out (pcg_recover; one uniform test otherwise, no launch of its own).
template <int recoverRB>
// nextW > 0: the next GN step is a sparse pair-mode step of weight nextW, whose k_transforms this launch
// does when the loop goes on (one launch fewer per GN step)
__global__ __launch_bounds__(WG) void k_gn_end(BA a, int gnIndex, int nNonLin, float wSparse, int nLin, float nextW) {
    __shared__ float sh[WG];
    if (a.ctrl[K_GN_DONE]) return;
    if (recoverRB && (a.ctrl[K_ERROR] & PP_ERR_TIMEOUT)) {
        pcg_recover<recoverRB ? recoverRB : 2>(a, sh, wSparse, nLin);
        __syncthreads();
    }
    float m = 0.0f;
    for (uint32_t v = 1 + threadIdx.x; v < a.N; v += blockDim.x) {
        if (a.valid[v] == 0) continue;
        f3 dR, dT;
        vload(a, V_DELTA, v, dR, dT);
        const float r = fmaxf(fmaxf(fmaxf(fabsf(dR.x), fabsf(dT.x)), fmaxf(fabsf(dR.y), fabsf(dT.y))), fmaxf(fabsf(dR.z), fabsf(dT.z)));
        m = fmaxf(m, r);
    }
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = fmaxf(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    const bool done = a.earlyOut && gnIndex < nNonLin - 1 && sh[0] < 0.005f;
    if (threadIdx.x == 0) {
        a.ctrl[K_GN_ITERS]++;
        if (done) a.ctrl[K_GN_DONE] = 1;
    }
    if (nextW > 0.0f && !done) {  // k_transforms(a, nextW, 0, 1, 1) of the next step
        transforms_rows(a, threadIdx.x, blockDim.x);
        if (threadIdx.x == 0) {
            a.ctrl[K_PCG_DONE] = 0;
            a.ctrl[K_TICKET] = 0;
            a.ctrl[K_LAST_W] = __float_as_uint(nextW);
            a.ctrl[K_USE_DENSE] = 0u;
        }
    }
}

}  // namespace
}  // namespace bf
