// kernels_attn_window.hip — decode attention of a window: T <= 8 query columns at the CONSECUTIVE positions p, p + 1, ... of one
// sequence, over that sequence's one KV cache (the per-token attention of the reference — AttentionScoreCalculationShader.cs:164-206,
// AttentionSoftmaxShader.cs:139-178, AttentionWeightedValueSumShader.cs:175-216 — for T tokens of the loop LlamaModel.cs:116-125 at
// once).  k_battn (kernels_gemv_batch.hip) would read the cached prefix once per column; here it is read once per kv head.
//
// k_wattn<LPP, G, F16>
//   grid      (slice, kv head); 512 threads.  Slices 0 .. ns - 1 cut the PREFIX rows [0, p) exactly as k_battn cuts a sequence
//             (at most 32 slices of at least 32 rows: a function of p alone); slice ns is the window's own rows [p, p + T), where
//             column i takes rows p .. p + i (causal inside the window).  The q|k|v launch before wrote those rows to the cache.
//   K / V     HBM -> VGPR (16-byte non-temporal loads, issued one tile ahead of the arithmetic) -> LDS as fp32, in tiles of 32 rows:
//             ONE fetch per workgroup, whatever T is.  LDS reads are 16 bytes per lane, consecutive lanes consecutive addresses.
//   columns   the register plan: q, the running output, max and sum of exp cost 10 VGPRs per (column, query head) row, 240 for
//             T = 8, G = 3 in one lane group.  So the eight waves split the COLUMNS: wave w carries column w (G rows, 80 VGPRs
//             at G = 8; two waves per SIMD cover each other's latencies) and walks every row of the tile out of LDS; its 64 / LPP
//             lane groups take the rows of a tile round-robin.  All waves read the same LDS tile, nobody reads HBM twice; the waves
//             of columns >= T only help to fetch.
//   order     column i's sums are formed by wave i: rows dealt to its lane groups by (row - slice start) % groups, online
//             softmax per group, groups merged in group order, slices merged in slice order by the workgroup whose ticket is last
//             (nobody waits).  None of that depends on T or on any other column: column i's output is bit-identical whatever T and
//             the other columns are.
//   bounds    p is clamped to the capacity and rows at or past it are never read; the q|k|v launch raises the error word.
#include <algorithm>
#include <atomic>

#include "common.h"

namespace nfai {

#define GLOBAL_AS __attribute__((address_space(1)))

constexpr uint32_t WA_NSPLIT = 32, WA_MIN_CHUNK = 32;   // the prefix is sliced as k_battn / k_attn_decode slice a sequence
constexpr uint32_t WA_TP = 32;                          // rows per LDS tile

struct WAttnParams {
    const float *q[BATCH_MAX];
    float *o[BATCH_MAX];
    const void *kc, *vc;
    uint64_t head_stride, pos_stride;
    uint32_t cap, n;
    const uint32_t *pos;
    uint32_t Hkv;
    float *partials;     // [Hkv][WA_NSPLIT + 1][BATCH_MAX * G][D + 2]
    uint32_t *tickets;   // [Hkv], zero between launches
};

template <bool F16>
__device__ __forceinline__ f32x4 wa_load4(const void *base, uint64_t idx)
{
    if constexpr (F16) {
        const u32x2 w = __builtin_nontemporal_load((const GLOBAL_AS u32x2 *)(reinterpret_cast<const _Float16 *>(base) + idx));
        return f32x4{h2f_lo(w[0]), h2f_hi(w[0]), h2f_lo(w[1]), h2f_hi(w[1])};
    } else {
        return __builtin_bit_cast(f32x4, load_nt16(reinterpret_cast<const float *>(base) + idx));
    }
}

// sum over the LPP lanes of a row (aligned groups of 16 or 32 lanes), inside the vector ALU (ba_pos_sum of k_battn)
template <int LPP> __device__ __forceinline__ float wa_pos_sum(float v)
{
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
    if constexpr (LPP == 32) {
        const uint32_t b = __builtin_bit_cast(uint32_t, v);
        const auto r = __builtin_amdgcn_permlane16_swap(b, b, false, false);
        v = __builtin_bit_cast(float, (uint32_t)r[0]) + __builtin_bit_cast(float, (uint32_t)r[1]);
    }
    return v;
}

constexpr size_t wa_lds_floats(uint32_t D, uint32_t G)
{
    // K tile | V tile | partial rows [BATCH_MAX * G][64 / LPP][D + 2] (reused by the merge: 3 [BATCH_MAX * G][WA_NSPLIT + 1] tables)
    const size_t part = (size_t)BATCH_MAX * G * (256 / D) * (D + 2);
    const size_t merge = (size_t)3 * BATCH_MAX * G * (WA_NSPLIT + 1) + BATCH_MAX * G;
    return (size_t)2 * WA_TP * D + (part > merge ? part : merge);
}

// LPP = D / 4 lanes per cached row; G query heads share every K / V row of their kv head (GQA), and so do the window's columns.
template <int LPP, int G, bool F16>
__global__ __launch_bounds__(512) void k_wattn(const WAttnParams p)
{
    constexpr int D = LPP * 4, GPW = 64 / LPP, PW = D + 2, NL = (int)WA_TP * LPP / 512, NR = (int)BATCH_MAX * G;
    extern __shared__ __attribute__((aligned(16))) float wa_lds[];
    float *kt = wa_lds, *vt = wa_lds + WA_TP * D, *part = wa_lds + 2 * WA_TP * D;
    __shared__ uint32_t s_last;
    const uint32_t slice = blockIdx.x, kvh = blockIdx.y, T = p.n;
    const uint32_t pz = min(p.pos[0], p.cap);   // never past the cache, whatever the position word holds
    uint32_t nsplit = (pz + WA_MIN_CHUNK - 1) / WA_MIN_CHUNK;
    if (nsplit > WA_NSPLIT) nsplit = WA_NSPLIT;
    uint32_t chunk = 0;
    if (nsplit) {
        chunk = (pz + nsplit - 1) / nsplit;
        nsplit = (pz + chunk - 1) / chunk;
    }
    const uint32_t ns = nsplit + 1;   // + the window's own rows
    if (slice >= ns) return;          // (workgroup-uniform)
    const bool own = slice == nsplit;
    const uint32_t p0 = own ? pz : slice * chunk;
    const uint32_t p1 = own ? min(pz + T, p.cap) : min(pz, p0 + chunk);
    const uint32_t lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t gi = lane / LPP, li = lane % LPP;
    const uint64_t hbase = (uint64_t)kvh * p.head_stride;

    // the wave's column
    const uint32_t c = wid;
    const bool live = c < T;
    const uint32_t last_row = pz + c;   // column c attends to rows <= p + c
    f32x4 qf[G], o[G];
    float m[G], l[G];
    {
        const float *qb = p.q[live ? c : 0];
#pragma unroll
        for (int g = 0; g < G; g++) {
            qf[g] = *reinterpret_cast<const GLOBAL_AS f32x4 *>((const GLOBAL_AS float *)qb + (size_t)(kvh * G + g) * D + li * 4);
            o[g] = f32x4{0.f, 0.f, 0.f, 0.f};
            m[g] = -INFINITY;
            l[g] = 0.f;
        }
    }
    const float sqrt_d = sqrtf((float)D);

    f32x4 kr[NL], vr[NL];
    auto fetch = [&](uint32_t base) {   // the tile's rows (clamped into the slice: what lies past it is loaded and never used)
#pragma unroll
        for (int j = 0; j < NL; j++) {
            const uint32_t e = threadIdx.x + j * 512;
            const uint32_t row = min(base + e / LPP, p1 - 1);
            const uint64_t idx = (uint64_t)row * p.pos_stride + hbase + (e % LPP) * 4;
            kr[j] = wa_load4<F16>(p.kc, idx);
            vr[j] = wa_load4<F16>(p.vc, idx);
        }
    };
    if (p0 < p1) fetch(p0);
    for (uint32_t base = p0; base < p1; base += WA_TP) {
        if (base > p0) __syncthreads();   // every wave is done with the previous tile
#pragma unroll
        for (int j = 0; j < NL; j++) {
            const uint32_t e = threadIdx.x + j * 512;
            *reinterpret_cast<f32x4 *>(kt + (size_t)e * 4) = kr[j];
            *reinterpret_cast<f32x4 *>(vt + (size_t)e * 4) = vr[j];
        }
        __syncthreads();
        if (base + WA_TP < p1) fetch(base + WA_TP);   // in flight under the arithmetic below
        const uint32_t rows = min(WA_TP, p1 - base);
        for (uint32_t r0 = 0; live && r0 < rows; r0 += GPW) {   // wave-uniform trip count
            const uint32_t r = r0 + gi;
            const uint32_t rr = min(r, rows - 1);
            const f32x4 k4 = *reinterpret_cast<const f32x4 *>(kt + (size_t)(rr * LPP + li) * 4);
            const f32x4 v4 = *reinterpret_cast<const f32x4 *>(vt + (size_t)(rr * LPP + li) * 4);
            const bool valid = r < rows && base + r <= last_row;
#pragma unroll
            for (int g = 0; g < G; g++) {
                float d = qf[g][0] * k4[0];
                d = fmaf(qf[g][1], k4[1], d);
                d = fmaf(qf[g][2], k4[2], d);
                d = fmaf(qf[g][3], k4[3], d);
                const float sc = wa_pos_sum<LPP>(d) / sqrt_d;   // AttentionScoreCalculationShader.cs:164-206
                if (valid) {
                    const float mn = fmaxf(m[g], sc);
                    const float cf = expf(m[g] - mn), e = expf(sc - mn);   // exp(-inf) = 0 on the first row
                    l[g] = l[g] * cf + e;
                    o[g][0] = o[g][0] * cf + e * v4[0];
                    o[g][1] = o[g][1] * cf + e * v4[1];
                    o[g][2] = o[g][2] * cf + e * v4[2];
                    o[g][3] = o[g][3] * cf + e * v4[3];
                    m[g] = mn;
                }
            }
        }
    }
    // every (column, head) row's lane groups -> LDS, merged in group order (a group that saw no row has m = -inf, l = 0: weight 0)
    if (live) {
#pragma unroll
        for (int g = 0; g < G; g++) {
            float *pp = part + ((size_t)(c * G + g) * GPW + gi) * PW;
            *reinterpret_cast<f32x2 *>(pp + li * 4) = f32x2{o[g][0], o[g][1]};
            *reinterpret_cast<f32x2 *>(pp + li * 4 + 2) = f32x2{o[g][2], o[g][3]};
            if (li == 0) { pp[D] = m[g]; pp[D + 1] = l[g]; }
        }
    }
    __syncthreads();
    float *gp = p.partials + (size_t)kvh * (WA_NSPLIT + 1) * NR * PW;
    for (uint32_t e = threadIdx.x; e < T * G * D; e += blockDim.x) {
        const uint32_t row = e / D, d = e % D, oc = row / G, g = row % G;
        const float *pr = part + (size_t)row * GPW * PW;
        float M = -INFINITY;
        for (int i = 0; i < GPW; i++) M = fmaxf(M, pr[i * PW + D]);
        float L = 0.f, O = 0.f;
        for (int i = 0; i < GPW; i++) {
            const float w = expf(pr[i * PW + D] - M);
            L += pr[i * PW + D + 1] * w;
            O += pr[i * PW + d] * w;
        }
        if (ns == 1) {
            p.o[oc][(size_t)(kvh * G + g) * D + d] = O / L;   // AttentionSoftmaxShader.cs:139-178 + …ValueSumShader.cs:175-216
        } else {
            float *ps = gp + ((size_t)slice * NR + row) * PW;
            __hip_atomic_store(ps + d, O, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (d == 0) {
                __hip_atomic_store(ps + D, M, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(ps + D + 1, L, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (ns == 1) return;
    // ticket hand-off as in k_battn: partials written through, every thread drains its stores, the workgroup meets, ONE lane takes a
    // ticket; the workgroup whose ticket is last merges the slices in slice order
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t tk = __hip_atomic_fetch_add(&p.tickets[kvh], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = tk == ns - 1 ? 1u : 0u;
        if (tk == ns - 1) __hip_atomic_store(&p.tickets[kvh], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm
    }
    __syncthreads();
    if (s_last == 0u) return;
    // (max, sum of exp) of every (row, slice) first, then every row's weights; `part` is free again (barriers above)
    constexpr uint32_t NSL = WA_NSPLIT + 1;
    float *s_m = part, *s_l = part + NR * NSL, *s_w = part + 2 * NR * NSL, *s_L = part + 3 * NR * NSL;
    const uint32_t nrow = T * G;
    for (uint32_t e = threadIdx.x; e < nrow * ns; e += blockDim.x) {
        const uint32_t row = e / ns, i = e % ns;
        const float *ps = gp + ((size_t)i * NR + row) * PW;
        s_m[row * NSL + i] = __hip_atomic_load(ps + D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_l[row * NSL + i] = __hip_atomic_load(ps + D + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (threadIdx.x < nrow) {
        const uint32_t row = threadIdx.x;
        float M = -INFINITY;
        for (uint32_t i = 0; i < ns; i++) M = fmaxf(M, s_m[row * NSL + i]);
        float L = 0.f;
        for (uint32_t i = 0; i < ns; i++) {
            const float w = expf(s_m[row * NSL + i] - M);
            s_w[row * NSL + i] = w;
            L += s_l[row * NSL + i] * w;
        }
        s_L[row] = L;
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < nrow * D; e += blockDim.x) {
        const uint32_t row = e / D, d = e % D, oc = row / G, g = row % G;
        float O = 0.f;
        for (uint32_t i0 = 0; i0 < ns; i0 += 8) {   // eight loads in flight; slices in order
            float ov[8];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const uint32_t i = min(i0 + j, ns - 1);
                ov[j] = __hip_atomic_load(gp + ((size_t)i * NR + row) * PW + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (i0 + j < ns) O += ov[j] * s_w[row * NSL + i0 + j];
        }
        p.o[oc][(size_t)(kvh * G + g) * D + d] = O / s_L[row];
    }
}

size_t window_attn_bytes(uint32_t H, uint32_t D) { return 4096 + (size_t)BATCH_MAX * (WA_NSPLIT + 1) * H * (D + 2) * 4; }

template <int LPP, int G, bool F16>
static hipError_t launch_wa1(const WAttnParams &p, dim3 grid, hipStream_t s)
{
    constexpr size_t lds = wa_lds_floats(LPP * 4, G) * 4;
    if (lds > 64 * 1024) {   // the kernel's dynamic-LDS limit is raised once per device (gfx950: 160 KB per CU)
        static std::atomic<uint64_t> raised{0};   // bit = device ordinal; ordinals past 63 raise it on every launch
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        const uint64_t bit = dev >= 0 && dev < 64 ? 1ull << dev : 0;
        if (!(raised.load(std::memory_order_relaxed) & bit)) {
            e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_wattn<LPP, G, F16>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            raised.fetch_or(bit, std::memory_order_relaxed);
        }
    }
    hipLaunchKernelGGL((k_wattn<LPP, G, F16>), grid, dim3(512), lds, s, p);
    return hipGetLastError();
}

template <int LPP, bool F16>
static hipError_t launch_wa(const WAttnParams &p, uint32_t G, dim3 grid, hipStream_t s)
{
    switch (G) {
        case 1: return launch_wa1<LPP, 1, F16>(p, grid, s);
        case 2: return launch_wa1<LPP, 2, F16>(p, grid, s);
        case 3: return launch_wa1<LPP, 3, F16>(p, grid, s);
        case 4: return launch_wa1<LPP, 4, F16>(p, grid, s);
        case 8: return launch_wa1<LPP, 8, F16>(p, grid, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_window_attn(const WindowAttnArgs &a, hipStream_t s)
{
    if (a.n < 1 || a.n > BATCH_MAX || a.Hkv == 0 || a.Hkv > 1024 || a.H % a.Hkv || !attn_group_ok(a.H / a.Hkv) || (a.D != 64 && a.D != 128) ||
        !a.work || !a.kc || !a.vc || !a.pos || a.cap == 0)
        return hipErrorInvalidValue;
    WAttnParams p{};
    for (uint32_t b = 0; b < a.n; b++) {
        if (!a.q[b] || !a.o[b]) return hipErrorInvalidValue;
        p.q[b] = a.q[b]; p.o[b] = a.o[b];
    }
    p.kc = a.kc; p.vc = a.vc; p.head_stride = a.kv_head_stride; p.pos_stride = a.kv_pos_stride; p.cap = a.cap; p.n = a.n; p.pos = a.pos;
    p.Hkv = a.Hkv;
    p.tickets = static_cast<uint32_t *>(a.work);                                       // [Hkv] <= 1024 words
    p.partials = reinterpret_cast<float *>(static_cast<char *>(a.work) + 4096);
    const dim3 grid(WA_NSPLIT + 1, a.Hkv);
    const uint32_t G = a.H / a.Hkv;
    const bool f16 = a.kv_type == NFAI_F16;
    if (a.D == 64) return f16 ? launch_wa<16, true>(p, G, grid, s) : launch_wa<16, false>(p, G, grid, s);
    return f16 ? launch_wa<32, true>(p, G, grid, s) : launch_wa<32, false>(p, G, grid, s);
}

}  // namespace nfai
