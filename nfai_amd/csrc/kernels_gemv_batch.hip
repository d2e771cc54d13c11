// kernels_gemv_batch.hip — the decode step for up to 8 sequences at once: every weight row is read from HBM ONCE and applied to the
// activation vectors of all sequences of the batch (MatrixMultiplyShader.cs:255-289 at M = B, with the same prologues / epilogues
// of TransformerBlock.Compute, TransformerBlock.cs:127-184, that kernels_gemv.hip fuses at M = 1), and the attention of all
// sequences in one launch.  A separate family: the batch-1 kernels (k_gemv, k_gemv_sk, k_attn_decode) are not touched.
//
// k_bgemv<B, MODE, NORM>
//   Bound: HBM (the weights), as at B = 1; the B-fold arithmetic rides on the same bytes (B = 8: ~15 % of the VALU rate).
//   weights   HBM -> VGPR, 16-byte non-temporal loads, each row read once, never through LDS (guide, row "GEMV / M <= 16").
//   x         LDS, fp32, one plane layout per column (lane l's two ds_read_b128 of a 512-element chunk sit at l * 16 bytes in two
//             1-KiB planes: conflict-free).  An x fragment read from LDS serves R = 4 rows (the register block is R x B sums), so
//             the LDS read rate is 4 B / 4 bytes per weight byte pair: B = 8 asks for 12 * 8 / 4 = 24 TB/s chip-wide at 6 TB/s of
//             weights, a sixth of what ds_read_b128 delivers.
//   capacity  B vectors of K floats do not always fit (B = 8, K = 8192: 256 KiB; K = 14336: 448 KiB; 160 KiB per CU): x is staged
//             in K tiles of at most 128 KiB.  One tile (every launch whose K is the embedding width, and everything at B = 2): a wave
//             walks its row groups one after another.  Several tiles (Wdown at B >= 4): every wave owns exactly ONE row group (the host
//             sizes the grid so) and carries its R x B sums across the tiles; the tile's first weight step is requested before the
//             workgroup meets to restage x.
//   order     a (row, column) sum is formed by lane l over k = 512 c + 8 l .. + 7 for c = 0, 1, ... in one fp32 chain, then summed
//             over the wave by one butterfly for all R x B sums (bg_reduce): the same chain and the same tree whatever B, the tile
//             size, the grid and the other columns are — a column's
//             result does not depend on its position in the batch, on the batch size or on its neighbours, bit for bit.
//   columns   >= n are dead: they read column 0's x and store nothing.
// k_battn<LPP, G, F16>
//   grid (KV slice, kv head, sequence); per-sequence pointers / strides / capacities arrive as a table in the kernel argument
//   (the caches are separate allocations of separate models).  One pass, online softmax per group of D/4 lanes, groups merged in LDS
//   in fixed order, slices merged by the workgroup whose ticket is last, in slice order: bit-reproducible, and nobody waits.
#include <stdlib.h>

#include <algorithm>

#include "common.h"

namespace nfai {

#define GLOBAL_AS __attribute__((address_space(1)))

constexpr int BG_R = 4, BG_U = 2;                 // rows per register block, 512-element chunks per step
constexpr uint32_t BG_LDS_X = 128 * 1024;         // bytes of LDS for the x tile
constexpr uint32_t BG_CS = 128;                   // cos / sin words per column (head_dim <= 128)
constexpr uint32_t BG_MAX_GRID = 1024;            // argmax partials per column

struct BGemvParams {
    const uint8_t *W[3];
    uint32_t seg_end[3];
    uint64_t row_bytes;
    uint32_t K, KT, ntiles, NU, n;
    const float *gamma;
    float eps;
    const float *x[BATCH_MAX];
    float *y[BATCH_MAX];
    const float *res[BATCH_MAX];
    void *kc[BATCH_MAX], *vc[BATCH_MAX];
    uint64_t head_stride[BATCH_MAX];
    uint32_t cap[BATCH_MAX];
    const uint32_t *pos[BATCH_MAX];
    uint32_t pos_off[BATCH_MAX];   // zeros for a batch; a window's column b sits b positions past the one position word
    uint64_t pos_stride;
    int kv_f16;
    const float *freqs;
    uint32_t rope_dims, D;
    uint32_t *err;
    // lm_head: per-column ArgMax
    float *part_v;       // [BATCH_MAX][BG_MAX_GRID]
    uint32_t *part_i;
    uint32_t *ticket;
    uint32_t *tok_batch;
    uint32_t *tok[BATCH_MAX], *pos_inc[BATCH_MAX], *ring[BATCH_MAX];
    uint32_t ring_len;
    const uint32_t *win_ctl;   // non-null: the columns are one sequence's window (win_tail, common.h)
};

__device__ __forceinline__ uint32_t bg_xs_index(uint32_t k)
{
    const uint32_t chunk = k >> 9, within = k & 511;
    return (chunk << 9) + (((within >> 2) & 1) << 8) + ((within >> 3) << 2) + (within & 3);
}

template <int MODE>
__device__ __forceinline__ const uint8_t *bg_row_ptr(const BGemvParams &p, uint32_t unit, int sub)
{
    if constexpr (MODE == GEMV_GATEUP) {
        return p.W[sub] + (uint64_t)unit * p.row_bytes;  // sub 0 = gate row, 1 = up row
    } else if constexpr (MODE == GEMV_QKV_ROPE) {
        const uint32_t row = unit * 2 + sub;
        if (row < p.seg_end[0]) return p.W[0] + (uint64_t)row * p.row_bytes;
        if (row < p.seg_end[1]) return p.W[1] + (uint64_t)(row - p.seg_end[0]) * p.row_bytes;
        return p.W[2] + (uint64_t)(row - p.seg_end[1]) * p.row_bytes;
    } else {
        return p.W[0] + (uint64_t)unit * p.row_bytes;
    }
}

// What a lane needs to finish rows of ITS column (the column is a function of the lane, see bg_reduce): selected once per launch.
struct BGLane {
    float *y;
    const float *res;
    void *kc, *vc;
    uint64_t head_stride;
    const float *cs;     // LDS: cos / sin of the column's position
    uint32_t pos;
    bool pos_ok;
};

// Epilogue of unit `unit` of the lane's column; fully reduced sums (the epilogues of kernels_gemv.hip, per column).
template <int MODE>
__device__ __forceinline__ void bg_epilogue(const BGemvParams &p, const BGLane &c, uint32_t unit, float a0, float a1)
{
    if constexpr (MODE == GEMV_PLAIN) {
        c.y[unit] = a0;
    } else if constexpr (MODE == GEMV_RESIDUAL) {
        c.y[unit] = c.res[unit] + a0;                    // TransformerBlock.cs:153-158 / 176-180: input + projection
    } else if constexpr (MODE == GEMV_GATEUP) {
        c.y[unit] = a1 * silu_ref(a0);                   // SiLUShader.cs:121-123, ElementWiseMultiplicationShader.cs:137
    } else {
        // RoPEShader.cs:249-262 on the pair (row, row + 1) at THIS column's position; V rows are stored unrotated
        const uint32_t row = unit * 2;
        const uint32_t seg = row < p.seg_end[0] ? 0u : (row < p.seg_end[1] ? 1u : 2u);
        const uint32_t r = seg == 0 ? row : (seg == 1 ? row - p.seg_end[0] : row - p.seg_end[1]);
        const uint32_t head = r / p.D, d = r % p.D;
        float o0 = a0, o1 = a1;
        if (seg < 2 && d < p.rope_dims) {
            const float cc = c.cs[d], ss = c.cs[d + 1];
            o0 = cc * a0 - ss * a1;
            o1 = ss * a0 + cc * a1;
        }
        if (seg == 0) {
            c.y[row] = o0;
            c.y[row + 1] = o1;
        } else if (c.pos_ok) {   // a position word at or past the capacity writes nothing (the launch reports it through p.err)
            const uint64_t idx = (uint64_t)c.pos * p.pos_stride + (uint64_t)head * c.head_stride + d;
            void *base = seg == 1 ? c.kc : c.vc;
            kv_store(base, p.kv_f16, idx, o0);
            kv_store(base, p.kv_f16, idx + 1, o1);
        }
    }
}

// Sum of NV per-lane values over the 64 lanes of the wave, all NV at once: a butterfly over the lane bits 32, 16, 8, 4, 2, 1 in
// which, while more than one value is left, the two lanes of a pair split the values between them (the lane with the bit clear
// keeps the even ones and hands over the odd ones, and the other way round).  NV + 5 exchanges instead of 6 NV, and no value
// travels through scalar registers.  Every value is summed by the same tree — pairs (l, l ^ 32), then ^ 16, ... ^ 1 — whatever
// NV is (fp32 addition commutes), so a (row, column) sum does not depend on the batch size.  Returns the total of value
// j(lane): bit s of j = bit (5 - s) of the lane for s < log2(NV); the 64 / NV lanes that agree in those bits hold the same total.
template <int N, int M>
__device__ __forceinline__ void bg_reduce_step(float (&v)[32], uint32_t lane)
{
    if constexpr (N > 1) {
        const bool hi = (lane & M) != 0;
#pragma unroll
        for (int i = 0; i < N / 2; i++) {
            const float keep = hi ? v[2 * i + 1] : v[2 * i];
            const float send = hi ? v[2 * i] : v[2 * i + 1];
            v[i] = keep + __shfl_xor(send, M);
        }
    } else {
        v[0] = v[0] + __shfl_xor(v[0], M);
    }
}
template <int NV>
__device__ __forceinline__ float bg_reduce(float (&v)[32], uint32_t lane)
{
    static_assert(NV == 8 || NV == 16 || NV == 32, "R x B values");
    bg_reduce_step<NV, 32>(v, lane);
    bg_reduce_step<(NV > 1 ? NV / 2 : 1), 16>(v, lane);
    bg_reduce_step<(NV > 2 ? NV / 4 : 1), 8>(v, lane);
    bg_reduce_step<(NV > 4 ? NV / 8 : 1), 4>(v, lane);
    bg_reduce_step<(NV > 8 ? NV / 16 : 1), 2>(v, lane);
    bg_reduce_step<(NV > 16 ? NV / 32 : 1), 1>(v, lane);
    return v[0];
}

template <int B, int MODE, bool NORM>
__global__ __launch_bounds__(512) void k_bgemv(const BGemvParams p)
{
    constexpr int RPU = (MODE == GEMV_QKV_ROPE || MODE == GEMV_GATEUP) ? 2 : 1;
    constexpr int R = BG_R, UPW = R / RPU, U = B == 8 ? 1 : BG_U;   // B = 8: one chunk per step keeps the R x B block and its x fragments in registers
    extern __shared__ __attribute__((aligned(16))) float xs[];  // [B][KT] x | [B][16] sums | [B][BG_CS] cos,sin | 64 words of the ArgMax
    const uint32_t KT = p.KT;
    float *red = xs + (size_t)B * KT;
    float *cs = red + B * 16;
    uint32_t *am_lds = reinterpret_cast<uint32_t *>(cs + B * BG_CS);

    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nwaves = blockDim.x >> 6;
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t gw = blockIdx.x * nwaves + wid, tw = gridDim.x * nwaves;
    const uint32_t total_groups = (p.NU + UPW - 1) / UPW;
    const uint32_t ngroups = total_groups > gw ? (total_groups - gw + tw - 1) / tw : 0;   // groups dealt round-robin over the waves
    auto unit_at = [&](uint32_t g, uint32_t q) { return (g * tw + gw) * UPW + q; };

    // positions (q|k|v only): a column whose position word is not below its capacity stores no K / V row and raises the error word
    uint32_t posv[B];
    bool pos_ok[B];
#pragma unroll
    for (int b = 0; b < B; b++) { posv[b] = 0; pos_ok[b] = true; }
    if constexpr (MODE == GEMV_QKV_ROPE) {
#pragma unroll
        for (int b = 0; b < B; b++) {
            posv[b] = p.pos[b][0] + p.pos_off[b];
            pos_ok[b] = posv[b] < p.cap[b];
            if (!pos_ok[b] && (uint32_t)b < p.n && blockIdx.x == 0 && threadIdx.x == 0) p.err[0] = 0x10000u | (uint32_t)b;
        }
        // cos / sin of every column's position, tabulated once per workgroup (read by its epilogues behind the staging barrier)
        const uint32_t n_freq = p.rope_dims / 2;
        for (uint32_t t = threadIdx.x; t < B * 64; t += blockDim.x) {
            const uint32_t b = t >> 6, pair = t & 63;
            if (pair < n_freq) {
                uint32_t pb = 0;
#pragma unroll
                for (int c = 0; c < B; c++) pb = (b == (uint32_t)c) ? posv[c] : pb;
                const f32x2 v = rope_cs_of(p.freqs, pair, pb);
                cs[b * BG_CS + 2 * pair] = v[0];
                cs[b * BG_CS + 2 * pair + 1] = v[1];
            }
        }
    }

    // The lane's share of a finished row group (bg_reduce): value j = column * R + row; lane bits 5, 4 = row, bits 3.. = column.
    constexpr int NV = R * B;
    const uint32_t l_row = ((lane >> 5) & 1u) | (((lane >> 4) & 1u) << 1);
    const uint32_t l_col = (((lane >> 3) & 1u) | (((lane >> 2) & 1u) << 1) | (((lane >> 1) & 1u) << 2)) & (uint32_t)(B - 1);
    // one lane per value stores (the 64 / NV replicas agree); row pairs (RoPE, SiLU * up) are finished by the lane of the even row
    const bool l_store = (lane & (uint32_t)(64 / NV - 1)) == 0 && l_col < p.n && (RPU == 1 || (l_row & 1u) == 0);
    const uint32_t l_q = l_row / RPU;
    BGLane lc;
    lc.y = p.y[0]; lc.res = p.res[0]; lc.kc = p.kc[0]; lc.vc = p.vc[0]; lc.head_stride = p.head_stride[0];
    lc.pos = posv[0]; lc.pos_ok = pos_ok[0];
#pragma unroll
    for (int c = 1; c < B; c++) {
        if (l_col == (uint32_t)c) {
            lc.y = p.y[c]; lc.res = p.res[c]; lc.kc = p.kc[c]; lc.vc = p.vc[c]; lc.head_stride = p.head_stride[c];
            lc.pos = posv[c]; lc.pos_ok = pos_ok[c];
        }
    }
    lc.cs = cs + l_col * BG_CS;

    // ---- weight stream: steps (group g, chunk group cg) of the current tile, two register buffers ------------------------------
    u32x4 bufA[R][U], bufB[R][U];
    const uint8_t *rows[R];
    uint32_t tile = 0, cpg = 0, nsteps = 0;
    uint32_t ig = 0, icg = 0;   // issue walker
    uint32_t cg_ = 0, ccg = 0;  // compute walker
    auto issue = [&](u32x4 (&buf)[R][U]) {
        if (icg == 0) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                const uint32_t u = min(unit_at(ig, r / RPU), p.NU - 1);   // clamped to a valid row: the loads are unconditional
                rows[r] = bg_row_ptr<MODE>(p, u, r % RPU);
            }
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
#pragma unroll
            for (int j = 0; j < U; j++) {
                // past the end of the row the address is clamped into it; x is zero there
                const uint32_t k = min(tile * KT + (icg * U + j) * 512 + lane * 8, p.K - 8);
                buf[r][j] = load_nt16(rows[r] + (uint64_t)k * 2);
            }
        }
        if (++icg == cpg) { icg = 0; ++ig; }
    };

    float acc[R][B];
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int b = 0; b < B; b++) acc[r][b] = 0.f;
    float best_v = -INFINITY;
    uint32_t best_i = 0xFFFFFFFFu;

    auto consume = [&](u32x4 (&buf)[R][U]) {
#pragma unroll
        for (int j = 0; j < U; j++) {
            const uint32_t off = ((ccg * U + j) << 9) + (lane << 2);
#pragma unroll
            for (int b = 0; b < B; b++) {
                const f32x4 x0 = *reinterpret_cast<const f32x4 *>(xs + (size_t)b * KT + off);
                const f32x4 x1 = *reinterpret_cast<const f32x4 *>(xs + (size_t)b * KT + off + 256);
#pragma unroll
                for (int r = 0; r < R; r++) acc[r][b] = dot8_f16(buf[r][j], x0, x1, acc[r][b]);
            }
        }
        if (ccg == cpg - 1 && tile == p.ntiles - 1) {
            float v[32];
#pragma unroll
            for (int b = 0; b < B; b++)
#pragma unroll
                for (int r = 0; r < R; r++) v[b * R + r] = acc[r][b];
            const float mine = bg_reduce<NV>(v, lane);
            float a0 = mine, a1 = 0.f;
            if constexpr (RPU == 2) a1 = __shfl_xor(mine, 32);   // the odd row of the pair lives in the lane with bit 5 set
            const uint32_t u = unit_at(cg_, l_q);
            if (l_store && u < p.NU) {
                bg_epilogue<MODE>(p, lc, u, a0, a1);
                if constexpr (MODE == GEMV_PLAIN) {
                    if (topk_better(a0, u, best_v, best_i)) { best_v = a0; best_i = u; }
                }
            }
#pragma unroll
            for (int r = 0; r < R; r++)
#pragma unroll
                for (int b = 0; b < B; b++) acc[r][b] = 0.f;
        }
        if (++ccg == cpg) { ccg = 0; ++cg_; }
    };

    const uint32_t kpad = (p.K + 1023) & ~1023u;   // K rounded up to whole steps
    for (tile = 0; tile < p.ntiles; tile++) {
        const uint32_t k0 = tile * KT;
        cpg = (min(KT, kpad - k0)) / (512 * U);
        nsteps = ngroups * cpg;
        ig = 0; icg = 0; cg_ = 0; ccg = 0;
        issue(bufA);                        // does not depend on x: in flight while the workgroup stages the tile
        if (tile > 0) __syncthreads();      // every wave is done with the previous tile
        // ---- x tile -> LDS (RMSNorm per column first: RMSNormShader.cs:136-149; NORM launches have one tile) ---------------------
        float rms[B];
#pragma unroll
        for (int b = 0; b < B; b++) rms[b] = 1.f;
        if constexpr (NORM) {
            float ss[B];
#pragma unroll
            for (int b = 0; b < B; b++) {
                ss[b] = 0.f;
                for (uint32_t i = threadIdx.x * 4; i < p.K; i += blockDim.x * 4) {
                    const f32x4 v = *reinterpret_cast<const GLOBAL_AS f32x4 *>((const GLOBAL_AS float *)p.x[b] + i);
                    ss[b] = fmaf(v[0], v[0], ss[b]);
                    ss[b] = fmaf(v[1], v[1], ss[b]);
                    ss[b] = fmaf(v[2], v[2], ss[b]);
                    ss[b] = fmaf(v[3], v[3], ss[b]);
                }
                ss[b] = wave_sum(ss[b]);
                if (lane == 0) red[b * 16 + wid] = ss[b];
            }
            __syncthreads();
#pragma unroll
            for (int b = 0; b < B; b++) {
                float t = 0.f;
                for (uint32_t w = 0; w < nwaves; w++) t += red[b * 16 + w];
                rms[b] = sqrtf(t / (float)p.K + p.eps);
            }
        }
#pragma unroll
        for (int b = 0; b < B; b++) {
            for (uint32_t i = threadIdx.x * 4; i < KT; i += blockDim.x * 4) {
                const uint32_t k = k0 + i;
                f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                if (k < p.K) {
                    v = *reinterpret_cast<const GLOBAL_AS f32x4 *>((const GLOBAL_AS float *)p.x[b] + k);
                    if constexpr (NORM) {
                        const f32x4 g = *reinterpret_cast<const GLOBAL_AS f32x4 *>((const GLOBAL_AS float *)p.gamma + k);
                        v[0] = (v[0] / rms[b]) * g[0];
                        v[1] = (v[1] / rms[b]) * g[1];
                        v[2] = (v[2] / rms[b]) * g[2];
                        v[3] = (v[3] / rms[b]) * g[3];
                    }
                }
                *reinterpret_cast<f32x4 *>(xs + (size_t)b * KT + bg_xs_index(i)) = v;
            }
        }
        __syncthreads();
        issue(bufB);
        // ---- ping-pong over the steps (refills inside the loop are unconditional; the last one to three steps are peeled) ------
        uint32_t st = 0;
        for (; st + 3 < nsteps; st += 2) {
            consume(bufA);
            issue(bufA);
            consume(bufB);
            issue(bufB);
        }
        const uint32_t rem = nsteps - st;
        if (rem == 3) {
            consume(bufA);
            issue(bufA);
            consume(bufB);
            consume(bufA);
        } else if (rem == 2) {
            consume(bufA);
            consume(bufB);
        } else if (rem == 1) {
            consume(bufA);
        }
    }

    if constexpr (MODE == GEMV_PLAIN) {
        // SamplingUtils.ArgMax per column in the same launch (SamplingUtils.cs:55-56: the LOWEST index among equal maxima), then the
        // end-of-token bookkeeping of every member: token word, ring, position.  l_col is the column a storing lane has finished rows of.
        float *sv = reinterpret_cast<float *>(am_lds);        // [B][16]... laid out [16][B]
        uint32_t *si = am_lds + 16 * B, *last = am_lds + 32 * B;
#pragma unroll
        for (int b = 0; b < B; b++) {
            const bool mine = l_store && l_col == (uint32_t)b;
            float v = mine ? best_v : -INFINITY;
            uint32_t i = mine ? best_i : 0xFFFFFFFFu;
            wave_best(v, i);
            if (lane == 0) { sv[wid * B + b] = v; si[wid * B + b] = i; }
        }
        __syncthreads();
        if (threadIdx.x < (uint32_t)B) {
            const uint32_t b = threadIdx.x;
            float v = sv[b];
            uint32_t i = si[b];
            for (uint32_t w = 1; w < nwaves; w++)
                if (topk_better(sv[w * B + b], si[w * B + b], v, i)) { v = sv[w * B + b]; i = si[w * B + b]; }
            __hip_atomic_store(&p.part_v[b * BG_MAX_GRID + blockIdx.x], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&p.part_i[b * BG_MAX_GRID + blockIdx.x], i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t tk = __hip_atomic_fetch_add(p.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            last[0] = (tk == gridDim.x - 1) ? 1u : 0u;
        }
        __syncthreads();
        if (last[0] == 0u) return;
        // the workgroup whose ticket is last: (value desc, index asc) is a total order, so the result does not depend on which it is
        if (wid < (uint32_t)B) {    // wave b combines column b (nwaves >= B is a launch rule)
            const uint32_t b = wid;
            float v = -INFINITY;
            uint32_t i = 0xFFFFFFFFu;
            for (uint32_t g = lane; g < gridDim.x; g += 64) {
                const float ov = __hip_atomic_load(&p.part_v[b * BG_MAX_GRID + g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t oi = __hip_atomic_load(&p.part_i[b * BG_MAX_GRID + g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (topk_better(ov, oi, v, i)) { v = ov; i = oi; }
            }
            wave_best(v, i);
            if (lane == 0 && b < p.n) {
                if (p.win_ctl) {
                    last[8 + b] = i;   // the accept rule needs every column's choice
                } else {
                    p.tok_batch[b] = i;
                    p.tok[b][0] = i;
                    const uint32_t pp = p.pos_inc[b][0];
                    p.ring[b][pp % p.ring_len] = i;
                    p.pos_inc[b][0] = pp + 1;
                }
            }
        }
        if (p.win_ctl) {   // (uniform over the launch)
            __syncthreads();
            if (threadIdx.x == 0) win_tail(last + 8, p.n, p.win_ctl, p.tok_batch, p.tok[0], p.pos_inc[0], p.ring[0], p.ring_len);
        }
        if (threadIdx.x == 0) __hip_atomic_store(p.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm (stream-ordered with the next launch)
    }
}

// ---- host side of k_bgemv -------------------------------------------------------------------------------------------------------
struct BGemvPlan { bool ok; int Bt; uint32_t KT, ntiles, nwaves, grid, NU; size_t lds; };

static BGemvPlan plan_bgemv(const BatchGemvArgs &a)
{
    BGemvPlan pl{};
    if (a.n < 1 || a.n > BATCH_MAX || a.K < 8 || a.K % 8 || a.n_cu == 0) return pl;
    pl.Bt = a.n <= 2 ? 2 : (a.n <= 4 ? 4 : 8);
    const uint32_t rows = a.seg_rows[0] + a.seg_rows[1] + a.seg_rows[2];
    const bool pairs = a.mode == GEMV_QKV_ROPE || a.mode == GEMV_GATEUP;
    if (a.mode == GEMV_QKV_ROPE) {
        if (a.seg_rows[0] % 2 || a.seg_rows[1] % 2 || a.seg_rows[2] % 2 || (a.D != 64 && a.D != 128) || a.rope_dims > a.D || a.rope_dims % 2) return pl;
        pl.NU = rows / 2;
    } else if (a.mode == GEMV_GATEUP) {
        if (a.seg_rows[0] != a.seg_rows[1] || a.seg_rows[2]) return pl;
        pl.NU = a.seg_rows[0];
    } else {
        if (a.seg_rows[1] || a.seg_rows[2]) return pl;
        pl.NU = rows;
    }
    if (pl.NU == 0) return pl;
    const uint32_t upw = BG_R / (pairs ? 2 : 1);
    const uint32_t groups = (pl.NU + upw - 1) / upw;
    const uint32_t kpad = (a.K + 1023) & ~1023u;
    const uint32_t kt_max = BG_LDS_X / (4 * (uint32_t)pl.Bt) / 1024 * 1024;
    pl.ntiles = (kpad + kt_max - 1) / kt_max;
    pl.KT = ((kpad / 1024 + pl.ntiles - 1) / pl.ntiles) * 1024;   // even tiles, whole steps
    pl.ntiles = (kpad + pl.KT - 1) / pl.KT;
    if (a.gamma && pl.ntiles > 1) return pl;   // the RMSNorm prologue sees the whole vector
    const uint32_t min_waves = a.mode == GEMV_PLAIN ? 8u : 4u;   // the ArgMax tail gives column b to wave b
    uint32_t nw = (groups + a.n_cu - 1) / a.n_cu;
    nw = std::min(8u, std::max(min_waves, nw));
    pl.nwaves = nw;
    pl.grid = std::min(a.n_cu, (groups + nw - 1) / nw);
    if (pl.ntiles > 1 && (uint64_t)pl.grid * nw < groups) return pl;   // tiled: one row group per wave
    if (a.mode == GEMV_PLAIN && pl.grid > BG_MAX_GRID) return pl;
    pl.lds = ((size_t)pl.Bt * pl.KT + (size_t)pl.Bt * 16 + (size_t)pl.Bt * BG_CS + 64 * 8) * 4;
    pl.ok = pl.lds <= 160 * 1024;
    return pl;
}

bool batch_gemv_ok(const BatchGemvArgs &a) { return plan_bgemv(a).ok; }

template <int B, int MODE, bool NORM>
static hipError_t launch_bg(const BGemvParams &p, const BGemvPlan &pl, hipStream_t s)
{
    static size_t allowed = 0;   // the kernel's dynamic-LDS limit is raised once per size class (gfx950: 160 KB per CU)
    if (pl.lds > 64 * 1024 && pl.lds > allowed) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bgemv<B, MODE, NORM>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        allowed = 160 * 1024;
    }
    hipLaunchKernelGGL((k_bgemv<B, MODE, NORM>), dim3(pl.grid), dim3(pl.nwaves * 64), pl.lds, s, p);
    return hipGetLastError();
}

template <int B>
static hipError_t dispatch_bg(const BGemvParams &p, const BGemvPlan &pl, int mode, bool norm, hipStream_t s)
{
    switch (mode) {
        case GEMV_PLAIN: return norm ? launch_bg<B, GEMV_PLAIN, true>(p, pl, s) : hipErrorInvalidValue;
        case GEMV_RESIDUAL: return norm ? hipErrorInvalidValue : launch_bg<B, GEMV_RESIDUAL, false>(p, pl, s);
        case GEMV_QKV_ROPE: return norm ? launch_bg<B, GEMV_QKV_ROPE, true>(p, pl, s) : hipErrorInvalidValue;
        case GEMV_GATEUP: return norm ? launch_bg<B, GEMV_GATEUP, true>(p, pl, s) : hipErrorInvalidValue;
    }
    return hipErrorInvalidValue;
}

hipError_t launch_batch_gemv(const BatchGemvArgs &a, hipStream_t s)
{
    const BGemvPlan pl = plan_bgemv(a);
    if (!pl.ok) return hipErrorInvalidValue;
    BGemvParams p{};
    uint32_t end = 0;
    for (int i = 0; i < 3; i++) {
        p.W[i] = static_cast<const uint8_t *>(a.W[i] ? a.W[i] : a.W[0]);
        end += a.seg_rows[i];
        p.seg_end[i] = end;
    }
    p.row_bytes = (uint64_t)a.K * 2;
    p.K = a.K; p.KT = pl.KT; p.ntiles = pl.ntiles; p.NU = pl.NU; p.n = a.n;
    p.gamma = a.gamma; p.eps = a.eps;
    for (uint32_t b = 0; b < BATCH_MAX; b++) {
        const uint32_t c = b < a.n ? b : 0;   // dead columns read column 0's input (and store nothing)
        p.x[b] = a.x[c]; p.y[b] = a.y[c]; p.res[b] = a.res[c];
        p.kc[b] = a.kc[c]; p.vc[b] = a.vc[c]; p.head_stride[b] = a.kv_head_stride[c]; p.cap[b] = a.cap[c]; p.pos[b] = a.pos[c]; p.pos_off[b] = a.pos_off[c];
        p.tok[b] = a.am_tok[c]; p.pos_inc[b] = a.am_pos[c]; p.ring[b] = a.am_ring[c];
        if (!p.x[b] || !p.y[b]) return hipErrorInvalidValue;
        if (a.mode == GEMV_RESIDUAL && !p.res[b]) return hipErrorInvalidValue;
        if (a.mode == GEMV_QKV_ROPE && (!p.kc[b] || !p.vc[b] || !p.pos[b])) return hipErrorInvalidValue;
        if (a.mode == GEMV_PLAIN && (!p.tok[b] || !p.pos_inc[b] || !p.ring[b])) return hipErrorInvalidValue;
    }
    p.pos_stride = a.kv_pos_stride; p.kv_f16 = a.kv_type == NFAI_F16 ? 1 : 0;
    p.freqs = a.freqs; p.rope_dims = a.rope_dims; p.D = a.D ? a.D : 64; p.err = a.err;
    if (a.mode == GEMV_QKV_ROPE && (!a.freqs || !a.err)) return hipErrorInvalidValue;
    if (a.mode == GEMV_PLAIN) {
        if (!a.am_work || !a.am_tok_batch || a.am_ring_len == 0) return hipErrorInvalidValue;
        p.part_v = static_cast<float *>(a.am_work);
        p.part_i = reinterpret_cast<uint32_t *>(p.part_v + BATCH_MAX * BG_MAX_GRID);
        p.ticket = p.part_i + BATCH_MAX * BG_MAX_GRID;
        p.tok_batch = a.am_tok_batch; p.ring_len = a.am_ring_len; p.win_ctl = a.win_ctl;
    }
    const bool norm = a.gamma != nullptr;
    if (pl.Bt == 2) return dispatch_bg<2>(p, pl, a.mode, norm, s);
    if (pl.Bt == 4) return dispatch_bg<4>(p, pl, a.mode, norm, s);
    return dispatch_bg<8>(p, pl, a.mode, norm, s);
}

// ---- embedding rows of the n tokens (TokenEmbedShader.cs:131-159, fp16 table) -----------------------------------------------------
struct BEmbedParams { const uint8_t *table; uint64_t n_rows; uint32_t E; const uint32_t *tok; float *x[BATCH_MAX]; };

__global__ __launch_bounds__(256) void k_bembed(const BEmbedParams p)
{
    const uint32_t b = blockIdx.y;
    uint64_t row = p.tok[b];
    if (row >= p.n_rows) row = p.n_rows - 1;   // (the host checks the tokens it is given; a fed-back ArgMax is always a row)
    for (uint32_t k = (blockIdx.x * blockDim.x + threadIdx.x) * 4; k < p.E; k += gridDim.x * blockDim.x * 4)
        *reinterpret_cast<f32x4 *>(p.x[b] + k) = embed_load4(p.table, NFAI_F16, p.n_rows, row, k, p.E);
}

hipError_t launch_batch_embed(const void *table, uint64_t n_rows, uint32_t E, const uint32_t *tok, float *const *x, uint32_t n, hipStream_t s)
{
    if (!table || !tok || n < 1 || n > BATCH_MAX || E % 4 || n_rows == 0) return hipErrorInvalidValue;
    BEmbedParams p{};
    p.table = static_cast<const uint8_t *>(table); p.n_rows = n_rows; p.E = E; p.tok = tok;
    for (uint32_t b = 0; b < n; b++) {
        if (!x[b]) return hipErrorInvalidValue;
        p.x[b] = x[b];
    }
    hipLaunchKernelGGL(k_bembed, dim3((E / 4 + 255) / 256, n), dim3(256), 0, s, p);
    return hipGetLastError();
}

// ---- attention of n sequences in one launch -----------------------------------------------------------------------------------------
constexpr uint32_t BA_NSPLIT = 32, BA_MIN_CHUNK = 32;   // the slicing of k_attn_decode (ATTN_NSPLIT_MAX, ATTN_MIN_CHUNK)

struct BAttnParams {
    const float *q[BATCH_MAX];
    float *o[BATCH_MAX];
    const void *kc[BATCH_MAX], *vc[BATCH_MAX];
    uint64_t head_stride[BATCH_MAX];
    uint32_t cap[BATCH_MAX];
    const uint32_t *pos[BATCH_MAX];
    uint64_t pos_stride;
    uint32_t Hkv;
    float *partials;     // [n][Hkv][BA_NSPLIT][G][D + 2]
    uint32_t *tickets;   // [n][Hkv], zero between launches
};

template <bool F16>
__device__ __forceinline__ f32x4 ba_load4(const void *base, uint64_t idx)
{
    if constexpr (F16) {
        const u32x2 w = __builtin_nontemporal_load((const GLOBAL_AS u32x2 *)(reinterpret_cast<const _Float16 *>(base) + idx));
        return f32x4{h2f_lo(w[0]), h2f_hi(w[0]), h2f_lo(w[1]), h2f_hi(w[1])};
    } else {
        return __builtin_bit_cast(f32x4, load_nt16(reinterpret_cast<const float *>(base) + idx));
    }
}

// sum over the LPP lanes of a position (aligned groups of 16 or 32 lanes), inside the vector ALU
template <int LPP> __device__ __forceinline__ float ba_pos_sum(float v)
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

// LPP = D / 4 lanes per cached position; G query heads share every K / V load of their kv head (GQA).
template <int LPP, int G, bool F16>
__global__ __launch_bounds__(256) void k_battn(const BAttnParams p)
{
    constexpr int D = LPP * 4, GPW = 64 / LPP, NG = 4 * GPW, PW = D + 2;
    __shared__ __attribute__((aligned(16))) float part[NG * G * PW];
    __shared__ uint32_t s_last;
    const uint32_t split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
    const uint32_t S = min(p.pos[b][0] + 1u, p.cap[b]);   // never past the cache, whatever the position word holds
    uint32_t nsplit = (S + BA_MIN_CHUNK - 1) / BA_MIN_CHUNK;
    if (nsplit > BA_NSPLIT) nsplit = BA_NSPLIT;
    const uint32_t chunk = (S + nsplit - 1) / nsplit;
    nsplit = (S + chunk - 1) / chunk;
    if (split >= nsplit) return;   // the slices a sequence's depth does not need (workgroup-uniform)
    const uint32_t p0 = split * chunk, p1 = min(S, p0 + chunk);
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint32_t grp = wid * GPW + lane / LPP, li = lane % LPP;
    const float *qb = p.q[b];
    const void *kc = p.kc[b], *vc = p.vc[b];
    const uint64_t hbase = (uint64_t)kvh * p.head_stride[b] + li * 4;

    f32x4 qf[G], o[G];
    float m[G], l[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
        qf[g] = *reinterpret_cast<const GLOBAL_AS f32x4 *>((const GLOBAL_AS float *)qb + (size_t)(kvh * G + g) * D + li * 4);
        o[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        m[g] = -INFINITY;
        l[g] = 0.f;
    }
    const float sqrt_d = sqrtf((float)D);
    // two positions per group and trip: four 16-byte loads per lane in flight; the loop is wave-uniform (positions past the slice
    // are clamped to its last one and their update is skipped)
    for (uint32_t base = p0; base < p1; base += 2 * NG) {
        f32x4 k4[2], v4[2];
        bool valid[2];
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const uint32_t pos = base + t * NG + grp;
            valid[t] = pos < p1;
            const uint64_t idx = (uint64_t)min(pos, p1 - 1) * p.pos_stride + hbase;
            k4[t] = ba_load4<F16>(kc, idx);
            v4[t] = ba_load4<F16>(vc, idx);
        }
#pragma unroll
        for (int t = 0; t < 2; t++) {
#pragma unroll
            for (int g = 0; g < G; g++) {
                float d = qf[g][0] * k4[t][0];
                d = fmaf(qf[g][1], k4[t][1], d);
                d = fmaf(qf[g][2], k4[t][2], d);
                d = fmaf(qf[g][3], k4[t][3], d);
                const float s = ba_pos_sum<LPP>(d) / sqrt_d;   // AttentionScoreCalculationShader.cs:164-206
                if (valid[t]) {
                    const float mn = fmaxf(m[g], s);
                    const float c = expf(m[g] - mn), e = expf(s - mn);   // exp(-inf) = 0 on the first position
                    l[g] = l[g] * c + e;
                    o[g][0] = o[g][0] * c + e * v4[t][0];
                    o[g][1] = o[g][1] * c + e * v4[t][1];
                    o[g][2] = o[g][2] * c + e * v4[t][2];
                    o[g][3] = o[g][3] * c + e * v4[t][3];
                    m[g] = mn;
                }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; g++) {
        float *pp = part + (size_t)(grp * G + g) * PW;
        *reinterpret_cast<f32x2 *>(pp + li * 4) = f32x2{o[g][0], o[g][1]};
        *reinterpret_cast<f32x2 *>(pp + li * 4 + 2) = f32x2{o[g][2], o[g][3]};
        if (li == 0) { pp[D] = m[g]; pp[D + 1] = l[g]; }
    }
    __syncthreads();
    // the groups of the workgroup, in group order (a group that saw no position has m = -inf, l = 0: weight exp(-inf) = 0)
    float *gp = p.partials + ((size_t)(b * p.Hkv + kvh) * BA_NSPLIT) * G * PW;
    for (uint32_t e = threadIdx.x; e < (uint32_t)(G * D); e += blockDim.x) {
        const uint32_t g = e / D, d = e % D;
        float M = -INFINITY;
        for (int i = 0; i < NG; i++) M = fmaxf(M, part[(size_t)(i * G + g) * PW + D]);
        float L = 0.f, O = 0.f;
        for (int i = 0; i < NG; i++) {
            const float *pp = part + (size_t)(i * G + g) * PW;
            const float w = expf(pp[D] - M);
            L += pp[D + 1] * w;
            O += pp[d] * w;
        }
        if (nsplit == 1) {
            p.o[b][(size_t)(kvh * G + g) * D + d] = O / L;   // AttentionSoftmaxShader.cs:139-178 + …ValueSumShader.cs:175-216
        } else {
            float *ps = gp + ((size_t)split * G + g) * PW;
            __hip_atomic_store(ps + d, O, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (d == 0) {
                __hip_atomic_store(ps + D, M, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(ps + D + 1, L, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (nsplit == 1) return;
    // ticket hand-off: partials written through, every thread drains its stores, the workgroup meets, ONE lane takes a ticket; the
    // workgroup whose ticket is last merges the slices in slice order
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t tk = __hip_atomic_fetch_add(&p.tickets[b * p.Hkv + kvh], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = tk == nsplit - 1 ? 1u : 0u;
        if (tk == nsplit - 1) __hip_atomic_store(&p.tickets[b * p.Hkv + kvh], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm
    }
    __syncthreads();
    if (s_last == 0u) return;
    // (max, sum of exp) of every slice first, one pair per thread, so that the slices' weights are known before the outputs are
    // walked: the merge costs a few memory round trips, not one per slice.  `part` is free again (barriers above).
    float *s_m = part, *s_l = part + 256, *s_w = part + 512, *s_L = part + 768;
    if (threadIdx.x < nsplit * G) {
        const float *ps = gp + (size_t)threadIdx.x * PW;   // [slice][g]
        s_m[threadIdx.x] = __hip_atomic_load(ps + D, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_l[threadIdx.x] = __hip_atomic_load(ps + D + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)G) {
        const uint32_t g = threadIdx.x;
        float M = -INFINITY;
        for (uint32_t i = 0; i < nsplit; i++) M = fmaxf(M, s_m[i * G + g]);
        float L = 0.f;
        for (uint32_t i = 0; i < nsplit; i++) {
            const float w = expf(s_m[i * G + g] - M);
            s_w[i * G + g] = w;
            L += s_l[i * G + g] * w;
        }
        s_L[g] = L;
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < (uint32_t)(G * D); e += blockDim.x) {
        const uint32_t g = e / D, d = e % D;
        float O = 0.f;
        for (uint32_t i0 = 0; i0 < nsplit; i0 += 8) {   // eight loads in flight; slices in order
            float ov[8];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const uint32_t i = min(i0 + j, nsplit - 1);
                ov[j] = __hip_atomic_load(gp + ((size_t)i * G + g) * PW + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (i0 + j < nsplit) O += ov[j] * s_w[(i0 + j) * G + g];
        }
        p.o[b][(size_t)(kvh * G + g) * D + d] = O / s_L[g];
    }
}

size_t batch_attn_bytes(uint32_t H, uint32_t D) { return 4096 + (size_t)BATCH_MAX * BA_NSPLIT * H * (D + 2) * 4; }

template <int LPP, bool F16>
static hipError_t launch_ba(const BAttnParams &p, uint32_t G, dim3 grid, hipStream_t s)
{
    switch (G) {
        case 1: hipLaunchKernelGGL((k_battn<LPP, 1, F16>), grid, dim3(256), 0, s, p); break;
        case 2: hipLaunchKernelGGL((k_battn<LPP, 2, F16>), grid, dim3(256), 0, s, p); break;
        case 3: hipLaunchKernelGGL((k_battn<LPP, 3, F16>), grid, dim3(256), 0, s, p); break;
        case 4: hipLaunchKernelGGL((k_battn<LPP, 4, F16>), grid, dim3(256), 0, s, p); break;
        case 8: hipLaunchKernelGGL((k_battn<LPP, 8, F16>), grid, dim3(256), 0, s, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_batch_attn(const BatchAttnArgs &a, hipStream_t s)
{
    if (a.n < 1 || a.n > BATCH_MAX || a.Hkv == 0 || a.H % a.Hkv || !attn_group_ok(a.H / a.Hkv) || (a.D != 64 && a.D != 128) || !a.work ||
        a.n * a.Hkv > 1024)
        return hipErrorInvalidValue;
    BAttnParams p{};
    for (uint32_t b = 0; b < a.n; b++) {
        if (!a.q[b] || !a.o[b] || !a.kc[b] || !a.vc[b] || !a.pos[b] || a.cap[b] == 0) return hipErrorInvalidValue;
        p.q[b] = a.q[b]; p.o[b] = a.o[b]; p.kc[b] = a.kc[b]; p.vc[b] = a.vc[b];
        p.head_stride[b] = a.kv_head_stride[b]; p.cap[b] = a.cap[b]; p.pos[b] = a.pos[b];
    }
    p.pos_stride = a.kv_pos_stride; p.Hkv = a.Hkv;
    p.tickets = static_cast<uint32_t *>(a.work);                                       // [n][Hkv] <= 1024 words
    p.partials = reinterpret_cast<float *>(static_cast<char *>(a.work) + 4096);
    const dim3 grid(BA_NSPLIT, a.Hkv, a.n);
    const uint32_t G = a.H / a.Hkv;
    const bool f16 = a.kv_type == NFAI_F16;
    if (a.D == 64) return f16 ? launch_ba<16, true>(p, G, grid, s) : launch_ba<16, false>(p, G, grid, s);
    return f16 ? launch_ba<32, true>(p, G, grid, s) : launch_ba<32, false>(p, G, grid, s);
}

}  // namespace nfai
