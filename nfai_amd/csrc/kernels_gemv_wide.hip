// kernels_gemv_wide.hip — the decode step for up to 16 sequences at once on the matrix cores: every fp16 weight row is read from HBM
// ONCE, as the A operand of v_mfma_f32_16x16x32_f16, and applied to the activation vectors of 16 sequences, the B operand's columns
// (MatrixMultiplyShader.cs:255-289 at M = B, with the prologues / epilogues of TransformerBlock.Compute, TransformerBlock.cs:127-184,
// that kernels_gemv_batch.hip fuses at B <= 8).  A separate family: k_bgemv and the batch-1 kernels are not touched.
//
// k_wgemv<MODE, NORM>, always 16 columns
//   Bound: HBM (the weights).  No conversion and no FMA per weight: two MFMAs per KiB of weights, a tenth of what the SIMDs issue.
//   weights   HBM -> VGPR, 16-byte non-temporal loads, each row read once, never through LDS.  A wave step is 16 rows x 128 k, four
//             MFMA A operands per lane: load m of lane l is k = 128 s + 32 m + 8 (l >> 4) .. + 7 of row l & 15, the MFMA's own k
//             order, so that one load instruction takes 64 contiguous bytes of each of the 16 rows and two of them a whole 128-byte
//             line.  (A lane holding ONE 64-byte run, with the k slots permuted to match, makes every instruction touch every
//             line of the step: the lm_head at 3B took 265 us that way, 187 this way.)  Two steps are in flight per wave; the first two are requested before the prologue.
//   x         fp32 in memory, fp32-class in the product: x = hi + 2^-11 lo with hi = half(x), lo = half((x - hi) * 2^11), staged
//             in LDS as two fp16 planes [k / 8][column][8] (a lane's B operand is one ds_read_b128; 16 lanes read 256 contiguous
//             bytes), two MFMAs into two fp32 accumulators, combined as acc_hi + 2^-11 acc_lo.  |x| >= 65504 overflows hi.
//   capacity  16 columns x 2 planes are 64 bytes per k: x is staged in panels of 2048 k (128 KiB); a wave carries its accumulators
//             across the panels.  RMSNorm's sum runs over the whole row before the first panel is staged.
//   split K   a workgroup is 16 waves; KS of them (1, 2, 4, 8 or 16, a function of the matrix shape alone) share a 16-row tile, each
//             taking a contiguous run of every panel's steps, and their partial sums meet in LDS, in slice order.  KS is the largest
//             power of two with tiles x KS <= 4096 and KS <= the steps of a panel: Wo at 3B has 192 row tiles for 1024 SIMDs, KS = 16.
//             Nothing is handed between workgroups.
//   order     a (row, column) sum is a function of K and of the matrix shape only: panel p, slice s covers the steps
//             [16 p + s n_p / KS, 16 p + (s + 1) n_p / KS) (n_p = steps of the panel); slice s chains them, panels ascending, through
//             the MFMA's accumulator; the total is ((slice 0 + slice 1) + ...).  The grid, the column's index and its neighbours do
//             not enter: a column's result is the same bit for bit wherever it sits and whatever the other columns hold.
//   columns   >= n are dead: they read column 0's x and store nothing.
#include <stdlib.h>

#include <algorithm>

#include "common.h"

namespace nfai {

#define GLOBAL_AS __attribute__((address_space(1)))

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr uint32_t WG_PANEL = 2048;               // k per staged x panel (64 bytes of LDS per k)
constexpr uint32_t WG_STEP = 128;                 // k per wave step
constexpr uint32_t WG_SPP = WG_PANEL / WG_STEP;   // steps per panel
constexpr uint32_t WG_WAVES = 16;                 // waves per workgroup
constexpr uint32_t WG_CS = 128;                   // cos / sin words per column (head_dim <= 128)
constexpr uint32_t WG_MAX_GRID = 1024;            // argmax partials per column
constexpr uint32_t WG_ITEMS = 4096;               // (row tile, slice) pairs a launch is cut into at most by the K split: 256 workgroups of 16

struct WGemvParams {
    const uint8_t *W[3];
    uint32_t seg_end[3];
    uint64_t row_bytes;
    uint32_t K, KT, steps, rows, NT, ks, n;
    const float *gamma;
    float eps;
    const float *x[WIDE_MAX];
    float *y[WIDE_MAX];
    const float *res[WIDE_MAX];
    void *kc[WIDE_MAX], *vc[WIDE_MAX];
    uint64_t head_stride[WIDE_MAX];
    uint32_t cap[WIDE_MAX];
    const uint32_t *pos[WIDE_MAX];
    uint64_t pos_stride;
    int kv_f16;
    const float *freqs;
    uint32_t rope_dims, D;
    uint32_t *err;
    // lm_head: per-column ArgMax
    float *part_v;       // [WIDE_MAX][WG_MAX_GRID]
    uint32_t *part_i;
    uint32_t *ticket;
    uint32_t *tok_batch;
    uint32_t *tok[WIDE_MAX], *pos_inc[WIDE_MAX], *ring[WIDE_MAX];
    uint32_t ring_len;
};

// A-row `ar` of row tile `tile`: plain / residual / q|k|v: row 16 tile + ar of the (concatenated) matrix; gate|up: rows 8 tile + ar / 2
// of gate (ar even) and up (ar odd), so that a lane's four accumulator rows are two whole (gate, up) pairs.  Clamped to a valid row:
// the loads are unconditional.
template <int MODE>
__device__ __forceinline__ const uint8_t *wg_row_ptr(const WGemvParams &p, uint32_t tile, uint32_t ar)
{
    if constexpr (MODE == GEMV_GATEUP) {
        const uint32_t unit = min(tile * 8 + (ar >> 1), p.rows / 2 - 1);
        return p.W[ar & 1] + (uint64_t)unit * p.row_bytes;
    } else if constexpr (MODE == GEMV_QKV_ROPE) {
        const uint32_t row = min(tile * 16 + ar, p.rows - 1);
        if (row < p.seg_end[0]) return p.W[0] + (uint64_t)row * p.row_bytes;
        if (row < p.seg_end[1]) return p.W[1] + (uint64_t)(row - p.seg_end[0]) * p.row_bytes;
        return p.W[2] + (uint64_t)(row - p.seg_end[1]) * p.row_bytes;
    } else {
        return p.W[0] + (uint64_t)min(tile * 16 + ar, p.rows - 1) * p.row_bytes;
    }
}

template <int MODE, bool NORM>
__global__ __launch_bounds__(WG_WAVES * 64) void k_wgemv(const WGemvParams p)
{
    // [KT / 8][16][8] hi | the same lo | [16 waves][64] partial sums | [16][WG_CS] cos, sin | [16] rms | [16] position, [16] in range |
    // the ArgMax's [16 waves][16] values, indices, one flag
    extern __shared__ __attribute__((aligned(16))) uint8_t wg_lds[];
    _Float16 *xh = reinterpret_cast<_Float16 *>(wg_lds);
    _Float16 *xl = xh + (size_t)p.KT * 16;
    f32x4 *red = reinterpret_cast<f32x4 *>(xl + (size_t)p.KT * 16);
    float *cs = reinterpret_cast<float *>(red + WG_WAVES * 64);
    float *rmsv = cs + 16 * WG_CS;
    uint32_t *posl = reinterpret_cast<uint32_t *>(rmsv + 16);
    uint32_t *am_lds = posl + 32;

    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t ks = p.ks, tpg = WG_WAVES / ks;          // waves per row tile | row tiles per workgroup pass
    const uint32_t myt = wid / ks, sl = wid % ks;
    const uint32_t ngroups = (p.NT + tpg - 1) / tpg;
    const uint32_t npanels = (p.steps + WG_SPP - 1) / WG_SPP;
    const uint32_t ar = lane & 15, ag = lane >> 4;          // A: row of the tile, k group | B and D: column, row group

    // ---- weight stream: two register buffers of one step each; the refills inside the loop are unconditional (the last one to three
    //      steps of a slice are peeled), so that a step's wait leaves the next step's four loads in flight ---------------------------
    u32x4 wa[4], wb[4];
    const uint8_t *wrow = wg_row_ptr<MODE>(p, min(blockIdx.x * tpg + myt, p.NT - 1), ar);
    auto issue = [&](u32x4 (&buf)[4], uint32_t st) {
#pragma unroll
        for (int m = 0; m < 4; m++) {
            // past the end of the row (or of the slice) the address is clamped into the row: x is zero there, or the step is not used
            const uint32_t k = min(st * WG_STEP + m * 32 + ag * 8, p.K - 8);
            buf[m] = load_nt16(wrow + (uint64_t)k * 2);
        }
    };
    // the wave's steps [s0, s1) of panel `panel`
    auto slice = [&](uint32_t panel, uint32_t &s0, uint32_t &s1) {
        const uint32_t st0 = panel * WG_SPP, spn = min(WG_SPP, p.steps - st0);
        s0 = st0 + sl * spn / ks;
        s1 = st0 + (sl + 1) * spn / ks;
    };
    {   // the first two steps of the first row tile do not depend on x: in flight during the whole prologue
        uint32_t s0, s1;
        slice(0, s0, s1);
        issue(wa, s0);
        issue(wb, s0 + (s1 - s0 > 1 ? 1 : 0));   // (a slice of one step: the same lines again)
    }

    if constexpr (MODE == GEMV_QKV_ROPE) {
        // positions: a column whose position word is not below its capacity stores no K / V row and raises the error word
        if (threadIdx.x < 16) {
            const uint32_t pv = p.pos[threadIdx.x][0];
            posl[threadIdx.x] = pv;
            posl[16 + threadIdx.x] = pv < p.cap[threadIdx.x] ? 1u : 0u;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0)
            for (uint32_t c = 0; c < p.n; c++)
                if (!(p.pos[c][0] < p.cap[c])) p.err[0] = 0x10000u | c;
        __syncthreads();
        // cos / sin of every column's position, tabulated once per workgroup (read by its epilogues behind the staging barriers)
        const uint32_t n_freq = p.rope_dims / 2;
        const uint32_t pair = lane;
        if (pair < n_freq) {
            const f32x2 v = rope_cs_of(p.freqs, pair, posl[wid]);
            cs[wid * WG_CS + 2 * pair] = v[0];
            cs[wid * WG_CS + 2 * pair + 1] = v[1];
        }
    }
    if constexpr (NORM) {
        // RMSNormShader.cs:136-149 per column, over the whole row whatever the panels are: wave c sums column c
        const GLOBAL_AS float *xc = (const GLOBAL_AS float *)p.x[wid];
        float ss = 0.f;
        for (uint32_t i = lane * 4; i < p.K; i += 256) {
            const f32x4 v = *reinterpret_cast<const GLOBAL_AS f32x4 *>(xc + i);
            ss = fmaf(v[0], v[0], ss);
            ss = fmaf(v[1], v[1], ss);
            ss = fmaf(v[2], v[2], ss);
            ss = fmaf(v[3], v[3], ss);
        }
        ss = wave_sum(ss);
        if (lane == 0) rmsv[wid] = sqrtf(ss / (float)p.K + p.eps);
    }
    __syncthreads();

    float best_v = -INFINITY;
    uint32_t best_i = 0xFFFFFFFFu;
    const uint32_t col = lane & 15, r0 = (lane >> 4) * 4;   // D: column, first of the lane's four rows of the tile
    const bool live = col < p.n;

    for (uint32_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const uint32_t tile = grp * tpg + myt;               // past the last tile: a clamped row is streamed and nothing stored
        if (grp != blockIdx.x) wrow = wg_row_ptr<MODE>(p, min(tile, p.NT - 1), ar);
        f32x4 ah = f32x4{0.f, 0.f, 0.f, 0.f}, al = f32x4{0.f, 0.f, 0.f, 0.f};
        for (uint32_t panel = 0; panel < npanels; panel++) {
            const uint32_t st0 = panel * WG_SPP, spn = min(WG_SPP, p.steps - st0);
            uint32_t s0, s1;
            slice(panel, s0, s1);
            auto consume = [&](u32x4 (&buf)[4], uint32_t st) {
                const uint32_t kg = (st - st0) * (WG_STEP / 8) + ag;
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    const size_t off = ((size_t)(kg + m * 4) * 16 + col) * 8;
                    const f16x8 bh = *reinterpret_cast<const f16x8 *>(xh + off);
                    const f16x8 bl = *reinterpret_cast<const f16x8 *>(xl + off);
                    const f16x8 a = __builtin_bit_cast(f16x8, buf[m]);
                    ah = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bh, ah, 0, 0, 0);
                    al = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bl, al, 0, 0, 0);
                }
            };
            if (panel > 0 || grp != blockIdx.x) {             // in flight while the workgroup stages the panel
                issue(wa, s0);
                issue(wb, s0 + (s1 - s0 > 1 ? 1 : 0));
            }
            if (npanels > 1 || grp == blockIdx.x) {           // one panel: staged once per launch
                if (panel > 0 || grp != blockIdx.x) __syncthreads();   // every wave is done with the previous panel
                const uint32_t k0 = panel * WG_PANEL;
                for (uint32_t idx = threadIdx.x; idx < spn * (WG_STEP / 8) * 16; idx += blockDim.x) {
                    const uint32_t c = idx & 15, k = k0 + (idx >> 4) * 8;
                    f32x4 v0 = f32x4{0.f, 0.f, 0.f, 0.f}, v1 = v0;
                    if (k < p.K) {
                        const GLOBAL_AS float *xc = (const GLOBAL_AS float *)p.x[c] + k;
                        v0 = *reinterpret_cast<const GLOBAL_AS f32x4 *>(xc);
                        v1 = *reinterpret_cast<const GLOBAL_AS f32x4 *>(xc + 4);
                        if constexpr (NORM) {
                            const f32x4 g0 = *reinterpret_cast<const GLOBAL_AS f32x4 *>((const GLOBAL_AS float *)p.gamma + k);
                            const f32x4 g1 = *reinterpret_cast<const GLOBAL_AS f32x4 *>((const GLOBAL_AS float *)p.gamma + k + 4);
                            const float r = rmsv[c];
#pragma unroll
                            for (int e = 0; e < 4; e++) {
                                v0[e] = (v0[e] / r) * g0[e];
                                v1[e] = (v1[e] / r) * g1[e];
                            }
                        }
                    }
                    f16x8 hi, lo;
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        hi[e] = (_Float16)v0[e];
                        hi[4 + e] = (_Float16)v1[e];
                        lo[e] = (_Float16)((v0[e] - (float)hi[e]) * 2048.f);
                        lo[4 + e] = (_Float16)((v1[e] - (float)hi[4 + e]) * 2048.f);
                    }
                    *reinterpret_cast<f16x8 *>(xh + (size_t)idx * 8) = hi;
                    *reinterpret_cast<f16x8 *>(xl + (size_t)idx * 8) = lo;
                }
                __syncthreads();
            }
            uint32_t st = s0;
            for (; st + 3 < s1; st += 2) {
                consume(wa, st);
                issue(wa, st + 2);
                consume(wb, st + 1);
                issue(wb, st + 3);
            }
            const uint32_t rem = s1 - st;
            if (rem == 3) {
                consume(wa, st);
                issue(wa, st + 2);
                consume(wb, st + 1);
                consume(wa, st + 2);
            } else if (rem == 2) {
                consume(wa, st);
                consume(wb, st + 1);
            } else if (rem == 1) {
                consume(wa, st);
            }
        }
        f32x4 acc;
#pragma unroll
        for (int j = 0; j < 4; j++) acc[j] = ah[j] + al[j] * 0x1p-11f;
        if (ks > 1) {   // (uniform over the launch) the slices of a row tile meet in LDS, in slice order
            __syncthreads();   // the previous pass's sums have been read
            red[wid * 64 + lane] = acc;
            __syncthreads();
            if (sl == 0)
                for (uint32_t s = 1; s < ks; s++) {
                    const f32x4 o = red[(wid + s) * 64 + lane];
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[j] = acc[j] + o[j];
                }
        }
        if (sl != 0 || tile >= p.NT || !live) continue;
        // ---- epilogue of the lane's column: rows r0 .. r0 + 3 of the tile (the epilogues of kernels_gemv.hip, per column) ----------
        if constexpr (MODE == GEMV_PLAIN || MODE == GEMV_RESIDUAL) {
            const uint32_t row = tile * 16 + r0;
            float *y = p.y[col] + row;
            if constexpr (MODE == GEMV_RESIDUAL) {   // TransformerBlock.cs:153-158 / 176-180: input + projection
                const float *res = p.res[col] + row;
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (row + j < p.rows) acc[j] = res[j] + acc[j];
            }
            if (row + 3 < p.rows && (p.rows & 3u) == 0) {
                *reinterpret_cast<f32x4 *>(y) = acc;
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (row + j < p.rows) y[j] = acc[j];
            }
            if constexpr (MODE == GEMV_PLAIN) {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (row + j < p.rows && topk_better(acc[j], row + j, best_v, best_i)) { best_v = acc[j]; best_i = row + j; }
            }
        } else if constexpr (MODE == GEMV_GATEUP) {
            const uint32_t unit = tile * 8 + r0 / 2, nu = p.rows / 2;
            float *y = p.y[col];
            if (unit < nu) y[unit] = acc[1] * silu_ref(acc[0]);           // SiLUShader.cs:121-123, ElementWiseMultiplicationShader.cs:137
            if (unit + 1 < nu) y[unit + 1] = acc[3] * silu_ref(acc[2]);
        } else {
            // RoPEShader.cs:249-262 on the pairs (row, row + 1) at THIS column's position; V rows are stored unrotated
            const float *ccs = cs + col * WG_CS;
            const uint32_t cpos = posl[col];
            const bool pos_ok = posl[16 + col] != 0u;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const uint32_t row = tile * 16 + r0 + 2 * h;
                if (row >= p.rows) continue;
                const uint32_t seg = row < p.seg_end[0] ? 0u : (row < p.seg_end[1] ? 1u : 2u);
                const uint32_t r = seg == 0 ? row : (seg == 1 ? row - p.seg_end[0] : row - p.seg_end[1]);
                const uint32_t head = r / p.D, d = r % p.D;
                const float a0 = acc[2 * h], a1 = acc[2 * h + 1];
                float o0 = a0, o1 = a1;
                if (seg < 2 && d < p.rope_dims) {
                    const float cc = ccs[d], ss = ccs[d + 1];
                    o0 = cc * a0 - ss * a1;
                    o1 = ss * a0 + cc * a1;
                }
                if (seg == 0) {
                    float *y = p.y[col];
                    y[row] = o0;
                    y[row + 1] = o1;
                } else if (pos_ok) {   // a position word at or past the capacity writes nothing (the launch reports it through p.err)
                    const uint64_t idx = (uint64_t)cpos * p.pos_stride + (uint64_t)head * p.head_stride[col] + d;
                    void *base = seg == 1 ? p.kc[col] : p.vc[col];
                    kv_store(base, p.kv_f16, idx, o0);
                    kv_store(base, p.kv_f16, idx + 1, o1);
                }
            }
        }
    }

    if constexpr (MODE == GEMV_PLAIN) {
        // SamplingUtils.ArgMax per column in the same launch (SamplingUtils.cs:55-56: the LOWEST index among equal maxima), then the
        // end-of-token bookkeeping of every member.  A column's rows sit in the lanes col, col + 16, col + 32, col + 48 of a wave.
        float *sv = reinterpret_cast<float *>(am_lds);        // [16 waves][16]
        uint32_t *si = am_lds + WG_WAVES * 16, *last = am_lds + 2 * WG_WAVES * 16;
#pragma unroll
        for (int m = 16; m <= 32; m *= 2) {
            const float ov = __shfl_xor(best_v, m);
            const uint32_t oi = __shfl_xor(best_i, m);
            if (topk_better(ov, oi, best_v, best_i)) { best_v = ov; best_i = oi; }
        }
        if (lane < 16) { sv[wid * 16 + lane] = best_v; si[wid * 16 + lane] = best_i; }
        __syncthreads();
        if (threadIdx.x < 16) {
            const uint32_t c = threadIdx.x;
            float v = sv[c];
            uint32_t i = si[c];
            for (uint32_t w = 1; w < WG_WAVES; w++)
                if (topk_better(sv[w * 16 + c], si[w * 16 + c], v, i)) { v = sv[w * 16 + c]; i = si[w * 16 + c]; }
            __hip_atomic_store(&p.part_v[c * WG_MAX_GRID + blockIdx.x], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&p.part_i[c * WG_MAX_GRID + blockIdx.x], i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t tk = __hip_atomic_fetch_add(p.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            last[0] = (tk == gridDim.x - 1) ? 1u : 0u;
        }
        __syncthreads();
        if (last[0] == 0u) return;
        // the workgroup whose ticket is last: (value desc, index asc) is a total order, so the result does not depend on which it is.
        // Wave c combines column c.
        {
            const uint32_t c = wid;
            float v = -INFINITY;
            uint32_t i = 0xFFFFFFFFu;
            for (uint32_t g = lane; g < gridDim.x; g += 64) {
                const float ov = __hip_atomic_load(&p.part_v[c * WG_MAX_GRID + g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t oi = __hip_atomic_load(&p.part_i[c * WG_MAX_GRID + g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (topk_better(ov, oi, v, i)) { v = ov; i = oi; }
            }
            wave_best(v, i);
            if (lane == 0 && c < p.n) {
                p.tok_batch[c] = i;
                p.tok[c][0] = i;
                const uint32_t pp = p.pos_inc[c][0];
                p.ring[c][pp % p.ring_len] = i;
                p.pos_inc[c][0] = pp + 1;
            }
        }
        if (threadIdx.x == 0) __hip_atomic_store(p.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm (stream-ordered with the next launch)
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
struct WGemvPlan { bool ok; uint32_t KT, steps, rows, NT, ks, grid; size_t lds; };

static WGemvPlan plan_wgemv(const WideGemvArgs &a)
{
    WGemvPlan pl{};
    if (a.n < 1 || a.n > WIDE_MAX || a.K < 8 || a.K % 8 || a.n_cu == 0) return pl;
    const uint32_t rows = a.seg_rows[0] + a.seg_rows[1] + a.seg_rows[2];
    if (a.mode == GEMV_QKV_ROPE) {
        if (a.seg_rows[0] % 2 || a.seg_rows[1] % 2 || a.seg_rows[2] % 2 || (a.D != 64 && a.D != 128) || a.rope_dims > a.D || a.rope_dims % 2) return pl;
    } else if (a.mode == GEMV_GATEUP) {
        if (a.seg_rows[0] != a.seg_rows[1] || a.seg_rows[2]) return pl;
    } else if (a.seg_rows[1] || a.seg_rows[2]) {
        return pl;
    }
    if (rows == 0) return pl;
    const bool norm = a.gamma != nullptr;
    if (norm != (a.mode != GEMV_RESIDUAL)) return pl;   // the instantiated forms
    pl.rows = rows;
    pl.NT = (rows + 15) / 16;
    pl.steps = (a.K + WG_STEP - 1) / WG_STEP;
    pl.KT = std::min(pl.steps, WG_SPP) * WG_STEP;
    // K split among the waves of one workgroup: a function of the matrix shape alone (the grid does not enter the summation order)
    pl.ks = 1;
    while (pl.ks < WG_WAVES && pl.NT * pl.ks * 2 <= WG_ITEMS && pl.ks * 2 <= std::min(pl.steps, WG_SPP)) pl.ks *= 2;
    const uint32_t tpg = WG_WAVES / pl.ks, ngroups = (pl.NT + tpg - 1) / tpg;
    pl.grid = std::min(a.n_cu, ngroups);
    if (a.mode == GEMV_PLAIN && pl.grid > WG_MAX_GRID) return pl;
    pl.lds = (size_t)pl.KT * 16 * 2 * 2 + (size_t)WG_WAVES * 64 * 16 + (16 * WG_CS + 16 + 32 + 2 * WG_WAVES * 16 + 4) * 4;
    pl.ok = pl.lds <= 160 * 1024;
    return pl;
}

bool wide_gemv_ok(const WideGemvArgs &a) { return plan_wgemv(a).ok; }

template <int MODE, bool NORM>
static hipError_t launch_wg(const WGemvParams &p, const WGemvPlan &pl, hipStream_t s)
{
    static bool raised = false;   // the kernel's dynamic-LDS limit is raised once (gfx950: 160 KB per CU)
    if (pl.lds > 64 * 1024 && !raised) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_wgemv<MODE, NORM>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        raised = true;
    }
    hipLaunchKernelGGL((k_wgemv<MODE, NORM>), dim3(pl.grid), dim3(WG_WAVES * 64), pl.lds, s, p);
    return hipGetLastError();
}

hipError_t launch_wide_gemv(const WideGemvArgs &a, hipStream_t s)
{
    const WGemvPlan pl = plan_wgemv(a);
    if (!pl.ok) return hipErrorInvalidValue;
    WGemvParams p{};
    uint32_t end = 0;
    for (int i = 0; i < 3; i++) {
        p.W[i] = static_cast<const uint8_t *>(a.W[i] ? a.W[i] : a.W[0]);
        end += a.seg_rows[i];
        p.seg_end[i] = end;
    }
    if (!p.W[0]) return hipErrorInvalidValue;
    p.row_bytes = (uint64_t)a.K * 2;
    p.K = a.K; p.KT = pl.KT; p.steps = pl.steps; p.rows = pl.rows; p.NT = pl.NT; p.ks = pl.ks; p.n = a.n;
    p.gamma = a.gamma; p.eps = a.eps;
    for (uint32_t b = 0; b < WIDE_MAX; b++) {
        const uint32_t c = b < a.n ? b : 0;   // dead columns read column 0's input (and store nothing)
        p.x[b] = a.x[c]; p.y[b] = a.y[c]; p.res[b] = a.res[c];
        p.kc[b] = a.kc[c]; p.vc[b] = a.vc[c]; p.head_stride[b] = a.kv_head_stride[c]; p.cap[b] = a.cap[c]; p.pos[b] = a.pos[c];
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
        p.part_i = reinterpret_cast<uint32_t *>(p.part_v + WIDE_MAX * WG_MAX_GRID);
        p.ticket = p.part_i + WIDE_MAX * WG_MAX_GRID;
        p.tok_batch = a.am_tok_batch; p.ring_len = a.am_ring_len;
    }
    switch (a.mode) {
        case GEMV_PLAIN: return launch_wg<GEMV_PLAIN, true>(p, pl, s);
        case GEMV_RESIDUAL: return launch_wg<GEMV_RESIDUAL, false>(p, pl, s);
        case GEMV_QKV_ROPE: return launch_wg<GEMV_QKV_ROPE, true>(p, pl, s);
        case GEMV_GATEUP: return launch_wg<GEMV_GATEUP, true>(p, pl, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace nfai
