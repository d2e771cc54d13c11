// kernels_gemv_batch_kqm.hip — the batched decode step (kernels_gemv_batch.hip) on IQ4_XS / Q3_K / Q4_0 / Q4_K / Q5_K / Q6_K / Q8_0 weights in the T16 layout: every
// quantised weight row is read from HBM ONCE, unpacked ONCE and multiplied on the matrix cores with the fixed-point activations of up to
// 8 sequences (MatrixMultiplyShader.cs:255-289 at M = B on weights the reference cannot load, Parser.cs:111-114; the prologues and
// epilogues of TransformerBlock.Compute, TransformerBlock.cs:127-184, per column as in k_bgemv).  A separate family: k_gemv_kqt and
// k_bgemv are not touched; numerics and MFMA operand roles are those of kernels_gemv_kqm.hip, and the step loads, the unpack and the dot
// products are the shared ones of kqm.h (layout: t16.h).
//
// k_bgemv_kq<QT, B, MODE, NORM, BPW>
//   split     a workgroup owns 16-row tiles ("units": one tile, or the gate and the up tile of the same rows), its waves split K.  A K
//             tile has NBT <= 16 super-blocks ("slots"); wave w owns slots w * BPW .. + BPW - 1 (BPW = 2 when NBT > 8: at most 8 waves, so
//             that a wave may use 256 VGPRs) and stages exactly those super-blocks of every column (kqm_stage: 2^S, three base-256
//             digits as A fragments, scale-group sums): nothing staged is read by another wave, and a K tile needs no barrier.
//   step      one super-block of one 16-row tile: 1760 B (Q3_K) / 2176 B (IQ4_XS) / 2304 B (Q4_K, Q4_0) / 2816 B (Q5_K) / 3360 B (Q6_K) / 4352 B (Q8_0) per wave, two steps
//             (B = 8; Q5_K, Q6_K and Q8_0 at B = 4) or four in flight.  The loads, the nibble / fifth-bit / 6-bit unpack and the
//             header decode (get_scale_min_k4, the int8 scales, the fp16 d of Q8_0 / Q4_0, the codebook lookup and the 6-bit scales of IQ4_XS) happen once (kqm_unpack); then per column,
//             in branch-free groups of up to four: four A fragments + the sums + S from LDS, four v_mfma_i32_16x16x64_i8 against the unpacked B
//             operand held in registers, the fp32 scale epilogue, ldexpf by the column's exponent, one add into the column's sum.
//   LDS       1 KiB of fragments + 64 B of sums + 4 B of S per super-block and column.  A K tile is at most 16 super-blocks (4096
//             elements): 8 columns x 16 x 1092 B = 136.5 KiB, beside 1 KiB of zeros (the A rows of the lanes that carry no digit) and
//             a reduction buffer that holds only the 16 finished rows of every (slot, column): 16 KiB at B = 8 with gate|up.  The
//             tiling is a function of K ALONE (never of B), tiles are even (K = 8192: 2 x 16, K = 14336: 4 x 14 super-blocks).  A
//             tiled launch (Wdown) gives every workgroup ONE unit and carries the B sums of a slot across the tiles in registers; the
//             next tile's x is requested while the current one is multiplied.
//   mixed     a q|k|v whose segments differ in type is split by type into up to three launches (llama_batch.hip), so a launch stages
//             one fragment layout only: Q4_K's (Q5_K stages as Q4_K: same sub-blocks, scales and mins; Q4_0 stages as Q4_K too: its
//             32-blocks are the sub-blocks, d the scale and 8 d the min, t16.h; IQ4_XS likewise: its operand bytes are the table values of its codes,
//             d * (ls - 32) the scale and the min 0, kqm.h), Q6_K's (Q3_K stages as Q6_K: same 16-weight groups,
//             its bytes biased by 28 so that Q6_K's -32 leaves q - 4, kqm.h) or Q8_0's.
//   order     a (row, column) sum: lane (G, r) adds its 64-weight partials of slot s of the K tiles in tile order; the four G meet by
//             rows4_sum; the slots are added in slot order in four interleaved chains.  Slots and tiles depend on K only (not on the
//             waves that own them), the grid decides only which workgroup owns a unit: a column's result does not depend on its
//             position in the batch, on the batch size or on its neighbours, bit for bit.
//   columns   >= n are dead: nothing is staged or stored for them.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "common.h"
#include "kqm.h"

namespace nfai {

constexpr uint32_t BK_NBT = 16;          // super-blocks (slots) per K tile, at most
constexpr uint32_t BK_CS = 128;          // cos / sin words per column (head_dim <= 128)
constexpr uint32_t BK_MAX_GRID = 1024;   // argmax partials per column (the layout of batch_argmax_bytes())
constexpr uint32_t BK_BLK_LDS = 1024 + 64 + 4;

struct BKqParams {
    const uint8_t *W[3];
    uint32_t seg_tiles[3];     // 16-row tiles per segment
    uint32_t seg_tile_end[3];  // running sum (unit -> segment)
    uint32_t seg_role[3];      // q|k|v: 0 = q, 1 = k, 2 = v (a launch may hold any subset)
    uint32_t K, NB, NBT, ntiles, NU, n;   // NBT: super-blocks ("slots") per K tile
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
    float *part_v;       // [BATCH_MAX][BK_MAX_GRID]
    uint32_t *part_i;
    uint32_t *ticket;
    uint32_t *tok_batch;
    uint32_t *tok[BATCH_MAX], *pos_inc[BATCH_MAX], *ring[BATCH_MAX];
    uint32_t ring_len;
    const uint32_t *win_ctl;   // non-null: the columns are one sequence's window (win_tail, common.h)
};

template <int MODE>
__device__ __forceinline__ void bk_unit(const BKqParams &p, uint32_t u, uint32_t t, uint32_t &seg, uint32_t &tile)
{
    if constexpr (MODE == GEMV_GATEUP) {
        seg = t; tile = u;
    } else if constexpr (MODE == GEMV_QKV_ROPE) {
        if (u < p.seg_tile_end[0]) { seg = 0; tile = u; }
        else if (u < p.seg_tile_end[1]) { seg = 1; tile = u - p.seg_tile_end[0]; }
        else { seg = 2; tile = u - p.seg_tile_end[1]; }
    } else {
        seg = 0; tile = u;
    }
}

// (at most 8 waves per workgroup and, by its LDS, one workgroup per CU: two waves per SIMD, so a wave may use 256 VGPRs)
template <int QT, int B, int MODE, bool NORM, int BPW>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_bgemv_kq(const BKqParams p)
{
    constexpr bool IS6 = QT == NFAI_Q6_K_T16, IS5 = QT == NFAI_Q5_K_T16, IS8 = QT == NFAI_Q8_0_T16, IS40 = QT == NFAI_Q4_0_T16, IS3 = QT == NFAI_Q3_K_T16;
    constexpr bool ISI4 = QT == NFAI_IQ4_XS_T16;
    static_assert(IS6 || IS5 || IS8 || IS40 || IS3 || ISI4 || QT == NFAI_Q4_K_T16, "IQ4_XS, Q3_K, Q4_0, Q4_K, Q5_K, Q6_K or Q8_0 in the T16 layout");
    using Regs = typename std::conditional<IS6, Q6T, typename std::conditional<IS5, Q5T, typename std::conditional<IS8, Q8T, typename std::conditional<IS40, Q40T, typename std::conditional<IS3, Q3T, typename std::conditional<ISI4, IQ4T, Q4T>::type>::type>::type>::type>::type>::type;
    constexpr int R = MODE == GEMV_GATEUP ? 2 : 1;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t tid = threadIdx.x, lane = tid & 63, nw = blockDim.x >> 6;
    const uint32_t wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t NBT = p.NBT;
    uint8_t *xa = smem;                                                       // [B][NBT][1024]: A fragments [slot][G][digit][16 B]
    uint8_t *zero = xa + (size_t)B * NBT * 1024;                              // 1 KiB of zeros: the A rows of the lanes that carry no digit
    float *sums = reinterpret_cast<float *>(zero + 1024);                     // [B][NBT][G][4]: sums of x' per scale group
    int *sexp = reinterpret_cast<int *>(sums + B * NBT * 16);                 // [B][NBT]: S of the super-block's fixed-point scale 2^S
    float *red = reinterpret_cast<float *>(sexp + B * NBT);                   // [R][NBT][B][16]: the 16 rows of every (slot, column)
    float *scal = red + R * NBT * B * 16;                                     // [NBT][B]: every slot's share of sum(x^2)
    float *cs = scal + NBT * B;                                               // [B][BK_CS] (q|k|v only)
    uint32_t *am_lds = reinterpret_cast<uint32_t *>(cs + (MODE == GEMV_QKV_ROPE ? B * BK_CS : 0));   // 64 words of the ArgMax
    // every wave writes the whole region itself (the same zeros): its own reads are ordered behind its own writes, no barrier
    *reinterpret_cast<u32x4 *>(zero + lane * 16) = u32x4{0u, 0u, 0u, 0u};

    const uint32_t nunits = (p.NU - blockIdx.x + gridDim.x - 1) / gridDim.x;
    const uint32_t nsteps = p.ntiles * nunits * R * BPW;   // step = (K tile, unit, tile of the unit, slot of the wave); a tiled launch has one unit and R = 1

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
        // cos / sin of every column's position, tabulated once per workgroup (read by its epilogues behind the reduction barrier)
        const uint32_t n_freq = p.rope_dims / 2;
        for (uint32_t t = threadIdx.x; t < B * 64; t += blockDim.x) {
            const uint32_t b = t >> 6, pair = t & 63;
            if (pair < n_freq) {
                uint32_t pb = 0;
#pragma unroll
                for (int c = 0; c < B; c++) pb = (b == (uint32_t)c) ? posv[c] : pb;
                const f32x2 v = rope_cs_of(p.freqs, pair, pb);
                cs[b * BK_CS + 2 * pair] = v[0];
                cs[b * BK_CS + 2 * pair + 1] = v[1];
            }
        }
    }

    // (the lambdas below are forced inline: an outlined one takes the kernel arguments through a stack copy)
    // ---- slot `wid * BPW + I` of K tile `tile`, every live column: load, (gains,) fixed-point staging.  Wave-local: no barrier.
    f32x4 xv[BPW][B], gv[BPW];
    auto load_x = [&](uint32_t tile, auto IC) __attribute__((always_inline)) {
        constexpr int I = decltype(IC)::value;
        const uint32_t kk = min(tile * NBT + wid * BPW + I, p.NB - 1) * 256 + lane * 4;
#pragma unroll
        for (int b = 0; b < B; b++)
            if ((uint32_t)b < p.n) xv[I][b] = *reinterpret_cast<const GLOBAL_AS f32x4 *>((const GLOBAL_AS float *)p.x[b] + kk);
        if constexpr (NORM) gv[I] = *reinterpret_cast<const GLOBAL_AS f32x4 *>((const GLOBAL_AS float *)p.gamma + kk);
    };
    auto stage_x = [&](uint32_t tile, auto IC) __attribute__((always_inline)) {
        constexpr int I = decltype(IC)::value;
        const uint32_t slot = wid * BPW + I;
        if (slot >= NBT) return;   // (an odd tile leaves the last wave's second slot empty)
        const bool live = tile * NBT + slot < p.NB;
#pragma unroll
        for (int b = 0; b < B; b++) {
            if ((uint32_t)b < p.n) {
                f32x4 v = live ? xv[I][b] : f32x4{0.f, 0.f, 0.f, 0.f};
                if constexpr (NORM) {
                    // RMSNorm (RMSNormShader.cs:136-149) in two parts as in k_gemv_kqt: the gains here, the division by rms on the
                    // finished sums.  A normed launch has one K tile, so a slot's share of sum(x^2) is written once.
                    float ss = 0.f;
#pragma unroll
                    for (int e = 0; e < 4; e++) ss = fmaf(v[e], v[e], ss);
                    ss = wave_sum(ss);
                    if (lane == 0) scal[slot * B + b] = ss;
                    v[0] = v[0] * gv[I][0];
                    v[1] = v[1] * gv[I][1];
                    v[2] = v[2] * gv[I][2];
                    v[3] = v[3] * gv[I][3];
                }
                uint8_t *xb = xa + (size_t)b * NBT * 1024;
                float *sb = sums + b * NBT * 16;
                kqm_stage<!IS6 && !IS8 && !IS3, IS6 || IS3, IS8>(v, slot, lane, xb, xb, sb, sb, sexp + b * NBT);   // (Q5_K, Q4_0 and IQ4_XS stage as Q4_K, Q3_K as Q6_K)
            }
        }
    };

    // ---- weight stream: two register buffers, walkers over (K tile, unit, tile of the unit, slot) ----------------------------------
    uint32_t ist = 0, i_tile = 0, i_ui = 0, i_t = 0, i_i = 0;
    auto issue = [&](Regs &buf) __attribute__((always_inline)) {
        if (ist < nsteps) {
            uint32_t seg, tile;
            bk_unit<MODE>(p, blockIdx.x + i_ui * gridDim.x, i_t, seg, tile);
            const uint32_t blk = min(i_tile * NBT + wid * BPW + i_i, p.NB - 1);   // past the end of K: the row's last super-block again (its sum is dropped)
            if constexpr (IS6) buf = q6t_load_raw(p.W[seg], p.seg_tiles[seg], p.NB, tile, blk, lane);
            else if constexpr (IS5) buf = q5t_load_raw(p.W[seg], p.seg_tiles[seg], p.NB, tile, blk, lane);
            else if constexpr (IS8) buf = q8t_load_raw(p.W[seg], p.seg_tiles[seg], p.NB, tile, blk, lane);
            else if constexpr (IS40) buf = q40t_load_raw(p.W[seg], p.seg_tiles[seg], p.NB, tile, blk, lane);
            else if constexpr (IS3) buf = q3t_load_raw(p.W[seg], p.seg_tiles[seg], p.NB, tile, blk, lane);
            else if constexpr (ISI4) buf = iq4t_load_raw(p.W[seg], p.seg_tiles[seg], p.NB, tile, blk, lane);
            else buf = q4t_load_raw(p.W[seg], p.seg_tiles[seg], p.NB, tile, blk, lane);
            ++ist;
            if (++i_i == (uint32_t)BPW) { i_i = 0; if (++i_t == (uint32_t)R) { i_t = 0; if (++i_ui == nunits) { i_ui = 0; ++i_tile; } } }
        }
    };

    load_x(0, std::integral_constant<int, 0>{});   // activations first: vmcnt retires in order, the staging must not wait behind weights
    if constexpr (BPW == 2) load_x(0, std::integral_constant<int, 1>{});
    __builtin_amdgcn_sched_barrier(0);
    // steps in flight per wave (the depth changes no result): four where the registers allow (18 per Q8_0 step, 17 per Q6_K step, 14
    // per Q5_K step, 12 per Q4_K step, 10 per Q3_K or IQ4_XS step, 9 per Q4_0 step).  Q8_0 takes Q6_K's depth and column groups: what compiles without scratch, not measured
    // against deeper buffering.
    constexpr bool WIDE = IS6 || IS8;
    constexpr int NBUF = (B == 8 || ((WIDE || IS5) && B == 4)) ? 2 : 4;
    Regs buf[NBUF];
#pragma unroll
    for (int j = 0; j < NBUF; j++) issue(buf[j]);
    // K tile 0 is staged here, in one place; the later tiles of a tiled launch (never a normed one) at their first step, with the
    // next tile's x requested right behind (it arrives while the tile's weights are multiplied)
    stage_x(0, std::integral_constant<int, 0>{});
    if constexpr (BPW == 2) stage_x(0, std::integral_constant<int, 1>{});
    // (B = 8 with two slots per wave: 16 x vectors ahead do not fit beside the columns in flight; the tile's x is requested at its first step)
    constexpr bool XPREF = !(B == 8 && BPW == 2);
    if constexpr (!NORM && XPREF) {
        if (p.ntiles > 1) {
            load_x(1, std::integral_constant<int, 0>{});
            if constexpr (BPW == 2) load_x(1, std::integral_constant<int, 1>{});
        }
    }

    const uint32_t g = lane >> 4, ra = lane & 15;
    const bool a_live = (ra >> 2) == g && (ra & 3) < 3;  // A rows 4G, 4G+1, 4G+2 = digits 0, 1, 2 of lane group G
    const uint32_t a_off = g * 64 + (ra & 3) * 16;

    float acc[BPW][B];   // per slot: a tiled launch carries them across the K tiles
#pragma unroll
    for (int i = 0; i < BPW; i++)
#pragma unroll
        for (int b = 0; b < B; b++) acc[i][b] = 0.f;
    float best_v[B];
    uint32_t best_i[B];
#pragma unroll
    for (int b = 0; b < B; b++) { best_v[b] = -INFINITY; best_i[b] = 0xFFFFFFFFu; }

    // rows of unit u, column b (b compile-time): lanes 0..15 of the finishing wave hold rows 0..15 (all four lane groups compute them)
    auto finish = [&](uint32_t u) __attribute__((always_inline)) {
#pragma unroll
        for (int b = 0; b < B; b++) {
            if ((uint32_t)b < p.n && (uint32_t)b % nw == wid) {   // wave b (mod nw) finishes column b
                float rms = 1.f;
                if constexpr (NORM) {
                    float tss = 0.f;
#pragma unroll
                    for (uint32_t i = 0; i < 16; i++) {  // fixed trip count and order: the LDS reads issue back to back
                        const float s_i = scal[min(i, NBT - 1) * B + b];
                        tss += i < NBT ? s_i : 0.f;
                    }
                    rms = sqrtf(tss / (float)p.K + p.eps);
                }
                float af[R];
#pragma unroll
                for (int t2 = 0; t2 < R; t2++) {
                    const float *rp = red + ((size_t)t2 * NBT * B + b) * 16 + ra;
                    float sp[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (uint32_t w = 0; w < 16; w++) {  // fixed trip count, four interleaved chains, slots in order
                        const float v = rp[min(w, NBT - 1) * B * 16];
                        sp[w & 3] += w < NBT ? v : 0.f;
                    }
                    af[t2] = (sp[0] + sp[1]) + (sp[2] + sp[3]);
                    if constexpr (NORM) af[t2] = af[t2] / rms;
                }
                const float a0 = af[0], a1 = af[R - 1];
                const uint32_t row0 = u * 16 + ra;
                if constexpr (MODE == GEMV_PLAIN) {
                    if (lane < 16) {
                        p.y[b][row0] = a0;
                        if (topk_better(a0, row0, best_v[b], best_i[b])) { best_v[b] = a0; best_i[b] = row0; }
                    }
                } else if constexpr (MODE == GEMV_RESIDUAL) {
                    if (lane < 16) p.y[b][row0] = p.res[b][row0] + a0;   // TransformerBlock.cs:153-158 / 176-180: input + projection
                } else if constexpr (MODE == GEMV_GATEUP) {
                    if (lane < 16) p.y[b][row0] = a1 * silu_ref(a0);     // SiLUShader.cs:121-123, ElementWiseMultiplicationShader.cs:137
                } else {
                    // RoPEShader.cs:249-262 on the pair (row, row ^ 1) at THIS column's position; V rows are stored unrotated
                    uint32_t seg, tile;
                    bk_unit<MODE>(p, u, 0, seg, tile);
                    const uint32_t role = p.seg_role[seg];
                    const uint32_t row = tile * 16 + ra, head = row / p.D, dd = row % p.D;
                    const float other = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, a0), 0xB1, 0xF, 0xF, true));
                    float o = a0;
                    const uint32_t de = dd & ~1u;  // the even element of the rotated pair
                    if (role < 2 && de < p.rope_dims) {
                        const float c = cs[b * BK_CS + de], sn = cs[b * BK_CS + de + 1];
                        o = (dd & 1) ? (sn * other + c * a0) : (c * a0 - sn * other);
                    }
                    if (lane < 16) {
                        if (role == 0) p.y[b][row] = o;
                        else if (pos_ok[b])   // a position word at or past the capacity writes nothing (the launch reports it through p.err)
                            kv_store(role == 1 ? p.kc[b] : p.vc[b], p.kv_f16, (uint64_t)posv[b] * p.pos_stride + (uint64_t)head * p.head_stride[b] + dd, o);
                    }
                }
            }
        }
    };

    uint32_t c_tile = 0, c_ui = 0, c_t = 0;
    auto consume = [&](Regs &buf, auto IC) __attribute__((always_inline)) {
        constexpr int I = decltype(IC)::value;
        const uint32_t slot = wid * BPW + I;
        if constexpr (!NORM) {
            if (c_tile > 0 && c_ui == 0 && c_t == 0) {   // the first step of a later K tile on this slot
                if constexpr (!XPREF) load_x(c_tile, IC);
                stage_x(c_tile, IC);
                if constexpr (XPREF) {
                    if (c_tile + 1 < p.ntiles) load_x(c_tile + 1, IC);
                }
            }
        }
        const bool live = slot < NBT && c_tile * NBT + slot < p.NB;
        const uint32_t sl_ = min(slot, NBT - 1);
        const auto uw = kqm_unpack(buf, g);
        // Columns in groups of up to four, without a branch between them (dead columns are multiplied too: their LDS is never
        // written and their sums never read), so that the LDS reads, the MFMAs and the scale epilogues of a group overlap.
        // A fragments: the lanes that carry digits read them, all others read zeros (one address: a broadcast).
        constexpr int CG = B < 4 ? B : ((B == 8 && !NORM) ? 1 : ((B == 8 && WIDE) ? 2 : 4));   // (what fits 256 VGPRs without scratch)
#pragma unroll
        for (int b0 = 0; b0 < B; b0 += CG) {
            i32x4 af[CG][4];
            f32x4 sm[CG];
            int sx[CG];
#pragma unroll
            for (int c = 0; c < CG; c++) {
                const uint8_t *abase = a_live ? xa + ((size_t)(b0 + c) * NBT + sl_) * 1024 + a_off : zero;
#pragma unroll
                for (int sl = 0; sl < 4; sl++) af[c][sl] = *reinterpret_cast<const i32x4 *>(abase + sl * 256);
                if constexpr (IS8) sm[c] = f32x4{0.f, 0.f, 0.f, 0.f};   // Q8_0 stages no sums of x' (no offset, no min): nothing to read
                else sm[c] = *reinterpret_cast<const f32x4 *>(sums + (((b0 + c) * NBT + sl_) * 4 + g) * 4);
                sx[c] = sexp[(b0 + c) * NBT + sl_];
            }
#pragma unroll
            for (int c = 0; c < CG; c++) {
                const float a = kqm_dot(uw, af[c], sm[c]);
                acc[I][b0 + c] += live ? ldexpf(a, -sx[c]) : 0.f;  // back from x' = x * 2^S
            }
        }
        if (c_tile == p.ntiles - 1) {   // the slot's share of this (unit, tile of the unit) is complete
#pragma unroll
            for (int b = 0; b < B; b++) {
                if ((uint32_t)b < p.n) {
                    const float s = rows4_sum(acc[I][b]);
                    if (lane < 16 && slot < NBT) red[((c_t * NBT + slot) * B + b) * 16 + lane] = s;
                }
                acc[I][b] = 0.f;
            }
        }
        if constexpr (I == BPW - 1) {
            if (c_tile == p.ntiles - 1 && c_t == (uint32_t)R - 1) {
                __syncthreads();
                finish(blockIdx.x + c_ui * gridDim.x);
                __syncthreads();   // `red` is written again by the next unit
            }
            if (++c_t == (uint32_t)R) { c_t = 0; if (++c_ui == nunits) { c_ui = 0; ++c_tile; } }
        }
    };

    for (uint32_t st = 0; st < nsteps; st += NBUF) {   // buffer j holds the steps j (mod NBUF): with two slots per wave, slot j & 1
#define BK_STEP(J)                                                           \
    if (st + (J) < nsteps) {                                                 \
        consume(buf[(J)], std::integral_constant<int, (J) % BPW>{});         \
        issue(buf[(J)]);                                                     \
    }
        BK_STEP(0)
        BK_STEP(1)
        if constexpr (NBUF == 4) {
            BK_STEP(2)
            BK_STEP(3)
        }
#undef BK_STEP
    }

    if constexpr (MODE == GEMV_PLAIN) {
        // SamplingUtils.ArgMax per column in the same launch (SamplingUtils.cs:55-56: the LOWEST index among equal maxima), then the
        // end-of-token bookkeeping of every member: token word, ring, position (the tail of k_bgemv).
        float *sv = reinterpret_cast<float *>(am_lds);
        uint32_t *si = am_lds + B, *last = am_lds + 2 * B;
#pragma unroll
        for (int b = 0; b < B; b++) {
            if ((uint32_t)b % nw == wid) {
                float v = lane < 16 ? best_v[b] : -INFINITY;
                uint32_t i = lane < 16 ? best_i[b] : 0xFFFFFFFFu;
                wave_best(v, i);
                if (lane == 0) { sv[b] = v; si[b] = i; }
            }
        }
        __syncthreads();
        if (threadIdx.x < (uint32_t)B) {
            const uint32_t b = threadIdx.x;
            __hip_atomic_store(&p.part_v[b * BK_MAX_GRID + blockIdx.x], sv[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&p.part_i[b * BK_MAX_GRID + blockIdx.x], si[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
#pragma unroll
        for (int b = 0; b < B; b++) {
            if ((uint32_t)b % nw == wid && (uint32_t)b < p.n) {
                float v = -INFINITY;
                uint32_t i = 0xFFFFFFFFu;
                for (uint32_t gI = lane; gI < gridDim.x; gI += 64) {
                    const float ov = __hip_atomic_load(&p.part_v[b * BK_MAX_GRID + gI], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const uint32_t oi = __hip_atomic_load(&p.part_i[b * BK_MAX_GRID + gI], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (topk_better(ov, oi, v, i)) { v = ov; i = oi; }
                }
                wave_best(v, i);
                if (lane == 0) {
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
        }
        if (p.win_ctl) {   // (uniform over the launch)
            __syncthreads();
            if (threadIdx.x == 0) win_tail(last + 8, p.n, p.win_ctl, p.tok_batch, p.tok[0], p.pos_inc[0], p.ring[0], p.ring_len);
        }
        if (threadIdx.x == 0) __hip_atomic_store(p.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm (stream-ordered with the next launch)
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
struct BKqPlan { bool ok; int Bt; uint32_t NB, NBT, bpw, ntiles, nw, grid, NU; size_t lds; };

static BKqPlan plan_bkq(const BatchKqArgs &a)
{
    BKqPlan pl{};
    if (a.n < 1 || a.n > BATCH_MAX || a.K == 0 || a.K % 256 || a.n_cu == 0) return pl;
    if (!is_t16(a.w_type)) return pl;
    pl.Bt = a.n <= 2 ? 2 : (a.n <= 4 ? 4 : 8);
    for (int i = 0; i < 3; i++)
        if (a.seg_rows[i] % 16 || (a.seg_rows[i] && !a.W[i])) return pl;
    const uint32_t rows = a.seg_rows[0] + a.seg_rows[1] + a.seg_rows[2];
    if (a.mode == GEMV_QKV_ROPE) {
        if ((a.D != 64 && a.D != 128) || a.rope_dims > a.D || a.rope_dims % 2 || a.seg_rows[0] == 0) return pl;
        for (int i = 0; i < 3; i++)
            if (a.seg_role[i] > 2) return pl;
        pl.NU = rows / 16;
    } else if (a.mode == GEMV_GATEUP) {
        if (a.seg_rows[0] != a.seg_rows[1] || a.seg_rows[2]) return pl;
        pl.NU = a.seg_rows[0] / 16;
    } else {
        if (a.seg_rows[1] || a.seg_rows[2]) return pl;
        pl.NU = rows / 16;
    }
    if (pl.NU == 0) return pl;
    // K tiles: a function of K alone (the order of a sum must not depend on the batch size): even tiles of at most BK_NBT super-blocks
    pl.NB = a.K / 256;
    pl.ntiles = (pl.NB + BK_NBT - 1) / BK_NBT;
    pl.NBT = (pl.NB + pl.ntiles - 1) / pl.ntiles;
    pl.bpw = pl.NBT > 8 ? 2 : 1;   // at most 8 waves: 256 VGPRs hold two weight buffers, the unpacked operand and B columns in flight
    pl.nw = (pl.NBT + pl.bpw - 1) / pl.bpw;
    if (pl.ntiles > 1 && a.mode != GEMV_RESIDUAL) return pl;   // the normed launches see the whole vector; gate|up carries one sum per lane
    pl.grid = pl.ntiles > 1 ? pl.NU : std::min(pl.NU, a.n_cu);  // tiled: one unit per workgroup, its sums stay in registers across the tiles
    if (a.mode == GEMV_PLAIN && pl.grid > BK_MAX_GRID) return pl;
    const size_t R = a.mode == GEMV_GATEUP ? 2 : 1;
    pl.lds = (size_t)pl.Bt * pl.NBT * BK_BLK_LDS + R * pl.NBT * pl.Bt * 16 * 4 + (size_t)pl.NBT * pl.Bt * 4 +
             (a.mode == GEMV_QKV_ROPE ? (size_t)pl.Bt * BK_CS * 4 : 0) + 64 * 4 + 1024;
    pl.ok = pl.lds <= 160 * 1024;
    return pl;
}

bool batch_gemv_kq_ok(const BatchKqArgs &a) { return plan_bkq(a).ok; }

template <int QT, int B, int MODE, bool NORM, int BPW>
static hipError_t launch_bkq_w(const BKqParams &p, const BKqPlan &pl, hipStream_t s)
{
    static size_t allowed = 0;   // the kernel's dynamic-LDS limit is raised once (gfx950: 160 KB per CU)
    if (pl.lds > 64 * 1024 && pl.lds > allowed) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bgemv_kq<QT, B, MODE, NORM, BPW>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        allowed = 160 * 1024;
    }
    hipLaunchKernelGGL((k_bgemv_kq<QT, B, MODE, NORM, BPW>), dim3(pl.grid), dim3(pl.nw * 64), pl.lds, s, p);
    return hipGetLastError();
}

template <int QT, int B, int MODE, bool NORM>
static hipError_t launch_bkq(const BKqParams &p, const BKqPlan &pl, hipStream_t s)
{
    return pl.bpw == 2 ? launch_bkq_w<QT, B, MODE, NORM, 2>(p, pl, s) : launch_bkq_w<QT, B, MODE, NORM, 1>(p, pl, s);
}

template <int QT, int B>
static hipError_t dispatch_bkq(const BKqParams &p, const BKqPlan &pl, int mode, bool norm, hipStream_t s)
{
    switch (mode) {
        case GEMV_PLAIN: return norm ? launch_bkq<QT, B, GEMV_PLAIN, true>(p, pl, s) : hipErrorInvalidValue;
        case GEMV_RESIDUAL: return norm ? hipErrorInvalidValue : launch_bkq<QT, B, GEMV_RESIDUAL, false>(p, pl, s);
        case GEMV_QKV_ROPE: return norm ? launch_bkq<QT, B, GEMV_QKV_ROPE, true>(p, pl, s) : hipErrorInvalidValue;
        case GEMV_GATEUP: return norm ? launch_bkq<QT, B, GEMV_GATEUP, true>(p, pl, s) : hipErrorInvalidValue;
    }
    return hipErrorInvalidValue;
}

template <int QT>
static hipError_t dispatch_bkq_b(const BKqParams &p, const BKqPlan &pl, int mode, bool norm, hipStream_t s)
{
    if (pl.Bt == 2) return dispatch_bkq<QT, 2>(p, pl, mode, norm, s);
    if (pl.Bt == 4) return dispatch_bkq<QT, 4>(p, pl, mode, norm, s);
    return dispatch_bkq<QT, 8>(p, pl, mode, norm, s);
}

hipError_t launch_batch_gemv_kq(const BatchKqArgs &a, hipStream_t s)
{
    const BKqPlan pl = plan_bkq(a);
    if (!pl.ok) return hipErrorInvalidValue;
    BKqParams p{};
    uint32_t end = 0;
    for (int i = 0; i < 3; i++) {
        p.W[i] = static_cast<const uint8_t *>(a.W[i] ? a.W[i] : a.W[0]);
        p.seg_tiles[i] = a.seg_rows[i] / 16;
        end += p.seg_tiles[i];
        p.seg_tile_end[i] = end;
        p.seg_role[i] = a.seg_role[i];
    }
    p.K = a.K; p.NB = pl.NB; p.NBT = pl.NBT; p.ntiles = pl.ntiles; p.NU = pl.NU; p.n = a.n;
    p.gamma = a.gamma; p.eps = a.eps;
    for (uint32_t b = 0; b < BATCH_MAX; b++) {
        const uint32_t c = b < a.n ? b : 0;   // dead columns carry column 0's pointers (nothing is read or stored through them)
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
        p.part_i = reinterpret_cast<uint32_t *>(p.part_v + BATCH_MAX * BK_MAX_GRID);
        p.ticket = p.part_i + BATCH_MAX * BK_MAX_GRID;
        p.tok_batch = a.am_tok_batch; p.ring_len = a.am_ring_len; p.win_ctl = a.win_ctl;
    }
    const bool norm = a.gamma != nullptr;
    if (a.w_type == NFAI_Q6_K_T16) return dispatch_bkq_b<NFAI_Q6_K_T16>(p, pl, a.mode, norm, s);
    if (a.w_type == NFAI_Q5_K_T16) return dispatch_bkq_b<NFAI_Q5_K_T16>(p, pl, a.mode, norm, s);
    if (a.w_type == NFAI_Q8_0_T16) return dispatch_bkq_b<NFAI_Q8_0_T16>(p, pl, a.mode, norm, s);
    if (a.w_type == NFAI_Q4_0_T16) return dispatch_bkq_b<NFAI_Q4_0_T16>(p, pl, a.mode, norm, s);
    if (a.w_type == NFAI_Q3_K_T16) return dispatch_bkq_b<NFAI_Q3_K_T16>(p, pl, a.mode, norm, s);
    if (a.w_type == NFAI_IQ4_XS_T16) return dispatch_bkq_b<NFAI_IQ4_XS_T16>(p, pl, a.mode, norm, s);
    return dispatch_bkq_b<NFAI_Q4_K_T16>(p, pl, a.mode, norm, s);
}

}  // namespace nfai
