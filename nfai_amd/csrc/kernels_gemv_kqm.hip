// kernels_gemv_kqm.hip — decode GEMV on ggml K-quant and Q8_0 weights, second generation: the integer dot products
// of the quantised weights with fixed-point activations run on the matrix cores (v_mfma_i32_16x16x64_i8 used as
// 64 independent 16-wide dot products per instruction), the K-quant / Q8_0 scales are applied in fp32 (K-quants: Q4_K, Q5_K, Q6_K).
// Same op as kernels_gemv_kq.hip (MatrixMultiplyShader.cs:255-289 on weights the reference cannot
// load at all, Parser.cs:111-114); that file stays as the path for row counts that are not a
// multiple of 16.
//
// Why: kernels_gemv_kq.hip spends ~2.8 VALU operations per weight and lane (cvt + fma per nibble,
// eight ds_read_b128 of activations per 32 weights) and runs at 1.8 TB/s on the gate/up matrix of
// Llama-3.2-3B — VALU/LDS-bound at a quarter of what HBM delivers.  Here four nibbles become four
// byte operands with ONE v_and_b32 (q & 0x0F0F0F0F; the high nibbles one shift more), the multiply-
// accumulate moves to MFMA, and the activations are read from LDS by 12 lanes per instruction
// instead of 64: 0.375 (Q4_K) / 0.8 (Q6_K) VALU operations per weight and lane.
//
// Numerics: each 256-element super-block of the activation vector (after the optional RMSNorm) is
// scaled by a power of two so that |x * 2^S| < 2^22, rounded to an integer and split into three
// signed base-256 digits; sum q * x' = S0 + 256 S1 + 65536 S2 is exact in int32, the K-quant scales
// (d * sc, dmin * m, the -32 offset of Q6_K via the group sums of x') are applied in fp32 exactly
// as ggml defines the block; Q8_0 (d * q, q a signed byte) needs neither sums nor offsets: one d per lane
// and MFMA; Q4_0 (d * (q - 8), q a nibble) takes Q4_K's staging and sums of x' with d and 8 d in place of the scale and the min; Q3_K (d * (sc - 32) * (q - 4), q three bits) takes Q6_K's staging, its -4 through the per-16 sums of x' as Q6_K's -32; IQ4_XS (d * (ls - 32) * KV[q], q a nibble that indexes a 16-entry table of signed bytes) takes Q4_K's staging and Q4_0's four MFMAs on the table values, looked up in registers (iq4_lut4, t16.h), and like Q8_0 needs no sums.  The only approximation is x' = round(x * 2^S): 24 bits relative to
// the largest |x| of the super-block.  Against the fp32 oracle the differences are at the level of
// fp32 summation-order noise (tests/test_gpu_kquant.py states the tolerance; max |dlogit| 1.5e-5 at 3B).
//
// HBM layout: "T16", repacked once at upload, same bytes: t16.h.  Lane (G, r) of a wave owns 64 weights of row r of a 16-row tile.
//
// Work split: a workgroup owns whole 16-row tiles ("units": one tile, or the gate and the up tile of
// the same rows); its waves split K (wave w owns super-blocks w*BPW .. w*BPW+BPW-1 of every tile and
// stages exactly those super-blocks of x: no workgroup barrier before the first dot product unless
// the RMSNorm sum needs one), partial sums meet in LDS every UB units.  MFMA operand roles:
// A = activations (rows 4G, 4G+1, 4G+2 of the 16x64 A matrix carry the three digits of the 16 k-slots
// of lane group G, zero elsewhere), B = weights (column r = row r of the tile), so D[4G + {0,1,2}][r]
// lands in registers 0..2 of lane (G, r): every lane receives the dot product of exactly the 16
// weights it unpacked.
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "kqm.h"

namespace nfai {

template <int MODE>
__device__ __forceinline__ void kqm_unit(const KqmParams &p, uint32_t u, int t, uint32_t &seg, uint32_t &tile)
{
    if constexpr (MODE == GEMV_GATEUP) {
        seg = t; tile = u;
    } else if constexpr (MODE == GEMV_QKV_ROPE) {
        u += p.rot;
        if (u >= p.NU) u -= p.NU;
        if (u < p.seg_tile_end[0]) { seg = 0; tile = u; }
        else if (u < p.seg_tile_end[1]) { seg = 1; tile = u - p.seg_tile_end[0]; }
        else { seg = 2; tile = u - p.seg_tile_end[1]; }
    } else {
        seg = 0; tile = u;
    }
}

// What the epilogue of unit u reads besides the dot products; loaded unconditionally (clamped) so that the
// first round's copy can be fetched at kernel start, a microsecond of latency off the tail of the short kernels.
struct KqmPre { float res; f32x2 cs; uint32_t pos; };

template <int MODE, bool BEGIN = false>
__device__ __forceinline__ KqmPre kqm_preload(const KqmParams &p, uint32_t u, uint32_t lane)
{
    KqmPre q;
    q.res = 0.f; q.cs = f32x2{1.f, 0.f}; q.pos = 0;
    const uint32_t r = lane & 15;
    if constexpr (MODE == GEMV_RESIDUAL) {
        q.res = *((const GLOBAL_AS float *)p.res + (u * 16 + r));
    } else if constexpr (MODE == GEMV_QKV_ROPE) {
        uint32_t seg, tile;
        kqm_unit<MODE>(p, u, 0, seg, tile);
        const uint32_t de = ((tile * 16 + r) % p.D) & ~1u;
        q.pos = *((const GLOBAL_AS uint32_t *)p.pos);
        if constexpr (!BEGIN)  // (first launch of a token: the epilogue takes cos/sin from the workgroup's own table in LDS, begin_bookkeeping)
            q.cs = *reinterpret_cast<const GLOBAL_AS f32x2 *>((const GLOBAL_AS float *)p.rope_cs + min(de, p.rope_dims - 2));
    }
    return q;
}

// lanes 0..15 hold the 16 rows of the unit (a0; a1 = up row for GATEUP)
template <int MODE>
__device__ __forceinline__ void kqm_epilogue(const KqmParams &p, uint32_t u, uint32_t lane, float a0, float a1, const KqmPre &pre, float &best_v,
                                             uint32_t &best_i)
{
    const uint32_t r = lane & 15;
    if constexpr (MODE == GEMV_PLAIN) {
        if (lane < 16) {
            p.y[u * 16 + r] = a0;
            if (topk_better(a0, u * 16 + r, best_v, best_i)) { best_v = a0; best_i = u * 16 + r; }  // lm_head + ArgMax in one launch
        }
    } else if constexpr (MODE == GEMV_RESIDUAL) {
        if (lane < 16) p.y[u * 16 + r] = pre.res + a0;
    } else if constexpr (MODE == GEMV_GATEUP) {
        if (lane < 16) p.y[u * 16 + r] = a1 * silu_ref(a0);
    } else {
        uint32_t seg, tile;
        kqm_unit<MODE>(p, u, 0, seg, tile);
        const uint32_t row = tile * 16 + r, head = row / p.D, dd = row % p.D;
        const float other = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, a0), 0xB1, 0xF, 0xF, true));
        float o = a0;
        const uint32_t de = dd & ~1u;  // the even element of the rotated pair
        if (seg < 2 && de < p.rope_dims) {
            const float c = pre.cs[0], sn = pre.cs[1];
            o = (dd & 1) ? (sn * other + c * a0) : (c * a0 - sn * other);
        }
        if (lane < 16) {
            if (seg == 0) p.y[row] = o;
            else kv_store(seg == 1 ? p.kc : p.vc, p.kv_f16, (uint64_t)pre.pos * p.kv_pos_stride + (uint64_t)head * p.kv_head_stride + dd, o);
        }
    }
}

// NS > 0 (1 or 2): no workgroup has more than NS steps — all of them are issued before the prologue and consumed
// in a straight line (the common case for the per-block matrices of a 3B model).  NS = 0: ping-pong over two buffers.
// (Measured and dropped: an s_barrier between the activation loads and the first weight loads, so that no wave's x
// queues behind another wave's weights — no effect; four steps in flight — slower, see the step list in DESIGN.md.)
// BEGIN (q|k|v with RMSNorm only): the first launch of a token — embedding row, cos/sin table and the token's bookkeeping in this launch.
// A template parameter and not a kernel argument: as a run-time branch the (dead) bookkeeping code sat between the activation loads and
// the first weight requests of EVERY q|k|v launch (stamps: weights requested at 1.16 us against 0.4 us in the other launches).
template <int QT, int MODE, int BPW, bool NORM, int NS, bool BEGIN = false>
__global__ __launch_bounds__(1024) void k_gemv_kqt(const KqmParams p)
{
    static_assert(!BEGIN || (MODE == GEMV_QKV_ROPE && NORM), "a token begins with a normed q|k|v launch");
    // QT = NFAI_KQ_MIXED (QKV only): Q4_K and Q6_K segments in one launch (Q4_K_M files keep attn_v in Q6_K on half of
    // the blocks); the activations are staged in both fragment layouts and every step branches on its segment's type.
    // QT = NFAI_Q8_0_T16: its own A-fragment layout, never mixed with the K-quants (llama.hip gives a Q8_0 segment its own launch).
    // QT = NFAI_Q5_K_T16: the Q4_K staging (fragments and sums of x'); NFAI_KQ_MIXED5: Q5_K and Q6_K segments as NFAI_KQ_MIXED.
    // QT = NFAI_Q4_0_T16: the Q4_K staging too (t16.h); launched on Q4_0 segments only (llama.hip gives them their own launch).
    // QT = NFAI_Q3_K_T16: the Q6_K staging (fragments and per-16 sums of x', t16.h); launched on Q3_K segments only, as Q4_0.
    // QT = NFAI_IQ4_XS_T16: the Q4_K staging (its sums of x' go unread); launched on IQ4_XS segments only, as Q4_0.
    constexpr bool HAS8 = QT == NFAI_Q8_0_T16, HAS5 = QT == NFAI_Q5_K_T16 || QT == NFAI_KQ_MIXED5, IS40 = QT == NFAI_Q4_0_T16, IS3 = QT == NFAI_Q3_K_T16;
    constexpr bool ISI4 = QT == NFAI_IQ4_XS_T16;
    constexpr bool HAS4 = !HAS8 && !IS3 && QT != NFAI_Q6_K_T16, HAS6 = !HAS8 && !IS40 && !ISI4 && QT != NFAI_Q4_K_T16 && QT != NFAI_Q5_K_T16, MIXED = HAS4 && HAS6;
    static_assert(!MIXED || MODE == GEMV_QKV_ROPE, "mixed encodings exist for the q|k|v launch only");
    using Regs = typename std::conditional<
        QT == NFAI_Q4_K_T16, Q4T,
        typename std::conditional<HAS8, Q8T, typename std::conditional<QT == NFAI_Q5_K_T16, Q5T, typename std::conditional<IS40, Q40T, typename std::conditional<IS3, Q3T, typename std::conditional<ISI4, IQ4T, Q6T>::type>::type>::type>::type>::type>::type;
    constexpr int R = MODE == GEMV_GATEUP ? 2 : 1;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t tid = threadIdx.x, lane = tid & 63, nw = blockDim.x >> 6;
    const uint32_t wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t kpad = nw * BPW * 256;
    const uint32_t UB = p.UB;
    uint8_t *xa = smem;                                               // kpad * 4 bytes: A fragments [blk][slot][G][digit][16 B]
    uint8_t *xa6 = MIXED ? smem + (size_t)kpad * 4 : xa;             // second fragment layout (Q6_K) when both are needed
    float *sums = reinterpret_cast<float *>(xa6 + (size_t)kpad * 4);  // [blk][G][4]: sums of x' per scale group
    float *sums6 = MIXED ? sums + nw * BPW * 16 : sums;
    int *sexp = reinterpret_cast<int *>(sums6 + nw * BPW * 16);       // [blk] S of the super-block's fixed-point scale 2^S
    float *red = reinterpret_cast<float *>(sexp + nw * BPW);          // [2][UB][R][nw][64]
    float *scal = red + 2 * UB * R * nw * 64;                       // 32 floats of reduction scratch

    const uint32_t nunits = (p.NU - blockIdx.x + gridDim.x - 1) / gridDim.x;
    const uint32_t nsteps = nunits * R * BPW;  // step = (unit, tile of the unit, super-block of this wave)
    STAMP_DECL;
    STAMP(0);  // wave started

    // ---- activations first (vmcnt is in order: what the prologue needs must not queue behind weights).
    // Wave w loads, scales and stages exactly the super-blocks it will consume (w*BPW .. w*BPW+BPW-1): the fixed-point
    // scale is per super-block (a wave reduction, no LDS), and nothing staged here is read by another wave — the only
    // workgroup barrier of the prologue is the one the RMSNorm sum needs.
    f32x4 xv[BPW], gv[NORM ? BPW : 1];
#pragma unroll
    for (int i = 0; i < BPW; i++) {
        const uint32_t bw = wid * BPW + i;
        const uint32_t kk = min(bw, p.NB - 1) * 256 + lane * 4;
        f32x4 v;
        if (BEGIN && p.begin.emb) {  // block-uniform: the token's embedding row (first launch of a token)
            v = embed_load4(p.begin.emb, p.begin.emb_type, p.begin.emb_rows, p.begin.tok[0], kk, p.K);
            if (blockIdx.x == 0 && bw < p.NB) *reinterpret_cast<f32x4 *>(p.begin.x_out + kk) = v;  // the residual the later launches read
        } else {
            v = *reinterpret_cast<const GLOBAL_AS f32x4 *>((const GLOBAL_AS float *)p.x + kk);
        }
        xv[i] = bw < p.NB ? v : f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (NORM) gv[i] = *reinterpret_cast<const GLOBAL_AS f32x4 *>((const GLOBAL_AS float *)p.gamma + kk);
    }

    // keep the activation loads FIRST in program order (vmcnt retires in order: the prologue must not wait behind
    // weights): without this fence hipcc's scheduler interleaves the loads below with them (measured: -2.5 % tokens/s)
    __builtin_amdgcn_sched_barrier(0);
    const KqmPre pre0 = kqm_preload<MODE, BEGIN>(p, min(blockIdx.x + wid * gridDim.x, p.NU - 1), lane);  // epilogue inputs of round 0
    float *cs_lds = scal + 32 + 48;  // behind the fused ArgMax words
    if constexpr (BEGIN) begin_bookkeeping(p.begin, pre0.pos, cs_lds);
    // ---- weights of the first steps
    constexpr int NBUF = NS > 0 ? NS : 2;
    // Steps issued before the prologue.  Q8_0 with eight super-blocks per wave and the RMSNorm gains (K > 16384): x, the gains and two
    // 18-VGPR steps did not fit 128 VGPRs together (scratch); the second step is issued once x is staged.
    constexpr int PRE = (HAS8 && BPW == 8 && NORM && NS == 0) ? 1 : NBUF;
    Regs buf[NBUF];
    uint32_t ist = 0;
    auto issue = [&](Regs &buf) {
        const uint32_t is = min(ist, nsteps - 1);  // past the end: the wave's own last step again
        const uint32_t ui = is / (R * BPW), tt = (is / BPW) % R, bi = is % BPW;
        const uint32_t u = blockIdx.x + ui * gridDim.x;
        const uint32_t blk = min(wid * BPW + bi, p.NB - 1);
        uint32_t seg, tile;
        kqm_unit<MODE>(p, u, tt, seg, tile);
        if constexpr (QT == NFAI_Q4_K_T16) {
            buf = q4t_load(p, seg, tile, blk, lane);
        } else if constexpr (QT == NFAI_Q6_K_T16) {
            buf = q6t_load(p, seg, tile, blk, lane);
        } else if constexpr (HAS8) {
            buf = q8t_load(p, seg, tile, blk, lane);
        } else if constexpr (QT == NFAI_Q5_K_T16) {
            buf = q5t_load(p, seg, tile, blk, lane);
        } else if constexpr (IS40) {
            buf = q40t_load(p, seg, tile, blk, lane);
        } else if constexpr (IS3) {
            buf = q3t_load(p, seg, tile, blk, lane);
        } else if constexpr (ISI4) {
            buf = iq4t_load(p, seg, tile, blk, lane);
        } else {
            if ((p.seg6 >> seg) & 1u) {
                buf = q6t_load(p, seg, tile, blk, lane);
            } else if constexpr (HAS5) {  // the high bits ride in the first two words of the Q6_K qh slot
                const Q5T q = q5t_load(p, seg, tile, blk, lane);
                buf.qla = q.q0; buf.qlb = q.q1; buf.sc = q.hdr; buf.qh[0] = q.qh[0]; buf.qh[1] = q.qh[1];
            } else {
                const Q4T q = q4t_load(p, seg, tile, blk, lane);
                buf.qla = q.q0; buf.qlb = q.q1; buf.sc = q.hdr;
            }
        }
        ++ist;
    };
#pragma unroll
    for (int j = 0; j < PRE; j++) issue(buf[j]);
    STAMP(1);  // activation loads and the first weight steps issued

    // ---- prologue: per-super-block power-of-two scale, three base-256 digits -> LDS, scale-group sums.
    // RMSNorm (RMSNormShader.cs:136-149: (x / rms) * g) is applied in two parts: the gains here, element by element (u = x * g), the
    // division by rms = sqrt(mean(x^2) + eps) on the finished dot products in the epilogue — it is one scalar per vector, and
    // waiting for it here meant a workgroup barrier on the slowest wave's x, whose request sits behind every other wave's first
    // weight requests in the CU's in-order memory queue (stamps, round 3: x staged at 2.7-3.4 us with the barrier, 0.8 us without;
    // 3B Q4_K_M 1026 -> 1088 tokens/s).  Every wave stages exactly the super-blocks it consumes, so nothing here waits for another
    // wave; its share of sum(x^2) goes to LDS and is combined in fixed wave order behind the barrier the cross-wave reduction needs
    // anyway.  The fixed-point rounding of u (24 bits relative to the super-block's maximum) dominates the two roundings the
    // reordering moves.
    {
        if constexpr (NORM) {
            float ss = 0.f;
#pragma unroll
            for (int i = 0; i < BPW; i++)
#pragma unroll
                for (int e = 0; e < 4; e++) ss = fmaf(xv[i][e], xv[i][e], ss);
            ss = wave_sum(ss);
            if (lane == 0) scal[wid] = ss;
        }
#pragma unroll
        for (int i = 0; i < BPW; i++) {
            const uint32_t blk = wid * BPW + i;
            f32x4 v = xv[i];
            if constexpr (NORM) {
                v[0] = v[0] * gv[i][0];
                v[1] = v[1] * gv[i][1];
                v[2] = v[2] * gv[i][2];
                v[3] = v[3] * gv[i][3];
            }
            kqm_stage<HAS4, HAS6, HAS8>(v, blk, lane, xa, xa6, sums, sums6, sexp);
        }
        // no barrier: every LDS word written above is read only by this wave (LDS operations of a wave execute in order)
    }
    if constexpr (PRE < NBUF) issue(buf[PRE]);
    STAMP(2);  // x normalised, scaled and staged as digits in LDS

    const uint32_t g = lane >> 4, ra = lane & 15;
    const bool a_live = (ra >> 2) == g && (ra & 3) < 3;  // A rows 4G, 4G+1, 4G+2 = digits 0, 1, 2 of lane group G
    const uint32_t a_off = g * 64 + (ra & 3) * 16;

    float acc = 0.f;
    float best_v = -INFINITY;
    uint32_t best_i = 0xFFFFFFFFu;
    uint32_t cst = 0, par = 0;
    auto consume = [&](Regs &buf) {
        const uint32_t ui = cst / (R * BPW), tt = (cst / BPW) % R, bi = cst % BPW;
        const uint32_t bc = wid * BPW + bi;
        const bool live = bc < p.NB;
        const uint32_t blk = min(bc, p.NB - 1);
        bool is6 = QT == NFAI_Q6_K_T16 || IS3;  // the Q6_K staging
        if constexpr (MIXED) {
            uint32_t seg, tile;
            kqm_unit<MODE>(p, blockIdx.x + ui * gridDim.x, tt, seg, tile);
            is6 = (p.seg6 >> seg) & 1u;
        }
        float a;
        // A fragments: only the lanes that carry digits read LDS (exec-masked), the rest supply zeros
        const uint8_t *abase = (is6 ? xa6 : xa) + (size_t)blk * 1024 + a_off;
        i32x4 af[4] = {i32x4{0, 0, 0, 0}, i32x4{0, 0, 0, 0}, i32x4{0, 0, 0, 0}, i32x4{0, 0, 0, 0}};
        if (a_live) {
#pragma unroll
            for (int sl = 0; sl < 4; sl++) af[sl] = *reinterpret_cast<const i32x4 *>(abase + sl * 256);
        }
        const int sx = sexp[blk];
        if constexpr (HAS8) {
            a = q8t_dot(buf, af);
        } else {
            if (is6) {
                if constexpr (HAS6) {
                    const f32x4 sm = *reinterpret_cast<const f32x4 *>(sums6 + (blk * 4 + g) * 4);
                    if constexpr (IS3) a = q3t_dot(buf, af, sm, g);
                    else a = q6t_dot(buf, af, sm, g);
                }
            } else {
                if constexpr (HAS4) {
                    const f32x4 sm = *reinterpret_cast<const f32x4 *>(sums + (blk * 4 + g) * 4);
                    if constexpr (QT == NFAI_Q4_K_T16) a = q4t_dot(buf, af, f32x2{sm[0], sm[1]}, g);
                    else if constexpr (QT == NFAI_Q5_K_T16) a = q5t_dot(buf, af, f32x2{sm[0], sm[1]}, g);
                    else if constexpr (IS40) a = q40t_dot(buf, af, f32x2{sm[0], sm[1]});
                    else if constexpr (ISI4) a = iq4t_dot(buf, af, g);
                    else if constexpr (HAS5) a = q5t_dot(Q5T{buf.qla, buf.qlb, buf.sc, u32x2{buf.qh[0], buf.qh[1]}}, af, f32x2{sm[0], sm[1]}, g);
                    else a = q4t_dot(Q4T{buf.qla, buf.qlb, buf.sc}, af, f32x2{sm[0], sm[1]}, g);
                }
            }
        }
        acc += live ? ldexpf(a, -sx) : 0.f;  // back from x' = x * 2^S (S up to 170 or down to -106: no float 2^-S)
        ++cst;
        if (bi == BPW - 1) {
            const uint32_t slot = ui % UB;
            red[(((par * UB + slot) * R + tt) * nw + wid) * 64 + lane] = acc;
            acc = 0.f;
            if (tt == R - 1 && (slot == UB - 1 || ui == nunits - 1)) {
                __syncthreads();
                if (wid <= slot) {  // wave q finishes unit q of this round
                    const uint32_t uq = blockIdx.x + (ui - slot + wid) * gridDim.x;
                    KqmPre pre = ui == slot ? pre0 : kqm_preload<MODE, BEGIN>(p, uq, lane);
                    if constexpr (BEGIN) {
                        {  // the table this workgroup tabulated before its first step (barrier above)
                            uint32_t seg, tile;
                            kqm_unit<MODE>(p, uq, 0, seg, tile);
                            const uint32_t de = ((tile * 16 + (lane & 15)) % p.D) & ~1u;
                            pre.cs = *reinterpret_cast<const f32x2 *>(cs_lds + min(de, p.rope_dims - 2));
                        }
                    }
                    float rms = 1.f;
                    if constexpr (NORM) {  // every wave's share of sum(x^2) is in LDS (written before its first step, barrier above)
                        float tss = 0.f;
#pragma unroll
                        for (uint32_t i = 0; i < 16; i++) {  // fixed trip count and order: the LDS reads issue back to back
                            const float s_i = scal[min(i, nw - 1)];
                            tss += i < nw ? s_i : 0.f;
                        }
                        rms = sqrtf(tss / (float)p.K + p.eps);
                    }
                    float af[R];
#pragma unroll
                    for (int t2 = 0; t2 < R; t2++) {
                        const float *rp = red + (((par * UB + wid) * R + t2) * nw) * 64 + lane;
                        float sp[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (uint32_t w = 0; w < 16; w++) {  // fixed trip count, four independent chains
                            const float v = rp[min(w, nw - 1) * 64];
                            sp[w & 3] += w < nw ? v : 0.f;
                        }
                        float s = (sp[0] + sp[1]) + (sp[2] + sp[3]);
                        af[t2] = rows4_sum(s);
                        if constexpr (NORM) af[t2] = af[t2] / rms;
                    }
                    kqm_epilogue<MODE>(p, uq, lane, af[0], af[R - 1], pre, best_v, best_i);
                }
                par ^= 1;
            }
        }
    };

    if constexpr (NS > 0) {
#pragma unroll
        for (int j = 0; j < NS; j++) {
            if ((uint32_t)j < nsteps) consume(buf[j]);
            if (j == 0) STAMP(3);  // first weight step landed, multiplied (and, with one step per unit, reduced)
        }
    } else {
        uint32_t st = 0;
#ifdef NFAI_STAMPS
        if (nsteps > 4) {
            consume(buf[0]);
            STAMP(3);
            issue(buf[0]);
            consume(buf[1]);
            issue(buf[1]);
            st = 2;
        } else {
            STAMP(3);
        }
#endif
        for (; st + 3 < nsteps; st += 2) {
            consume(buf[0]);
            issue(buf[0]);
            consume(buf[1]);
            issue(buf[1]);
        }
        const uint32_t rem = nsteps - st;
        if (rem == 3) {
            consume(buf[0]);
            issue(buf[0]);
            consume(buf[1]);
            consume(buf[0]);
        } else if (rem == 2) {
            consume(buf[0]);
            consume(buf[1]);
        } else if (rem == 1) {
            consume(buf[0]);
        }
    }
#ifdef NFAI_STAMPS
    STAMP(4);  // last step consumed, reductions and epilogue stores issued
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    STAMP(5);  // stores acknowledged
    STAMP_FLUSH(p.stamps, blockIdx.x * nw + wid, 6);
#endif
    if constexpr (MODE == GEMV_PLAIN) {
        // SamplingUtils.ArgMax over the outputs in the same launch (block-uniform: a kernel argument); its 48 LDS words sit behind `scal`
        if (p.am.ticket != nullptr) argmax_fused_tail(best_v, best_i, p.am, reinterpret_cast<uint32_t *>(scal + 32));
    }
}

// ---- repack: native ggml blocks (row-major) -> T16 planes (same bytes), one workgroup per (tile, super-block) -----------------------
template <class Kern>
static hipError_t launch_repack_t16(Kern kern, uint32_t block, const void *native, void *tiled, uint64_t rows, uint64_t cols, hipStream_t s)
{
    if (rows == 0) return hipSuccess;
    if (rows % 16 || cols % 256) return hipErrorInvalidValue;
    const uint64_t nb = cols / 256, grid = rows / 16 * nb;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    kern<<<(uint32_t)grid, block, 0, s>>>(static_cast<const uint8_t *>(native), static_cast<uint8_t *>(tiled), (uint32_t)(rows / 16), (uint32_t)nb);
    return hipGetLastError();
}

// ---- Q4_K repack: native 144-byte blocks (row-major: d, dmin, scales[12], qs[128]) -> T16 planes (same bytes) ---------------------
__global__ void k_repack_q4k_t16(const uint8_t *src, uint8_t *dst, uint32_t n_tiles, uint32_t NB)
{
    const uint64_t tb = blockIdx.x;  // tile * NB + blk
    const uint32_t tile = (uint32_t)(tb / NB), blk = (uint32_t)(tb % NB), t = threadIdx.x;
    const uint64_t nblk = t16_nblk(n_tiles, NB);
    if (t < 128) {
        const uint32_t h = t >> 6, ln = t & 63, G = ln >> 4, r = ln & 15;
        const uint8_t *s = src + ((uint64_t)(tile * 16 + r) * NB + blk) * GGML_Q4_K_BLOCK + 16 + 32 * G + 16 * h;
        *reinterpret_cast<u32x4 *>(t16_k4_qs(dst, tb) + h * 1024 + ln * 16) = *reinterpret_cast<const u32x4 *>(s);
    } else if (t < 144) {
        const uint32_t r = t - 128;
        const uint8_t *s = src + ((uint64_t)(tile * 16 + r) * NB + blk) * GGML_Q4_K_BLOCK;
        *reinterpret_cast<u32x4 *>(t16_k4_hdr(dst, nblk, tb) + r * 16) = *reinterpret_cast<const u32x4 *>(s);
    }
}

// ---- Q6_K repack: native 210-byte blocks (row-major: ql[128], qh[64], scales[16], d) -> T16 planes (same bytes) -----------------
__global__ void k_repack_q6k_t16(const uint8_t *src, uint8_t *dst, uint32_t n_tiles, uint32_t NB)
{
    const uint64_t tb = blockIdx.x;
    const uint32_t tile = (uint32_t)(tb / NB), blk = (uint32_t)(tb % NB), t = threadIdx.x;
    const uint64_t nblk = t16_nblk(n_tiles, NB);
    // native blocks are only 2-byte aligned: byte copies
    for (uint32_t e = t; e < 3072; e += blockDim.x) {
        const uint32_t piece = e >> 10, ln = (e >> 4) & 63, b = e & 15, G = ln >> 4, r = ln & 15, n = G >> 1, lh = G & 1;
        const uint8_t *s = src + ((uint64_t)(tile * 16 + r) * NB + blk) * GGML_Q6_K_BLOCK;
        const uint32_t off = piece == 0 ? 64 * n + 16 * lh : (piece == 1 ? 64 * n + 32 + 16 * lh : 128 + 32 * n + 16 * lh);
        t16_q6k_q(dst, tb)[e] = s[off + b];
    }
    for (uint32_t e = t; e < 256; e += blockDim.x) {
        const uint32_t r = e >> 4, b = e & 15;
        t16_q6k_sc(dst, nblk, tb)[e] = src[((uint64_t)(tile * 16 + r) * NB + blk) * GGML_Q6_K_BLOCK + 192 + b];
    }
    if (t < 32) t16_q6k_d(dst, nblk, tb)[t] = src[((uint64_t)(tile * 16 + (t >> 1)) * NB + blk) * GGML_Q6_K_BLOCK + 208 + (t & 1)];
}

// ---- Q8_0 repack: native 34-byte blocks (row-major: d, qs[32]) -> T16 planes (same bytes) ---------------------------------
__global__ void k_repack_q80_t16(const uint8_t *src, uint8_t *dst, uint32_t n_tiles, uint32_t NB)
{
    const uint64_t tb = blockIdx.x;
    const uint32_t tile = (uint32_t)(tb / NB), blk = (uint32_t)(tb % NB), t = threadIdx.x;
    const uint64_t nblk = t16_nblk(n_tiles, NB);
    // native blocks are only 2-byte aligned: byte copies
    for (uint32_t e = t; e < 4096; e += blockDim.x) {
        const uint32_t h = e >> 10, ln = (e >> 4) & 63, b = e & 15, G = ln >> 4, r = ln & 15, kk = 64 * h + 16 * G + b;
        const uint8_t *s = src + ((uint64_t)(tile * 16 + r) * NB * 8 + blk * 8 + (kk >> 5)) * GGML_Q8_0_BLOCK;
        t16_q80_qs(dst, tb)[e] = s[2 + (kk & 31)];
    }
    for (uint32_t e = t; e < 256; e += blockDim.x) {
        const uint32_t r = e >> 4, i = (e & 15) >> 1, b32 = 2 * (i & 3) + (i >> 2);  // half i of the row = d of 32-block b32
        t16_q80_d(dst, nblk, tb)[e] = src[((uint64_t)(tile * 16 + r) * NB * 8 + blk * 8 + b32) * GGML_Q8_0_BLOCK + (e & 1)];
    }
}

// ---- Q4_0 repack: native 18-byte blocks (row-major: d, qs[16]) -> T16 planes (same bytes) ---------------------------------
__global__ void k_repack_q40_t16(const uint8_t *src, uint8_t *dst, uint32_t n_tiles, uint32_t NB)
{
    const uint64_t tb = blockIdx.x;
    const uint32_t tile = (uint32_t)(tb / NB), blk = (uint32_t)(tb % NB), t = threadIdx.x;
    const uint64_t nblk = t16_nblk(n_tiles, NB);
    // native blocks are only 2-byte aligned: byte copies
    for (uint32_t e = t; e < 2048; e += blockDim.x) {
        const uint32_t h = e >> 10, ln = (e >> 4) & 63, b = e & 15, G = ln >> 4, r = ln & 15;
        const uint8_t *s = src + ((uint64_t)(tile * 16 + r) * NB * 8 + blk * 8 + 2 * G + h) * GGML_Q4_0_BLOCK;
        t16_q40_qs(dst, tb)[e] = s[2 + b];
    }
    for (uint32_t e = t; e < 256; e += blockDim.x) {
        const uint32_t r = e >> 4, b32 = (e & 15) >> 1;  // half b32 of the row = d of 32-block b32
        t16_q40_d(dst, nblk, tb)[e] = src[((uint64_t)(tile * 16 + r) * NB * 8 + blk * 8 + b32) * GGML_Q4_0_BLOCK + (e & 1)];
    }
}

// ---- IQ4_XS repack: native 136-byte blocks (row-major: d, scales_h, scales_l[4], qs[128]) -> T16 planes (same bytes) -----------------
// Plane 0: qs[16 (2G + h) .. + 16) of the row's block to lane (G, r) of half h (Q4_0's plane); plane 1: the block's first 8 bytes.
__global__ void k_repack_iq4xs_t16(const uint8_t *src, uint8_t *dst, uint32_t n_tiles, uint32_t NB)
{
    const uint64_t tb = blockIdx.x;
    const uint32_t tile = (uint32_t)(tb / NB), blk = (uint32_t)(tb % NB), t = threadIdx.x;
    const uint64_t nblk = t16_nblk(n_tiles, NB);
    // native blocks are 8-byte aligned within a row of an aligned buffer, but a caller's device pointer need not be: byte copies
    for (uint32_t e = t; e < 2048; e += blockDim.x) {
        const uint32_t h = e >> 10, ln = (e >> 4) & 63, b = e & 15, G = ln >> 4, r = ln & 15;
        t16_iq4_qs(dst, tb)[e] = src[((uint64_t)(tile * 16 + r) * NB + blk) * GGML_IQ4_XS_BLOCK + 8 + 16 * (2 * G + h) + b];
    }
    if (t < 128) t16_iq4_hdr(dst, nblk, tb)[t] = src[((uint64_t)(tile * 16 + (t >> 3)) * NB + blk) * GGML_IQ4_XS_BLOCK + (t & 7)];
}

// ---- Q3_K repack: native 110-byte blocks (row-major: hmask[32], qs[64], scales[12], d) -> T16 planes (same bytes) --------------------
// Plane 0: the lane's 16 qs bytes as they are; plane 1: the bit order of t16.h; planes 2 and 3: the scale bytes and d as they are.
__global__ void k_repack_q3k_t16(const uint8_t *src, uint8_t *dst, uint32_t n_tiles, uint32_t NB)
{
    const uint64_t tb = blockIdx.x;
    const uint32_t tile = (uint32_t)(tb / NB), blk = (uint32_t)(tb % NB), t = threadIdx.x;
    const uint64_t nblk = t16_nblk(n_tiles, NB);
    // native blocks are only 2-byte aligned: byte copies
    for (uint32_t e = t; e < 1024; e += blockDim.x) {
        const uint32_t ln = e >> 4, b = e & 15, G = ln >> 4, r = ln & 15, n = G >> 1, lh = G & 1;
        t16_q3k_qs(dst, tb)[e] = src[((uint64_t)(tile * 16 + r) * NB + blk) * GGML_Q3_K_BLOCK + 32 + 32 * n + 16 * lh + b];
    }
    for (uint32_t e = t; e < 512; e += blockDim.x) {  // byte b of word w of lane ln: weights l = 8w + 4 i2 + b, bit 4 i2 + j
        const uint32_t ln = e >> 3, w = (e >> 2) & 1, b = e & 3, G = ln >> 4, r = ln & 15, n = G >> 1, lh = G & 1;
        const uint8_t *hm = src + ((uint64_t)(tile * 16 + r) * NB + blk) * GGML_Q3_K_BLOCK + 16 * lh;
        uint32_t byte = 0;
        for (uint32_t i2 = 0; i2 < 2; i2++)
            for (uint32_t j = 0; j < 4; j++) byte |= ((hm[8 * w + 4 * i2 + b] >> (4 * n + j)) & 1u) << (4 * i2 + j);
        t16_q3k_hm(dst, nblk, tb)[e] = (uint8_t)byte;
    }
    for (uint32_t e = t; e < 192; e += blockDim.x)
        t16_q3k_sc(dst, nblk, tb)[e] = src[((uint64_t)(tile * 16 + e / 12) * NB + blk) * GGML_Q3_K_BLOCK + 96 + e % 12];
    if (t < 32) t16_q3k_d(dst, nblk, tb)[t] = src[((uint64_t)(tile * 16 + (t >> 1)) * NB + blk) * GGML_Q3_K_BLOCK + 108 + (t & 1)];
}

// ---- Q5_K repack: native 176-byte blocks (row-major: d, dmin, scales[12], qh[32], qs[128]) -> T16 planes -------------------
// Planes 0 and 1 as k_repack_q4k_t16 (qs at byte 48 of the block, the header is its first 16 bytes); plane 2: the bit order of t16.h.
__global__ void k_repack_q5k_t16(const uint8_t *src, uint8_t *dst, uint32_t n_tiles, uint32_t NB)
{
    const uint64_t tb = blockIdx.x;
    const uint32_t tile = (uint32_t)(tb / NB), blk = (uint32_t)(tb % NB), t = threadIdx.x;
    const uint64_t nblk = t16_nblk(n_tiles, NB);
    if (t < 128) {
        const uint32_t h = t >> 6, ln = t & 63, G = ln >> 4, r = ln & 15;
        const uint8_t *s = src + ((uint64_t)(tile * 16 + r) * NB + blk) * GGML_Q5_K_BLOCK + 48 + 32 * G + 16 * h;
        *reinterpret_cast<u32x4 *>(t16_k4_qs(dst, tb) + h * 1024 + ln * 16) = *reinterpret_cast<const u32x4 *>(s);
    } else if (t < 256) {
        const uint32_t hf = t & 1, ln = (t - 128) >> 1, G = ln >> 4, r = ln & 15;
        const uint8_t *blkp = src + ((uint64_t)(tile * 16 + r) * NB + blk) * GGML_Q5_K_BLOCK;
        if (t < 144) *reinterpret_cast<u32x4 *>(t16_k4_hdr(dst, nblk, tb) + (t - 128) * 16) =
            *reinterpret_cast<const u32x4 *>(src + ((uint64_t)(tile * 16 + (t - 128)) * NB + blk) * GGML_Q5_K_BLOCK);
        const u32x4 qh = *reinterpret_cast<const u32x4 *>(blkp + 16 + 16 * hf);  // qh[16hf .. 16hf + 16)
        uint32_t word = 0;
#pragma unroll
        for (int l = 0; l < 16; l++) {
            const uint32_t byte = (qh[l >> 2] >> (8 * (l & 3))) & 0xFFu, i = l >> 2, b = l & 3;
            word |= ((byte >> (2 * G)) & 1u) << (8 * b + i);
            word |= ((byte >> (2 * G + 1)) & 1u) << (8 * b + 4 + i);
        }
        *reinterpret_cast<uint32_t *>(t16_q5k_qh(dst, nblk, tb) + ln * 8 + hf * 4) = word;
    }
}

hipError_t launch_repack_q4k_t16(const void *native, void *tiled, uint64_t rows, uint64_t cols, hipStream_t s)
{
    return launch_repack_t16(k_repack_q4k_t16, 192, native, tiled, rows, cols, s);
}
hipError_t launch_repack_q6k_t16(const void *native, void *tiled, uint64_t rows, uint64_t cols, hipStream_t s)
{
    return launch_repack_t16(k_repack_q6k_t16, 256, native, tiled, rows, cols, s);
}
hipError_t launch_repack_q80_t16(const void *native, void *tiled, uint64_t rows, uint64_t cols, hipStream_t s)
{
    return launch_repack_t16(k_repack_q80_t16, 256, native, tiled, rows, cols, s);
}
hipError_t launch_repack_q5k_t16(const void *native, void *tiled, uint64_t rows, uint64_t cols, hipStream_t s)
{
    return launch_repack_t16(k_repack_q5k_t16, 256, native, tiled, rows, cols, s);
}
hipError_t launch_repack_q40_t16(const void *native, void *tiled, uint64_t rows, uint64_t cols, hipStream_t s)
{
    return launch_repack_t16(k_repack_q40_t16, 256, native, tiled, rows, cols, s);
}
hipError_t launch_repack_q3k_t16(const void *native, void *tiled, uint64_t rows, uint64_t cols, hipStream_t s)
{
    return launch_repack_t16(k_repack_q3k_t16, 256, native, tiled, rows, cols, s);
}
hipError_t launch_repack_iq4xs_t16(const void *native, void *tiled, uint64_t rows, uint64_t cols, hipStream_t s)
{
    return launch_repack_t16(k_repack_iq4xs_t16, 256, native, tiled, rows, cols, s);
}

// ---- rows of a T16 table -> fp32 (embedding gather): row tok[t] to y + t * E (prefill, single token) or, y == nullptr, to x[t] (the
// members of a decode batch), four elements per thread -------------------------------------------------------------------------------
struct EmbedT16Params { const uint8_t *table; int type; uint64_t n_rows; uint32_t E; const uint32_t *tok; float *y; float *x[BATCH_MAX]; };

__global__ __launch_bounds__(256) void k_embed_t16(const EmbedT16Params p)
{
    const uint32_t t = blockIdx.y;
    uint64_t row = p.tok[t];
    if (row >= p.n_rows) row = p.n_rows - 1;   // (the host checks the tokens it is given; a fed-back ArgMax is always a row)
    float *out = p.y ? p.y + (uint64_t)t * p.E : p.x[t];
    for (uint32_t k = (blockIdx.x * blockDim.x + threadIdx.x) * 4; k < p.E; k += gridDim.x * blockDim.x * 4)
        *reinterpret_cast<f32x4 *>(out + k) = t16_row_load4(p.table, p.type, p.n_rows, row, k, p.E);
}

hipError_t launch_embed_rows_kqt(const void *table, int type, uint64_t n_rows, const uint32_t *toks, float *y, uint32_t T, uint32_t E, hipStream_t s)
{
    if (E % 256 || n_rows == 0 || n_rows % 16 || T == 0 || !y || !is_t16(type)) return hipErrorInvalidValue;
    EmbedT16Params p{};
    p.table = static_cast<const uint8_t *>(table); p.type = type; p.n_rows = n_rows; p.E = E; p.tok = toks; p.y = y;
    hipLaunchKernelGGL(k_embed_t16, dim3((E / 4 + 255) / 256, T), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_embed_kqt(const void *table, int type, uint64_t n_rows, const uint32_t *tok, float *y, uint32_t E, hipStream_t s)
{
    return launch_embed_rows_kqt(table, type, n_rows, tok, y, 1, E, s);
}

hipError_t launch_batch_embed_kq(const void *table, int type, uint64_t n_rows, uint32_t E, const uint32_t *tok, float *const *x, uint32_t n, hipStream_t s)
{
    if (!table || !tok || n < 1 || n > BATCH_MAX || E % 256 || n_rows == 0 || n_rows % 16) return hipErrorInvalidValue;
    if (!is_t16(type)) return hipErrorInvalidValue;
    EmbedT16Params p{};
    p.table = static_cast<const uint8_t *>(table); p.type = type; p.n_rows = n_rows; p.E = E; p.tok = tok;
    for (uint32_t b = 0; b < n; b++) {
        if (!x[b]) return hipErrorInvalidValue;
        p.x[b] = x[b];
    }
    hipLaunchKernelGGL(k_embed_t16, dim3((E / 4 + 255) / 256, n), dim3(256), 0, s, p);
    return hipGetLastError();
}

// ---- T16 tensor -> fp16 [rows][cols] (K-quant prefill: one block's matrices are widened into a scratch buffer and
// go through the fp16 MFMA GEMMs of kernels_prefill.hip; the decode path never dequantises to memory) -------------------
// One wave per (tile, super-block); lane (G, r) expands the 64 weights it also owns in the GEMV.  The wave's 16 x 256 fp16 go through
// LDS (rows padded by 16 bytes) so that every store instruction writes two whole 512-byte row pieces: stored straight from the
// lanes that expand them, an instruction wrote 64 separate 16-byte pieces in 64 different lines (13.2 us per tensor on average at
// 3B, a third of the K-quant prefill).
constexpr uint32_t DQ_ROW = 512 + 16;
// fp16 of a product rounded as written: to fp32, then to fp16 (as the oracle's dequantisation).  Without the empty asm the backend
// folds (_Float16)(a * b) into one v_fma_mix{lo,hi}_f16 a, b, 0: a single rounding, and +0 where a negative a times a zero b is -0.
__device__ __forceinline__ _Float16 f16_of_f32(float v)
{
    asm("" : "+v"(v));
    return (_Float16)v;
}
template <int QT>
__global__ __launch_bounds__(256) void k_dequant_t16(const uint8_t *W, _Float16 *out, uint32_t n_tiles, uint32_t NB, uint32_t tile0, uint32_t all_tiles)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[4][16 * DQ_ROW];
    // the launch covers tiles [tile0, tile0 + n_tiles) of a tensor of all_tiles tiles: `tile` counts output rows, `tb` the tensor's records
    const uint64_t tb_out = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tb_out >= (uint64_t)n_tiles * NB) return;
    const uint32_t lane = threadIdx.x & 63, g = lane >> 4, r = lane & 15;
    const uint32_t tile = (uint32_t)(tb_out / NB), blk = (uint32_t)(tb_out % NB);
    const uint64_t tb = tb_out + (uint64_t)tile0 * NB;
    const uint64_t nblk = t16_nblk(all_tiles, NB);
    _Float16 *orow = reinterpret_cast<_Float16 *>(stage[threadIdx.x >> 6] + r * DQ_ROW);
    if constexpr (QT == NFAI_Q4_K_T16 || QT == NFAI_Q5_K_T16) {
        const u32x4 q0 = load_nt16(t16_k4_qs(W, tb) + lane * 16), q1 = load_nt16(t16_k4_qs(W, tb) + 1024 + lane * 16);
        const u32x4 hdr = load_nt16(t16_k4_hdr(W, nblk, tb) + r * 16);
        u32x2 qh5 = {0u, 0u};  // Q5_K: the high-bit plane (bit order of q5t_dot)
        if constexpr (QT == NFAI_Q5_K_T16) qh5 = *reinterpret_cast<const u32x2 *>(t16_q5k_qh(W, nblk, tb) + lane * 8);
        const float d = h2f_lo(hdr[0]), dmin = h2f_hi(hdr[0]);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t sb = 2 * g + h;
            uint32_t sc, mn;
            k4_scale_min(hdr, sb, sc, mn);
            const float d1 = d * (float)sc, m1 = dmin * (float)mn;
#pragma unroll
            for (int c = 0; c < 4; c++) {  // 8 weights = bytes 8c .. 8c+7 of the 32-byte run
                const u32x4 q = c < 2 ? q0 : q1;
                const uint32_t wa = q[2 * (c & 1)], wb = q[2 * (c & 1) + 1];
                f16x8 o;
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const uint32_t byte = ((e < 4 ? wa : wb) >> (8 * (e & 3))) & 0xFFu;
                    uint32_t nib = h ? (byte >> 4) : (byte & 0xFu);
                    if constexpr (QT == NFAI_Q5_K_T16)  // weight 8c + e: dword 2 (c & 1) + (e >> 2) of q{c >> 1}
                        nib |= ((qh5[c >> 1] >> (8 * (e & 3) + 4 * h + 2 * (c & 1) + (e >> 2))) & 1u) << 4;
                    o[e] = (_Float16)(d1 * (float)nib - m1);
                }
                *reinterpret_cast<f16x8 *>(orow + sb * 32 + c * 8) = o;
            }
        }
    } else if constexpr (QT == NFAI_Q4_0_T16) {
        const uint32_t dw = *reinterpret_cast<const uint32_t *>(t16_q40_d(W, nblk, tb) + r * 16 + g * 4);
#pragma unroll
        for (int h = 0; h < 2; h++) {  // 32-block 2g + h of row r: weights 0..15 = low nibbles, 16..31 = high nibbles of its 16 bytes
            const u32x4 q = load_nt16(t16_q40_qs(W, tb) + h * 1024 + lane * 16);
            const float d = h ? h2f_hi(dw) : h2f_lo(dw);
#pragma unroll
            for (int c = 0; c < 4; c++) {  // 8 weights: nibble c >> 1 of bytes 8 (c & 1) .. + 8
                f16x8 o;
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const uint32_t byte = (q[2 * (c & 1) + (e >> 2)] >> (8 * (e & 3))) & 0xFFu;
                    o[e] = f16_of_f32(d * (float)((int)((c >> 1) ? (byte >> 4) : (byte & 0xFu)) - 8));
                }
                *reinterpret_cast<f16x8 *>(orow + (2 * g + h) * 32 + c * 8) = o;
            }
        }
    } else if constexpr (QT == NFAI_IQ4_XS_T16) {
        const u32x2 hdr = *reinterpret_cast<const u32x2 *>(t16_iq4_hdr(W, nblk, tb) + r * 8);
        const float d = h2f_lo(hdr[0]);
#pragma unroll
        for (int h = 0; h < 2; h++) {  // sub-block 2g + h of row r: weights 0..15 = the table values of the low nibbles, 16..31 = of the high nibbles
            const u32x4 q = load_nt16(t16_iq4_qs(W, tb) + h * 1024 + lane * 16);
            const float dl = d * (float)(iq4xs_scale(hdr[0], hdr[1], 2 * g + h) - 32);  // (d * (ls - 32)) * KV[q], as the format writes it
#pragma unroll
            for (int c = 0; c < 4; c++) {  // 8 weights: nibble c >> 1 of bytes 8 (c & 1) .. + 8
                f16x8 o;
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const uint32_t qw = q[2 * (c & 1) + i], v4 = iq4_lut4((c >> 1) ? (qw >> 4) : qw);
#pragma unroll
                    for (int e = 0; e < 4; e++) o[4 * i + e] = f16_of_f32(dl * (float)(int8_t)((v4 >> (8 * e)) & 0xFFu));
                }
                *reinterpret_cast<f16x8 *>(orow + (2 * g + h) * 32 + c * 8) = o;
            }
        }
    } else if constexpr (QT == NFAI_Q3_K_T16) {
        const u32x4 q = load_nt16(t16_q3k_qs(W, tb) + lane * 16);
        const u32x2 hm = *reinterpret_cast<const u32x2 *>(t16_q3k_hm(W, nblk, tb) + lane * 8);
        const uint32_t *scw = reinterpret_cast<const uint32_t *>(t16_q3k_sc(W, nblk, tb) + r * 12);
        const uint32_t s0 = scw[0], s1 = scw[1], s2 = scw[2];
        const float d = (float)*reinterpret_cast<const _Float16 *>(t16_q3k_d(W, nblk, tb) + r * 2);
        const uint32_t n = g >> 1, lh = g & 1;
#pragma unroll
        for (int qd = 0; qd < 4; qd++) {  // weights 128n + 32qd + 16lh .. +16 of row r: (d * (sc - 32)) * (q - 4), as ggml writes it
            const float dl = d * (float)(q3k_scale(s0, s1, s2, 8 * n + lh + 2 * qd) - 32);
#pragma unroll
            for (int c = 0; c < 2; c++) {
                f16x8 o;
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const uint32_t l = c * 8 + e;  // byte l & 3 of dword l >> 2; its high bit at 8 (l & 3) + 4 ((l >> 2) & 1) + qd of word l >> 3
                    const uint32_t lo = (q[l >> 2] >> (8 * (l & 3) + 2 * qd)) & 3u;
                    const uint32_t hb = (hm[l >> 3] >> (8 * (l & 3) + 4 * ((l >> 2) & 1) + qd)) & 1u;
                    o[e] = f16_of_f32(dl * (float)((int)(lo | (hb << 2)) - 4));
                }
                *reinterpret_cast<f16x8 *>(orow + n * 128 + qd * 32 + lh * 16 + c * 8) = o;
            }
        }
    } else if constexpr (QT == NFAI_Q8_0_T16) {
        const u32x4 dv = load_nt16(t16_q80_d(W, nblk, tb) + r * 16);
#pragma unroll
        for (int h = 0; h < 4; h++) {  // weights 64h + 16g .. +16 of row r: 32-block 2h + (g >> 1), its d at half (g >> 1) * 4 + h
            const u32x4 q = load_nt16(t16_q80_qs(W, tb) + h * 1024 + lane * 16);
            const uint32_t dw = (g >> 1) ? dv[2 + (h >> 1)] : dv[h >> 1];
            const float d = (h & 1) ? h2f_hi(dw) : h2f_lo(dw);
#pragma unroll
            for (int c = 0; c < 2; c++) {
                f16x8 o;
#pragma unroll
                for (int e = 0; e < 8; e++) o[e] = f16_of_f32(d * (float)(int8_t)((q[2 * c + (e >> 2)] >> (8 * (e & 3))) & 0xFFu));
                *reinterpret_cast<f16x8 *>(orow + 64 * h + 16 * g + 8 * c) = o;
            }
        }
    } else {
        const u32x4 qla = load_nt16(t16_q6k_q(W, tb) + lane * 16), qlb = load_nt16(t16_q6k_q(W, tb) + 1024 + lane * 16);
        const u32x4 qh = load_nt16(t16_q6k_q(W, tb) + 2048 + lane * 16);
        const u32x4 scv = load_nt16(t16_q6k_sc(W, nblk, tb) + r * 16);
        const float d = (float)*reinterpret_cast<const _Float16 *>(t16_q6k_d(W, nblk, tb) + r * 2);
        const uint32_t n = g >> 1, lh = g & 1;
#pragma unroll
        for (int qd = 0; qd < 4; qd++) {
            const u32x4 ql = (qd & 1) ? qlb : qla;
            const float dsc = d * (float)q6k_scale(scv, 8 * n + lh + 2 * qd);
#pragma unroll
            for (int c = 0; c < 2; c++) {
                f16x8 o;
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const uint32_t j = c * 8 + e;
                    const uint32_t lb = (ql[j >> 2] >> (8 * (j & 3))) & 0xFFu, hb = (qh[j >> 2] >> (8 * (j & 3))) & 0xFFu;
                    const int q = (int)(((qd >= 2) ? (lb >> 4) : (lb & 0xFu)) | (((hb >> (2 * qd)) & 3u) << 4)) - 32;
                    o[e] = f16_of_f32(dsc * (float)q);
                }
                *reinterpret_cast<f16x8 *>(orow + n * 128 + qd * 32 + lh * 16 + c * 8) = o;
            }
        }
    }
    // LDS operations of a wave execute in order: the row pieces written above are complete when these reads are served
    const uint8_t *st = stage[threadIdx.x >> 6];
    const uint64_t row_bytes = (uint64_t)NB * 512;
    uint8_t *obase = reinterpret_cast<uint8_t *>(out) + (uint64_t)tile * 16 * row_bytes + (uint64_t)blk * 512;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t row = 2 * i + (lane >> 5), piece = lane & 31;
        const u32x4 v = *reinterpret_cast<const u32x4 *>(st + row * DQ_ROW + piece * 16);
        *reinterpret_cast<u32x4 *>(obase + row * row_bytes + piece * 16) = v;
    }
}

hipError_t launch_dequant_t16_f16(const void *W, int type, uint64_t rows, uint64_t cols, uint64_t tile0, uint64_t n_tiles, void *out_f16, hipStream_t s)
{
    if (n_tiles == 0) return hipSuccess;
    if (rows % 16 || cols % 256 || tile0 + n_tiles > rows / 16) return hipErrorInvalidValue;
    const uint64_t all = rows / 16, nb = cols / 256, grid = (n_tiles * nb + 3) / 4;
    if (grid > 0x7FFFFFFFull || all > 0xFFFFFFFFull) return hipErrorInvalidValue;
#define NFAI_DQ(QT) k_dequant_t16<QT><<<(uint32_t)grid, 256, 0, s>>>(static_cast<const uint8_t *>(W), static_cast<_Float16 *>(out_f16), (uint32_t)n_tiles, (uint32_t)nb, (uint32_t)tile0, (uint32_t)all)
    if (type == NFAI_Q4_K_T16) NFAI_DQ(NFAI_Q4_K_T16);
    else if (type == NFAI_Q6_K_T16) NFAI_DQ(NFAI_Q6_K_T16);
    else if (type == NFAI_Q5_K_T16) NFAI_DQ(NFAI_Q5_K_T16);
    else if (type == NFAI_Q4_0_T16) NFAI_DQ(NFAI_Q4_0_T16);
    else if (type == NFAI_Q3_K_T16) NFAI_DQ(NFAI_Q3_K_T16);
    else if (type == NFAI_IQ4_XS_T16) NFAI_DQ(NFAI_IQ4_XS_T16);
    else if (type == NFAI_Q8_0_T16) NFAI_DQ(NFAI_Q8_0_T16);
    else return hipErrorInvalidValue;
#undef NFAI_DQ
    return hipGetLastError();
}

hipError_t launch_dequant_t16_f16(const void *W, int type, uint64_t rows, uint64_t cols, void *out_f16, hipStream_t s)
{
    return launch_dequant_t16_f16(W, type, rows, cols, 0, rows / 16, out_f16, s);
}

// ---- dispatch ------------------------------------------------------------------------------------------
template <int QT, int MODE, int BPW>
static hipError_t q4t_launch(const KqmParams &p, int ns, uint32_t grid, uint32_t block, size_t lds, hipStream_t s)
{
    auto go = [&](auto kern) {
        static bool attr_done = false;  // per instantiation
        if (!attr_done) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (e != hipSuccess) return e;
            attr_done = true;
        }
        hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, s, p);
        return hipGetLastError();
    };
    const bool norm = p.gamma != nullptr;
    if constexpr (MODE == GEMV_QKV_ROPE) {
        if (p.begin.on) {  // (launch_gemv_kqm: only with gamma)
            switch (ns) {
                case 1: return go(k_gemv_kqt<QT, MODE, BPW, true, 1, true>);
                case 2: return go(k_gemv_kqt<QT, MODE, BPW, true, 2, true>);
            }
            return go(k_gemv_kqt<QT, MODE, BPW, true, 0, true>);
        }
    }
    switch (ns) {
        case 1: return norm ? go(k_gemv_kqt<QT, MODE, BPW, true, 1>) : go(k_gemv_kqt<QT, MODE, BPW, false, 1>);
        case 2: return norm ? go(k_gemv_kqt<QT, MODE, BPW, true, 2>) : go(k_gemv_kqt<QT, MODE, BPW, false, 2>);
    }
    return norm ? go(k_gemv_kqt<QT, MODE, BPW, true, 0>) : go(k_gemv_kqt<QT, MODE, BPW, false, 0>);
}

template <int QT, int MODE>
static hipError_t q4t_bpw(const KqmParams &p, int bpw, uint32_t grid, uint32_t block, size_t lds, hipStream_t s)
{
    // steps of the busiest workgroup; all-upfront variants exist for 1, 2 and (<= 12 waves) 4 steps
    constexpr int R = MODE == GEMV_GATEUP ? 2 : 1;
    const uint32_t max_steps = (p.NU + grid - 1) / grid * R * bpw;
    static const int env_ns = getenv("NFAI_KQM_NS") ? atoi(getenv("NFAI_KQM_NS")) : 1;
    int ns = 0;
    if (env_ns) {
        if (max_steps == 1) ns = 1;
        else if (max_steps == 2) ns = 2;
    }
    if (bpw == 1) return q4t_launch<QT, MODE, 1>(p, ns, grid, block, lds, s);
    if (bpw == 2) return q4t_launch<QT, MODE, 2>(p, ns, grid, block, lds, s);
    if (bpw == 4) return q4t_launch<QT, MODE, 4>(p, ns, grid, block, lds, s);
    return q4t_launch<QT, MODE, 8>(p, ns, grid, block, lds, s);
}

template <int QT>
static hipError_t q4t_mode(const KqmParams &p, int mode, int bpw, uint32_t grid, uint32_t block, size_t lds, hipStream_t s)
{
    switch (mode) {
        case GEMV_PLAIN: return q4t_bpw<QT, GEMV_PLAIN>(p, bpw, grid, block, lds, s);
        case GEMV_RESIDUAL: return q4t_bpw<QT, GEMV_RESIDUAL>(p, bpw, grid, block, lds, s);
        case GEMV_QKV_ROPE: return q4t_bpw<QT, GEMV_QKV_ROPE>(p, bpw, grid, block, lds, s);
        case GEMV_GATEUP: return q4t_bpw<QT, GEMV_GATEUP>(p, bpw, grid, block, lds, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_gemv_kqm(const GemvArgs &a, hipStream_t s)
{
    if (!is_t16(a.w_type) && a.w_type != NFAI_KQ_MIXED && a.w_type != NFAI_KQ_MIXED5) return hipErrorInvalidValue;
    if ((a.w_type == NFAI_KQ_MIXED || a.w_type == NFAI_KQ_MIXED5) && a.mode != GEMV_QKV_ROPE) return hipErrorInvalidValue;
    if (a.K == 0 || a.K % 256 != 0 || a.K > 32768) return hipErrorInvalidValue;
    KqmParams p{};
    uint32_t total_tiles = 0;
    for (int i = 0; i < 3; i++) {
        if (a.seg_rows[i] % 16) return hipErrorInvalidValue;
        p.W[i] = reinterpret_cast<const uint8_t *>(a.W[i]);
        p.seg_tiles[i] = a.seg_rows[i] / 16;
        total_tiles += p.seg_tiles[i];
        p.seg_tile_end[i] = total_tiles;
    }
    if (a.mode == GEMV_QKV_ROPE) {
        if (a.D & 1u) return hipErrorInvalidValue;
        p.NU = total_tiles;
    } else if (a.mode == GEMV_GATEUP) {
        if (a.seg_rows[0] != a.seg_rows[1]) return hipErrorInvalidValue;
        p.NU = p.seg_tiles[0];
    } else {
        p.NU = p.seg_tiles[0];
    }
    if (p.NU == 0) return hipSuccess;
    p.x = a.x; p.gamma = a.gamma; p.eps = a.eps; p.K = a.K;
    p.NB = a.K / 256;
    p.y = a.y; p.res = a.res; p.kc = a.kcache; p.vc = a.vcache;
    p.kv_pos_stride = a.kv_pos_stride; p.kv_head_stride = a.kv_head_stride;
    p.rope_cs = a.rope_cs; p.rope_dims = a.rope_dims; p.D = a.D ? a.D : 2; p.pos = a.pos_dev;
    p.kv_f16 = a.kv_type == NFAI_F16;
    p.seg6 = a.seg6_mask;
    if (a.begin.on) {
        if (a.mode != GEMV_QKV_ROPE || !a.gamma || !a.begin.freqs || !a.begin.cs_out || (a.begin.emb && (!a.begin.tok || !a.begin.x_out))) return hipErrorInvalidValue;
        p.begin.on = 1; p.begin.emb = static_cast<const uint8_t *>(a.begin.emb); p.begin.emb_type = a.begin.emb_type; p.begin.emb_rows = a.begin.emb_rows;
        p.begin.tok = a.begin.tok; p.begin.x_out = a.begin.x_out; p.begin.freqs = a.begin.freqs; p.begin.cs_out = a.begin.cs_out;
        p.begin.n_freq = a.begin.n_freq; p.begin.epoch = a.begin.epoch;
    }
    if (a.argmax_part) {
        if (a.mode != GEMV_PLAIN || !a.argmax_out) return hipErrorInvalidValue;
        p.am.part_v = static_cast<float *>(a.argmax_part);
        p.am.part_i = reinterpret_cast<uint32_t *>(p.am.part_v + ARGMAX_FUSED_MAX_BLOCKS);
        p.am.ticket = p.am.part_i + ARGMAX_FUSED_MAX_BLOCKS;
        p.am.out_idx = a.argmax_out; p.am.pos_inc = a.argmax_pos_inc; p.am.ring = a.argmax_ring; p.am.ring_len = a.argmax_ring_len;
    }
    static const int env_bpw = getenv("NFAI_KQM_BPW") ? atoi(getenv("NFAI_KQM_BPW")) : 0;  // sweep knob: super-blocks per wave
    int bpw = p.NB <= 16 ? 1 : (p.NB <= 32 ? 2 : (p.NB <= 64 ? 4 : 8));  // K <= 32768 (Llama-70B: ffn length 28672)
    if ((env_bpw == 2 || env_bpw == 4) && env_bpw > bpw && p.NB % env_bpw == 0) bpw = env_bpw;
    const uint32_t nw = (p.NB + bpw - 1) / bpw;
    // workgroups per CU.  One, except for q|k|v: its 320 tiles (3B) on 256 single workgroups leave 64 of them two tiles in a row; as 320
    // workgroups, two of them share 64 CUs instead (3B Q4_K_M: 8.97 against 9.19 us per launch; the lm_head loses 3 us with two)
    static const int env_bpc_all = getenv("NFAI_KQM_BPC") ? atoi(getenv("NFAI_KQM_BPC")) : 0;  // sweep knobs
    const int env_bpc = env_bpc_all ? env_bpc_all : (a.mode == GEMV_QKV_ROPE ? 2 : 1);
    static const int env_ub = getenv("NFAI_KQM_UB") ? atoi(getenv("NFAI_KQM_UB")) : 4;
    const uint32_t grid = min(p.NU, a.n_cu * (uint32_t)max(1, min(env_bpc, 8)));
    if (a.argmax_part && grid > ARGMAX_FUSED_MAX_BLOCKS) return hipErrorInvalidValue;
    const uint32_t upb = (p.NU + grid - 1) / grid;
    // q|k|v as one workgroup per tile with more tiles than CUs (3B: 320 on 256): workgroups b and b + n_cu share a CU.  Rotating the
    // tile numbering by NU - n_cu puts the FIRST tiles (q rows, Q4_K) on the shared CUs and the last ones — the v rows, Q6_K in half
    // of a Q4_K_M file's blocks: 40 KB per tile instead of 27 — on CUs of their own (3B Q4_K_M 1071 -> 1078-1088 tokens/s, 8B 646 -> 651).
    // NFAI_KQM_ROT=n forces a rotation, -1 none.
    static const int env_rot = getenv("NFAI_KQM_ROT") ? atoi(getenv("NFAI_KQM_ROT")) : 0;
    p.rot = 0;
    if (a.mode == GEMV_QKV_ROPE) {
        if (env_rot > 0 && (uint32_t)env_rot < p.NU) p.rot = (uint32_t)env_rot;
        else if (env_rot == 0 && grid == p.NU && p.NU > a.n_cu && p.NU <= 2 * a.n_cu) p.rot = p.NU - a.n_cu;
    }
    p.UB = min((uint32_t)max(1, min(env_ub, 8)), min(upb, nw));
    const int R = a.mode == GEMV_GATEUP ? 2 : 1;
    const size_t nlay = (a.w_type == NFAI_KQ_MIXED || a.w_type == NFAI_KQ_MIXED5) ? 2 : 1;  // fragment layouts staged
    auto lds_bytes = [&](uint32_t ub) {
        return nlay * ((size_t)nw * bpw * 1024 + (size_t)nw * bpw * 64) + (size_t)nw * bpw * 4 + (size_t)2 * ub * R * nw * 256 + 128 + 192 + BEGIN_CS_WORDS * 4;  // + 48 words of the fused ArgMax + the cos/sin table of a token's first launch
    };
    while (p.UB > 1 && lds_bytes(p.UB) > 160 * 1024) p.UB--;  // very long K: fewer units per reduction round
    const size_t lds = lds_bytes(p.UB);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    {
        static const char *names[] = {"kqm_plain", "kqm_residual", "kqm_qkv_rope", "kqm_gateup"};
        NFAI_STAMP_SET(p, names[a.mode & 3], grid, nw * 64);
    }
    if (a.w_type == NFAI_KQ_MIXED) return q4t_bpw<NFAI_KQ_MIXED, GEMV_QKV_ROPE>(p, bpw, grid, nw * 64, lds, s);
    if (a.w_type == NFAI_KQ_MIXED5) return q4t_bpw<NFAI_KQ_MIXED5, GEMV_QKV_ROPE>(p, bpw, grid, nw * 64, lds, s);
    if (a.w_type == NFAI_Q5_K_T16) return q4t_mode<NFAI_Q5_K_T16>(p, a.mode, bpw, grid, nw * 64, lds, s);
    if (a.w_type == NFAI_Q8_0_T16) return q4t_mode<NFAI_Q8_0_T16>(p, a.mode, bpw, grid, nw * 64, lds, s);
    if (a.w_type == NFAI_Q4_0_T16) return q4t_mode<NFAI_Q4_0_T16>(p, a.mode, bpw, grid, nw * 64, lds, s);
    if (a.w_type == NFAI_Q3_K_T16) return q4t_mode<NFAI_Q3_K_T16>(p, a.mode, bpw, grid, nw * 64, lds, s);
    if (a.w_type == NFAI_IQ4_XS_T16) return q4t_mode<NFAI_IQ4_XS_T16>(p, a.mode, bpw, grid, nw * 64, lds, s);
    if (a.w_type == NFAI_Q4_K_T16) return q4t_mode<NFAI_Q4_K_T16>(p, a.mode, bpw, grid, nw * 64, lds, s);
    return q4t_mode<NFAI_Q6_K_T16>(p, a.mode, bpw, grid, nw * 64, lds, s);
}

}  // namespace nfai
