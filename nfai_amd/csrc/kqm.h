// kqm.h — what the int8-MFMA GEMVs on T16 weights share (kernels_gemv_kqm.hip: one sequence, numerics and operand roles are described
// there; kernels_gemv_batch_kqm.hip: up to 8 sequences): a wave's step registers and loads per type, the unpack of a step into MFMA B
// operands, the dot products with their fp32 scale epilogues, and the fixed-point staging of the activations.  The layout itself
// (plane addresses, block decode) is t16.h.
#pragma once
#include "common.h"
#include "t16.h"

namespace nfai {

#ifndef GLOBAL_AS
#define GLOBAL_AS __attribute__((address_space(1)))
#endif

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

struct KqmParams {
    const uint8_t *W[3];
    uint32_t seg_tiles[3];     // 16-row tiles per segment
    uint32_t seg_tile_end[3];  // running sum (QKV unit -> segment)
    const float *x;
    const float *gamma;
    float eps;
    uint32_t K, NB, NU, UB;
    uint32_t seg6;             // NFAI_KQ_MIXED(5): bit i set = segment i is Q6_K (else Q4_K, or Q5_K for NFAI_KQ_MIXED5)
    uint32_t rot;              // q|k|v: unit u works on tile (u + rot) mod NU
    float *y;
    const float *res;
    void *kc, *vc;
    uint64_t kv_pos_stride, kv_head_stride;
    const float *rope_cs;
    uint32_t rope_dims, D;
    const uint32_t *pos;
    int kv_f16;
    ArgmaxFused am;            // GEMV_PLAIN: first index of the largest output, taken in this launch (am.ticket == nullptr: off)
    BeginParams begin;         // GEMV_QKV_ROPE: the per-token prologue in this launch (begin.on == 0: off)
    NFAI_STAMP_PARAM
};

struct Q4T { u32x4 q0, q1, hdr; };
struct Q8T { u32x4 q[4]; u32x2 d; };
struct Q5T { u32x4 q0, q1, hdr; u32x2 qh; };
struct Q6T { u32x4 qla, qlb, qh, sc; uint32_t d; };
struct Q40T { u32x4 q0, q1; uint32_t d; };
struct Q3T { u32x4 q; u32x2 h; uint32_t s0, s1, s2, d; };
struct IQ4T { u32x4 q0, q1; u32x2 hdr; };

__device__ __forceinline__ uint32_t and_or(uint32_t a, uint32_t mask, uint32_t bits) { return (a & mask) | bits; }

__device__ __forceinline__ float dpp_add8(float v)  // sum within aligned groups of 8 lanes
{
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
    return v;
}

// One step of a wave: the quants (2 x 1 KiB) and the 16 row headers (256 B) of super-block `blk` of 16-row tile `tile`; `base` = the
// tensor in the T16 layout, `n_tiles` its tiles, NB = super-blocks per row.
__device__ __forceinline__ Q4T q4t_load_raw(const uint8_t *base, uint64_t n_tiles, uint32_t NB, uint32_t tile, uint32_t blk, uint32_t lane)
{
    const uint64_t tb = t16_tb(tile, NB, blk), nblk = t16_nblk(n_tiles, NB);
    Q4T r;
    r.q0 = load_nt16(t16_k4_qs(base, tb) + lane * 16);
    r.q1 = load_nt16(t16_k4_qs(base, tb) + 1024 + lane * 16);
    r.hdr = load_nt16(t16_k4_hdr(base, nblk, tb) + (lane & 15) * 16);
    return r;
}

__device__ __forceinline__ Q4T q4t_load(const KqmParams &p, uint32_t seg, uint32_t tile, uint32_t blk, uint32_t lane)
{
    return q4t_load_raw(p.W[seg], p.seg_tiles[seg], p.NB, tile, blk, lane);
}

// One step of a wave on a Q8_0 T16 tensor: the quants (4 x 1 KiB) and the d of the 16 rows (256 B) of super-block `blk`; a lane of
// group G takes the 8-byte half G >> 1 of its row's d: the d of its four 32-blocks 2h + (G >> 1), h = 0..3 (18 VGPRs per step with
// the quants; with the 16 bytes of the row the q|k|v launch at K > 16384 spilled).
__device__ __forceinline__ Q8T q8t_load_raw(const uint8_t *base, uint64_t n_tiles, uint32_t NB, uint32_t tile, uint32_t blk, uint32_t lane)
{
    const uint64_t tb = t16_tb(tile, NB, blk), nblk = t16_nblk(n_tiles, NB);
    Q8T r;
#pragma unroll
    for (int h = 0; h < 4; h++) r.q[h] = load_nt16(t16_q80_qs(base, tb) + h * 1024 + lane * 16);
    r.d = __builtin_nontemporal_load((const GLOBAL_AS u32x2 *)(t16_q80_d(base, nblk, tb) + (lane & 15) * 16 + (lane >> 5) * 8));
    return r;
}

__device__ __forceinline__ Q8T q8t_load(const KqmParams &p, uint32_t seg, uint32_t tile, uint32_t blk, uint32_t lane)
{
    return q8t_load_raw(p.W[seg], p.seg_tiles[seg], p.NB, tile, blk, lane);
}

// 64 weights of one lane: qs bytes 64h + 16G .. +16 of its row for h = 0..3 (block32 2h + (G >> 1)), already signed bytes: one MFMA and
// one d per h, no offset and no min, so no sums of x'.  af: this lane's four A fragments (slot h).
__device__ __forceinline__ float q8t_dot(const Q8T &w, const i32x4 (&af)[4])
{
    float a = 0.f;
#pragma unroll
    for (int h = 0; h < 4; h++) {
        const i32x4 dq = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[h], __builtin_bit_cast(i32x4, w.q[h]), i32x4{0, 0, 0, 0}, 0, 0, 0);
        const float v = fmaf((float)dq[2], 65536.0f, fmaf((float)dq[1], 256.0f, (float)dq[0]));
        const float d = (h & 1) ? h2f_hi(w.d[h >> 1]) : h2f_lo(w.d[h >> 1]);
        a = fmaf(d, v, a);
    }
    return a;
}

// 64 weights of one lane (sub-blocks 2G: low nibbles, 2G+1: high nibbles) against the activations.
// af: this lane's four A fragments (slot 2n + hf; all zero for the lanes whose A rows are zero);
// sums = {SX[2G], SX[2G+1]} of this super-block.
__device__ __forceinline__ float q4t_dot(const Q4T &w, const i32x4 (&af)[4], f32x2 sums, uint32_t g)
{
    constexpr uint32_t M = 0x0F0F0F0Fu;
    i32x4 dlo = {0, 0, 0, 0}, dhi = {0, 0, 0, 0};
#pragma unroll
    for (int hf = 0; hf < 2; hf++) {
        const u32x4 q = hf ? w.q1 : w.q0;
        const u32x4 blo = q & M, bhi = (q >> 4) & M;  // 16 weights each, one byte per weight, k-slot j = byte j
        dlo = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[0 * 2 + hf], __builtin_bit_cast(i32x4, blo), dlo, 0, 0, 0);
        dhi = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[1 * 2 + hf], __builtin_bit_cast(i32x4, bhi), dhi, 0, 0, 0);
    }
    // scale and min of sub-blocks 2G and 2G+1
    const float d = h2f_lo(w.hdr[0]), dmin = h2f_hi(w.hdr[0]);
    float scv[2], mv[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        uint32_t sc, mn;
        k4_scale_min(w.hdr, 2 * g + h, sc, mn);
        scv[h] = d * (float)sc;
        mv[h] = dmin * (float)mn;
    }
    // three signed base-256 digits of the fixed-point activations: sum q*x' = S0 + 256*S1 + 65536*S2 (integers, exact)
    const float vlo = fmaf((float)dlo[2], 65536.0f, fmaf((float)dlo[1], 256.0f, (float)dlo[0]));
    const float vhi = fmaf((float)dhi[2], 65536.0f, fmaf((float)dhi[1], 256.0f, (float)dhi[0]));
    float a = scv[0] * vlo;
    a = fmaf(-mv[0], sums[0], a);
    a = fmaf(scv[1], vhi, a);
    a = fmaf(-mv[1], sums[1], a);
    return a;
}

// One step of a wave on a Q4_0 T16 tensor: the quants (2 x 1 KiB: q{h} = the 16 qs bytes of the lane's 32-block 2G + h) and the d of
// the 16 rows (256 B); a lane of group G takes dword G of its row's d: d of 32-block 2G in the low half, of 2G + 1 in the high half
// (9 VGPRs per step).
__device__ __forceinline__ Q40T q40t_load_raw(const uint8_t *base, uint64_t n_tiles, uint32_t NB, uint32_t tile, uint32_t blk, uint32_t lane)
{
    const uint64_t tb = t16_tb(tile, NB, blk), nblk = t16_nblk(n_tiles, NB);
    Q40T r;
    r.q0 = load_nt16(t16_q40_qs(base, tb) + lane * 16);
    r.q1 = load_nt16(t16_q40_qs(base, tb) + 1024 + lane * 16);
    r.d = __builtin_nontemporal_load((const GLOBAL_AS uint32_t *)(t16_q40_d(base, nblk, tb) + (lane & 15) * 16 + (lane >> 4) * 4));
    return r;
}

__device__ __forceinline__ Q40T q40t_load(const KqmParams &p, uint32_t seg, uint32_t tile, uint32_t blk, uint32_t lane)
{
    return q40t_load_raw(p.W[seg], p.seg_tiles[seg], p.NB, tile, blk, lane);
}

// 64 weights of one lane (32-blocks 2G: q0, 2G+1: q1) against the activations staged as for Q4_K.  The low nibbles of q{h} are weights
// 0..15 of 32-block 2G + h (A-fragment slot 2h), the high nibbles weights 16..31 (slot 2h + 1): both halves of a 32-block accumulate
// into ONE int32 accumulator, the block has one d.  The -8 of ggml's d * (q - 8) goes through the sum of x' over the block, as the mins
// of Q4_K do: d * sum q x' - 8 d * sum x' (8 d is exact in fp32).  sums = {SX[2G], SX[2G+1]} of this super-block.
__device__ __forceinline__ float q40t_dot(const Q40T &w, const i32x4 (&af)[4], f32x2 sums)
{
    constexpr uint32_t M = 0x0F0F0F0Fu;
    i32x4 d0 = {0, 0, 0, 0}, d1 = {0, 0, 0, 0};
    d0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[0], __builtin_bit_cast(i32x4, w.q0 & M), d0, 0, 0, 0);
    d1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[2], __builtin_bit_cast(i32x4, w.q1 & M), d1, 0, 0, 0);
    d0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[1], __builtin_bit_cast(i32x4, (w.q0 >> 4) & M), d0, 0, 0, 0);
    d1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[3], __builtin_bit_cast(i32x4, (w.q1 >> 4) & M), d1, 0, 0, 0);
    const float da = h2f_lo(w.d), db = h2f_hi(w.d);
    // three signed base-256 digits of the fixed-point activations: sum q*x' = S0 + 256*S1 + 65536*S2 (integers, exact)
    const float v0 = fmaf((float)d0[2], 65536.0f, fmaf((float)d0[1], 256.0f, (float)d0[0]));
    const float v1 = fmaf((float)d1[2], 65536.0f, fmaf((float)d1[1], 256.0f, (float)d1[0]));
    float a = da * v0;
    a = fmaf(-(da * 8.0f), sums[0], a);
    a = fmaf(db, v1, a);
    a = fmaf(-(db * 8.0f), sums[1], a);
    return a;
}

// One step of a wave on a Q5_K T16 tensor: the Q4_K planes (low nibbles, headers) plus the high-bit plane, 8 bytes per lane: one
// contiguous 512-byte load per wave (14 VGPRs per step).
__device__ __forceinline__ Q5T q5t_load_raw(const uint8_t *base, uint64_t n_tiles, uint32_t NB, uint32_t tile, uint32_t blk, uint32_t lane)
{
    const uint64_t tb = t16_tb(tile, NB, blk), nblk = t16_nblk(n_tiles, NB);
    Q5T r;
    r.q0 = load_nt16(t16_k4_qs(base, tb) + lane * 16);
    r.q1 = load_nt16(t16_k4_qs(base, tb) + 1024 + lane * 16);
    r.hdr = load_nt16(t16_k4_hdr(base, nblk, tb) + (lane & 15) * 16);
    r.qh = __builtin_nontemporal_load((const GLOBAL_AS u32x2 *)(t16_q5k_qh(base, nblk, tb) + lane * 8));
    return r;
}

__device__ __forceinline__ Q5T q5t_load(const KqmParams &p, uint32_t seg, uint32_t tile, uint32_t blk, uint32_t lane)
{
    return q5t_load_raw(p.W[seg], p.seg_tiles[seg], p.NB, tile, blk, lane);
}

// q4t_dot with the fifth bit of every weight: q = nibble | bit << 4 (0..31, still a non-negative byte operand).  Word hf of w.qh holds
// the bits of the 32 weights of q{hf}: weight byte b of dword i at bit 8b + i (low nibbles, sub-block 2G) and 8b + 4 + i (high nibbles,
// sub-block 2G+1), so each dword of four weights takes one shift and one v_and_or_b32 onto its masked nibbles.
__device__ __forceinline__ float q5t_dot(const Q5T &w, const i32x4 (&af)[4], f32x2 sums, uint32_t g)
{
    constexpr uint32_t M = 0x0F0F0F0Fu, B = 0x10101010u;
    i32x4 dlo = {0, 0, 0, 0}, dhi = {0, 0, 0, 0};
#pragma unroll
    for (int hf = 0; hf < 2; hf++) {
        const u32x4 q = hf ? w.q1 : w.q0;
        const uint32_t h = w.qh[hf];
        u32x4 blo, bhi;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            blo[i] = and_or(h << (4 - i), B, q[i] & M);
            bhi[i] = and_or(h >> i, B, (q[i] >> 4) & M);
        }
        dlo = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[0 * 2 + hf], __builtin_bit_cast(i32x4, blo), dlo, 0, 0, 0);
        dhi = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[1 * 2 + hf], __builtin_bit_cast(i32x4, bhi), dhi, 0, 0, 0);
    }
    // the Q4_K epilogue: scale and min of sub-blocks 2G and 2G+1, d * sc * sum q x' - dmin * m * sum x'
    const float d = h2f_lo(w.hdr[0]), dmin = h2f_hi(w.hdr[0]);
    float scv[2], mv[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        uint32_t sc, mn;
        k4_scale_min(w.hdr, 2 * g + h, sc, mn);
        scv[h] = d * (float)sc;
        mv[h] = dmin * (float)mn;
    }
    const float vlo = fmaf((float)dlo[2], 65536.0f, fmaf((float)dlo[1], 256.0f, (float)dlo[0]));
    const float vhi = fmaf((float)dhi[2], 65536.0f, fmaf((float)dhi[1], 256.0f, (float)dhi[0]));
    float a = scv[0] * vlo;
    a = fmaf(-mv[0], sums[0], a);
    a = fmaf(scv[1], vhi, a);
    a = fmaf(-mv[1], sums[1], a);
    return a;
}

// One step of a wave on a Q6_K T16 tensor: the three quant pieces (3 x 1 KiB), the 16 rows' scales (256 B) and d (32 B) of tile-block tb.
__device__ __forceinline__ Q6T q6t_load_at(const uint8_t *base, uint64_t nblk, uint64_t tb, uint32_t lane)
{
    Q6T r;
    r.qla = load_nt16(t16_q6k_q(base, tb) + lane * 16);
    r.qlb = load_nt16(t16_q6k_q(base, tb) + 1024 + lane * 16);
    r.qh = load_nt16(t16_q6k_q(base, tb) + 2048 + lane * 16);
    r.sc = load_nt16(t16_q6k_sc(base, nblk, tb) + (lane & 15) * 16);
    r.d = *reinterpret_cast<const GLOBAL_AS uint16_t *>(t16_q6k_d((const GLOBAL_AS uint8_t *)base, nblk, tb) + (lane & 15) * 2);
    return r;
}

__device__ __forceinline__ Q6T q6t_load_raw(const uint8_t *base, uint64_t n_tiles, uint32_t NB, uint32_t tile, uint32_t blk, uint32_t lane)
{
    const uint64_t tb = t16_tb(tile, NB, blk), nblk = t16_nblk(n_tiles, NB);
    return q6t_load_at(base, nblk, tb, lane);
}

// (the tensor's pointer is fetched last, as this kernel family was tuned: k_gemv_kqt's schedule follows the order of these argument reads)
__device__ __forceinline__ Q6T q6t_load(const KqmParams &p, uint32_t seg, uint32_t tile, uint32_t blk, uint32_t lane)
{
    const uint64_t tb = t16_tb(tile, p.NB, blk), nblk = t16_nblk(p.seg_tiles[seg], p.NB);
    return q6t_load_at(p.W[seg], nblk, tb, lane);
}

// 64 weights of one lane: half n = G>>1 of the super-block, columns l = 16*(G&1) .. +15 of all four quarters
// (ggml dequantize_row_q6_K: quarter 0/2 = low/high nibbles of ql[l], quarter 1/3 = of ql[l+32], bits 2q..2q+1 of qh[l]);
// one MFMA per quarter = one 16-weight scale group.  sums = sum of x' over each of the four groups.
__device__ __forceinline__ float q6t_dot(const Q6T &w, const i32x4 (&af)[4], f32x4 sums, uint32_t g)
{
    constexpr uint32_t M4 = 0x0F0F0F0Fu, M2 = 0x30303030u;
    const float d = h2f_lo(w.d);
    float tot = 0.f;
#pragma unroll
    for (int qd = 0; qd < 4; qd++) {
        const u32x4 ql = (qd & 1) ? w.qlb : w.qla;
        const u32x4 lo4 = (qd >= 2) ? ((ql >> 4) & M4) : (ql & M4);
        const u32x4 hs = qd == 0 ? (w.qh << 4) : (qd == 1 ? (w.qh << 2) : (qd == 2 ? w.qh : (w.qh >> 2)));
        const u32x4 b = (hs & M2) | lo4;  // unsigned 6-bit value per byte
        const i32x4 dq = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[qd], __builtin_bit_cast(i32x4, b), i32x4{0, 0, 0, 0}, 0, 0, 0);
        const float v = fmaf((float)dq[2], 65536.0f, fmaf((float)dq[1], 256.0f, (float)dq[0]));
        // scales[8n + (G&1) + 2*qd] of the row
        const uint32_t si = 8 * (g >> 1) + (g & 1) + 2 * qd;
        const uint32_t sw = si < 8 ? (si < 4 ? w.sc[0] : w.sc[1]) : (si < 12 ? w.sc[2] : w.sc[3]);
        const int sc = (int)(int8_t)((sw >> ((si & 3) * 8)) & 0xFFu);
        tot = fmaf((float)sc, fmaf(-32.0f, sums[qd], v), tot);
    }
    return d * tot;
}

// One step of a wave on a Q3_K T16 tensor: the low bits (1 KiB), the high bits (512 B), the 16 rows' scale bytes (192 B) and d (32 B) of
// tile-block tb: 1760 bytes, 10 VGPRs per step.
__device__ __forceinline__ Q3T q3t_load_raw(const uint8_t *base, uint64_t n_tiles, uint32_t NB, uint32_t tile, uint32_t blk, uint32_t lane)
{
    const uint64_t tb = t16_tb(tile, NB, blk), nblk = t16_nblk(n_tiles, NB);
    Q3T r;
    r.q = load_nt16(t16_q3k_qs(base, tb) + lane * 16);
    r.h = __builtin_nontemporal_load((const GLOBAL_AS u32x2 *)(t16_q3k_hm(base, nblk, tb) + lane * 8));
    const GLOBAL_AS uint32_t *sc = (const GLOBAL_AS uint32_t *)(t16_q3k_sc(base, nblk, tb) + (lane & 15) * 12);
    r.s0 = __builtin_nontemporal_load(sc);
    r.s1 = __builtin_nontemporal_load(sc + 1);
    r.s2 = __builtin_nontemporal_load(sc + 2);
    r.d = *reinterpret_cast<const GLOBAL_AS uint16_t *>(t16_q3k_d((const GLOBAL_AS uint8_t *)base, nblk, tb) + (lane & 15) * 2);
    return r;
}

__device__ __forceinline__ Q3T q3t_load(const KqmParams &p, uint32_t seg, uint32_t tile, uint32_t blk, uint32_t lane)
{
    return q3t_load_raw(p.W[seg], p.seg_tiles[seg], p.NB, tile, blk, lane);
}

// The B operand of quarter qd of a Q3_K step, one unsigned byte q + BIAS per weight (q = low two bits | high bit << 2, 0..7): dword i takes
// its low bits with one shift and mask of w.q[i], its four high bits with one shift of word i >> 1 of w.h (bit 8b + 4 (i & 1) + qd -> 8b + 2)
// and one v_and_or_b32.  BIAS (a byte value, no carry: q + BIAS < 256) is added per dword when not zero.
template <uint32_t BIAS>
__device__ __forceinline__ i32x4 q3t_operand(const Q3T &w, int qd)
{
    constexpr uint32_t M2 = 0x03030303u, B = 0x04040404u;
    u32x4 b;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t h = w.h[i >> 1];
        const int c = 4 * (i & 1) + qd;  // the bit's place in each byte of h
        b[i] = and_or(c >= 2 ? h >> (c - 2) : h << (2 - c), B, (w.q[i] >> (2 * qd)) & M2);
        if constexpr (BIAS != 0) b[i] += BIAS * 0x01010101u;
    }
    return __builtin_bit_cast(i32x4, b);
}

// 64 weights of one lane: Q6_K's ownership (half n = G>>1 of the super-block, columns l = 16*(G&1) .. +15 of all four quarters), so the
// activations are Q6_K's A fragments and per-16 sums of x' (kqm_stage<HAS6>); one MFMA per quarter = one 16-weight scale group on
// unsigned 3-bit byte operands.  Weight = d * (sc - 32) * (q - 4): the -4 goes through the group's sum of x', the 6-bit scale
// (q3k_scale) is applied as an integer-valued float, d last: d * sum (sc - 32) * (v - 4 * sums[qd]).
__device__ __forceinline__ float q3t_dot(const Q3T &w, const i32x4 (&af)[4], f32x4 sums, uint32_t g)
{
    const float d = h2f_lo(w.d);
    float tot = 0.f;
#pragma unroll
    for (int qd = 0; qd < 4; qd++) {
        const i32x4 dq = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[qd], q3t_operand<0>(w, qd), i32x4{0, 0, 0, 0}, 0, 0, 0);
        const float v = fmaf((float)dq[2], 65536.0f, fmaf((float)dq[1], 256.0f, (float)dq[0]));
        const int sc = q3k_scale(w.s0, w.s1, w.s2, 8 * (g >> 1) + (g & 1) + 2 * qd) - 32;  // scale[8n + 2 qd + lh] of the row
        tot = fmaf((float)sc, fmaf(-4.0f, sums[qd], v), tot);
    }
    return d * tot;
}

// One step of a wave on an IQ4_XS T16 tensor: the codes (2 x 1 KiB: q{h} = the 16 qs bytes of the lane's sub-block 2G + h, Q4_0's plane)
// and the 8-byte headers of the 16 rows (128 B): d | scales_h in hdr[0], scales_l[4] in hdr[1].  2176 bytes, 10 VGPRs per step.
__device__ __forceinline__ IQ4T iq4t_load_raw(const uint8_t *base, uint64_t n_tiles, uint32_t NB, uint32_t tile, uint32_t blk, uint32_t lane)
{
    const uint64_t tb = t16_tb(tile, NB, blk), nblk = t16_nblk(n_tiles, NB);
    IQ4T r;
    r.q0 = load_nt16(t16_iq4_qs(base, tb) + lane * 16);
    r.q1 = load_nt16(t16_iq4_qs(base, tb) + 1024 + lane * 16);
    r.hdr = __builtin_nontemporal_load((const GLOBAL_AS u32x2 *)(t16_iq4_hdr(base, nblk, tb) + (lane & 15) * 8));
    return r;
}

__device__ __forceinline__ IQ4T iq4t_load(const KqmParams &p, uint32_t seg, uint32_t tile, uint32_t blk, uint32_t lane)
{
    return iq4t_load_raw(p.W[seg], p.seg_tiles[seg], p.NB, tile, blk, lane);
}

// The B operand of the low (HI = false) or high nibbles of 16 code bytes: one signed table byte per weight (iq4_lut4: the codebook
// lookup in registers, 7 VALU operations per dword of low nibbles, 8 of high ones (one more shift): 120 per step, where Q4_0's
// nibble masks take 24).
template <bool HI>
__device__ __forceinline__ i32x4 iq4t_operand(const u32x4 q)
{
    u32x4 b;
#pragma unroll
    for (int i = 0; i < 4; i++) b[i] = iq4_lut4(HI ? q[i] >> 4 : q[i]);
    return __builtin_bit_cast(i32x4, b);
}

// The fp32 scales d * (ls - 32) of the lane's sub-blocks 2G and 2G+1 (the product rounded to fp32, as the format writes dl).
__device__ __forceinline__ void iq4t_scales(const IQ4T &w, uint32_t g, float &da, float &db)
{
    const float d = h2f_lo(w.hdr[0]);
    da = d * (float)(iq4xs_scale(w.hdr[0], w.hdr[1], 2 * g) - 32);
    db = d * (float)(iq4xs_scale(w.hdr[0], w.hdr[1], 2 * g + 1) - 32);
}

// 64 weights of one lane (sub-blocks 2G: q0, 2G+1: q1) against the activations staged as for Q4_K: Q4_0's four MFMAs (the low nibbles
// of q{h} are weights 0..15 of sub-block 2G + h, A-fragment slot 2h, the high nibbles weights 16..31, slot 2h + 1; both halves of a
// sub-block accumulate into ONE int32 accumulator) on the table values of the codes: signed bytes -127 .. 113, as Q8_0's operands
// are (32 x 127 x 128 per accumulator at the most).  No offset and no min, so no term in the sums of x'.
__device__ __forceinline__ float iq4t_dot(const IQ4T &w, const i32x4 (&af)[4], uint32_t g)
{
    i32x4 d0 = {0, 0, 0, 0}, d1 = {0, 0, 0, 0};
    d0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[0], iq4t_operand<false>(w.q0), d0, 0, 0, 0);
    d1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[2], iq4t_operand<false>(w.q1), d1, 0, 0, 0);
    d0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[1], iq4t_operand<true>(w.q0), d0, 0, 0, 0);
    d1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[3], iq4t_operand<true>(w.q1), d1, 0, 0, 0);
    float da, db;
    iq4t_scales(w, g, da, db);
    // three signed base-256 digits of the fixed-point activations: sum q*x' = S0 + 256*S1 + 65536*S2 (integers, exact)
    const float v0 = fmaf((float)d0[2], 65536.0f, fmaf((float)d0[1], 256.0f, (float)d0[0]));
    const float v1 = fmaf((float)d1[2], 65536.0f, fmaf((float)d1[1], 256.0f, (float)d1[0]));
    return fmaf(db, v1, da * v0);
}

// ---- a step against several activation vectors (the batched decode): unpack once, then one dot per column ------------------------------
// The part of q4t_dot / q5t_dot / q6t_dot / q8t_dot / q40t_dot / q3t_dot / iq4t_dot that does not depend on x, done once per step: the four B operands (one byte per
// weight) and the scales.
struct KqmW4 { i32x4 b[4]; float scv[2], mv[2]; };   // b[2n + hf]: low (n = 0) / high (n = 1) nibbles of q{hf}, the slot order of the A fragments
struct KqmW6 { i32x4 b[4]; float sc[4]; float d; };  // b[qd], scales[8n + (G&1) + 2 qd] as floats

__device__ __forceinline__ KqmW4 kqm_unpack(const Q4T &w, uint32_t g)
{
    constexpr uint32_t M = 0x0F0F0F0Fu;
    KqmW4 u;
    u.b[0] = __builtin_bit_cast(i32x4, w.q0 & M);
    u.b[1] = __builtin_bit_cast(i32x4, w.q1 & M);
    u.b[2] = __builtin_bit_cast(i32x4, (w.q0 >> 4) & M);
    u.b[3] = __builtin_bit_cast(i32x4, (w.q1 >> 4) & M);
    // scale and min of sub-blocks 2G and 2G+1
    const float d = h2f_lo(w.hdr[0]), dmin = h2f_hi(w.hdr[0]);
#pragma unroll
    for (int h = 0; h < 2; h++) {
        uint32_t sc, mn;
        k4_scale_min(w.hdr, 2 * g + h, sc, mn);
        u.scv[h] = d * (float)sc;
        u.mv[h] = dmin * (float)mn;
    }
    return u;
}

__device__ __forceinline__ KqmW6 kqm_unpack(const Q6T &w, uint32_t g)
{
    constexpr uint32_t M4 = 0x0F0F0F0Fu, M2 = 0x30303030u;
    KqmW6 u;
    u.d = h2f_lo(w.d);
#pragma unroll
    for (int qd = 0; qd < 4; qd++) {
        const u32x4 ql = (qd & 1) ? w.qlb : w.qla;
        const u32x4 lo4 = (qd >= 2) ? ((ql >> 4) & M4) : (ql & M4);
        const u32x4 hs = qd == 0 ? (w.qh << 4) : (qd == 1 ? (w.qh << 2) : (qd == 2 ? w.qh : (w.qh >> 2)));
        u.b[qd] = __builtin_bit_cast(i32x4, (hs & M2) | lo4);  // unsigned 6-bit value per byte
        const uint32_t si = 8 * (g >> 1) + (g & 1) + 2 * qd;
        const uint32_t sw = si < 8 ? (si < 4 ? w.sc[0] : w.sc[1]) : (si < 12 ? w.sc[2] : w.sc[3]);
        u.sc[qd] = (float)(int)(int8_t)((sw >> ((si & 3) * 8)) & 0xFFu);
    }
    return u;
}

// Q3_K: the operand of Q6_K's columns.  The bytes carry q + 28 (28..35, still an unsigned 6-bit value), so that the -32 of
// kqm_dot(KqmW6) leaves q - 4: no offset field in KqmW6, and Q6_K's column dot is untouched.  sc[qd] = scale - 32 as a float.
__device__ __forceinline__ KqmW6 kqm_unpack(const Q3T &w, uint32_t g)
{
    KqmW6 u;
    u.d = h2f_lo(w.d);
#pragma unroll
    for (int qd = 0; qd < 4; qd++) {
        u.b[qd] = q3t_operand<28>(w, qd);
        u.sc[qd] = (float)(q3k_scale(w.s0, w.s1, w.s2, 8 * (g >> 1) + (g & 1) + 2 * qd) - 32);
    }
    return u;
}

// Q5_K: the nibbles of q4t with the fifth bit merged in as q5t_dot does (q = nibble | bit << 4, a non-negative byte operand), once
// per step; scales and mins are Q4_K's, so the columns run kqm_dot(KqmW4) unchanged.
__device__ __forceinline__ KqmW4 kqm_unpack(const Q5T &w, uint32_t g)
{
    constexpr uint32_t M = 0x0F0F0F0Fu, B = 0x10101010u;
    KqmW4 u;
#pragma unroll
    for (int hf = 0; hf < 2; hf++) {
        const u32x4 q = hf ? w.q1 : w.q0;
        const uint32_t h = w.qh[hf];
        u32x4 blo, bhi;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            blo[i] = and_or(h << (4 - i), B, q[i] & M);
            bhi[i] = and_or(h >> i, B, (q[i] >> 4) & M);
        }
        u.b[hf] = __builtin_bit_cast(i32x4, blo);
        u.b[2 + hf] = __builtin_bit_cast(i32x4, bhi);
    }
    const float d = h2f_lo(w.hdr[0]), dmin = h2f_hi(w.hdr[0]);
#pragma unroll
    for (int h = 0; h < 2; h++) {
        uint32_t sc, mn;
        k4_scale_min(w.hdr, 2 * g + h, sc, mn);
        u.scv[h] = d * (float)sc;
        u.mv[h] = dmin * (float)mn;
    }
    return u;
}

// Q4_0: the operand of Q4_K's columns.  b[] in the slot order of the Q4_K staging (slot 2h = low, 2h + 1 = high nibbles of q{h}), so
// kqm_dot(KqmW4) sums slots 0, 1 (32-block 2G) and 2, 3 (32-block 2G+1); scale d, "min" 8 d: the arithmetic of q40t_dot.
__device__ __forceinline__ KqmW4 kqm_unpack(const Q40T &w, uint32_t)
{
    constexpr uint32_t M = 0x0F0F0F0Fu;
    KqmW4 u;
    u.b[0] = __builtin_bit_cast(i32x4, w.q0 & M);
    u.b[1] = __builtin_bit_cast(i32x4, (w.q0 >> 4) & M);
    u.b[2] = __builtin_bit_cast(i32x4, w.q1 & M);
    u.b[3] = __builtin_bit_cast(i32x4, (w.q1 >> 4) & M);
    u.scv[0] = h2f_lo(w.d);
    u.scv[1] = h2f_hi(w.d);
    u.mv[0] = u.scv[0] * 8.0f;
    u.mv[1] = u.scv[1] * 8.0f;
    return u;
}

// IQ4_XS: the operand of Q4_K's columns, in Q4_0's slot order.  b[] carries the table values of the codes (signed bytes, looked up once
// per step for all columns), scv the two d * (ls - 32); there is no offset and no min: mv = 0, so kqm_dot(KqmW4) adds -0 * sums (nothing)
// and is untouched.
__device__ __forceinline__ KqmW4 kqm_unpack(const IQ4T &w, uint32_t g)
{
    KqmW4 u;
    u.b[0] = iq4t_operand<false>(w.q0);
    u.b[1] = iq4t_operand<true>(w.q0);
    u.b[2] = iq4t_operand<false>(w.q1);
    u.b[3] = iq4t_operand<true>(w.q1);
    iq4t_scales(w, g, u.scv[0], u.scv[1]);
    u.mv[0] = 0.f;
    u.mv[1] = 0.f;
    return u;
}

// Q8_0: the quants are the B operands as loaded (signed bytes); d of the lane's four 32-blocks 2h + (G >> 1) widened once.
struct KqmW8 { i32x4 b[4]; float d[4]; };

__device__ __forceinline__ KqmW8 kqm_unpack(const Q8T &w, uint32_t)
{
    KqmW8 u;
#pragma unroll
    for (int h = 0; h < 4; h++) {
        u.b[h] = __builtin_bit_cast(i32x4, w.q[h]);
        u.d[h] = (h & 1) ? h2f_hi(w.d[h >> 1]) : h2f_lo(w.d[h >> 1]);
    }
    return u;
}

// 64 weights of one lane against one column: the arithmetic of q4t_dot / q6t_dot / q8t_dot on the unpacked operand
__device__ __forceinline__ float kqm_dot(const KqmW4 &u, const i32x4 (&af)[4], f32x4 sums)
{
    i32x4 dlo = {0, 0, 0, 0}, dhi = {0, 0, 0, 0};
    dlo = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[0], u.b[0], dlo, 0, 0, 0);
    dhi = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[2], u.b[2], dhi, 0, 0, 0);
    dlo = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[1], u.b[1], dlo, 0, 0, 0);
    dhi = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[3], u.b[3], dhi, 0, 0, 0);
    // three signed base-256 digits of the fixed-point activations: sum q*x' = S0 + 256*S1 + 65536*S2 (integers, exact)
    const float vlo = fmaf((float)dlo[2], 65536.0f, fmaf((float)dlo[1], 256.0f, (float)dlo[0]));
    const float vhi = fmaf((float)dhi[2], 65536.0f, fmaf((float)dhi[1], 256.0f, (float)dhi[0]));
    float a = u.scv[0] * vlo;
    a = fmaf(-u.mv[0], sums[0], a);
    a = fmaf(u.scv[1], vhi, a);
    a = fmaf(-u.mv[1], sums[1], a);
    return a;
}

__device__ __forceinline__ float kqm_dot(const KqmW6 &u, const i32x4 (&af)[4], f32x4 sums)
{
    float tot = 0.f;
#pragma unroll
    for (int qd = 0; qd < 4; qd++) {
        const i32x4 dq = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[qd], u.b[qd], i32x4{0, 0, 0, 0}, 0, 0, 0);
        const float v = fmaf((float)dq[2], 65536.0f, fmaf((float)dq[1], 256.0f, (float)dq[0]));
        tot = fmaf(u.sc[qd], fmaf(-32.0f, sums[qd], v), tot);
    }
    return u.d * tot;
}

// (Q8_0 has no offset and no min: the sums of x' go unused)
__device__ __forceinline__ float kqm_dot(const KqmW8 &u, const i32x4 (&af)[4], f32x4)
{
    float a = 0.f;
#pragma unroll
    for (int h = 0; h < 4; h++) {
        const i32x4 dq = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[h], u.b[h], i32x4{0, 0, 0, 0}, 0, 0, 0);
        const float v = fmaf((float)dq[2], 65536.0f, fmaf((float)dq[1], 256.0f, (float)dq[0]));
        a = fmaf(u.d[h], v, a);
    }
    return a;
}

// Fixed-point staging of ONE 256-element super-block of the activation vector by one wave (lane holds elements 4*lane .. +3, after the
// optional RMSNorm): power-of-two scale so that |x * 2^S| < 2^22, three signed base-256 digits per element written as MFMA A
// fragments [blk][slot:4][G][digit][16 B] (Q4_K / Q5_K / Q4_0 / IQ4_XS layout in xa, Q6_K / Q3_K layout in xa6, Q8_0 layout in xa), the sums of x' per scale group
// (K-quants and Q4_0 only; IQ4_XS reads none) and the exponent S (sexp[blk]; the consumer applies ldexpf(partial, -S)).  Nothing written here is read by another wave.
// S = 21 - ilogb(max|x|) for every finite non-zero maximum, fp32 subnormals (S up to 170) to FLT_MAX (S = -106) alike, and x is scaled
// with ldexpf on the value, so neither 2^S nor 2^-S is ever formed as a float: every finite super-block keeps 22+ bits of its maximum.
// An all-zero super-block stages zeros (S = 0).  Non-finite x is not supported: Inf / NaN in a super-block make its digits and sums
// meaningless (the float -> int conversion of a non-finite value), and the launch's outputs with them.
template <bool HAS4, bool HAS6, bool HAS8 = false>
__device__ __forceinline__ void kqm_stage(const f32x4 v, const uint32_t blk, const uint32_t lane, uint8_t *xa, uint8_t *xa6, float *sums,
                                          float *sums6, int *sexp)
{
    const uint32_t k = lane * 4;  // position inside the super-block
    const float am = wave_max(fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
    const int S = am > 0.f ? 21 - ilogbf(am) : 0;  // |x * 2^S| < 2^22: a 24-bit signed integer after rounding
    if (lane == 0) sexp[blk] = S;
    uint32_t d0 = 0, d1 = 0, d2 = 0;  // digit planes of the four elements, one byte each
    float sx = 0.f;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const float vs = ldexpf(v[e], S);
        const int xi = (int)rintf(vs);
        const int b0 = (int)(int8_t)(xi & 0xFF);
        const int r1 = (xi - b0) >> 8;
        const int b1 = (int)(int8_t)(r1 & 0xFF);
        const int b2 = (r1 - b1) >> 8;
        d0 |= (uint32_t)(b0 & 0xFF) << (8 * e);
        d1 |= (uint32_t)(b1 & 0xFF) << (8 * e);
        d2 |= (uint32_t)(b2 & 0xFF) << (8 * e);
        sx += (float)xi;
    }
    // A fragments [blk][slot:4][G][digit][16 bytes]; a lane reads slot s at +256*s from its (G, digit) base.
    //   Q4_K: k = (2G+n)*32 + hf*16 + j, slot = 2n + hf, sums per sub-block of 32 -> [blk][G][n]
    //   Q6_K, Q3_K: k = n*128 + qd*32 + lh*16 + j, G = 2n + lh, slot = qd, sums per group of 16 -> [blk][G][qd]
    //   Q8_0: k = 64*slot + 16G + j, no sums
    const uint32_t j = k & 15;
    // sums over aligned groups of 4 lanes (16 elements) and of 8 lanes (32 elements)
    sx += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, sx), 0xB1, 0xF, 0xF, true));
    sx += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, sx), 0x4E, 0xF, 0xF, true));
    const float sx16 = sx;
    const float sx32 = sx + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, sx), 0x141, 0xF, 0xF, true));
    if constexpr (HAS4) {
        const uint32_t sb = (k >> 5) & 7, hf = (k >> 4) & 1, g = sb >> 1, slot = (sb & 1) * 2 + hf;
        uint8_t *frag = xa + (size_t)blk * 1024 + (slot * 4 + g) * 64 + j;
        *reinterpret_cast<uint32_t *>(frag) = d0;
        *reinterpret_cast<uint32_t *>(frag + 16) = d1;
        *reinterpret_cast<uint32_t *>(frag + 32) = d2;
        if ((lane & 7) == 0) sums[(blk * 4 + g) * 4 + (sb & 1)] = sx32;
    }
    if constexpr (HAS6) {
        const uint32_t g = ((k >> 7) & 1) * 2 + ((k >> 4) & 1), slot = (k >> 5) & 3;
        uint8_t *frag = xa6 + (size_t)blk * 1024 + (slot * 4 + g) * 64 + j;
        *reinterpret_cast<uint32_t *>(frag) = d0;
        *reinterpret_cast<uint32_t *>(frag + 16) = d1;
        *reinterpret_cast<uint32_t *>(frag + 32) = d2;
        if ((lane & 3) == 0) sums6[(blk * 4 + g) * 4 + slot] = sx16;
    }
    if constexpr (HAS8) {
        const uint32_t g = (k >> 4) & 3, slot = k >> 6;
        uint8_t *frag = xa + (size_t)blk * 1024 + (slot * 4 + g) * 64 + j;
        *reinterpret_cast<uint32_t *>(frag) = d0;
        *reinterpret_cast<uint32_t *>(frag + 16) = d1;
        *reinterpret_cast<uint32_t *>(frag + 32) = d2;
    }
}

}  // namespace nfai
