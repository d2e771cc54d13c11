// t16.h — the "T16" layout of ggml IQ4_XS / Q3_K / Q4_0 / Q4_K / Q5_K / Q6_K / Q8_0 tensors in HBM: what it is, where every plane's bytes are, and how a
// block decodes.  The ONE definition: the repack kernels write it, the int8-MFMA GEMVs (kqm.h), the fp16 widening, the dequant-in-LDS
// GEMM and the embedding gather read it, all through the helpers below.  Part of common.h (included there, behind the vector types
// and load helpers it uses): include common.h, never this file alone.
//
// Repacked once at upload, same bytes as the native blocks.  Rows are grouped in tiles of 16; a "super-block" is 256 weights of one
// row (one K-quant or IQ4_XS block, eight Q8_0 or Q4_0 blocks), NB of them per row.  The native block is split into planes, one per field; inside a
// plane the records of (tile, blk) follow each other in the order tb = tile * NB + blk, 16 rows per record:
//   Q4_K: plane 0  [tile][blk][h:2][lane:64][16 B]  lane = G*16 + r holds qs[32G+16h .. +16) of row 16*tile+r,
//                  i.e. lane group G owns sub-blocks 2G (low nibbles) and 2G+1 (high nibbles) of its row;
//         plane 1  [tile][blk][r:16][16 B]          d, dmin, 12 scale bytes of row 16*tile+r.
//   Q5_K: planes 0 and 1 of Q4_K (same bytes: qs and the 16-byte header), and
//         plane 2  [tile][blk][lane:64][8 B]        the 64 fifth bits (qh) of the weights lane (G, r) unpacks, in the order of
//                                                   q5t_dot (kqm.h): one shift and one v_and_or_b32 per four weights.  Word hf of
//                  lane (G, r) holds, for the weights l = 16hf + 4i + b (b = byte of dword i of q{hf}), bit 2G of qh[l] at 8b + i
//                  and bit 2G+1 at 8b + 4 + i.
//   Q6_K: plane 0  [tile][blk][piece:3][lane:64][16 B]  lane = G*16 + r, n = G>>1, lh = G&1:
//                  piece 0 = ql[64n + 16lh ..+16), piece 1 = ql[64n + 32 + 16lh ..+16), piece 2 = qh[32n + 16lh ..+16);
//         plane 1  [tile][blk][r:16][16 B]          the 16 int8 scales;
//         plane 2  [tile][blk][r:16] fp16           d.
//   Q8_0: plane 0  [tile][blk][h:4][lane:64][16 B]  lane = G*16 + r holds qs bytes 64h + 16G .. +16 of super-block blk of
//                  row 16*tile+r: 16 weights of ONE 32-block (2h + (G >> 1)), so one d per lane and MFMA;
//         plane 1  [tile][blk][r:16][16 B]          the eight fp16 d of that row and super-block, d of 32-block b at half
//                                                   (b & 1) * 4 + (b >> 1): lanes of group G read the 8 bytes of their four d.
//   Q4_0: plane 0  [tile][blk][h:2][lane:64][16 B]  lane = G*16 + r holds the 16 qs bytes of native 32-block 2G + h of super-block blk of
//                  row 16*tile+r: its low nibbles are weights 32(2G+h) .. +16, its high nibbles weights 32(2G+h) + 16 .. +16, the
//                  k ranges of A-fragment slots 2h and 2h + 1 of the Q4_K staging (kqm_stage<HAS4>), so lane group G owns
//                  32-blocks 2G and 2G+1 as it owns sub-blocks 2G and 2G+1 of a Q4_K block: Q4_K's register shape per step;
//         plane 1  [tile][blk][r:16][16 B]          the eight fp16 d of that row and super-block in block order: lanes of group G read
//                                                   dword G, the d of their 32-blocks 2G (low half) and 2G+1 (high half).
//   Q3_K: plane 0  [tile][blk][lane:64][16 B]       lane = G*16 + r, n = G>>1, lh = G&1, holds qs[32n + 16lh .. +16) of row 16*tile+r: bits 2j..2j+1
//                  of byte l are the low two bits of weight 128n + 32j + 16lh + l, so ONE load gives the lane all four quarters j of the
//                  64 weights it owns (Q6_K's ownership: group G, A-fragment slot j of kqm_stage<HAS6>);
//         plane 1  [tile][blk][lane:64][8 B]        the 64 high bits (hmask) of exactly those weights, in the order of q3t_dot (kqm.h): one
//                  shift and one v_and_or_b32 per four weights.  Word w of lane (G, r) holds, for the weights l = 8w + 4i2 + b (b = byte of
//                  operand dword i = 2w + i2) of quarter j, bit 4n + j of hmask[16lh + l] at 8b + 4 i2 + j;
//         plane 2  [tile][blk][r:16][12 B]          the 12 scale bytes of row 16*tile+r (sixteen 6-bit scales, q3k_scale);
//         plane 3  [tile][blk][r:16] fp16           d.
//   IQ4_XS: plane 0  [tile][blk][h:2][lane:64][16 B]  Q4_0's plane 0 byte for byte: lane = G*16 + r holds the 16 qs bytes of sub-block 2G + h of
//                  super-block blk of row 16*tile+r (qs[16 (2G+h) .. +16) of the native block): its low nibbles are the codes of weights
//                  32(2G+h) .. +16, its high nibbles of weights 32(2G+h) + 16 .. +16, the k ranges of A-fragment slots 2h and 2h + 1 of the
//                  Q4_K staging (kqm_stage<HAS4>).  A code is an index into the 16-entry table IQ4_KV (iq4_lut4), not a magnitude;
//         plane 1  [tile][blk][r:16][8 B]           the first 8 bytes of the native block of row 16*tile+r: fp16 d | uint16 scales_h |
//                                                   scales_l[4] (eight 6-bit scales ls, iq4xs_scale; the weight's factor is d * (ls - 32)).
// Every wave-wide load is one contiguous kilobyte (quants), 512 bytes (Q5_K / Q3_K high bits), 256 bytes (headers), 192 bytes (Q3_K scales) or
// 128 bytes (IQ4_XS headers).
// (The planar Q6_K layout of kernels_gemv_kq.hip, for row counts that are not a multiple of 16, is another format.)
#pragma once

namespace nfai {

// Bytes per row and super-block of every plane: the native ggml block, split up.
constexpr uint32_t GGML_Q4_K_BLOCK = 144, GGML_Q5_K_BLOCK = 176, GGML_Q6_K_BLOCK = 210, GGML_Q8_0_BLOCK = 34, GGML_Q4_0_BLOCK = 18, GGML_Q3_K_BLOCK = 110, GGML_IQ4_XS_BLOCK = 136;
constexpr uint32_t T16_K4_QS = 128, T16_K4_HDR = 16, T16_Q5K_QH = 32;  // Q4_K / Q5_K: qs | d, dmin, scales[12] | qh
constexpr uint32_t T16_Q6K_Q = 192, T16_Q6K_SC = 16, T16_Q6K_D = 2;    // Q6_K: ql[128] + qh[64] | scales[16] | d
constexpr uint32_t T16_Q80_QS = 256, T16_Q80_D = 16;                   // Q8_0: 8 x qs[32] | 8 x d
constexpr uint32_t T16_Q40_QS = 128, T16_Q40_D = 16;                   // Q4_0: 8 x qs[16] | 8 x d
constexpr uint32_t T16_Q3K_QS = 64, T16_Q3K_HM = 32, T16_Q3K_SC = 12, T16_Q3K_D = 2;  // Q3_K: qs[64] | hmask[32] | scales[12] | d
constexpr uint32_t T16_IQ4_QS = 128, T16_IQ4_HDR = 8;                  // IQ4_XS: qs[128] | d, scales_h, scales_l[4]
static_assert(T16_IQ4_QS + T16_IQ4_HDR == GGML_IQ4_XS_BLOCK, "the T16 planes are the bytes of the native blocks (weight_row_bytes)");
static_assert(T16_Q3K_QS + T16_Q3K_HM + T16_Q3K_SC + T16_Q3K_D == GGML_Q3_K_BLOCK, "the T16 planes are the bytes of the native blocks (weight_row_bytes)");
static_assert(T16_Q40_QS + T16_Q40_D == 8 * GGML_Q4_0_BLOCK, "the T16 planes are the bytes of the native blocks (weight_row_bytes)");
static_assert(T16_K4_QS + T16_K4_HDR == GGML_Q4_K_BLOCK && T16_K4_QS + T16_K4_HDR + T16_Q5K_QH == GGML_Q5_K_BLOCK &&
                  T16_Q6K_Q + T16_Q6K_SC + T16_Q6K_D == GGML_Q6_K_BLOCK && T16_Q80_QS + T16_Q80_D == 8 * GGML_Q8_0_BLOCK,
              "the T16 planes are the bytes of the native blocks (weight_row_bytes)");

// ---- plane addresses: the record of tile-block tb = tile * NB + blk in each plane of the tensor at `base` (P: a byte pointer of any
// address space; nblk = row-blocks of the tensor).  Pointer in, pointer out, one term per step: the address arithmetic the readers
// were written with, so the compiler sees what it saw when the offsets were spelled out in place.
#define T16_ADDR template <class P> __host__ __device__ __forceinline__ P
__host__ __device__ __forceinline__ uint64_t t16_nblk(uint64_t n_tiles, uint32_t NB) { return n_tiles * 16 * NB; }
__host__ __device__ __forceinline__ uint64_t t16_tb(uint64_t tile, uint32_t NB, uint32_t blk) { return tile * NB + blk; }
T16_ADDR t16_k4_qs(P base, uint64_t tb) { return base + tb * (16 * T16_K4_QS); }                                                   // + h * 1024 + lane * 16
T16_ADDR t16_k4_hdr(P base, uint64_t nblk, uint64_t tb) { return base + nblk * T16_K4_QS + tb * (16 * T16_K4_HDR); }               // + r * 16
T16_ADDR t16_q5k_qh(P base, uint64_t nblk, uint64_t tb) { return base + nblk * (T16_K4_QS + T16_K4_HDR) + tb * (16 * T16_Q5K_QH); }  // + lane * 8
T16_ADDR t16_q6k_q(P base, uint64_t tb) { return base + tb * (16 * T16_Q6K_Q); }                                                   // + piece * 1024 + lane * 16
T16_ADDR t16_q6k_sc(P base, uint64_t nblk, uint64_t tb) { return base + nblk * T16_Q6K_Q + tb * (16 * T16_Q6K_SC); }               // + r * 16
T16_ADDR t16_q6k_d(P base, uint64_t nblk, uint64_t tb) { return base + nblk * (T16_Q6K_Q + T16_Q6K_SC) + tb * (16 * T16_Q6K_D); }  // + r * 2
T16_ADDR t16_q80_qs(P base, uint64_t tb) { return base + tb * (16 * T16_Q80_QS); }                                                 // + h * 1024 + lane * 16
T16_ADDR t16_q80_d(P base, uint64_t nblk, uint64_t tb) { return base + nblk * T16_Q80_QS + tb * (16 * T16_Q80_D); }                // + r * 16
T16_ADDR t16_q40_qs(P base, uint64_t tb) { return base + tb * (16 * T16_Q40_QS); }                                                 // + h * 1024 + lane * 16
T16_ADDR t16_q40_d(P base, uint64_t nblk, uint64_t tb) { return base + nblk * T16_Q40_QS + tb * (16 * T16_Q40_D); }                // + r * 16
T16_ADDR t16_q3k_qs(P base, uint64_t tb) { return base + tb * (16 * T16_Q3K_QS); }                                                 // + lane * 16
T16_ADDR t16_q3k_hm(P base, uint64_t nblk, uint64_t tb) { return base + nblk * T16_Q3K_QS + tb * (16 * T16_Q3K_HM); }              // + lane * 8
T16_ADDR t16_q3k_sc(P base, uint64_t nblk, uint64_t tb) { return base + nblk * (T16_Q3K_QS + T16_Q3K_HM) + tb * (16 * T16_Q3K_SC); }  // + r * 12
T16_ADDR t16_q3k_d(P base, uint64_t nblk, uint64_t tb) { return base + nblk * (T16_Q3K_QS + T16_Q3K_HM + T16_Q3K_SC) + tb * (16 * T16_Q3K_D); }  // + r * 2
T16_ADDR t16_iq4_qs(P base, uint64_t tb) { return base + tb * (16 * T16_IQ4_QS); }                                                 // + h * 1024 + lane * 16
T16_ADDR t16_iq4_hdr(P base, uint64_t nblk, uint64_t tb) { return base + nblk * T16_IQ4_QS + tb * (16 * T16_IQ4_HDR); }            // + r * 8
#undef T16_ADDR

// ---- block decode ------------------------------------------------------------------------------------------------------------------
// ggml get_scale_min_k4: the 6-bit scale and min of sub-block sb (0..7) of a Q4_K / Q5_K block, branch-free on the header words
// (hdr[0] = d | dmin, hdr[1..3] = the 12 scale bytes).
__device__ __forceinline__ void k4_scale_min(const u32x4 hdr, uint32_t sb, uint32_t &sc, uint32_t &mn)
{
    const uint32_t sh = (sb & 3) * 8;
    const uint32_t lo8 = (hdr[1] >> sh) & 0xFFu, mid = (hdr[2] >> sh) & 0xFFu, hi8 = (hdr[3] >> sh) & 0xFFu;
    const bool low = sb < 4;
    sc = low ? (lo8 & 63u) : ((hi8 & 0xFu) | ((lo8 >> 6) << 4));
    mn = low ? (mid & 63u) : ((hi8 >> 4) | ((mid >> 6) << 4));
}

// The same on the 12 scale bytes in memory (P: a byte pointer of any address space).
template <class P>
__device__ __forceinline__ void k4_scale_min_bytes(P scales, uint32_t sb, uint32_t &sc, uint32_t &m)
{
    if (sb < 4) { sc = scales[sb] & 63; m = scales[sb + 4] & 63; }
    else { sc = (scales[sb + 4] & 0xF) | ((scales[sb - 4] >> 6) << 4); m = (scales[sb + 4] >> 4) | ((scales[sb] >> 6) << 4); }
}

// Q6_K: the int8 scale of 16-weight group si (0..15) from the four scale words of the block.
__device__ __forceinline__ int q6k_scale(const u32x4 sc, uint32_t si)
{
    const uint32_t sw = si < 8 ? (si < 4 ? sc[0] : sc[1]) : (si < 12 ? sc[2] : sc[3]);
    return (int)(int8_t)((sw >> ((si & 3) * 8)) & 0xFFu);
}

// Q3_K: the 6-bit scale (0..63; the weight's factor is scale - 32) of 16-weight group si (0..15) from the three scale words of the
// block: low nibble = nibble si >> 3 of byte si & 7, high two bits = bits 2 (si >> 2) .. + 1 of byte 8 + (si & 3).
__device__ __forceinline__ int q3k_scale(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t si)
{
    const uint32_t lw = (si & 4) ? s1 : s0;
    const uint32_t lo = (lw >> (8 * (si & 3) + 4 * (si >> 3))) & 0xFu;
    const uint32_t hi = (s2 >> (8 * (si & 3) + 2 * (si >> 2))) & 3u;
    return (int)(lo | (hi << 4));
}

// IQ4_XS: the 6-bit scale ls (0..63; the weight's factor is ls - 32) of sub-block ib (0..7) from the two header words of the block
// (hdr_lo = d | scales_h << 16, hdr_hi = scales_l[4]): low nibble = nibble ib of scales_l, high two bits = bits 2 ib .. + 1 of scales_h.
__device__ __forceinline__ int iq4xs_scale(uint32_t hdr_lo, uint32_t hdr_hi, uint32_t ib)
{
    return (int)(((hdr_hi >> (4 * ib)) & 0xFu) | (((hdr_lo >> (16 + 2 * ib)) & 3u) << 4));
}

// IQ4_XS / IQ4_NL codebook, looked up in registers: four codes (bits 0..3 of each byte of c4; the other bits are ignored) -> their four
// table values as signed bytes.  The table is two register pairs of eight bytes; v_perm_b32 picks entry code & 7 from each, a third
// v_perm_b32 takes byte i from the upper pair's result where bit 3 of code i is set (selector i + 4) and from the lower pair's where
// it is clear (selector i).  As compiled for gfx950: 3 v_perm_b32 + 2 v_and_b32 + v_lshrrev_b32 + v_or_b32 = 7 VALU operations per four
// weights (the selector's and / or stay two instructions: a VOP3 takes one literal), no LDS, no table in memory.
constexpr uint32_t IQ4_KV_0 = 0xBFAD9881u, IQ4_KV_1 = 0xF6EADDCFu;  // -127, -104, -83, -65 | -49, -35, -22, -10
constexpr uint32_t IQ4_KV_2 = 0x26190D01u, IQ4_KV_3 = 0x71594535u;  // 1, 13, 25, 38 | 53, 69, 89, 113
__device__ __forceinline__ uint32_t iq4_lut4(uint32_t c4)
{
    const uint32_t s = c4 & 0x07070707u;
    const uint32_t lo = __builtin_amdgcn_perm(IQ4_KV_1, IQ4_KV_0, s), hi = __builtin_amdgcn_perm(IQ4_KV_3, IQ4_KV_2, s);
    return __builtin_amdgcn_perm(hi, lo, ((c4 >> 1) & 0x04040404u) | 0x03020100u);
}

// Four consecutive elements k .. k+3 (k % 4 == 0) of row `row` of a T16 tensor with E columns and n_rows rows, as fp32: the block
// exactly as ggml dequantises it (d * sc * q - dmin * m; d * sc * (q - 32); d * q; d * (q - 8); (d * (sc - 32)) * (q - 4); (d * (ls - 32)) * KV[q]), products and the difference rounded as written.
__device__ __forceinline__ f32x4 t16_row_load4(const uint8_t *table, int type, uint64_t n_rows, uint64_t row, uint32_t k, uint32_t E)
{
    typedef __attribute__((address_space(1))) uint8_t g8;
    const g8 *t = (const g8 *)table;
    const uint32_t NB = E / 256, blk = k >> 8, kk = k & 255;
    const uint64_t tile = row >> 4, r = row & 15, tb = t16_tb(tile, NB, blk), nblk = n_rows * NB;
    f32x4 out;
    if (type == NFAI_Q8_0_T16) {
        const uint32_t ln = ((kk >> 4) & 3) * 16 + (uint32_t)r;
        const uint32_t q4 = *reinterpret_cast<const __attribute__((address_space(1))) uint32_t *>(t16_q80_qs(t, tb) + (kk >> 6) * 1024 + ln * 16 + (kk & 15));
        const uint32_t b32 = kk >> 5;  // its d: half (b32 & 1) * 4 + (b32 >> 1) of the row's 16 bytes
        const float d = (float)reinterpret_cast<const __attribute__((address_space(1))) _Float16 *>(t16_q80_d(t, nblk, tb) + r * 16)[(b32 & 1) * 4 + (b32 >> 1)];
#pragma unroll
        for (int e = 0; e < 4; e++) out[e] = d * (float)(int8_t)((q4 >> (8 * e)) & 0xFFu);
    } else if (type == NFAI_Q4_0_T16) {
        const uint32_t b32 = kk >> 5, l = kk & 31;  // 32-block b32: lane group b32 >> 1, half b32 & 1; weight l: nibble l >> 4 of qs[l & 15]
        const uint32_t q4 = *reinterpret_cast<const __attribute__((address_space(1))) uint32_t *>(t16_q40_qs(t, tb) + (b32 & 1) * 1024 + ((b32 >> 1) * 16 + r) * 16 + (l & 15));
        const float d = (float)reinterpret_cast<const __attribute__((address_space(1))) _Float16 *>(t16_q40_d(t, nblk, tb) + r * 16)[b32];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t q = (q4 >> (8 * e)) & 0xFFu;
            out[e] = d * (float)((int)((l >> 4) ? (q >> 4) : (q & 0xFu)) - 8);
        }
    } else if (type == NFAI_IQ4_XS_T16) {
        const uint32_t ib = kk >> 5, l = kk & 31;  // sub-block ib: lane group ib >> 1, half ib & 1; weight l: nibble l >> 4 of qs[l & 15]
        const uint32_t q4 = *reinterpret_cast<const __attribute__((address_space(1))) uint32_t *>(t16_iq4_qs(t, tb) + (ib & 1) * 1024 + ((ib >> 1) * 16 + r) * 16 + (l & 15));
        const __attribute__((address_space(1))) uint32_t *hdr = reinterpret_cast<const __attribute__((address_space(1))) uint32_t *>(t16_iq4_hdr(t, nblk, tb) + r * 8);
        const uint32_t h0 = hdr[0], h1 = hdr[1];
        const float dl = h2f_lo(h0) * (float)(iq4xs_scale(h0, h1, ib) - 32);
        const uint32_t v4 = iq4_lut4((l >> 4) ? (q4 >> 4) : q4);
#pragma unroll
        for (int e = 0; e < 4; e++) out[e] = dl * (float)(int8_t)((v4 >> (8 * e)) & 0xFFu);
    } else if (type == NFAI_Q3_K_T16) {
        const uint32_t n = kk >> 7, j = (kk >> 5) & 3, lh = (kk >> 4) & 1, l = kk & 15;  // l % 4 == 0: the four weights are one operand dword
        const uint32_t ln = (n * 2 + lh) * 16 + (uint32_t)r;
        const uint32_t q4 = *reinterpret_cast<const __attribute__((address_space(1))) uint32_t *>(t16_q3k_qs(t, tb) + ln * 16 + l);
        const uint32_t h4 = *reinterpret_cast<const __attribute__((address_space(1))) uint32_t *>(t16_q3k_hm(t, nblk, tb) + ln * 8 + (l >> 3) * 4) >>
                            (4 * ((l >> 2) & 1) + j);  // the high bits of the four weights at bits 8e
        const g8 *scb = t16_q3k_sc(t, nblk, tb) + r * 12;
        const uint32_t si = 8 * n + 2 * j + lh;  // the scale as q3k_scale forms it, on the two bytes that hold it
        const int sc = (int)(((scb[si & 7] >> (4 * (si >> 3))) & 0xFu) | (((scb[8 + (si & 3)] >> (2 * (si >> 2))) & 3u) << 4));
        const float d = (float)reinterpret_cast<const __attribute__((address_space(1))) _Float16 *>(t16_q3k_d(t, nblk, tb))[r];
        const float dl = d * (float)(sc - 32);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int q = (int)(((q4 >> (8 * e + 2 * j)) & 3u) | (((h4 >> (8 * e)) & 1u) << 2)) - 4;
            out[e] = dl * (float)q;
        }
    } else if (type == NFAI_Q4_K_T16 || type == NFAI_Q5_K_T16) {
        const uint32_t sb = kk >> 5, l = kk & 31;
        const g8 *hdr = t16_k4_hdr(t, nblk, tb) + r * 16;
        const float d = (float)*reinterpret_cast<const __attribute__((address_space(1))) _Float16 *>(hdr);
        const float dmin = (float)*reinterpret_cast<const __attribute__((address_space(1))) _Float16 *>(hdr + 2);
        uint32_t sc, m;
        k4_scale_min_bytes(hdr + 4, sb, sc, m);
        const uint32_t q4 = *reinterpret_cast<const __attribute__((address_space(1))) uint32_t *>(t16_k4_qs(t, tb) + (l >> 4) * 1024 + ((sb >> 1) * 16 + r) * 16 + (l & 15));
        uint32_t h5 = 0;  // Q5_K: the fifth bits of the four weights at bits 8e of h5
        if (type == NFAI_Q5_K_T16)
            h5 = *reinterpret_cast<const __attribute__((address_space(1))) uint32_t *>(t16_q5k_qh(t, nblk, tb) + ((sb >> 1) * 16 + r) * 8 + (l >> 4) * 4) >>
                 (4 * (sb & 1) + ((l >> 2) & 3));
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t q = (q4 >> (8 * e)) & 0xFFu;
            const uint32_t q5 = ((sb & 1) ? (q >> 4) : (q & 0xF)) | (((h5 >> (8 * e)) & 1u) << 4);
            out[e] = d * (float)sc * (float)q5 - dmin * (float)m;
        }
    } else {  // NFAI_Q6_K_T16
        const uint32_t n = kk >> 7, qd = (kk >> 5) & 3, l = kk & 31, lh = l >> 4, b = l & 15;
        const uint32_t ln = (n * 2 + lh) * 16 + (uint32_t)r;
        const uint32_t ql4 = *reinterpret_cast<const __attribute__((address_space(1))) uint32_t *>(t16_q6k_q(t, tb) + (qd & 1) * 1024 + ln * 16 + b);
        const uint32_t qh4 = *reinterpret_cast<const __attribute__((address_space(1))) uint32_t *>(t16_q6k_q(t, tb) + 2048 + ln * 16 + b);
        const int sc = (int)(int8_t)t16_q6k_sc(t, nblk, tb)[r * 16 + 8 * n + lh + 2 * qd];
        const float d = (float)reinterpret_cast<const __attribute__((address_space(1))) _Float16 *>(t16_q6k_d(t, nblk, tb))[r];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t ql = (ql4 >> (8 * e)) & 0xFFu, qh = (qh4 >> (8 * e)) & 0xFFu;
            const int q = (int)(((qd >= 2) ? (ql >> 4) : (ql & 0xF)) | (((qh >> (2 * qd)) & 3) << 4)) - 32;
            out[e] = d * (float)sc * (float)q;
        }
    }
    return out;
}

}  // namespace nfai
