// common.h — shared host/device helpers of libnfai_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdio.h>
#include <string>

#include "../../include/nfai_hip.h"

#define NFAI_API extern "C" __attribute__((visibility("default")))

namespace nfai {

// ---- error plumbing -------------------------------------------------------------------------
void set_error(const char *fmt, ...);
int fail(int code, const char *fmt, ...);

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return nfai::fail(_e == hipErrorOutOfMemory ? NFAI_ERR_OOM : NFAI_ERR_HIP,         \
                              "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                              __LINE__);                                                       \
    } while (0)

#define NFAI_REQUIRE(cond, ...)                                      \
    do {                                                             \
        if (!(cond)) return nfai::fail(NFAI_ERR_INVALID, __VA_ARGS__); \
    } while (0)

// ---- in-kernel time stamps (diagnostic build only: python -m nfai_amd.build --stamps -> libnfai_hip_stamps.so) -------------
// Every wave of a stamped kernel records up to 8 readings of s_memrealtime (100 MHz, one clock for the whole chip) into its
// launch's slot of a buffer the tool hands in; no stamp exists in the product build (MI355X guide, "In-kernel stamps").
#ifdef NFAI_STAMPS
constexpr uint32_t STAMP_WAVES = 4096, STAMP_WORDS = 8;
struct StampSlot { char name[48]; uint32_t grid, block; };
unsigned long long *stamp_next_slot(const char *name, uint32_t grid, uint32_t block);  // null when no buffer is installed
#define NFAI_STAMP_PARAM unsigned long long *stamps;
#define NFAI_STAMP_SET(p, name, grid, block) (p).stamps = nfai::stamp_next_slot(name, grid, block)
#else
#define NFAI_STAMP_PARAM
#define NFAI_STAMP_SET(p, name, grid, block) ((void)0)
#endif

// ---- handles --------------------------------------------------------------------------------
struct Ctx {
    uint32_t magic = 0x4E464358;  // 'NFCX'
    int device = 0;
    // per-XCD streaming shares (gemv_xcd_calibrate, first model created on the context): 0 = not yet measured, 1 = measured, 2 = off
    int xcd_state = 0;
    uint16_t xcd_shares[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float xcd_probe_us[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // mean end of a workgroup of each label in the probe launch (equal shares)
    bool xcd_ops = false;  // test hook (nfai_hip_debug_xcd_shares): the op-level GEMV entries pass xcd_shares as gemv_base does
    hipStream_t stream = nullptr;
    bool owns_stream = true;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipDeviceProp_t prop;
    void *scratch = nullptr;  // small workspace for ops that need one (argmax partials, attention partials)
    size_t scratch_bytes = 0;
};

struct Buf {
    uint32_t magic = 0x4E464246;  // 'NFBF'
    int w_layout = 0;  // internal weight-type code when nfai_hip_weight_upload repacked the tensor (else 0)
    uint64_t w_rows = 0;  // rows of that tensor (the T16 planes depend on it)
    void *ptr = nullptr;
    uint64_t bytes = 0;
    bool owned = true;
    Ctx *ctx = nullptr;
    void *guard_base = nullptr;  // NFAI_HIP_DEBUG_CANARY: start of the allocation (256-byte guard | buffer | 256-byte guard)
};

Ctx *ctx_of(nfai_ctx_t h);
Buf *buf_of(nfai_buf_t h);
void handle_register(const void *p);
void handle_unregister(const void *p);
bool handle_live(uint64_t h);

uint64_t weight_row_bytes(int ggml_type, uint64_t n_cols);  // 0 if unsupported / misaligned

// ---- launch entry points implemented in the kernel translation units --------------------------
// Plain pointers; every function enqueues on `s` and returns hipGetLastError().
struct GemvArgs {
    // up to three weight segments (QKV) or two (gate/up); rows are [seg_rows[i]] each, all K wide
    const void *W[3] = {nullptr, nullptr, nullptr};
    uint32_t seg_rows[3] = {0, 0, 0};
    int w_type = NFAI_F16;
    uint32_t seg6_mask = 0;        // NFAI_KQ_MIXED: bit i = segment i is Q6_K_T16
    const float *x = nullptr;      // K floats
    const float *gamma = nullptr;  // non-null => RMSNorm(x, gamma, eps) prologue
    float eps = 0.f;
    uint32_t K = 0;
    // epilogues
    int mode = 0;                  // GemvMode
    float *y = nullptr;            // PLAIN/RESIDUAL/GATEUP output, QKV: q output (H*D)
    const float *res = nullptr;    // RESIDUAL
    // QKV
    void *kcache = nullptr, *vcache = nullptr;  // layer base pointers
    int kv_type = NFAI_F32;
    uint64_t kv_pos_stride = 0;    // elements between consecutive positions
    uint64_t kv_head_stride = 0;   // elements between consecutive kv heads
    const float *rope_cs = nullptr;  // [rope_dims/2][2] cos,sin for the current position (device)
    uint32_t rope_dims = 0, H = 0, Hkv = 0, D = 0;
    const uint32_t *pos_dev = nullptr;  // current position (device scalar)
    uint32_t n_cu = 256;
    // Rows dealt to the XCDs in proportion to how fast each one streams (calibrated once per context: gemv_xcd_calibrate): 8 shares
    // (rows per dealing round for the workgroups with blockIdx % 8 == x), or nullptr = equal shares.  Speed only: every row is
    // computed exactly once by the same arithmetic whatever the shares are.  Honoured by the fp16 / fp32 k_gemv for GEMV_PLAIN and
    // GEMV_GATEUP launches whose grid is a multiple of 8 (the lm_head and the gate | up launch).
    const uint16_t *xcd_shares = nullptr;
    bool prefetch_only = false;  // side-stream launch that only touches the first two steps of every wave's weights
    // GEMV_QKV_ROPE with RMSNorm only — the per-token prologue folded into the FIRST q|k|v launch of a token (LlamaModel.cs:116 +
    // the RoPE angles RoPEShader.cs:254-256 recomputes per element): begin.on: the activation vector is row tok[0] of the
    // embedding table `emb` (emb == nullptr: x as usual, e.g. a pipeline stage that received its hidden state), workgroup 0 also
    // stores it to x_out (later launches read it as the residual), writes the cos/sin table of the current position for the
    // other blocks' launches and advances the hand-off epoch; this launch's own RoPE forms cos/sin itself
    struct Begin {
        bool on = false;
        const void *emb = nullptr;   // [emb_rows][K]: F16 / F32 row-major, or the T16 layout of an IQ4_XS / Q3_K / Q4_0 / Q4_K / Q5_K / Q6_K / Q8_0 table
        int emb_type = NFAI_F16;
        uint64_t emb_rows = 0;
        const uint32_t *tok = nullptr;
        float *x_out = nullptr;
        const float *freqs = nullptr;  // [n_freq] RoPE frequencies (TransformerBlock.cs:33-38)
        float *cs_out = nullptr;       // [n_freq][2]
        uint32_t n_freq = 0;
        uint32_t *epoch = nullptr;
    } begin;
    // GEMV_PLAIN only: SamplingUtils.ArgMax over the N outputs in the same launch (the lm_head): argmax_part = workspace of
    // argmax_fused_bytes() bytes, zeroed once; the first index of the maximum -> argmax_out; then, if argmax_pos_inc != nullptr, the
    // end-of-token bookkeeping of launch_argmax (ring[pos % ring_len] = token, ++pos)
    void *argmax_part = nullptr;
    uint32_t *argmax_out = nullptr, *argmax_pos_inc = nullptr, *argmax_ring = nullptr;
    uint32_t argmax_ring_len = 0;
};
constexpr size_t argmax_fused_bytes() { return 1024 * 8 + 256; }  // [1024] values | [1024] indices | ticket
enum GemvMode { GEMV_PLAIN = 0, GEMV_RESIDUAL = 1, GEMV_QKV_ROPE = 2, GEMV_GATEUP = 3 };

// Internal weight-type codes of the T16 layouts (t16.h): same bytes as the ggml type, rows
// grouped in tiles of 16.  Never seen across the C ABI: uploads with rows % 16 == 0 are repacked into them.
// Q8_0, Q5_K, Q4_0, Q3_K and IQ4_XS exist only in the T16 layout (rows % 16 == 0 is a rule of their upload); is_kquant covers them (block-quantised,
// same paths).
constexpr int NFAI_Q4_0_T16 = 102, NFAI_Q8_0_T16 = 108, NFAI_Q3_K_T16 = 111, NFAI_Q4_K_T16 = 112, NFAI_Q5_K_T16 = 113, NFAI_Q6_K_T16 = 114, NFAI_IQ4_XS_T16 = 123;
constexpr int NFAI_KQ_MIXED = 115;   // GemvArgs::w_type of a q|k|v launch whose segments are Q4_K_T16 / Q6_K_T16 per seg6_mask
constexpr int NFAI_KQ_MIXED5 = 116;  // the same with Q5_K_T16 / Q6_K_T16 segments (Q5_K_M files)
inline bool is_kquant(int t)
{
    return t == NFAI_Q4_K || t == NFAI_Q6_K || t == NFAI_Q4_K_T16 || t == NFAI_Q6_K_T16 || t == NFAI_Q8_0 || t == NFAI_Q8_0_T16 ||
           t == NFAI_Q5_K || t == NFAI_Q5_K_T16 || t == NFAI_Q4_0 || t == NFAI_Q4_0_T16 || t == NFAI_Q3_K || t == NFAI_Q3_K_T16 ||
           t == NFAI_IQ4_XS || t == NFAI_IQ4_XS_T16;
}
inline bool is_t16(int t) { return t == NFAI_Q4_K_T16 || t == NFAI_Q6_K_T16 || t == NFAI_Q8_0_T16 || t == NFAI_Q5_K_T16 || t == NFAI_Q4_0_T16 || t == NFAI_Q3_K_T16 || t == NFAI_IQ4_XS_T16; }
inline int ggml_type_of(int t)
{
    return t == NFAI_Q4_K_T16 ? NFAI_Q4_K
                              : (t == NFAI_Q6_K_T16 ? NFAI_Q6_K : (t == NFAI_Q8_0_T16 ? NFAI_Q8_0 : (t == NFAI_Q5_K_T16 ? NFAI_Q5_K : (t == NFAI_Q4_0_T16 ? NFAI_Q4_0 : (t == NFAI_Q3_K_T16 ? NFAI_Q3_K : (t == NFAI_IQ4_XS_T16 ? NFAI_IQ4_XS : t))))));
}

hipError_t launch_gemv(const GemvArgs &a, hipStream_t s);     // any weight type; K-quants go to launch_gemv_kq / _kqm
// How one fp16 / fp32 GEMV is launched, sixteen words: what gemv_plan decides, what launch_gemv launches from, and what the test
// hooks nfai_hip_debug_gemv_plan / nfai_hip_debug_gemv_last report.
struct GemvDesc {
    uint32_t kernel;             // 0: k_gemv (persistent), 1: k_gemv_sk (split-K)
    uint32_t w_type, mode, norm;
    uint32_t begin;              // first launch of a token (GemvArgs::Begin)
    uint32_t xd;                 // rows dealt to the XCDs by share
    uint32_t upw_ch, u_rw;       // k_gemv: UPW, U; k_gemv_sk: CH, RW
    uint32_t guard;
    uint32_t threads, grid, lds_bytes;   // threads per workgroup, workgroups, dynamic LDS bytes of the launch
    uint32_t NU, K;
    uint32_t argmax;             // fused ArgMax
    uint32_t prefetch_only;
};
constexpr uint32_t GEMV_RING_N = 256;
hipError_t gemv_plan(const GemvArgs &a, GemvDesc &d);  // host arithmetic only (no HIP call); d.NU == 0 with hipSuccess: nothing to launch
uint32_t gemv_last(GemvDesc *out, uint32_t max_desc);  // the launch_gemv calls of the fp16 / fp32 path since the last call, oldest first (the newest GEMV_RING_N at most)
bool gemv_begin_ok(const GemvArgs &a);                         // can this q|k|v launch carry the per-token prologue (GemvArgs::Begin)?
// Measures how fast the workgroups of each blockIdx % 8 label (= one XCD each) stream from HBM with every CU streaming, and derives
// the dealing shares of GemvArgs::xcd_shares; nullptr when switched off (NFAI_XCD_DEAL=0) or when the probe could not run.
const uint16_t *gemv_xcd_calibrate(Ctx *c);
uint64_t gemv_dealt_launches();  // k_gemv launches that took the XD instantiations (GemvParams::xd.S != 0) since the library was loaded
hipError_t launch_gemv_kq(const GemvArgs &a, hipStream_t s);  // Q4_K (native blocks) / Q6_K (plane layout)
hipError_t launch_gemv_kqm(const GemvArgs &a, hipStream_t s); // Q4_K_T16: MFMA dot products
hipError_t launch_repack_q4k_t16(const void *native, void *tiled, uint64_t rows, uint64_t cols, hipStream_t s);
hipError_t launch_repack_q6k_t16(const void *native, void *tiled, uint64_t rows, uint64_t cols, hipStream_t s);
hipError_t launch_repack_q80_t16(const void *native, void *tiled, uint64_t rows, uint64_t cols, hipStream_t s);
hipError_t launch_repack_q5k_t16(const void *native, void *tiled, uint64_t rows, uint64_t cols, hipStream_t s);
hipError_t launch_repack_q40_t16(const void *native, void *tiled, uint64_t rows, uint64_t cols, hipStream_t s);
hipError_t launch_repack_q3k_t16(const void *native, void *tiled, uint64_t rows, uint64_t cols, hipStream_t s);
hipError_t launch_repack_iq4xs_t16(const void *native, void *tiled, uint64_t rows, uint64_t cols, hipStream_t s);
hipError_t launch_embed_kqt(const void *table, int type, uint64_t n_rows, const uint32_t *tok, float *y, uint32_t E, hipStream_t s);
hipError_t launch_embed_rows_kqt(const void *table, int type, uint64_t n_rows, const uint32_t *toks, float *y, uint32_t T, uint32_t E, hipStream_t s);
hipError_t launch_dequant_t16_f16(const void *W, int type, uint64_t rows, uint64_t cols, void *out_f16, hipStream_t s);  // T16 K-quant / Q8_0 -> fp16 [rows][cols]
// Tiles [tile0, tile0 + n_tiles) of the same tensor (rows 16 * tile0 ..) -> fp16 [16 * n_tiles][cols]: the planes are addressed
// through the tensor's TOTAL row count (t16.h), so a row range cannot be widened by offsetting W.
hipError_t launch_dequant_t16_f16(const void *W, int type, uint64_t rows, uint64_t cols, uint64_t tile0, uint64_t n_tiles, void *out_f16, hipStream_t s);
// Q6_K super-blocks are 210 bytes (not 16-byte aligned): in HBM they live as four planes
// ql | qh | scales | d (same bytes, naturally aligned accesses).  nblk = rows * cols / 256.
hipError_t launch_repack_q6k(const void *native, void *planes, uint64_t nblk, hipStream_t s);
hipError_t launch_embed_kq(const void *table, int type, uint64_t n_rows, const uint32_t *tok, float *y, uint32_t E,
                           hipStream_t s);

// ---- MFMA prefill (kernels_prefill.hip) ---------------------------------------------------------
// epi 3 (the q | k | v projection of a prompt chunk): RoPE and every store of RoPEShader / the KV-cache writes in the GEMM's epilogue —
// row t of the product is position pos0 + t; columns are q heads | k heads | v heads.  cs = cos / sin of the chunk's positions
// (launch_rope_table).  No fp32 q | k | v round trip through HBM and no separate launch.
struct GemmRope {
    const float *cs = nullptr;            // [T][D/2][2]
    void *qh = nullptr, *kh = nullptr, *vt = nullptr;   // fp16: q [T][H*D], K rows [Hkv][Spad][D], V^T [Hkv][D][Spad]
    void *kc = nullptr, *vc = nullptr;    // the KV cache of the block (fp32 or fp16)
    uint64_t pos_stride = 0, head_stride = 0;
    uint32_t H = 0, Hkv = 0, D = 0, rope_dims = 0, pos0 = 0, Spad = 0, kv_f16 = 0;
};
hipError_t launch_rope_table(const float *freqs, uint32_t pos0, uint32_t T, uint32_t D, uint32_t rope_dims, float *cs, hipStream_t s);

struct GemmArgs {  // C[M][N] (+R) = alpha * A[M][K] * B[N][K]^T, fp16 operands, fp32 accumulate / output
    const void *A = nullptr;   // fp16, or fp32 when a_f32 (converted while staging)
    bool a_f32 = false;
    const void *B = nullptr;   // fp16 [N][ldb]
    const void *B1 = nullptr, *B2 = nullptr;  // optional 2nd / 3rd row segment (rows n0.., n0+n1..); all segments ldb wide
    uint32_t n0 = 0, n1 = 0;
    void *C = nullptr;         // fp32 [M][ldc]; fp16 when epi != 0
    int epi = 0;               // 0: fp32 (+R)   1: fp16 out   2: fp16 out = up * silu(gate), B = gate rows, B1 = up rows, N = 2F, C is [M][F]
                               // 3: RoPE + q / KV-cache stores (rope; C unused)
    GemmRope rope;
    uint32_t n_cu = 256;
    const float *R = nullptr;  // optional residual, same layout as C (epi 0)
    uint32_t M = 0, N = 0, K = 0, lda = 0, ldb = 0, ldc = 0;
    uint32_t batch = 1, b_div = 1;
    uint64_t a_bs = 0, b_bs = 0, c_bs = 0;
    float alpha = 1.0f;
    int b_type = NFAI_F16;     // launch_gemm_kq: NFAI_Q4_K_T16 / NFAI_Q6_K_T16 (all weight segments of one type)
    int variant = 0;           // 0: chosen from the shape.  1: 128x64 tiles (4x1 waves)  2: 128x128 (2x2 waves)  3 / 4: direct-to-LDS 128x128, 2 / 3 stages  5 / 6 / 7: direct-to-LDS 128x64, 2 / 3 / 4 stages
    uint32_t causal = 0, causal_pos0 = 0;  // 1: C is a causal score matrix, 2: A is a causal probability matrix (skip masked tiles)
};
hipError_t launch_gemm_f16(const GemmArgs &a, hipStream_t s);
// Test hook (nfai_hip_debug_gemm_last): what one k_gemm_f16 / k_gemm_f16_glds launch was instantiated with, sixteen words.
struct GemmDesc {
    uint32_t BM, BN, WM, WN, BK;
    uint32_t stages, stages_b;   // LDS stages of the A / B ring (direct-to-LDS) or register sets (register-staged: both = RING)
    uint32_t KS, pipe, lds_staged, epi, batch, ksplit, M, N, K;
};
constexpr uint32_t GEMM_RING_N = 256;
uint32_t gemm_last(GemmDesc *out, uint32_t max_desc);  // the launches since the last call, oldest first (the newest GEMM_RING_N at most)
hipError_t launch_gemm_kq(const GemmArgs &a, hipStream_t s);   // dequant-in-LDS GEMM on T16 K-quant weights
hipError_t launch_f32_to_f16(const float *x, void *y_f16, uint64_t n, hipStream_t s);
hipError_t launch_sum_slabs(const float *slabs, uint32_t ks, uint64_t n, const float *R, float *C, hipStream_t s);  // C = R + sum of ks slabs of n floats
hipError_t launch_read_ahead(const void *w, uint64_t bytes, uint32_t n_cu, hipStream_t s);  // side-stream hint: the next GEMM's weights -> Infinity Cache
hipError_t launch_rmsnorm_rows(const float *x, const float *g, void *y_f16, uint32_t T, uint32_t E, float eps, hipStream_t s);
// x_out = R + slab 0 + ... + slab ks-1 (slabs of T * E floats; the order of launch_sum_slabs), y = RMSNorm(x_out) * g as fp16: combine + norm in one pass
hipError_t launch_rmsnorm_rows_combine(const float *slabs, uint32_t ks, const float *R, float *x_out, const float *g, void *y_f16, uint32_t T, uint32_t E, float eps,
                                       hipStream_t s);
hipError_t launch_rope_store_rows(const float *q, const float *k, const float *v, void *qh_f16, void *kc, void *vc, int kv_f16,
                                  uint64_t pos_stride, uint64_t head_stride, const float *freqs, uint32_t rope_dims, uint32_t H,
                                  uint32_t Hkv, uint32_t D, uint32_t pos0, uint32_t T, uint32_t ld, void *kh_f16, void *vt_f16,
                                  uint32_t Spad, hipStream_t s);
hipError_t launch_kv_to_f16(const void *kc, const void *vc, int kv_f16, uint64_t pos_stride, uint64_t head_stride, void *kh, void *vt,
                            uint32_t Hkv, uint32_t D, uint32_t S, uint32_t Spad, uint32_t skip_lo, uint32_t skip_hi, hipStream_t s);
// causal attention of a prompt chunk in one launch: qh [T][H*D], kh [Hkv][Spad][D], vt [Hkv][D][Spad] (fp16) -> out [T][H*D] fp16
hipError_t launch_attn_prefill(const void *qh, const void *kh, const void *vt, void *out_f16, uint32_t T, uint32_t H, uint32_t Hkv,
                               uint32_t D, uint32_t Spad, uint32_t pos0, hipStream_t s);
hipError_t launch_softmax_causal_rows(const float *sc, void *p_f16, uint32_t H, uint32_t T, uint32_t Spad, uint32_t pos0, float scale,
                                      hipStream_t s);
hipError_t launch_silu_mul_rows(const float *gate, const float *up, void *act_f16, uint32_t T, uint32_t F, uint32_t ld, hipStream_t s);
hipError_t launch_embed_rows(const void *table, int type, const uint32_t *toks, float *x, uint32_t T, uint32_t E, hipStream_t s);

struct AttnArgs {
    const float *q = nullptr;  // [H][D] fp32 (after RoPE)
    const void *kcache = nullptr, *vcache = nullptr;
    int kv_type = NFAI_F32;
    uint64_t kv_pos_stride = 0, kv_head_stride = 0;
    float *o = nullptr;        // [H][D]
    uint32_t H = 0, Hkv = 0, D = 0, C = 0;
    const uint32_t *pos_dev = nullptr;  // S = *pos_dev + 1
    float *partials = nullptr;          // workspace: attn_partials_bytes()
    uint32_t n_cu = 256;
    // Slice hand-off.  epoch == nullptr: ticket form (partials written through, one ticket per block, the last block of a kv head
    // merges).  epoch != nullptr: granule form — every partial word travels as an 8-byte {value, tag} granule and the block of
    // the LAST slice polls the granules themselves; tag = epoch[0] * tag_mul + tag_add must differ from the tag of every earlier
    // launch that used this workspace (the model: per-token epoch x blocks + block index).  A poll that gives up sets *err.
    const uint32_t *epoch = nullptr;
    uint32_t tag_mul = 1, tag_add = 0;
    uint32_t *err = nullptr;
    uint32_t debug_withhold = 0;  // test hook: slice (value - 1) of kv head 0 publishes nothing, so the others' bounded waits give up
};
constexpr uint32_t ATTN_NSPLIT_MAX = 32;
// query heads per kv head that the decode attention is instantiated for (k_attn_decode<…, G, …>)
constexpr bool attn_group_ok(uint32_t G) { return G == 1 || G == 2 || G == 3 || G == 4 || G == 8; }
size_t attn_partials_bytes(uint32_t H, uint32_t Hkv, uint32_t D, bool granules = false);  // granules: the {value, tag} form (AttnArgs::epoch set)
hipError_t launch_attn_decode(const AttnArgs &a, hipStream_t s);
size_t attn_wo_extra_bytes(uint32_t H, uint32_t D);  // workspace behind attn_partials_bytes(…, true) for the fused launch below
// attention + (Wo + residual) in ONE launch (kernels_attn.hip, k_attn_wo): `g` is the Wo launch that would follow `a` (x = a.o).
// attn_wo_ok: the shapes / modes it is built for; everything else takes the two launches.
bool attn_wo_ok(const AttnArgs &a, const GemvArgs &g);
hipError_t launch_attn_wo(const AttnArgs &a, const GemvArgs &g, hipStream_t s);

// ---- batched decode (kernels_gemv_batch.hip): one weight stream applied to the activation vectors of up to 8 sequences ------------
// Column b of a launch is sequence b: its own activation vectors, KV cache, position word.  Columns >= n are dead (a batch of 3 runs
// the B = 4 kernel): they read column 0's input and store nothing.
constexpr uint32_t BATCH_MAX = 8;
struct BatchGemvArgs {
    const void *W[3] = {nullptr, nullptr, nullptr};   // fp16 [seg_rows[i]][K]
    uint32_t seg_rows[3] = {0, 0, 0};
    uint32_t K = 0, n = 0;
    int mode = 0;                      // GemvMode
    const float *gamma = nullptr;      // non-null: RMSNorm prologue per column
    float eps = 0.f;
    const float *x[BATCH_MAX] = {};
    float *y[BATCH_MAX] = {};
    const float *res[BATCH_MAX] = {};
    // GEMV_QKV_ROPE
    void *kc[BATCH_MAX] = {}, *vc[BATCH_MAX] = {};
    uint64_t kv_head_stride[BATCH_MAX] = {};
    uint32_t cap[BATCH_MAX] = {};
    const uint32_t *pos[BATCH_MAX] = {};
    uint32_t pos_off[BATCH_MAX] = {};  // column b works at position pos[b][0] + pos_off[b]: zeros for a batch, b for a window (one position word)
    uint64_t kv_pos_stride = 0;
    int kv_type = NFAI_F32;
    const float *freqs = nullptr;
    uint32_t rope_dims = 0, H = 0, Hkv = 0, D = 0;
    uint32_t *err = nullptr;           // device word: 0x10000 | column when a column's position word is at or past its capacity
    // GEMV_PLAIN (lm_head): first index of the maximum per column + the end-of-token bookkeeping of every member
    void *am_work = nullptr;           // batch_argmax_bytes(), zeroed once
    uint32_t *am_tok_batch = nullptr;  // [BATCH_MAX]: the batch's token words (next step's input)
    uint32_t *am_tok[BATCH_MAX] = {}, *am_pos[BATCH_MAX] = {}, *am_ring[BATCH_MAX] = {};
    uint32_t am_ring_len = 0;
    // GEMV_PLAIN of a window (non-null): the columns are consecutive positions of ONE sequence (am_tok / am_pos / am_ring of column 0)
    // and the tail applies the accept rule of greedy speculative decoding instead of the per-member bookkeeping (win_tail below).
    // win_ctl: [0..7] draft tokens, [8] their count k (0xFFFFFFFF: keep every column); the count of emitted tokens goes to
    // am_tok_batch[WIN_NOUT].
    const uint32_t *win_ctl = nullptr;
    uint32_t n_cu = 256;
};
constexpr uint32_t WIN_NOUT = BATCH_MAX + 1;   // (word BATCH_MAX is the error word of the q|k|v launches)
constexpr uint32_t WIN_ALL = 0xFFFFFFFFu;
constexpr size_t batch_argmax_bytes() { return (size_t)BATCH_MAX * 1024 * 8 + 256; }
bool batch_gemv_ok(const BatchGemvArgs &a);   // shape rules of launch_batch_gemv (checked by nfai_hip_llama_batch_create)
hipError_t launch_batch_gemv(const BatchGemvArgs &a, hipStream_t s);
struct BatchAttnArgs {
    uint32_t n = 0;
    const float *q[BATCH_MAX] = {};
    float *o[BATCH_MAX] = {};
    const void *kc[BATCH_MAX] = {}, *vc[BATCH_MAX] = {};
    uint64_t kv_head_stride[BATCH_MAX] = {};
    uint32_t cap[BATCH_MAX] = {};
    const uint32_t *pos[BATCH_MAX] = {};
    uint64_t kv_pos_stride = 0;
    int kv_type = NFAI_F32;
    uint32_t H = 0, Hkv = 0, D = 0;
    void *work = nullptr;              // batch_attn_bytes(), zeroed once
};
size_t batch_attn_bytes(uint32_t H, uint32_t D);
hipError_t launch_batch_attn(const BatchAttnArgs &a, hipStream_t s);
// Attention of a window (kernels_attn_window.hip): n query columns at the consecutive positions pos[0] + i of ONE cache; column i
// attends to rows 0 .. pos[0] + i.  The rows below pos[0] are read once per kv head for all columns.
struct WindowAttnArgs {
    uint32_t n = 0;
    const float *q[BATCH_MAX] = {};
    float *o[BATCH_MAX] = {};
    const void *kc = nullptr, *vc = nullptr;
    uint64_t kv_head_stride = 0, kv_pos_stride = 0;
    uint32_t cap = 0;
    const uint32_t *pos = nullptr;
    int kv_type = NFAI_F32;
    uint32_t H = 0, Hkv = 0, D = 0;
    void *work = nullptr;              // window_attn_bytes(), zeroed once
};
size_t window_attn_bytes(uint32_t H, uint32_t D);
hipError_t launch_window_attn(const WindowAttnArgs &a, hipStream_t s);
// x[b] = row tok[b] of the fp16 embedding table, widened (TokenEmbedShader.cs:131-159), b < n
hipError_t launch_batch_embed(const void *table, uint64_t n_rows, uint32_t E, const uint32_t *tok, float *const *x, uint32_t n, hipStream_t s);
// The same launches on IQ4_XS / Q3_K / Q4_0 / Q4_K / Q5_K / Q6_K / Q8_0 matrices in the T16 layout (kernels_gemv_batch_kqm.hip): W[i] are T16 tensors of ONE
// type (a q|k|v of mixed types is split by type into up to three launches), seg_role[i] says which of q (0), k (1), v (2) segment i of a q|k|v launch is.
struct BatchKqArgs : BatchGemvArgs {
    int w_type = 0;                    // a T16 type (is_t16)
    uint32_t seg_role[3] = {0, 1, 2};
};
bool batch_gemv_kq_ok(const BatchKqArgs &a);   // shape and LDS rules of launch_batch_gemv_kq (checked by nfai_hip_llama_batch_create_ex)
hipError_t launch_batch_gemv_kq(const BatchKqArgs &a, hipStream_t s);
hipError_t launch_batch_embed_kq(const void *table, int type, uint64_t n_rows, uint32_t E, const uint32_t *tok, float *const *x, uint32_t n, hipStream_t s);

// ---- wide batched decode (kernels_gemv_wide.hip): up to 16 sequences per weight pass on the fp16 MFMA ------------------------------
// The five launch forms of BatchGemvArgs with 16 columns: the weights are the MFMA's A operand, the columns its B operand (fp32 x as
// two fp16 planes).  Columns >= n are dead.  fp16 matrices only.
constexpr uint32_t WIDE_MAX = 16;
static_assert(WIDE_MAX == NFAI_BATCH_WIDE_MAX, "nfai_hip.h");
struct WideGemvArgs {
    const void *W[3] = {nullptr, nullptr, nullptr};   // fp16 [seg_rows[i]][K]
    uint32_t seg_rows[3] = {0, 0, 0};
    uint32_t K = 0, n = 0;
    int mode = 0;                      // GemvMode
    const float *gamma = nullptr;      // RMSNorm prologue per column: every form but GEMV_RESIDUAL has it
    float eps = 0.f;
    const float *x[WIDE_MAX] = {};
    float *y[WIDE_MAX] = {};
    const float *res[WIDE_MAX] = {};
    // GEMV_QKV_ROPE
    void *kc[WIDE_MAX] = {}, *vc[WIDE_MAX] = {};
    uint64_t kv_head_stride[WIDE_MAX] = {};
    uint32_t cap[WIDE_MAX] = {};
    const uint32_t *pos[WIDE_MAX] = {};
    uint64_t kv_pos_stride = 0;
    int kv_type = NFAI_F32;
    const float *freqs = nullptr;
    uint32_t rope_dims = 0, H = 0, Hkv = 0, D = 0;
    uint32_t *err = nullptr;           // device word: 0x10000 | column when a column's position word is at or past its capacity
    // GEMV_PLAIN (lm_head): first index of the maximum per column + the end-of-token bookkeeping of every member
    void *am_work = nullptr;           // wide_argmax_bytes(), zeroed once
    uint32_t *am_tok_batch = nullptr;  // [WIDE_MAX]: the batch's token words (next step's input)
    uint32_t *am_tok[WIDE_MAX] = {}, *am_pos[WIDE_MAX] = {}, *am_ring[WIDE_MAX] = {};
    uint32_t am_ring_len = 0;
    uint32_t n_cu = 256;
};
constexpr size_t wide_argmax_bytes() { return (size_t)WIDE_MAX * 1024 * 8 + 256; }
bool wide_gemv_ok(const WideGemvArgs &a);   // shape rules of launch_wide_gemv (checked by nfai_hip_llama_batch_create_wide)
hipError_t launch_wide_gemv(const WideGemvArgs &a, hipStream_t s);

// the weight-streaming engine (kernels_engine.hip): Wo + residual -> gate|up -> Wdown + residual -> next block's q|k|v, one launch
struct EngineArgs {
    uint32_t n_ops = 3;              // 3: ends with Wdown (last block of the range); 4: + the next block's q|k|v
    uint32_t E = 0, F = 0, HD = 0;
    const void *Wo = nullptr, *Wgate = nullptr, *Wup = nullptr, *Wdown = nullptr;   // fp16 [N][K]
    const void *Wqkv[3] = {nullptr, nullptr, nullptr};
    uint32_t qkv_rows[3] = {0, 0, 0};
    const float *att = nullptr, *x_in = nullptr, *gamma_ffn = nullptr, *gamma_next = nullptr;
    float eps = 0.f;
    uint64_t *g_h = nullptr, *g_act = nullptr, *g_x = nullptr;   // granule vectors (E, F, E), zero-initialised once
    const uint32_t *epoch = nullptr;                             // device word, advanced once per token
    float *x_out = nullptr;          // plain [E]: the block's output
    float *q_out = nullptr;
    void *kcache = nullptr, *vcache = nullptr;                   // the NEXT block's caches
    int kv_type = NFAI_F32;
    uint64_t kv_pos_stride = 0, kv_head_stride = 0;
    const float *rope_cs = nullptr;
    uint32_t rope_dims = 0, D = 0;
    const uint32_t *pos_dev = nullptr;
    uint32_t *err = nullptr;         // device word: non-zero after a bounded wait gave up
    uint32_t n_cu = 256;
};
struct EnginePlan {  // a planned engine launch: the op table in device memory, the kernel argument, the launch geometry
    void *params_dev = nullptr;
    alignas(8) unsigned char params[256] = {};
    uint32_t lds_bytes = 0, n_cu = 0;
    int ahead = 0;  // U: chunks per step (4, 6 or 8 = embedding width / 512)
};
size_t engine_params_bytes();
hipError_t engine_plan(const EngineArgs &a, void *params_dev, EnginePlan &plan);  // synchronous copy: outside stream capture
hipError_t launch_engine(const EnginePlan &plan, hipStream_t s);

// basic 1:1 ops
hipError_t launch_embed(const void *table, int type, const uint32_t *tok, float *y, uint32_t E, hipStream_t s);
hipError_t launch_rmsnorm(const float *x, const float *g, float *y, uint32_t E, float eps, hipStream_t s);
hipError_t launch_rope(const float *in, float *out, const float *freqs, uint32_t rope_dims, uint32_t n_heads,
                       uint32_t head_dim, uint32_t pos, hipStream_t s);
hipError_t launch_attn_scores(const float *q, const float *K, float *sc, uint32_t H, uint32_t Hkv, uint32_t D,
                              uint32_t S, hipStream_t s);
hipError_t launch_attn_softmax(const float *sc, float *w, uint32_t H, uint32_t S, float eps, hipStream_t s);
hipError_t launch_attn_wsum(const float *w, const float *V, float *o, uint32_t H, uint32_t Hkv, uint32_t D,
                            uint32_t S, hipStream_t s);
hipError_t launch_silu(const float *x, float *y, uint32_t n, hipStream_t s);
hipError_t launch_mul(const float *a, const float *b, float *y, uint32_t n, hipStream_t s);
hipError_t launch_add(const float *a, const float *b, float *y, uint32_t n, hipStream_t s);
// argmax over n floats -> out_idx; `partials` needs 2*ARGMAX_BLOCKS*4 bytes. If pos_inc != null it is
// incremented by the final block (end-of-token bookkeeping for graph replay); ring != null records
// the token at ring[(*pos_inc_old) % ring_len].
constexpr uint32_t ARGMAX_BLOCKS = 128;
hipError_t launch_argmax(const float *x, uint32_t n, uint32_t *out_idx, void *partials, uint32_t *pos_inc,
                         uint32_t *ring, uint32_t ring_len, hipStream_t s);
// top-k candidates of SamplingUtils.TopP on the device (kernels_basic.hip): the k largest of n logits (descending, ties: lower
// index first) + max(l / T) + sum exp(l / T - max) -> the head of `work` (topk_out_offset(): k floats, at +TOPK_MAX*4 k indices,
// at +TOPK_MAX*8 M and S).  work: topk_work_bytes(n) bytes, zeroed once.
constexpr uint32_t TOPK_MAX = 64, TOPK_THREADS = 256, TOPK_NT = 8, TOPK_BLOCKS_MAX = 1024;
inline uint32_t topk_blocks(uint32_t n)
{
    const uint32_t per = TOPK_THREADS * TOPK_NT;  // logits a block can hold in registers
    const uint32_t need = (n + per - 1) / per, spread = (n + TOPK_THREADS - 1) / TOPK_THREADS;
    const uint32_t b = need > (spread < 128 ? spread : 128) ? need : (spread < 128 ? spread : 128);  // a vocabulary is spread over >= 128 blocks
    return b > TOPK_BLOCKS_MAX ? TOPK_BLOCKS_MAX : (b ? b : 1);
}
size_t topk_work_bytes(uint32_t n);
size_t topk_out_offset();
hipError_t launch_topk(const float *x, uint32_t n, float temperature, uint32_t k, void *work, hipStream_t s);
// The same for R <= BATCH_MAX vectors of n floats in ONE pair of launches, grid (topk_blocks(n), R): row r reads x[r] (the rows need
// not be contiguous, and may repeat), keeps ticket, candidate counter, heads, sums and candidates in its own slice of `work` (at
// r * topk_rows_stride(n); R slices, zeroed once) and leaves its TopkOut in out[r] of one contiguous device array.  Per row the
// arithmetic, the range partition and the order of the sums are launch_topk's: a row's result is bit-identical to it.
struct TopkOut { float v[TOPK_MAX]; uint32_t i[TOPK_MAX]; float M, S; };   // what one vector leaves for the host half (topk_finish)
struct TopkRowsArgs {
    const float *x[BATCH_MAX] = {};
};
inline size_t topk_rows_stride(uint32_t n) { return (topk_work_bytes(n) + 255) & ~(size_t)255; }
hipError_t launch_topk_rows(const TopkRowsArgs &rows, uint32_t R, uint32_t n, float temperature, uint32_t k, void *work, TopkOut *out, hipStream_t s);
// launch + 8k + 8 bytes back + the host half (api.hip); blocking
void topk_finish(const float *vals, const uint32_t *ids, float M, float S, float temperature, uint32_t k, uint32_t *ids_out, float *probs_out);
int topk_run(Ctx *c, const float *logits_dev, uint32_t n, float temperature, uint32_t k, void *work, uint32_t *ids_out, float *probs_out);
// ---- log-probabilities of logit rows (kernels_score.hip) ----------------------------------------------------------------------------
// The running state of one row across column slabs: an online softmax (SamplingUtils.cs:35-41) + ArgMax (:55-56) + the target's logit.
struct ScoreState {
    float m;        // max of the columns folded so far
    float s;        // sum exp(l - m) over them
    uint32_t idx;   // first index of m
    float tl;       // logit of the row's target, once its column has passed
};
constexpr uint32_t SCORE_NO_TARGET = 0xFFFFFFFFu;
// Folds columns [c0, c0 + ns) of T rows into state[T]: row r's columns are slab[r * ld + 0 .. ns) (`slab` points AT column c0).
// c0 == 0 starts a row's state.  targets[r] >= V and not SCORE_NO_TARGET: *err |= 1 (checked in the c0 == 0 pass).  One workgroup per row.
hipError_t launch_score_slab(const float *slab, uint32_t T, uint64_t ld, uint32_t c0, uint32_t ns, uint32_t V, const uint32_t *targets,
                             ScoreState *state, uint32_t *err, hipStream_t s);
// logprob[r] = tl - m - log s (0 without a target), argmax[r] = idx, logprob_max[r] = -log s; writes nothing when *err != 0
hipError_t launch_score_finish(const ScoreState *state, uint32_t T, const uint32_t *targets, const uint32_t *err, float *logprob, uint32_t *argmax,
                               float *logprob_max, hipStream_t s);
// per-token prologue: embed row -> x, cos/sin table for the current position
hipError_t launch_token_begin(const void *table, int type, const uint32_t *tok, float *x, uint32_t E,
                              const float *freqs, float *rope_cs, uint32_t n_freq, const uint32_t *pos_dev,
                              hipStream_t s, uint32_t *epoch = nullptr);  // epoch: the engine's per-token tag, advanced here
hipError_t launch_pos_advance(uint32_t *pos_dev, hipStream_t s);

}  // namespace nfai

// ---- device helpers (HIP translation units only) ------------------------------------------------
#if defined(__HIPCC__)
namespace nfai {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

constexpr int WAVE = 64;

// Sum across the 64 lanes of a wave; every lane gets the total.
// DPP within rows of 16 (quad_perm xor1, xor2; row_half_mirror; row_mirror), then the four row
// totals are read with v_readlane (wave-uniform) and added.
__device__ __forceinline__ float wave_sum(float v)
{
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));  // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));  // row_mirror
    int iv = __builtin_bit_cast(int, v);
    float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 0));
    float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 16));
    float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 32));
    float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 48));
    return (r0 + r1) + (r2 + r3);
}

// Max across the 64 lanes, same shape as wave_sum (four DPP steps inside rows of 16, then the four row maxima by
// v_readlane): no ds_bpermute round trips through the LDS crossbar (six of them in the shuffle form).
__device__ __forceinline__ float wave_max(float v)
{
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true)));
    const int iv = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 0));
    const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 32));
    const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 48));
    return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}

// Sum over the four rows of 16 lanes (lane r, r + 16, r + 32, r + 48), every lane gets it: (v[r] + v[r+16]) + (v[r+32] + v[r+48]),
// the order of `v += shfl_xor(v, 16); v += shfl_xor(v, 32)`, but inside the vector ALU (gfx950: v_permlane16_swap / v_permlane32_swap)
// instead of two dependent ds_bpermute round trips through the LDS crossbar with an s_waitcnt each.
__device__ __forceinline__ float rows4_sum(float v)
{
    const uint32_t b = __builtin_bit_cast(uint32_t, v);
    const auto r16 = __builtin_amdgcn_permlane16_swap(b, b, false, false);  // [0]: rows {0,0,2,2}, [1]: rows {1,1,3,3}
    const float t = __builtin_bit_cast(float, (uint32_t)r16[0]) + __builtin_bit_cast(float, (uint32_t)r16[1]);
    const uint32_t tb = __builtin_bit_cast(uint32_t, t);
    const auto r32 = __builtin_amdgcn_permlane32_swap(tb, tb, false, false);  // [0]: halves {lo, lo}, [1]: halves {hi, hi}
    return __builtin_bit_cast(float, (uint32_t)r32[0]) + __builtin_bit_cast(float, (uint32_t)r32[1]);
}

// Sum within aligned groups of `width` lanes (power of two <= 64); every lane of the group gets it.
template <int width>
__device__ __forceinline__ float group_sum(float v)
{
#pragma unroll
    for (int o = width / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// 16-byte streaming load of read-once data (weights, KV): non-temporal so it does not displace
// the activations in L2 (MI355X guide, row nt-weights).
// The pointer is cast to the GLOBAL address space explicitly: through struct-carried pointers and
// selects hipcc otherwise emits flat_load, which counts on vmcnt AND lgkmcnt, completes out of order
// and forces s_waitcnt vmcnt(0) — i.e. no load pipelining at all.
__device__ __forceinline__ u32x4 load_nt16(const void *p)
{
    return __builtin_nontemporal_load((const __attribute__((address_space(1))) u32x4 *)p);
}

__device__ __forceinline__ float h2f_lo(uint32_t w) { return (float)__builtin_bit_cast(f16x2, w)[0]; }
__device__ __forceinline__ float h2f_hi(uint32_t w) { return (float)__builtin_bit_cast(f16x2, w)[1]; }

// dot of 8 fp16 weights (one 16-byte load) with 8 fp32 activations, fp32 accumulate.
// fmaf((float)h, x, acc) lowers to v_fma_mix_f32 (fp16 operand converted inside the FMA).
__device__ __forceinline__ float dot8_f16(u32x4 w, f32x4 x0, f32x4 x1, float acc)
{
    acc = fmaf(h2f_lo(w[0]), x0[0], acc);
    acc = fmaf(h2f_hi(w[0]), x0[1], acc);
    acc = fmaf(h2f_lo(w[1]), x0[2], acc);
    acc = fmaf(h2f_hi(w[1]), x0[3], acc);
    acc = fmaf(h2f_lo(w[2]), x1[0], acc);
    acc = fmaf(h2f_hi(w[2]), x1[1], acc);
    acc = fmaf(h2f_lo(w[3]), x1[2], acc);
    acc = fmaf(h2f_hi(w[3]), x1[3], acc);
    return acc;
}

// one element of a KV cache (fp16 or fp32 per the model's kv_type)
__device__ __forceinline__ void kv_store(void *base, int f16, uint64_t idx, float v)
{
    if (f16) reinterpret_cast<_Float16 *>(base)[idx] = (_Float16)v;
    else reinterpret_cast<float *>(base)[idx] = v;
}

}  // namespace nfai
#include "t16.h"  // the T16 layout of quantised tensors: plane addresses and block decode (uses the types and loads above)
namespace nfai {

// ---- the per-token prologue inside the first q|k|v launch (GemvArgs::Begin) -------------------------------------------------------
struct BeginParams {
    const uint8_t *emb;
    uint64_t emb_rows;
    const uint32_t *tok;
    float *x_out;
    const float *freqs;
    float *cs_out;
    uint32_t *epoch;
    uint32_t n_freq;
    int emb_type;
    uint32_t on;
};

// four consecutive elements k .. k+3 (k % 4 == 0) of row `row` of an embedding table with E columns, widened to fp32 exactly as
// TokenEmbedShader (TokenEmbedShader.cs:131-159) gives them; a quantised table is in the T16 layout (t16_row_load4)
__device__ __forceinline__ f32x4 embed_load4(const uint8_t *table, int type, uint64_t n_rows, uint64_t row, uint32_t k, uint32_t E)
{
    typedef __attribute__((address_space(1))) uint8_t g8;
    const g8 *t = (const g8 *)table;
    if (type == NFAI_F16) {
        const u32x2 w = *reinterpret_cast<const __attribute__((address_space(1))) u32x2 *>(t + (row * E + k) * 2);
        return f32x4{h2f_lo(w[0]), h2f_hi(w[0]), h2f_lo(w[1]), h2f_hi(w[1])};
    }
    if (type == NFAI_F32) return *reinterpret_cast<const __attribute__((address_space(1))) f32x4 *>(t + (row * E + k) * 4);
    return t16_row_load4(table, type, n_rows, row, k, E);
}

// cos / sin of RoPE pair `pair` at position pos, as k_token_begin tabulates them (RoPEShader.cs:254-256)
__device__ __forceinline__ f32x2 rope_cs_of(const float *freqs, uint32_t pair, uint32_t pos)
{
    const float theta = ((const __attribute__((address_space(1))) float *)freqs)[pair] * (float)pos;
    return f32x2{cosf(theta), sinf(theta)};
}

// First q|k|v launch of a token: every workgroup tabulates cos/sin of the position once, in LDS (cs_lds: 2 * n_freq floats, read by
// its own RoPE epilogues behind a workgroup barrier; libm range reduction at theta ~ 1e2 is too slow to repeat per finished row);
// workgroup 0 also writes the table for the other blocks' launches and advances the hand-off epoch.
__device__ __forceinline__ void begin_bookkeeping(const BeginParams &b, uint32_t pos, float *cs_lds)
{
    for (uint32_t d = threadIdx.x; d < b.n_freq; d += blockDim.x) {
        const f32x2 cs = rope_cs_of(b.freqs, d, pos);
        cs_lds[2 * d] = cs[0];
        cs_lds[2 * d + 1] = cs[1];
        if (blockIdx.x == 0) {
            b.cs_out[2 * d] = cs[0];
            b.cs_out[2 * d + 1] = cs[1];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && b.epoch) b.epoch[0] = b.epoch[0] + 1;
}
constexpr uint32_t BEGIN_CS_WORDS = 128;  // LDS words of that table (head_dim <= 128)

// ---- "first index of the largest value" across lanes / waves / workgroups (SamplingUtils.ArgMax, SamplingUtils.cs:55-56: values.Max()
//      then IndexOf: the LOWEST index among equal maxima) ---------------------------------------------------------------------------
__device__ __forceinline__ bool topk_better(float av, uint32_t ai, float bv, uint32_t bi) { return av > bv || (av == bv && ai < bi); }

// The lm_head tail of a window (one thread of the workgroup whose ticket is last; am[i] = ArgMax of column i, in LDS): the accept
// rule of greedy speculative decoding.  Column 0 carried the token just sampled, column i > 0 the draft ctl[i - 1]; acc = the number
// of leading drafts that ARE the model's own choice (ctl[i] == am[i] for all i < acc, acc <= k), so am[0 .. acc] are exactly the
// tokens acc + 1 passes of the loop LlamaModel.cs:116-125 with SamplingUtils.ArgMax (SamplingUtils.cs:43-57) would have emitted.
// The sequence is left as those passes would have left it: ring extended by am[0 .. acc], token word am[acc], position + acc + 1 (the
// K / V rows of the rejected columns stay above the position, where nothing reads them).  k = WIN_ALL keeps every column (a
// multi-token step: the caller's tokens are the sequence).
__device__ __forceinline__ void win_tail(const uint32_t *am, uint32_t n, const uint32_t *ctl, uint32_t *out, uint32_t *tok, uint32_t *pos,
                                         uint32_t *ring, uint32_t ring_len)
{
    const uint32_t k = ctl[BATCH_MAX];
    const uint32_t lim = k == WIN_ALL ? n - 1 : (k < n - 1 ? k : n - 1);
    uint32_t acc = 0;
    while (acc < lim && (k == WIN_ALL || ctl[acc] == am[acc])) acc++;
    const uint32_t pp = pos[0];
    for (uint32_t i = 0; i < n; i++) out[i] = am[i];
    for (uint32_t i = 0; i <= acc; i++) ring[(pp + i) % ring_len] = am[i];
    out[WIN_NOUT] = acc + 1;
    tok[0] = am[acc];
    pos[0] = pp + acc + 1;
}

__device__ __forceinline__ void wave_best(float &v, uint32_t &i)
{
#define NFAI_BEST_STEP(CTRL)                                                                                                      \
    {                                                                                                                             \
        const float ov = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true)); \
        const uint32_t oi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)i, CTRL, 0xF, 0xF, true);                                 \
        if (topk_better(ov, oi, v, i)) { v = ov; i = oi; }                                                                        \
    }
    NFAI_BEST_STEP(0xB1)   // quad_perm [1,0,3,2]
    NFAI_BEST_STEP(0x4E)   // quad_perm [2,3,0,1]
    NFAI_BEST_STEP(0x141)  // row_half_mirror
    NFAI_BEST_STEP(0x140)  // row_mirror
#undef NFAI_BEST_STEP
    // every lane of a row of 16 now holds the row's best; the four rows meet through scalar registers
    float bv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
    uint32_t bi = (uint32_t)__builtin_amdgcn_readlane((int)i, 0);
#pragma unroll
    for (int r = 16; r < 64; r += 16) {
        const float ov = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), r));
        const uint32_t oi = (uint32_t)__builtin_amdgcn_readlane((int)i, r);
        if (topk_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    v = bv;
    i = bi;
}


// ArgMax folded into the launch that produces the values (the lm_head GEMV): every thread arrives with the best (value, index) it
// has finished itself ((-inf, 0xFFFFFFFF) if none); the workgroup's best goes to part[blockIdx.x] (write-through), ONE lane takes a
// ticket, and the workgroup whose ticket is last combines the partials — (value desc, index asc) is a total order, so the result does
// not depend on which workgroup that is — and does the end-of-token bookkeeping of k_argmax: token fed back, ring, position.
// lds: 34 words no other code of the kernel touches.  Called by ALL threads of the workgroup, once, at the end of the kernel.
struct ArgmaxFused {
    float *part_v;        // [gridDim.x]
    uint32_t *part_i;     // [gridDim.x]
    uint32_t *ticket;     // zero between launches
    uint32_t *out_idx, *pos_inc, *ring;
    uint32_t ring_len;
};
constexpr uint32_t ARGMAX_FUSED_MAX_BLOCKS = 1024;
__device__ __forceinline__ void argmax_fused_tail(float bv, uint32_t bi, const ArgmaxFused &t, uint32_t *lds)
{
    float *sv = reinterpret_cast<float *>(lds);
    uint32_t *si = lds + 16, *last = lds + 32;
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    wave_best(bv, bi);
    if (lane == 0) { sv[wid] = bv; si[wid] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < nw; w++)
            if (topk_better(sv[w], si[w], bv, bi)) { bv = sv[w]; bi = si[w]; }
        __hip_atomic_store(&t.part_v[blockIdx.x], bv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&t.part_i[blockIdx.x], bi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t tk = __hip_atomic_fetch_add(t.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last[0] = (tk == gridDim.x - 1) ? 1u : 0u;
    }
    __syncthreads();
    if (last[0] == 0u) return;
    bv = -INFINITY;
    bi = 0xFFFFFFFFu;
    for (uint32_t b = threadIdx.x; b < gridDim.x; b += blockDim.x) {
        const float v = __hip_atomic_load(&t.part_v[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t i = __hip_atomic_load(&t.part_i[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (topk_better(v, i, bv, bi)) { bv = v; bi = i; }
    }
    wave_best(bv, bi);
    __syncthreads();
    if (lane == 0) { sv[wid] = bv; si[wid] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < nw; w++)
            if (topk_better(sv[w], si[w], bv, bi)) { bv = sv[w]; bi = si[w]; }
        t.out_idx[0] = bi;
        __hip_atomic_store(t.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm (stream-ordered with the next launch)
        if (t.pos_inc) {
            const uint32_t pp = t.pos_inc[0];
            if (t.ring) t.ring[pp % t.ring_len] = bi;
            t.pos_inc[0] = pp + 1;
        }
    }
}

#ifdef NFAI_STAMPS
// STAMP(i): reading i of this wave (wave-uniform scalar registers; written out by stamp_flush at the end of the kernel)
struct Stamps {
    unsigned long long t[STAMP_WORDS] = {};
    __device__ __forceinline__ void at(int i) { __builtin_amdgcn_sched_barrier(0); t[i] = __builtin_amdgcn_s_memrealtime(); __builtin_amdgcn_sched_barrier(0); }
    __device__ __forceinline__ void flush(unsigned long long *base, uint32_t wave_global, int n)
    {
        if (!base || wave_global >= STAMP_WAVES) return;
        if ((threadIdx.x & 63) == 0)
            for (int i = 0; i < n; i++) base[(size_t)wave_global * STAMP_WORDS + i] = t[i];
    }
};
#define STAMP_DECL nfai::Stamps _st
#define STAMP(i) _st.at(i)
#define STAMP_FLUSH(base, wg, n) _st.flush(base, wg, n)
#else
#define STAMP_DECL
#define STAMP(i) ((void)0)
#define STAMP_FLUSH(base, wg, n) ((void)0)
#endif

__device__ __forceinline__ float silu_ref(float x)
{
    // SiLUShader.cs:121-123: x * (1.0 / (1.0 + exp(-x)))
    float sig = 1.0f / (1.0f + expf(-x));
    return x * sig;
}

// Block-wide sum (<= 16 waves); every thread gets the total.  `red` is >= 16 floats of LDS.
// FRESH: `red` has not been read or written in this launch yet, so nothing has to be kept apart from the write below (the GEMV
// prologues: one barrier fewer on the way to the first FMA).
template <bool FRESH = false>
__device__ __forceinline__ float block_sum(float v, float *red)
{
    v = wave_sum(v);
    const int wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if constexpr (!FRESH) __syncthreads();
    if ((threadIdx.x & 63) == 0) red[wid] = v;
    __syncthreads();
    // fixed trip count (<= 16 waves): the LDS reads issue back to back; with the runtime bound hipcc emits a serial
    // read-wait-add chain (measured on the K-quant GEMV: +3 % tokens/s from this change alone).  Same summation order.
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const float v = red[min(i, nw - 1)];
        t += i < nw ? v : 0.f;
    }
    return t;
}

}  // namespace nfai
#endif
