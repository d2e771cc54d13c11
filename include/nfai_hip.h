/*
 * nfai_hip.h — C ABI of libnfai_hip.so: the MI355X (gfx950) backend for NFAI's Llama-3
 * TransformerBlock decode path.
 *
 * The reference (NicuTheodorAlexandru/NFAI) has no FFI of its own: its backend boundary is the
 * C# class VulkanBufferManager plus the ShaderWrapper-derived op classes that call it.  A C#
 * `NFAI.HIP` assembly binds the functions below with [LibraryImport("nfai_hip")] (stubs in
 * INTEGRATION.md / csharp/NFAI.HIP/); each entry cites the reference member it replaces.
 * All paths are relative to the reference root.
 *
 * Conventions
 *  - every function returns an int32 status (NFAI_OK == 0); nfai_hip_last_error() returns a
 *    thread-local UTF-8 message for the last non-zero status (the C# wrapper throws on non-zero,
 *    matching the reference's exceptions on any non-Success VkResult,
 *    NFAI.Vulkan/VulkanBufferManager.cs:61-87);
 *  - handles are opaque 64-bit values; the caller owns host memory, the library owns device
 *    memory (except buffers adopted with nfai_hip_buf_wrap);
 *  - one context per device, one HIP stream per context; a context is NOT thread-safe (the
 *    reference is single-threaded and blocking, VulkanBufferManager.cs:474-494); different
 *    contexts may be used from different threads;
 *  - op calls ENQUEUE on the context stream and return; upload/download/synchronize block.
 *    (The reference fence-waits every dispatch, ShaderWrapper.cs:208-245; results are identical
 *    because everything is stream-ordered.)
 *  - element counts are in ELEMENTS, offsets (`*_off`) in elements of the buffer's type unless a
 *    parameter says bytes;
 *  - no torch / C++ types cross this boundary.
 */
#ifndef NFAI_HIP_H
#define NFAI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NFAI_HIP_ABI_VERSION 1

typedef uint64_t nfai_ctx_t;
typedef uint64_t nfai_buf_t;
typedef uint64_t nfai_model_t;
typedef uint64_t nfai_pp_t;
typedef uint64_t nfai_batch_t;
typedef uint64_t nfai_window_t;

enum nfai_status {
    NFAI_OK = 0,
    NFAI_ERR_INVALID = 1,     /* bad argument / shape the kernels do not support */
    NFAI_ERR_HIP = 2,         /* a HIP runtime call failed (message has hipGetErrorString) */
    NFAI_ERR_OOM = 3,
    NFAI_ERR_KV_FULL = 4,     /* position == KV capacity; the reference has no check
                                 (MatrixMultiplyShader.cs:248-252) and writes out of bounds */
    NFAI_ERR_UNSUPPORTED = 5, /* e.g. a ggml tensor type without a kernel */
    NFAI_ERR_STATE = 6        /* call order (missing tensor, model not finalised, ...) */
};

/* ggml tensor type ids as stored in GGUF (NFAI.GGUF/Parser.cs:262-293 names the same ids).
 * Q8_0 (ggml block_q8_0: fp16 d, int8 qs[32]; weight = d * q) is accepted wherever Q4_K is, for matrices with
 * rows %% 16 == 0, cols %% 256 == 0 and cols <= 32768; any other Q8_0 shape is NFAI_ERR_UNSUPPORTED.
 * Q5_K (ggml block_q5_K: fp16 d, fp16 dmin, 12 scale bytes, qh[32], qs[128] per 256 weights; weight = d * sc * q - dmin * m with
 * q = nibble | fifth bit << 4) is accepted under the same shape rules as Q8_0; any other Q5_K shape is NFAI_ERR_UNSUPPORTED.
 * Q4_0 (ggml block_q4_0: fp16 d, qs[16] per 32 weights; weight j = d * ((qs[j] & 0xF) - 8), weight j + 16 = d * ((qs[j] >> 4) - 8),
 * d signed) is accepted under the same shape rules as Q8_0; any other Q4_0 shape is NFAI_ERR_UNSUPPORTED.
 * Q3_K (ggml block_q3_K: hmask[32], qs[64], 12 scale bytes, fp16 d per 256 weights; weight = d * (sc - 32) * (q - 4) with q = two low
 * bits | high bit << 2 and sc a 6-bit scale per 16 weights) is accepted under the same shape rules as Q8_0; any other Q3_K shape is
 * NFAI_ERR_UNSUPPORTED.
 * IQ4_XS (ggml block_iq4_xs: fp16 d, uint16 scales_h, scales_l[4], qs[128] per 256 weights; weight 32 ib + j = d * (ls - 32) * KV[qs[16 ib + j] & 0xF],
 * weight 32 ib + 16 + j = d * (ls - 32) * KV[qs[16 ib + j] >> 4] with ls the 6-bit scale of sub-block ib and KV the 16-entry table
 * {-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113}) is accepted under the same shape rules as Q8_0; any other
 * IQ4_XS shape is NFAI_ERR_UNSUPPORTED. */
enum nfai_dtype { NFAI_F32 = 0, NFAI_F16 = 1, NFAI_Q4_0 = 2, NFAI_Q8_0 = 8, NFAI_Q3_K = 11, NFAI_Q4_K = 12, NFAI_Q5_K = 13, NFAI_Q6_K = 14, NFAI_IQ4_XS = 23 };

const char *nfai_hip_last_error(void);
int32_t nfai_hip_abi_version(void);

/* ---- context: replaces VulkanHelper.CreateVulkanInstance/PickPhysicalDevice/CreateLogicalDevice
 *      (NFAI.Vulkan/VulkanHelper.cs:12-242) + VulkanBufferManager ctor/Dispose
 *      (VulkanBufferManager.cs:20-35, 499-509), as used by LlamaModelFactory.cs:15-32. ---- */
typedef struct nfai_device_info {
    char name[128];
    char arch[64];            /* gcnArchName, must start with "gfx950" */
    uint64_t total_mem_bytes;
    uint32_t compute_units;
    uint32_t wavefront_size;
    uint32_t lds_bytes_per_cu;
    uint32_t clock_khz;
} nfai_device_info;

int32_t nfai_hip_ctx_create(int32_t device_ordinal, nfai_ctx_t *out);
/* Same, but enqueue on a stream owned by the caller (e.g. the stream RCCL point-to-point ops of
 * a pipeline stage run on); `hip_stream` is a hipStream_t. */
int32_t nfai_hip_ctx_create_on_stream(int32_t device_ordinal, void *hip_stream, nfai_ctx_t *out);
int32_t nfai_hip_ctx_destroy(nfai_ctx_t ctx);
int32_t nfai_hip_ctx_synchronize(nfai_ctx_t ctx);   /* ≙ vkQueueWaitIdle, VulkanBufferManager.cs:334 */
int32_t nfai_hip_ctx_device_info(nfai_ctx_t ctx, nfai_device_info *info);
/* Run record: how the rows of the long weight-streaming launches (lm_head, gate | up) are dealt to the 8 XCDs on this device.  The
 * first nfai_hip_llama_finalize on a context times a streaming probe (every workgroup reads an equal share of a 768 MB buffer) and
 * gives the workgroups of each blockIdx % 8 label a share of the rows proportional to their measured rate - a launch ends with its
 * slowest XCD.  Speed only: every row is computed once, by the same arithmetic, whatever the shares.  shares8 / probe_us8: 8 values
 * each (may be NULL); zeros before the first finalize or with NFAI_XCD_DEAL=0.  (No reference counterpart: VulkanHelper.cs:149-150
 * picks a device and never looks at its topology.) */
int32_t nfai_hip_ctx_xcd_shares(nfai_ctx_t ctx, uint16_t *shares8, float *probe_us8);
/* hipEvent pair on the context stream (bench.py times the launches with these, not with
 * torch.cuda.Event, which only sees torch's stream). */
int32_t nfai_hip_timer_begin(nfai_ctx_t ctx);
int32_t nfai_hip_timer_end(nfai_ctx_t ctx, float *elapsed_ms);

/* ---- buffers: replaces VulkanBufferManager.CreateBuffer / DestoryBuffer / UploadDeviceConstants /
 *      UploadDataToDeviceLocal / ReadDeviceBufferData / CopyBuffer
 *      (VulkanBufferManager.cs:42-88, 90-103, 196-244, 105-125, 283-303, 305-318) and the
 *      ShaderProperty<T> storage they back (NFAI.Vulkan.Shaders/ShaderProperty.cs:32-92). ---- */
int32_t nfai_hip_buf_alloc(nfai_ctx_t ctx, uint64_t bytes, nfai_buf_t *out);      /* zero-filled */
int32_t nfai_hip_buf_wrap(nfai_ctx_t ctx, void *device_ptr, uint64_t bytes, nfai_buf_t *out); /* non-owning */
int32_t nfai_hip_buf_free(nfai_ctx_t ctx, nfai_buf_t buf);
int32_t nfai_hip_buf_upload(nfai_ctx_t ctx, nfai_buf_t buf, uint64_t byte_off, const void *host, uint64_t bytes);
int32_t nfai_hip_buf_download(nfai_ctx_t ctx, nfai_buf_t buf, uint64_t byte_off, void *host, uint64_t bytes);
int32_t nfai_hip_buf_copy(nfai_ctx_t ctx, nfai_buf_t dst, uint64_t dst_byte_off, nfai_buf_t src,
                          uint64_t src_byte_off, uint64_t bytes);
int32_t nfai_hip_buf_zero(nfai_ctx_t ctx, nfai_buf_t buf);
int32_t nfai_hip_buf_info(nfai_ctx_t ctx, nfai_buf_t buf, void **device_ptr, uint64_t *bytes);
/* Weights stay in their native GGUF encoding in HBM (fp16 is NOT widened to fp32 as
 * AbstractComputeCollection.cs:62-77 does; the kernels convert in-register — same operand
 * values).  Validates (type, rows, cols) and uploads rows*row_bytes(type, cols) bytes.  Q8_0: rows*cols/32*34 bytes, Q4_0: rows*cols/32*18 bytes, Q3_K: rows*cols/256*110 bytes, IQ4_XS: rows*cols/256*136 bytes, Q5_K:
 * rows*cols/256*176 bytes, only under their shape rules of enum nfai_dtype (NFAI_ERR_UNSUPPORTED otherwise), repacked at upload for
 * the matrix cores. */
int32_t nfai_hip_weight_upload(nfai_ctx_t ctx, int32_t ggml_type, uint64_t n_rows, uint64_t n_cols,
                               const void *host_bytes, nfai_buf_t *out);
int32_t nfai_hip_weight_bytes(int32_t ggml_type, uint64_t n_rows, uint64_t n_cols, uint64_t *bytes);

/* ---- 1:1 operators: one per ShaderWrapper subclass of the reference.  fp32 activations. ---- */
/* TokenEmbedShader.Compute (TokenEmbedShader.cs:108-119, GLSL :131-159): y[0:E] = table[tok][0:E];
 * `tok` is a device buffer holding one uint32.  Q8_0 / Q5_K / Q4_0 / Q3_K / IQ4_XS tables: E %% 256 == 0, uploaded whole with a multiple of 16 rows. */
int32_t nfai_hip_embed(nfai_ctx_t ctx, nfai_buf_t table, int32_t table_type, nfai_buf_t tok, nfai_buf_t y, uint32_t E);
/* RMSNormShader.Compute (RMSNormShader.cs:111-122, GLSL :124-151). */
int32_t nfai_hip_rmsnorm(nfai_ctx_t ctx, nfai_buf_t x, nfai_buf_t gamma, nfai_buf_t y, uint32_t E, float eps);
/* MatrixMultiplyShader.Compute, M = 1 (MatrixMultiplyShader.cs:230-253, GLSL :255-289):
 * y[y_off + j] = sum_k x[k] * W[j][k]; y_off = currentContextSize * N for the KV-cached variant. */
int32_t nfai_hip_gemv(nfai_ctx_t ctx, nfai_buf_t W, int32_t w_type, nfai_buf_t x, nfai_buf_t y,
                      uint64_t y_off, uint32_t N, uint32_t K);
/* RoPEShader.Compute(position) (RoPEShader.cs:188-212, GLSL :231-272) on ONE vector of
 * n_heads*head_dim floats at in[in_off], written to out[out_off] (may alias: the K variant is in
 * place on cache row `pos`, TransformerBlock.cs:73-74).  freqs: rope_dims/2 floats. */
int32_t nfai_hip_rope(nfai_ctx_t ctx, nfai_buf_t in, uint64_t in_off, nfai_buf_t out, uint64_t out_off,
                      nfai_buf_t freqs, uint32_t rope_dims, uint32_t n_heads, uint32_t head_dim, uint32_t pos);
/* AttentionScoreCalculationShader.ComputeAttention(seqLen) (…ScoreCalculationShader.cs:141-162,
 * GLSL :164-206): s[h*S + t], K cache [C][Hkv*D]; only t < S is written. */
int32_t nfai_hip_attn_scores(nfai_ctx_t ctx, nfai_buf_t q, nfai_buf_t kcache, nfai_buf_t s,
                             uint32_t H, uint32_t Hkv, uint32_t D, uint32_t S);
/* AttentionSoftmaxShader.ComputeSoftmax(seqLen) (AttentionSoftmaxShader.cs:117-132, GLSL :139-178). */
int32_t nfai_hip_attn_softmax(nfai_ctx_t ctx, nfai_buf_t s, nfai_buf_t w, uint32_t H, uint32_t S, float eps);
/* AttentionWeightedValueSumShader.ComputeWeightedSum(seqLen) (…ValueSumShader.cs:151-173, GLSL :175-216). */
int32_t nfai_hip_attn_wsum(nfai_ctx_t ctx, nfai_buf_t w, nfai_buf_t vcache, nfai_buf_t o,
                           uint32_t H, uint32_t Hkv, uint32_t D, uint32_t S);
/* SiLUShader.Compute (SiLUShader.cs:92-104, GLSL :106-128). */
int32_t nfai_hip_silu(nfai_ctx_t ctx, nfai_buf_t x, nfai_buf_t y, uint32_t n);
/* ElementWiseMultiplicationShader.Compute (ElementWiseMultiplicationShader.cs:99-119, GLSL :121-139). */
int32_t nfai_hip_mul(nfai_ctx_t ctx, nfai_buf_t a, nfai_buf_t b, nfai_buf_t y, uint32_t n);
/* the two host-side residual adds of TransformerBlock.Compute (TransformerBlock.cs:151-161, 174-181),
 * done on the device instead of read-back/add/upload. */
int32_t nfai_hip_add(nfai_ctx_t ctx, nfai_buf_t a, nfai_buf_t b, nfai_buf_t y, uint32_t n);
/* SamplingUtils.ArgMax (NFAI.Models.Llama3/SamplingUtils.cs:43-57): index of the first maximum,
 * written as one uint32 to `out_idx`. */
int32_t nfai_hip_argmax(nfai_ctx_t ctx, nfai_buf_t x, uint32_t n, nfai_buf_t out_idx);
/* The device half of SamplingUtils.TopP (NFAI.Models.Llama3/SamplingUtils.cs:5-13): values / temperature (:7), Softmax over all n
 * (:8, :35-41), OrderByDescending(Prob) (stable: equal probabilities in index order, :9-12), Take(k) (:13) -> ids_out[k],
 * probs_out[k] (host arrays; k <= 64, the reference's topK is 40).  One launch over the logits and 8k + 8 bytes back instead of n
 * floats; the nucleus cut and the Random.Shared draw (:14-31) stay with the caller.  Blocking. */
int32_t nfai_hip_topk(nfai_ctx_t ctx, nfai_buf_t x, uint32_t n, float temperature, uint32_t k, uint32_t *ids_out, float *probs_out);
/* nfai_hip_topk for `rows` (1..8) vectors of n floats: SamplingUtils.TopP's candidate half (SamplingUtils.cs:7-13) once per row, in ONE
 * pair of launches and one copy back.  x[r] is row r's buffer (rows need not be adjacent in memory; the same buffer may be named more
 * than once); row r's candidates land in ids_out[r * k ..], probs_out[r * k ..] and are bit-identical to nfai_hip_topk on x[r].
 * NFAI_ERR_INVALID: what nfai_hip_topk refuses (k outside [1, min(64, n)], temperature not > 0, n = 0), rows outside [1, 8], a dead
 * buffer, a buffer shorter than n floats, rows * n beyond the context's top-k scratch.  Blocking. */
int32_t nfai_hip_topk_rows(nfai_ctx_t ctx, const nfai_buf_t *x /* [rows] */, uint32_t rows, uint32_t n, float temperature, uint32_t k,
                           uint32_t *ids_out /* [rows][k] */, float *probs_out /* [rows][k] */);
/* Log-probabilities of T rows of fp32 logits ([T][ld], row r at r * ld, V <= ld columns used): per row the log of
 * SamplingUtils.Softmax (SamplingUtils.cs:35-41: exp(l - max) / sum) at targets[r] -> logprob[r], SamplingUtils.ArgMax
 * (SamplingUtils.cs:55-56: the FIRST index of the maximum) -> argmax[r], and the log-probability of that maximum -> logprob_max[r].
 * targets[r] == NFAI_SCORE_NO_TARGET: logprob[r] = 0.  The row is folded into a running state {max, sum exp(l - max), first index
 * of the max, target logit} `slab` columns per pass (0 = all V in one pass; otherwise a multiple of 64, the last pass is shorter):
 * an online softmax, the sum rescaled whenever the maximum moves.  Deterministic for a given slab width; columns at or past V are
 * never read.  NFAI_ERR_INVALID: T or V = 0, ld < V, slab not 0 and not a multiple of 64, a buffer too small, a target >= V that is
 * not NFAI_SCORE_NO_TARGET (found on the device: none of the three outputs is written by that call).  Blocking. */
#define NFAI_SCORE_NO_TARGET 0xFFFFFFFFu
int32_t nfai_hip_score_rows(nfai_ctx_t ctx, nfai_buf_t logits, uint32_t T, uint32_t V, uint32_t ld, uint32_t slab /* columns per pass, 0 = V */,
                            nfai_buf_t targets /* [T] u32 */, nfai_buf_t logprob /* [T] f32 */, nfai_buf_t argmax /* [T] u32 */,
                            nfai_buf_t logprob_max /* [T] f32 */);

/* ---- fused operators (no reference counterpart: each replaces the chain named) ---- */
/* scores -> softmax -> weighted sum in one KV-cache pass, GQA heads sharing each K/V read.
 * K/V caches [C][Hkv*D] (reference layout), kv_type NFAI_F32 or NFAI_F16; D 64 or 128, H/Hkv in {1, 2, 3, 4, 8}, C <= 32768. */
int32_t nfai_hip_attn_decode(nfai_ctx_t ctx, nfai_buf_t q, nfai_buf_t kcache, nfai_buf_t vcache, nfai_buf_t o,
                             uint32_t H, uint32_t Hkv, uint32_t D, uint32_t S, uint32_t C, int32_t kv_type);
/* [RMSNorm ->] GEMV [-> + residual]: y = res + W * (norm ? rmsnorm(x, gamma) : x).  gamma / res
 * may be 0 (absent).  As every GEMV entry point: Q8_0 / Q5_K / Q4_0 / Q3_K / IQ4_XS weights under the rules of enum nfai_dtype (K %% 256 == 0, K <= 32768,
 * a buffer uploaded whole with N %% 16 == 0 rows). */
/* Batched form of MatrixMultiplyShader (inputRowCount = M > 1, which the reference never uses: MatrixMultiplyShader.cs:31-47
 * takes the row count, TransformerBlock.cs:47-101 always passes 1): C[M][N] fp32 (+ residual R, may be 0) = A[M][K] * W[N][K]^T
 * with fp16 operands on the matrix cores — the GEMM of the MFMA prefill, exposed for tests and tools.  variant: 0 = chosen
 * from the shape, 1 = 128x64 tiles, 2 = 128x128 tiles, 3 / 4 = direct-to-LDS staging of 128x128 tiles with 2 / 3 stages (N %% 128 == 0),
 * 5 / 6 / 7 = direct-to-LDS staging of 128x64 tiles with 2 / 3 / 4 stages. */
int32_t nfai_hip_gemm_f16(nfai_ctx_t ctx, nfai_buf_t A_f16, nfai_buf_t W_f16, nfai_buf_t R, nfai_buf_t C, uint32_t M, uint32_t N,
                          uint32_t K, int32_t variant);
/* nfai_hip_gemm_f16 with every epilogue and operand form the MFMA prefill launches (tests / tools; same reference member,
 * MatrixMultiplyShader.cs:31-47 with inputRowCount = M): epi 0 fp32 (+R), 1 fp16, 2 fp16 = up * silu(gate) (SiLUShader.cs:121-123 +
 * ElementWiseMultiplicationShader.cs:137 fused; W = gate rows, W1 = up rows, N = 2F, C is [M][N/2]); head-batched operands
 * A [batch][M][K], W [batch / b_div][N][K], C [batch][M][N]; causal 1: C is a score matrix [t][s], tiles with only s > causal_pos0 + t
 * are skipped (unwritten); causal 2: A is a probability matrix [t][s] (K = keys), K tiles past the last unmasked key are skipped. */
int32_t nfai_hip_gemm_f16_ex(nfai_ctx_t ctx, nfai_buf_t A_f16, nfai_buf_t W_f16, nfai_buf_t W1_f16, nfai_buf_t R, nfai_buf_t C,
                             uint32_t M, uint32_t N, uint32_t K, int32_t variant, int32_t epi, uint32_t batch, uint32_t b_div,
                             uint32_t causal, uint32_t causal_pos0);
/* Causal attention of a prompt chunk in ONE launch (the MFMA prefill's attention; the reference runs AttentionScoreCalculationShader.cs:
 * 164-206, AttentionSoftmaxShader.cs:139-178 and AttentionWeightedValueSumShader.cs:175-216 once per token): Q [T][H*D] fp16 (after
 * RoPE), K [Hkv][Spad][D] fp16, V^T [Hkv][D][Spad] fp16 (rows / columns past pos0 + T zero), O [T][H*D] fp16; query t sees keys
 * 0 .. pos0 + t.  D in {64, 128}, Spad %% 32 == 0, pos0 + T <= Spad. */
int32_t nfai_hip_attn_prefill(nfai_ctx_t ctx, nfai_buf_t Q_f16, nfai_buf_t K_f16, nfai_buf_t Vt_f16, nfai_buf_t O_f16, uint32_t T, uint32_t H,
                              uint32_t Hkv, uint32_t D, uint32_t Spad, uint32_t pos0);
/* The same batched product with W in Q4_K / Q6_K blocks (a buffer from nfai_hip_weight_upload with N %% 16 == 0 rows): the
 * dequant-in-LDS GEMM — quantised bytes -> registers -> fp16 tile in LDS -> MFMA; the weights are never widened in HBM.
 * Q8_0 / Q5_K / Q4_0 / Q3_K / IQ4_XS weights: NFAI_ERR_UNSUPPORTED (the model's prefill widens them to fp16 instead). */
int32_t nfai_hip_gemm_kq(nfai_ctx_t ctx, nfai_buf_t A_f16, nfai_buf_t W, int32_t w_type, nfai_buf_t R, nfai_buf_t C, uint32_t M,
                         uint32_t N, uint32_t K);
int32_t nfai_hip_gemv_fused(nfai_ctx_t ctx, nfai_buf_t W, int32_t w_type, nfai_buf_t x, nfai_buf_t gamma,
                            float eps, nfai_buf_t res, nfai_buf_t y, uint32_t N, uint32_t K);
/* output RMSNorm (gamma may be 0) -> lm_head GEMV -> SamplingUtils.ArgMax in ONE launch (LlamaModel.cs:123-125, SamplingUtils.cs:43-57):
 * V logits and the first index of their maximum (one uint32 in out_idx).  F16 / F32 tables, and IQ4_XS / Q3_K / Q4_0 / Q4_K / Q5_K / Q6_K / Q8_0 tables with
 * V %% 16 == 0 (Q8_0 / Q5_K / Q4_0 / Q3_K / IQ4_XS also E %% 256 == 0, E <= 32768). */
int32_t nfai_hip_lmhead_argmax(nfai_ctx_t ctx, nfai_buf_t W, int32_t w_type, nfai_buf_t x, nfai_buf_t gamma, float eps,
                               nfai_buf_t logits, nfai_buf_t out_idx, uint32_t V, uint32_t E);
/* RMSNorm -> Wgate, Wup GEMVs -> SiLU(gate) * up (TransformerBlock.cs:163-171 in one launch). */
int32_t nfai_hip_gemv_gateup_silu(nfai_ctx_t ctx, nfai_buf_t Wgate, nfai_buf_t Wup, int32_t w_type,
                                  nfai_buf_t x, nfai_buf_t gamma, float eps, nfai_buf_t y,
                                  uint32_t F, uint32_t K);
/* RMSNorm -> Wq, Wk, Wv GEMVs -> RoPE(q), RoPE(k) -> q buffer, K/V cache rows `pos`
 * (TransformerBlock.cs:129-141 in one launch).  Caches [C][Hkv*D]. */
int32_t nfai_hip_gemv_qkv_rope(nfai_ctx_t ctx, nfai_buf_t Wq, nfai_buf_t Wk, nfai_buf_t Wv, int32_t w_type,
                               nfai_buf_t x, nfai_buf_t gamma, float eps, nfai_buf_t freqs,
                               uint32_t rope_dims, nfai_buf_t q, nfai_buf_t kcache, nfai_buf_t vcache,
                               uint32_t H, uint32_t Hkv, uint32_t D, uint32_t pos, int32_t kv_type, uint32_t E);

/* Wo + residual -> RMSNorm + Wgate|Wup + SiLU*up -> Wdown + residual [-> RMSNorm + next block's Wq|Wk|Wv + RoPE + KV write] of one
 * TransformerBlock (TransformerBlock.cs:150-181, then :129-141 of the next block) as ONE launch of the weight-streaming engine
 * (kernels_engine.hip), fp16 weights, E / F / HD multiples of 512, on caller-held buffers: the op-level form of what the model
 * enqueues per block under NFAI_LLAMA_ENGINE.  Wq == 0: the launch ends with Wdown.  K/V caches in the reference layout
 * [C][Hkv*D].  scratch: (2E + F) * 8 + 64 bytes, zeroed once by the caller (hand-off granules {value, tag} of h | act | x, then
 * control words). */
int32_t nfai_hip_engine_block(nfai_ctx_t ctx, nfai_buf_t Wo, nfai_buf_t Wgate, nfai_buf_t Wup, nfai_buf_t Wdown, nfai_buf_t att,
                              nfai_buf_t x_in, nfai_buf_t gamma_ffn, float eps, uint32_t E, uint32_t F, uint32_t HD,
                              nfai_buf_t Wq, nfai_buf_t Wk, nfai_buf_t Wv, nfai_buf_t gamma_next, nfai_buf_t freqs,
                              uint32_t rope_dims, nfai_buf_t q_out, nfai_buf_t kcache, nfai_buf_t vcache, uint32_t H, uint32_t Hkv,
                              uint32_t D, uint32_t pos, int32_t kv_type, nfai_buf_t x_out, nfai_buf_t scratch);

/* ---- model level: replaces LlamaModel (graph LlamaModel.cs:21-68, token loop :99-174) and
 *      TransformerBlock (wiring TransformerBlock.cs:31-125, sequence :127-184). ---- */
enum nfai_llama_flags {
    NFAI_LLAMA_UNFUSED = 1u << 0,   /* run the 16-op chain 1:1 with the reference (parity mode) */
    NFAI_LLAMA_NO_GRAPH = 1u << 1,  /* fused kernels, eager launches (no hipGraph) */
    NFAI_LLAMA_KV_F16 = 1u << 2,    /* fp16 KV cache (default fp32 = the reference's) */
    NFAI_LLAMA_PREFETCH = 1u << 3,  /* side-stream prefetch of the next GEMV's first weight bytes (perf hint only) */
    NFAI_LLAMA_ENGINE = 1u << 4     /* fp16 models: Wo -> gate|up -> Wdown -> next q|k|v of a block as ONE launch of the
                                       weight-streaming engine (kernels_engine.hip) instead of four; same results up to the
                                       summation order.  Ignored (five-launch path) when a tensor is not fp16 or a width is
                                       not a multiple of 512.  The environment variable NFAI_ENGINE=0/1 overrides the flag. */
};

typedef struct nfai_llama_desc {
    uint32_t E, L, H, Hkv, D, F, V;
    uint32_t C;              /* KV capacity = ModelOptions.KVCacheSize (NFAI.Models/ModelOptions.cs:7) */
    float eps;               /* first metadata key containing "epsilon" (LlamaModel.cs:28) */
    float rope_base;         /* reference hard-codes 500000 (TransformerBlock.cs:33) */
    uint32_t rope_dims;      /* llama.rope.dimension_count (LlamaModel.cs:27) */
    uint32_t rope_n_freqs;   /* valid entries of the frequency table: rope_dims/2 = spec-correct;
                                32 reproduces the reference's truncation (TransformerBlock.cs:66) */
    uint32_t layer_begin, layer_end; /* this context's pipeline stage owns blocks [begin, end) */
    uint32_t flags;          /* nfai_llama_flags */
    uint32_t max_batch;      /* prefill chunk capacity in tokens (0 = decode only) */
} nfai_llama_desc;

/* H/Hkv must be 1, 2, 3, 4 or 8 (NFAI_ERR_UNSUPPORTED otherwise) unless NFAI_LLAMA_UNFUSED, which takes any H/Hkv <= 8;
 * D 64 or 128; C <= 32768.
 * RoPE and eps (NFAI_ERR_INVALID otherwise): rope_dims even and <= D; rope_n_freqs <= rope_dims / 2.  Pairs (2i, 2i + 1) with
 * 2i < rope_dims are rotated by pos * rope_base^(-i / (rope_dims / 2)), by angle 0 where i >= rope_n_freqs; the elements at and
 * past rope_dims are left as they are.  rope_dims = 0 means no rotation at all: every kernel then only reads (and ignores)
 * in-bounds entries of tables that are sized by D.  eps is added to the mean square in every RMSNorm (each block's two and the
 * output norm), on every path.  The members of a batch must agree in all four values (NFAI_ERR_UNSUPPORTED from _batch_create*).
 * Tested on every path (tests/test_gpu_desc_forms.py): rope_dims in {0, 6, 24, D / 2, D}, rope_n_freqs full, 5 of 12 and 32 of
 * 64, rope_base 1000, 10000 and 500000, eps 1e-5 and 1e-3. */
int32_t nfai_hip_llama_create(nfai_ctx_t ctx, const nfai_llama_desc *desc, nfai_model_t *out);
int32_t nfai_hip_llama_destroy(nfai_model_t model);
/* GGUF tensor by name ("token_embd.weight", "blk.3.attn_q.weight", ..., "output_norm.weight",
 * optional "output.weight"; absent => lm_head tied to token_embd as LlamaModel.cs:64-67).
 * n_rows x n_cols = ggml ne1 x ne0.  Tensors of blocks outside [layer_begin, layer_end) are
 * ignored.  _set_tensor uploads from host; _set_tensor_device adopts bytes already in HBM.  Q8_0 / Q5_K / Q4_0 / Q3_K / IQ4_XS tensors follow the shape
 * rules of enum nfai_dtype and are repacked into an owned copy by both. */
int32_t nfai_hip_llama_set_tensor(nfai_model_t model, const char *name, int32_t ggml_type,
                                  uint64_t n_rows, uint64_t n_cols, const void *host_bytes);
int32_t nfai_hip_llama_set_tensor_device(nfai_model_t model, const char *name, int32_t ggml_type,
                                         uint64_t n_rows, uint64_t n_cols, void *device_ptr);
int32_t nfai_hip_llama_finalize(nfai_model_t model);
/* Make `model` use the device-resident tensors `donor` already holds (same layer range, no copy, no second K-quant
 * repack): the in-flight sequences (slots) of a pipeline stage are separate models — own KV cache and position — over ONE set
 * of weights.  The reference aliases buffers the same way with ShaderProperty.BindShaderProprty (ShaderProperty.cs:95-108,
 * no reference count): `donor` must outlive `model`.  Call before nfai_hip_llama_finalize(model).
 * Replacing a tensor of `donor` afterwards (_set_tensor + _finalize on the donor) INVALIDATES every model that shares it: the donor
 * frees the storage the sharers still point to, and nothing tells them.  Replace tensors only on a model nobody shares, or destroy
 * the sharers first and share again afterwards.  (A model that replaces its own tensor drops its graphs, engine plans and fp16
 * prefill copies and rebuilds them on the next call; batches and windows over it answer NFAI_ERR_INVALID, "tensors changed", until
 * they are created anew: tests/test_gpu_handoffs.py.) */
int32_t nfai_hip_llama_share_tensors(nfai_model_t model, nfai_model_t donor);
/* ---- what an advancing entry point leaves behind.  A sequence is the model's KV cache, position word, token word, token ring and
 *      hidden-state pointer (_read which = 0).  Every entry point below may follow every other (tests/test_gpu_handoffs.py runs each
 *      ordered pair); n is the number of tokens it ran, "last" the last of them.
 *
 *      entry point                               position   token word          ring              _read(0)
 *      _decode_step, _decode_topk                + 1        ArgMax of the token  + that ArgMax     the token's hidden state
 *      _decode_enqueue, _decode_greedy           + n        last ArgMax          + n ArgMaxes      last token's
 *      _profile_step                             + 1        ArgMax               + 1               the token's
 *      _profile_kernel                           + 1        ArgMax               + 1               unspecified (the replay overwrites
 *                                                                                                  the activation vectors; _read(4),
 *                                                                                                  the logits, are the token's)
 *      _prefill, MFMA path (max_batch > 0)       + n        last token's ArgMax  not written       last token's
 *      _ingest, MFMA path                        + n        unchanged            not written       last token's
 *      _prefill / _ingest, token by token        as n _decode_step calls
 *      _score, MFMA path                         + n        last token's ArgMax  not written       last token's (as _prefill)
 *      _score, M = 1 path                        as n _decode_step calls
 *      _batch_step, _batch_step_topk (member i)  + 1        member i's ArgMax    + 1               member i's own vector
 *      _batch_greedy (member i)                  + n        last ArgMax          + n               last token's
 *      _window_step (t columns)                  + t        last column's ArgMax + t               last column's (held by the window)
 *      _window_verify                            + acc + 1  a_acc                + acc + 1         last emitted column's
 *      _set_pos, _reset                          = pos      unchanged            unchanged         unchanged
 *
 *      "not written": _fetch_tokens over positions the MFMA prefill ran returns whatever the ring held there.  _decode_enqueue
 *      and _stage_step(NFAI_TOKEN_ON_DEVICE) continue from the token word, so behind an MFMA _ingest they feed the ArgMax of the last
 *      token that formed logits; call _set_token first.  K / V rows at or above the position (rejected drafts, a rewound sequence,
 *      the row _profile_kernel's replay writes) are never read and are overwritten by the next token. ---- */
/* One token through embed -> blocks -> output_norm -> lm_head (LlamaModel.cs:116-125) at the
 * current position; logits_host (V floats) and argmax may be NULL.  Blocking. */
int32_t nfai_hip_llama_decode_step(nfai_model_t model, uint32_t token, float *logits_host, uint32_t *argmax);
/* One token as _decode_step, then the candidates of the reference's DEFAULT sampler (LlamaModel.cs:128-130,165 call
 * SamplingUtils.TopP on V logits read back to the host): the k most probable tokens under softmax(logits / temperature) and their
 * probabilities, as nfai_hip_topk.  The caller finishes TopP (SamplingUtils.cs:14-31: nucleus 0.95, renormalise, draw).  Blocking;
 * less than 1 KB crosses PCIe per token. */
int32_t nfai_hip_llama_decode_topk(nfai_model_t model, uint32_t token, float temperature, uint32_t k, uint32_t *ids_out, float *probs_out);
/* Greedy loop with the token fed back on the device (ArgMax in place of the stochastic TopP,
 * SamplingUtils.cs:5-33 vs :43-57): n_steps tokens starting from `first_token`; tokens_out[i] is
 * the argmax after step i.  One hipGraph replay per token, no host round trip. */
int32_t nfai_hip_llama_decode_greedy(nfai_model_t model, uint32_t first_token, uint32_t n_steps, uint32_t *tokens_out);
/* Enqueue n_steps greedy steps without waiting (bench timing region); tokens land in the
 * model's device ring and are fetched with _fetch_tokens after a synchronize. */
int32_t nfai_hip_llama_decode_enqueue(nfai_model_t model, uint32_t n_steps);
int32_t nfai_hip_llama_set_token(nfai_model_t model, uint32_t token);
int32_t nfai_hip_llama_fetch_tokens(nfai_model_t model, uint32_t n, uint32_t *tokens_out);
/* Batched prompt ingestion on the MFMA path (the reference feeds the prompt token by token,
 * LlamaModel.cs:103-126): n tokens at positions pos..pos+n-1; logits of the LAST token.
 * K-quant and Q8_0 models: the first call widens every block's matrices to fp16 copies for the MFMA GEMMs (2 bytes per weight,
 * kept until a tensor is replaced) when all of them fit a quarter of the device's memory, else one block's scratch is re-widened
 * per block (NFAI_PREFILL_WIDE_ALL=0 / 1 forces either); the decode path always streams the quantised blocks.  Under
 * NFAI_PREFILL_FUSED=1 Q4_K / Q6_K matrices go through the dequant-in-LDS GEMM, Q8_0, Q5_K, Q4_0, Q3_K and IQ4_XS matrices are still widened (a Q4_0
 * weight d * (q - 8) is rounded to fp16 there: |d| * 8 must stay below 65504, as |d| * 127 must for Q8_0; a widened IQ4_XS weight is
 * d * (ls - 32) * KV[q] rounded to fp16: |d| * 32 * 127 must stay below 65504). */
int32_t nfai_hip_llama_prefill(nfai_model_t model, const uint32_t *tokens, uint32_t n, float *logits_last_host);
/* The prompt phase of LlamaModel.RunAsync (LlamaModel.cs:103-126 feeds tokenIds one by one and keeps only the LAST token's logits,
 * :128-130): n tokens at positions pos..pos+n-1 leave their K / V rows in the cache, nothing is sampled and no logits are formed
 * (no output norm, no lm_head).  The caller then runs the last prompt token through _decode_step / _decode_topk, whose output IS
 * sampled.  Same engine as _prefill: the MFMA path in chunks of desc.max_batch tokens when the model was created with max_batch > 0
 * (fp16 operands: the cache rows agree with the token-by-token path to the fp16 tolerance, 2e-2 absolute on unit-scale rows), the
 * M = 1 path token by token otherwise (bit-identical to _decode_step).  n == 0 is a no-op.  NFAI_ERR_KV_FULL when pos + n exceeds
 * the KV capacity, before anything runs.  Blocking. */
int32_t nfai_hip_llama_ingest(nfai_model_t model, const uint32_t *tokens, uint32_t n);
/* Score a token sequence: n passes of the loop LlamaModel.cs:116-125, each followed by SamplingUtils.Softmax on its logits
 * (SamplingUtils.cs:35-41; the reference overwrites those logits, LlamaModel.cs:103-126) — here every position's are kept long
 * enough to take, per row i: logprob[i] = log softmax(logits_i)[targets[i]], argmax[i] = SamplingUtils.ArgMax(logits_i)
 * (SamplingUtils.cs:55-56) and logprob_max[i], its log-probability (nfai_hip_score_rows per row).  targets == NULL scores the
 * sequence itself: row i takes tokens[i + 1], the last row no target (logprob[n - 1] = 0); a target NFAI_SCORE_NO_TARGET scores
 * nothing on its row.  Any of the three outputs may be NULL.  Tokens run at positions pos..pos+n-1 and leave their K / V rows.
 * MFMA path (the admission of _prefill, V %% 64 == 0 and an fp16 / IQ4_XS / Q3_K / Q4_0 / Q4_K / Q5_K / Q6_K / Q8_0 head): chunks of max_batch
 * rows through the blocks as _prefill, then per chunk the output norm of all rows and the head as fp16 GEMMs over slabs of 8192
 * vocabulary columns (a quantised head is widened one slab at a time), each folded into the rows' running state: no [n][V] logits
 * and no fp16 copy of the head exist.  The rows' logits come from fp16 operands (normalised row rounded to fp16 x fp16 head,
 * fp32 accumulate): 2e-2 * max(1, max|logit|) per logit, twice that per log-probability.  The last token then runs the head exactly
 * as _prefill does (fp32 GEMV + ArgMax), so the model is left bit for bit where nfai_hip_llama_prefill(tokens, n) leaves it.
 * M = 1 path (anything else): per token the body of _decode_step, then the row kernels on its fp32 logits: the reference's
 * arithmetic; the model is left as n _decode_step calls leave it.
 * Workspace, allocated by the first call and freed with the model: the fp32 slab [max_batch rounded up to 128][min(V, 8192)], the
 * fp16 scratch [min(V, 8192)][E] of a quantised head, 16 bytes of state per row and 16 bytes per KV position for targets and
 * outputs — 16.8 + 50.3 MB at 3B with max_batch 512; the M = 1 path takes the per-position part only.
 * Errors, before anything runs: NFAI_ERR_INVALID for NULL tokens, n = 0, a token >= V, a target >= V that is not
 * NFAI_SCORE_NO_TARGET; NFAI_ERR_KV_FULL when pos + n exceeds the KV capacity; NFAI_ERR_UNSUPPORTED for a pipeline stage that is
 * not the whole network.  Blocking. */
int32_t nfai_hip_llama_score(nfai_model_t model, const uint32_t *tokens, uint32_t n,
                             const uint32_t *targets /* [n] or NULL = tokens[i + 1], last row no target */,
                             float *logprob /* [n] or NULL */, uint32_t *argmax /* [n] or NULL */, float *logprob_max /* [n] or NULL */);
/* Pipeline stage: run this stage's blocks on a hidden state resident in device memory.
 * First stage: hidden_in == NULL and `token` is embedded.  Last stage: lm_head + argmax run and
 * `logits_host`/`argmax` are filled (blocking) when non-NULL.  Otherwise enqueue only. */
#define NFAI_TOKEN_ON_DEVICE 0xFFFFFFFFu /* stage_step: use the token word already in device memory */
int32_t nfai_hip_llama_stage_step(nfai_model_t model, uint32_t token, const void *hidden_in_dev,
                                  void *hidden_out_dev, float *logits_host, uint32_t *argmax);
/* The prompt phase of ONE pipeline stage (LlamaModel.cs:103-126 feeds the prompt token by token through every block; a stage runs
 * the blocks [layer_begin, layer_end) of that loop, :118-121): n prompt tokens at positions pos..pos+n-1 leave their K / V rows in
 * this stage's cache; nothing is sampled, no logits are formed.  The stage's position advances by n: the next _stage_step (the last
 * prompt token, whose output IS sampled, :128-130) continues from there.
 * First stage: `tokens` (host, n entries) are embedded, hidden_in_dev must be NULL.  Other stages: hidden_in_dev = [n][n_embd] fp32
 * (device), tokens must be NULL.  Non-last stage: hidden_out_dev = [n][n_embd] fp32 (device) receives the stage's output rows,
 * which the next stage takes as its hidden_in.  Last stage: hidden_out_dev must be NULL.
 * Engine: with a prefill workspace (desc.max_batch > 0) and the MFMA rules of _ingest (the token-embedding rule on the first stage
 * only), the MFMA prefill in chunks of max_batch rows (same precision as _ingest); otherwise n times the body of _stage_step, row i
 * in -> row i out, bit-identical to n _stage_step calls.  A model that is first AND last stage: exactly nfai_hip_llama_ingest.
 * Ordering: enqueued on the context stream, in order with _stage_step and nfai_hip_pp_*; a non-first stage does not block and makes
 * no host round trip.  The first stage blocks until the copies out of the caller's (pageable) `tokens` have run.
 * K-quant stages: the first call widens the stage's matrices to fp16 as _prefill does (2 bytes per weight of the stage's blocks,
 * kept); slots made with _share_tensors on the same context reuse the donor's copy — one copy per stage, not one per slot.
 * Errors, returned before anything is enqueued: NFAI_ERR_KV_FULL when pos + n exceeds the capacity, NFAI_ERR_INVALID for a token
 * >= V or a missing / superfluous pointer for this stage's role.  n == 0 is a no-op. */
int32_t nfai_hip_llama_stage_ingest(nfai_model_t model, const uint32_t *tokens, const void *hidden_in_dev,
                                    void *hidden_out_dev, uint32_t n);
/* 4-byte device-to-device copies of the model's token word (the last stage's argmax / the first
 * stage's next input), stream-ordered: lets RCCL carry the token between pipeline ends with no
 * host round trip (the reference reads V logits back and samples on the host, LlamaModel.cs:128-130). */
int32_t nfai_hip_llama_token_to_device(nfai_model_t model, void *dst_dev);
int32_t nfai_hip_llama_token_from_device(nfai_model_t model, const void *src_dev);
int32_t nfai_hip_llama_reset(nfai_model_t model);   /* ≙ MatrixMultiplyShader.ResetCache (:153-159) + currentToken = 0 */
int32_t nfai_hip_llama_set_pos(nfai_model_t model, uint32_t pos);
int32_t nfai_hip_llama_pos(nfai_model_t model, uint32_t *pos);
/* Debug / parity: copy an internal activation to host.  which: 0 hidden (E), 1 q after RoPE (H*D),
 * 2 attention output (H*D), 3 ffn activation (F), 4 logits (V). */
int32_t nfai_hip_llama_read(nfai_model_t model, int32_t which, float *host, uint64_t n);
int32_t nfai_hip_llama_read_kv(nfai_model_t model, uint32_t layer, int32_t is_v, uint32_t pos, float *host /* Hkv*D */);
/* Algorithmic HBM bytes one decode step at position `pos` reads+writes (SURVEY.md §8d formula),
 * and the bytes of the dominant (largest) GEMV launch. */
int32_t nfai_hip_llama_bytes_per_token(nfai_model_t model, uint32_t pos, uint64_t *total, uint64_t *dominant_kernel);
/* Per-kernel-class device time (hipEvents around every launch of one eager step; slow path, for
 * bench.py's roofline object).  ids: 0 qkv, 1 attn, 2 wo, 3 gateup, 4 down, 5 lmhead, 6 other. */
int32_t nfai_hip_llama_profile_step(nfai_model_t model, uint32_t token, float *ms_by_class /* 8 */, uint32_t *launches_by_class /* 8 */);
/* Average duration (us) of ONE kernel class: all its launches of a decode step (one per block, each on its own weights)
 * are replayed back to back, `reps` rounds, between a single pair of hipEvents on the launch stream.  This is the per-launch
 * duration rocprofv3 --kernel-trace reports; bench.py's roofline uses it.
 * The token runs at position pos like _profile_step; the replay then runs with the position word already at pos + 1: a replayed
 * q|k|v stores its K / V rows at pos + 1, a replayed attention reads rows 0 .. pos + 1.  Capacity rule: pos + 2 <= desc.C, else
 * NFAI_ERR_KV_FULL before anything runs (position, logits and every cache row untouched).  A token >= n_vocab is NFAI_ERR_INVALID.
 * Afterwards position, token word, ring, logits and every K / V row up to pos are what _decode_step leaves; the row at pos + 1 and
 * the activation vectors (_read 0 .. 3) are unspecified. */
int32_t nfai_hip_llama_profile_kernel(nfai_model_t model, uint32_t token, int32_t kernel_class, uint32_t reps, float *us_avg);

/* ---- batched decode: n sequences advance one token each in ONE pass over the weights.  The reference serves one sequence per
 *      LlamaModel (the token loop LlamaModel.cs:116-125); n conversations are n such loops, each streaming every weight again.  A
 *      batch is a fixed, ordered set of 1..8 models that read the same tensors (a donor and models made with
 *      nfai_hip_llama_share_tensors): every weight row is read once per step and applied to all members' activation vectors, and
 *      member i's KV rows are read and written in member i's own cache at member i's own position.  fp16 matrices, or Q4_K / Q6_K
 *      ones through nfai_hip_llama_batch_create_ex. ---- */
/* ≙ n LlamaModel instances over one set of weights entering the loop LlamaModel.cs:116-125 together.  The batch owns a workspace and
 * its graphs, no weights and no KV cache; creation is cheap.  Members: distinct, finalized, whole models (layer_begin == 0,
 * layer_end == n_layers) on one context, reading the same tensors, all matrices NFAI_F16 (norm gains F32), the fused path (neither
 * NFAI_LLAMA_UNFUSED nor the engine), one KV element type.  NFAI_ERR_INVALID: dead handle, duplicate, n outside [1, 8], different
 * contexts, not finalized.  NFAI_ERR_UNSUPPORTED: K-quant / Q8_0 weights, a pipeline stage, mixed KV types, separate weights, the 1:1
 * or engine path.  nfai_hip_last_error names the member and the reason; nothing stays allocated.  A member stays a normal model:
 * _decode_step, _ingest, _set_pos, _read, _read_kv, _pos work on it between batch steps and see the state the batch left. */
int32_t nfai_hip_llama_batch_create(const nfai_model_t *models, uint32_t n, nfai_batch_t *out);
/* ≙ the same n LlamaModel instances entering the loop LlamaModel.cs:116-125 together, on weights the reference cannot load at all
 * (Parser.cs:111-114 rejects every quantised ggml type).  flags = 0: exactly nfai_hip_llama_batch_create.  NFAI_BATCH_QUANT also
 * admits members whose matrices (token_embd and output included) are all Q4_K or Q6_K in any per-tensor mix, as _set_tensor +
 * _finalize leave them for Q4_K_M files: one step reads every quantised row once, unpacks it once and multiplies it on the matrix
 * cores with the fixed-point activations of all members (kernels_gemv_batch_kqm.hip); a q|k|v whose matrices differ in type runs as
 * two launches.  NFAI_BATCH_QUANT | NFAI_BATCH_QUANT_ANY also admits Q5_K, Q8_0, Q4_0, Q3_K and IQ4_XS matrices (Q5_K_M, Q8_0, Q4_0, Q3_K_S/M and IQ4_XS files), in any
 * per-tensor mix of the seven types; a q|k|v then runs as one launch per type present, three at the most.  NFAI_ERR_INVALID: unknown
 * flag bits, NFAI_BATCH_QUANT_ANY without NFAI_BATCH_QUANT, and everything _batch_create answers so.  Bit 1 is reserved and stays an
 * unknown bit: flags 2 and 3 have always been answered NFAI_ERR_INVALID, and callers may rely on that answer, so no meaning is given
 * to it.  NFAI_ERR_UNSUPPORTED under the flag(s), naming member, tensor and ggml type: Q5_K / Q8_0 / Q4_0 / Q3_K / IQ4_XS matrices without
 * NFAI_BATCH_QUANT_ANY, fp16 and quantised matrices in one model, a quantised matrix whose row count is not a multiple of 16 (the
 * VALU fallback), a shape the kernels' LDS plan does not hold, and every refusal of _batch_create.
 * The handle works with _batch_step, _batch_step_topk, _batch_greedy, _batch_bytes_per_token (quantised bytes: every T16 plane and norm gain once, an
 * embedding row per member where the table is not the head's, each member's KV rows), _batch_profile_step and _batch_destroy. */
enum nfai_batch_flags {
    NFAI_BATCH_QUANT     = 1u << 0,   /* admit members whose matrices are all Q4_K / Q6_K */
    /* 1u << 1 is reserved (see above): it stays an unknown bit */
    NFAI_BATCH_QUANT_ANY = 1u << 2,   /* with NFAI_BATCH_QUANT: also Q5_K, Q8_0, Q4_0, Q3_K and IQ4_XS matrices, any per-tensor mix of the seven */
};
int32_t nfai_hip_llama_batch_create_ex(const nfai_model_t *models, uint32_t n, uint32_t flags, nfai_batch_t *out);
/* ≙ up to 16 LlamaModel instances over one set of weights entering the loop LlamaModel.cs:116-125 together: the wide batch.  Every
 * projection is MatrixMultiplyShader.cs:255-289 at M = B as in _batch_create, run on the matrix cores: a tile of 16 fp16 weight rows
 * is the A operand of v_mfma_f32_16x16x32_f16 straight from HBM, the members' activation vectors are its 16 B columns
 * (kernels_gemv_wide.hip).  The activations stay fp32-class: each x enters as two fp16 operands hi = half(x) and
 * lo = half((x - hi) * 2^11), the two fp32 products are combined as hi + 2^-11 lo; |x| >= 65504 overflows, as in the prefill
 * (tested: activations from 2^-17 of the synthetic models' up to 32768 and subnormal fp16 weights, which the MFMA takes at full value).
 * n: 1 to NFAI_BATCH_WIDE_MAX members; flags must be 0.  Members are admitted as _batch_create admits them (fp16 matrices only: a
 * quantised member is NFAI_ERR_UNSUPPORTED, naming the tensor; member 0's KV element type for all; graph-less members are admitted),
 * with the same answers.  _batch_create and _batch_create_ex keep their limit of 8.  The handle is an ordinary batch: _batch_step,
 * _batch_step_topk, _batch_greedy, _batch_bytes_per_token, _batch_profile_step and _batch_destroy work on it with arrays of n, and
 * after a step every member is exactly where its own _decode_step would have left it. */
#define NFAI_BATCH_WIDE_MAX 16
int32_t nfai_hip_llama_batch_create_wide(const nfai_model_t *models, uint32_t n, uint32_t flags, nfai_batch_t *out);
/* Frees the workspace and the graphs; the members are not touched (≙ leaving the loop LlamaModel.cs:116-125: the models live on). */
int32_t nfai_hip_llama_batch_destroy(nfai_batch_t batch);
/* ≙ one pass of the loop body LlamaModel.cs:116-125 for every member: tokens[i] is embedded, runs through every block at member
 * i's position, lm_head, ArgMax (SamplingUtils.cs:55-56: the first index of the maximum); every member's position advances by one.
 * Blocking: token words in from pinned memory, ONE hipGraphLaunch, ArgMax words and the error word back, one synchronisation.
 * logits_host: [n][n_vocab] fp32 or NULL; argmax: [n] or NULL.  A member at its KV capacity: NFAI_ERR_KV_FULL before anything is
 * enqueued, no member's position moves.  A member destroyed or re-finalized since _batch_create: NFAI_ERR_INVALID. */
int32_t nfai_hip_llama_batch_step(nfai_batch_t batch, const uint32_t *tokens /* [n] */, float *logits_host /* [n][V] or NULL */,
                                  uint32_t *argmax /* [n] */);
/* ≙ one pass of the loop body LlamaModel.cs:116-125 for every member, as _batch_step, then for every member the candidates of the
 * reference's DEFAULT sampler (LlamaModel.cs:128-130,165 call SamplingUtils.TopP on the V logits read back to the host): member i's
 * k most probable tokens under softmax(logits / temperature) and their probabilities (SamplingUtils.cs:5-13) in ids_out[i * k ..],
 * probs_out[i * k ..], exactly what nfai_hip_llama_decode_topk returns for one model and nfai_hip_topk for member i's logits.  The
 * caller finishes TopP per member (SamplingUtils.cs:14-31: nucleus, renormalise, draw).  Blocking: token words in from pinned memory,
 * ONE hipGraphLaunch (the token's launches, two candidate launches for all members, the result words and 520 bytes per member back),
 * one synchronisation; the graph is re-captured when (temperature, k) change.  fp16 and quantised batches alike.  Every argument is
 * checked before anything is enqueued, and a refused call moves no member's position: NFAI_ERR_INVALID for a NULL pointer, a
 * token >= n_vocab, k outside [1, min(64, n_vocab)], a temperature that is not > 0 (NaN included), a member destroyed or re-finalized
 * since _batch_create; NFAI_ERR_KV_FULL for a member at its KV capacity.  Afterwards every member is where _batch_step leaves it:
 * position + 1, logits readable with nfai_hip_llama_read, usable by _decode_step / _batch_step / _batch_greedy. */
int32_t nfai_hip_llama_batch_step_topk(nfai_batch_t batch, const uint32_t *tokens /* [n] */, float temperature, uint32_t k,
                                       uint32_t *ids_out /* [n][k] */, float *probs_out /* [n][k] */);
/* ≙ n_steps passes of LlamaModel.cs:116-125 per member with ArgMax in place of TopP (SamplingUtils.cs:43-57) and the token fed back on
 * the device, as nfai_hip_llama_decode_greedy: member i's ArgMax of step s is its token of step s + 1.  tokens_out[s * n + i]. */
int32_t nfai_hip_llama_batch_greedy(nfai_batch_t batch, const uint32_t *first_tokens /* [n] */, uint32_t n_steps,
                                    uint32_t *tokens_out /* [n_steps][n] */);
/* Algorithmic HBM bytes of ONE batch step at the members' current positions: every weight once, plus per member its
 * embedding row and its KV rows (p + 1 read, 1 written) — against n times nfai_hip_llama_bytes_per_token for n loops LlamaModel.cs:116-125. */
int32_t nfai_hip_llama_batch_bytes_per_token(nfai_batch_t batch, uint64_t *total);
/* One batch step (as _batch_step without results: every member advances) launch by launch between hipEvents: device time and launch
 * count by kernel class, the ids of nfai_hip_llama_profile_step (slow path, for tools/batch_decode_bench.py; the reference has no
 * counterpart: its loop LlamaModel.cs:116-125 is not instrumented). */
int32_t nfai_hip_llama_batch_profile_step(nfai_batch_t batch, const uint32_t *tokens /* [n] */, float *ms_by_class /* 8 */,
                                          uint32_t *launches_by_class /* 8 */);

/* ---- window: up to 8 CONSECUTIVE positions of one sequence in ONE pass over the weights (lossless greedy speculative decoding).
 *      The reference emits one token per pass of the loop LlamaModel.cs:116-125; with SamplingUtils.ArgMax (SamplingUtils.cs:43-57)
 *      in place of TopP the next tokens are a function of the sequence alone, so guessed continuations (drafts) can be run as extra
 *      columns of the batched kernels and kept exactly as far as the model's own ArgMax agrees.  The columns share ONE model: its
 *      weights, its KV cache (the window attention reads the cached prefix once for all columns, kernels_attn_window.hip), its
 *      position word, token word and ring. ---- */
/* ≙ preparing to run up to max_tokens passes of the loop LlamaModel.cs:116-125 of ONE LlamaModel at once.  max_tokens in [2, 8].
 * flags: 0 (all matrices NFAI_F16), NFAI_BATCH_QUANT (all matrices Q4_K / Q6_K) or NFAI_BATCH_QUANT | NFAI_BATCH_QUANT_ANY (all
 * matrices IQ4_XS / Q3_K / Q4_0 / Q4_K / Q5_K / Q6_K / Q8_0).  The model is admitted as _batch_create /
 * _batch_create_ex admit a member, with the same answers: NFAI_ERR_INVALID for a dead handle, max_tokens outside [2, 8], unknown flag
 * bits, a model not finalized; NFAI_ERR_UNSUPPORTED, naming tensor and ggml type, for a pipeline stage, the 1:1 or engine path,
 * Q5_K / Q8_0 / Q4_0 / Q3_K / IQ4_XS matrices without NFAI_BATCH_QUANT_ANY, fp16 and quantised matrices in one model, quantised rows % 16 != 0, a shape the kernels' LDS plan does not
 * hold.  The window owns the columns' activation vectors, workspaces, token / draft / result words, pinned staging and its graphs
 * (one per column count, captured on first use); no weights, no KV cache.  The model stays a normal model: _decode_step, _ingest,
 * _set_pos, _read_kv, _pos between window calls see, and are seen by, the window.  _read: logits are what the model's OWN last token
 * left (a window's logits are returned by the window calls); the hidden state (which = 0) is that of the last token the model kept,
 * whichever path ran it: after a window call the last emitted column's, held by that window until the model's next token or the
 * window's destruction (then the model's own vector again). */
int32_t nfai_hip_llama_window_create(nfai_model_t model, uint32_t max_tokens, uint32_t flags, nfai_window_t *out);
/* Frees the window's memory and graphs; the model is not touched (≙ leaving the loop LlamaModel.cs:116-125: the model lives on). */
int32_t nfai_hip_llama_window_destroy(nfai_window_t window);
/* ≙ t passes of the loop body LlamaModel.cs:116-125 on the caller's tokens: column i carries tokens[i] at position p + i (p = the
 * model's position word on the device): RoPE at p + i, its K / V row written at p + i of the model's cache, attention over rows
 * 0 .. p + i, its own logits and ArgMax (SamplingUtils.cs:55-56: the first index of the maximum).  1 <= t <= max_tokens.  The
 * position advances by t, the token word is the last column's ArgMax, the ring takes all t.  Column i's logits do not depend on t nor
 * on the tokens of the columns after it, bit for bit.  Blocking: ONE hipGraphLaunch and one synchronisation; logits_host adds t
 * device-to-host copies of one row each in front of that synchronisation.  logits_host: [t][n_vocab] fp32 or NULL; argmax: [t] or NULL.  p + t past the KV capacity: NFAI_ERR_KV_FULL before anything is enqueued.  A model
 * destroyed or re-finalized since _window_create: NFAI_ERR_INVALID. */
int32_t nfai_hip_llama_window_step(nfai_window_t window, const uint32_t *tokens /* [t] */, uint32_t t, float *logits_host /* [t][V] or NULL */,
                                   uint32_t *argmax /* [t] or NULL */);
/* ≙ 1 to k + 1 passes of the loop LlamaModel.cs:116-125 with SamplingUtils.ArgMax (SamplingUtils.cs:43-57), decided by the model:
 * the columns are token, draft[0 .. k - 1] (0 <= k <= max_tokens - 1); with a_i column i's ArgMax, acc is the largest j with
 * draft[i] == a_i for all i < j.  *n_out = acc + 1, tokens_out[0 .. acc] = a_0 .. a_acc: exactly the tokens acc + 1 plain greedy
 * steps would emit.  Afterwards the model is where feeding token, a_0 .. a_(acc-1) one by one would have left it: position
 * p + acc + 1, token word a_acc, ring extended by the emitted tokens; K / V rows at or above the position hold rejected drafts, are
 * never read and are overwritten by the next step.  The rule runs on the device in the tail of the lm_head launch: one graph launch,
 * one synchronisation.  logits_host: [k + 1][n_vocab] (all columns) or NULL; tokens_out: [k + 1].  k = 0 is a plain greedy step.
 * Errors as _window_step (the capacity must hold all k + 1 columns). */
int32_t nfai_hip_llama_window_verify(nfai_window_t window, uint32_t token, const uint32_t *draft /* [k] */, uint32_t k,
                                     float *logits_host /* [k+1][V] or NULL */, uint32_t *tokens_out /* [k+1] */, uint32_t *n_out);
/* Algorithmic HBM bytes of ONE window step of t tokens at the model's position p: every weight once, t embedding
 * rows, the p cached K / V rows ONCE, column i's i + 1 window rows, t rows written — against t times
 * nfai_hip_llama_bytes_per_token for t passes of LlamaModel.cs:116-125. */
int32_t nfai_hip_llama_window_bytes_per_step(nfai_window_t window, uint32_t t, uint64_t *total);
/* One window step of t tokens (as _window_step without results: the position advances by t) launch by launch between hipEvents:
 * device time and launch count by kernel class, the ids of nfai_hip_llama_profile_step (slow path, for tools/spec_decode_bench.py; the
 * reference's loop LlamaModel.cs:116-125 is not instrumented). */
int32_t nfai_hip_llama_window_profile_step(nfai_window_t window, const uint32_t *tokens /* [t] */, uint32_t t, float *ms_by_class /* 8 */,
                                           uint32_t *launches_by_class /* 8 */);

/* ---- layer pipeline across GPUs (no reference counterpart: the reference is single-device, it takes the last enumerated
 *      Vulkan device, VulkanHelper.cs:149-150).  One process per GPU owns a contiguous range of TransformerBlocks (a slice of
 *      the block loop LlamaModel.cs:118-121, nfai_llama_desc.layer_begin/end); between stages the hidden state (n_embd fp32)
 *      moves point to point over RCCL/xGMI and the sampled token returns from the last stage to the first.  All operations
 *      are enqueued on the context's stream, in order with nfai_hip_llama_stage_step; RCCL is bound with dlopen on first use
 *      (NFAI_ERR_UNSUPPORTED when it is absent).  Operations that must progress together (one tick of the schedule) are
 *      posted between _begin and _end (ncclGroupStart / ncclGroupEnd). ---- */
int32_t nfai_hip_pp_unique_id(uint8_t *out128);   /* rank 0 creates it; the host hands the 128 bytes to every rank */
int32_t nfai_hip_pp_init(nfai_ctx_t ctx, uint32_t rank, uint32_t world, const uint8_t *unique_id128, nfai_pp_t *out);
int32_t nfai_hip_pp_destroy(nfai_pp_t pp);
int32_t nfai_hip_pp_begin(nfai_pp_t pp);
int32_t nfai_hip_pp_end(nfai_pp_t pp);
int32_t nfai_hip_pp_send_hidden(nfai_pp_t pp, const void *hidden_dev, uint32_t n_floats, uint32_t peer);
int32_t nfai_hip_pp_recv_hidden(nfai_pp_t pp, void *hidden_dev, uint32_t n_floats, uint32_t peer);
int32_t nfai_hip_pp_send_token(nfai_pp_t pp, const void *token_dev, uint32_t peer);   /* one uint32 */
int32_t nfai_hip_pp_recv_token(nfai_pp_t pp, void *token_dev, uint32_t peer);
int32_t nfai_hip_pp_bcast_token(nfai_pp_t pp, void *token_dev, uint32_t root);        /* in place, every rank */
/* A tick's whole exchange in one call: group start, the listed sends / receives, group end (same stream, same semantics as the
 * per-operation entry points between _begin and _end). */
typedef struct nfai_pp_op {
    void *buf;        /* device pointer */
    uint32_t count;   /* floats (kinds 0, 1); ignored for tokens */
    uint32_t peer;
    uint32_t kind;    /* 0 send hidden, 1 receive hidden, 2 send token, 3 receive token */
    uint32_t reserved;
} nfai_pp_op;
int32_t nfai_hip_pp_exchange(nfai_pp_t pp, const nfai_pp_op *ops, uint32_t n_ops);
/* RCCL's own view of the communicator (ncclCommCount, ncclCommUserRank, ncclCommCuDevice) and the device's PCI bus id
 * (32-byte buffer): for run records.  Any output may be NULL. */
int32_t nfai_hip_pp_info(nfai_pp_t pp, uint32_t *nranks, uint32_t *rank, int32_t *device, char *pci_bus_id32);
/* Failure detection (the reference has none: a failed Vulkan call throws, VulkanBufferManager.cs:61-87, and nothing watches a queue).
 * RCCL reports a dead peer or a broken link asynchronously, after the enqueue calls returned.  _check: NFAI_OK, or NFAI_ERR_HIP with
 * RCCL's message and this rank when ncclCommGetAsyncError holds an error.  _wait: the bounded form of "synchronise the stage
 * stream" - polls the stream and the communicator until the stream is idle (NFAI_OK), an asynchronous error shows up, or
 * timeout_ms passes (NFAI_ERR_HIP naming the rank).  _abort: ncclCommAbort - releases operations that can no longer complete so that
 * the process can leave; the handle stays valid for _destroy only. */
int32_t nfai_hip_pp_check(nfai_pp_t pp);
int32_t nfai_hip_pp_wait(nfai_pp_t pp, uint32_t timeout_ms);
int32_t nfai_hip_pp_abort(nfai_pp_t pp);

#ifdef __cplusplus
}
#endif
#endif /* NFAI_HIP_H */
