// llama_prefill.hip — the prompt phase of the model level: chunks of prompt tokens through every block on the MFMA path
// (kernels_prefill.hip), for a whole model (nfai_hip_llama_prefill / _ingest) and for a pipeline stage (nfai_hip_llama_stage_ingest).
#include "llama.h"

using namespace nfai;

// Does the MFMA prefill widen a matrix of this type to fp16?  Every quantised one; under NFAI_PREFILL_FUSED=1 (Q4_K / Q6_K take
// the dequant-in-LDS GEMM) only Q8_0, Q5_K, Q4_0, Q3_K and IQ4_XS, which have no such GEMM.  A widened Q4_0 weight is d * (q - 8) rounded to fp16:
// |d| * 8 must stay below 65504 there, as |d| * 127 must for Q8_0, and |d| * 32 * 4 for a widened Q3_K weight d * (sc - 32) * (q - 4),
// and |d| * 32 * 127 for a widened IQ4_XS weight d * (ls - 32) * KV[q].
static bool prefill_widens(int type, bool fused) { return type != NFAI_F16 && (!fused || type == NFAI_Q8_0_T16 || type == NFAI_Q5_K_T16 || type == NFAI_Q4_0_T16 || type == NFAI_Q3_K_T16 || type == NFAI_IQ4_XS_T16); }

// One chunk of T prompt tokens through every block on the MFMA path (kernels_prefill.hip).  A pipeline stage (nfai_hip_llama_stage_ingest)
// passes hidden_in ([T][E] fp32, device: the previous stage's rows) in place of tokens, and hidden_out ([T][E]) to take this stage's
// output rows; `stage` sets the position word from the stream (no pageable host source behind it).
static int prefill_chunk(Model *m, const uint32_t *tokens, uint32_t T, const float *hidden_in = nullptr, float *hidden_out = nullptr,
                         bool stage = false)
{
    const nfai_llama_desc &d = m->d;
    Model::Prefill &w = m->pf;
    hipStream_t s = m->ctx->stream;
    const uint32_t pos0 = m->pos_host, S = pos0 + T, Spad = (S + 63) / 64 * 64, HD = d.H * d.D, KD = d.Hkv * d.D;
    const uint32_t G = d.H / d.Hkv;
    const int kvf16 = m->kv_f16 ? 1 : 0;
#define P_TRY(expr)                                                                                               \
    do {                                                                                                          \
        hipError_t _e = (expr);                                                                                   \
        if (_e != hipSuccess)                                                                                     \
            return fail(_e == hipErrorInvalidValue ? NFAI_ERR_INVALID : NFAI_ERR_HIP, "prefill: %s failed: %s", #expr, \
                        hipGetErrorString(_e));                                                                   \
    } while (0)
    // One projection: up to three weight tensors side by side in the output columns.  Runs of tensors with the same
    // encoding share a launch (fp16: k_gemm_f16*, T16 K-quants: the dequant-in-LDS k_gemm_kq); a Q4_K_M q|k|v with a
    // Q6_K attn_v is two launches writing two column blocks of the same [T][ldc] buffer.
    // A projection whose K range was split (long chunks, below) may leave its slabs in w.SC for the NEXT block's attention norm to add
    // up (combine + RMSNorm in one pass): pend_ks > 0 until that launch, or the plain combine after the last block, has consumed them.
    uint32_t pend_ks = 0;
    const float *pend_R = nullptr;
    const bool fuse_combine = !(getenv("NFAI_PREFILL_COMBINE_FUSED") && atoi(getenv("NFAI_PREFILL_COMBINE_FUSED")) == 0);   // read per call (a test flips it)
    auto gemm = [&](const void *A, uint32_t lda, const Tensor &W, const Tensor *W1, const Tensor *W2, float *C, const float *R, uint32_t N,
                    uint32_t K, bool may_defer = false) -> hipError_t {
        const Tensor *seg[3] = {&W, W1, W2};
        const int nseg = W2 ? 3 : (W1 ? 2 : 1);
        uint32_t col = 0;
        for (int first = 0; first < nseg;) {
            int last = first;
            while (last + 1 < nseg && seg[last + 1]->type == seg[first]->type) last++;
            GemmArgs g;
            g.A = A; g.lda = lda; g.ldb = K; g.ldc = N; g.M = T; g.K = K;
            g.B = seg[first]->ptr;
            g.N = (uint32_t)seg[first]->rows;
            if (last > first) { g.B1 = seg[first + 1]->ptr; g.n0 = (uint32_t)seg[first]->rows; g.N += (uint32_t)seg[first + 1]->rows; }
            if (last > first + 1) { g.B2 = seg[first + 2]->ptr; g.n1 = (uint32_t)seg[first + 1]->rows; g.N += (uint32_t)seg[first + 2]->rows; }
            g.C = C + col;
            g.R = R ? R + col : nullptr;
            g.n_cu = (uint32_t)m->ctx->prop.multiProcessorCount;
            hipError_t e;
            // Short prompts (17 .. 128 rows; the provider path's templated chat prompts): one row of 128 x BN tiles is N / BN = 48-64
            // workgroups walking all of K — a quarter of the chip, 45 us for Wdown at 3B.  The K range is split over `ks` launches' worth of
            // workgroups instead (the GEMM's batch dimension: batch z multiplies columns [z K / ks, (z + 1) K / ks) of A and W into slab
            // z) and k_sum_slabs adds residual + slabs in order (deterministic).  One tensor, fp16, fp32 output only (Wo, Wdown).
            static const bool split_short = !(getenv("NFAI_PREFILL_SPLITK_SHORT") && atoi(getenv("NFAI_PREFILL_SPLITK_SHORT")) == 0);
            if (split_short && seg[first]->type == NFAI_F16 && nseg == 1 && T <= 128 && g.N % 64 == 0 && C != nullptr) {
                const uint64_t tiles = g.N / 64, n_cu = g.n_cu, sc_floats = (uint64_t)d.H * w.T * w.Spad;
                uint32_t best = 1;
                uint64_t best_cost = ((tiles + n_cu - 1) / n_cu) * K;
                for (uint32_t ks : {2u, 3u, 4u, 6u, 8u}) {
                    if (K % (ks * 128) || K / ks < 512 || (uint64_t)ks * T * g.N > sc_floats) continue;
                    const uint64_t cost = ((tiles * ks + n_cu - 1) / n_cu) * (K / ks);
                    if (cost < best_cost) { best = ks; best_cost = cost; }
                }
                if (best > 1) {
                    GemmArgs gs = g;
                    gs.batch = best; gs.K = K / best; gs.a_bs = K / best; gs.b_bs = K / best; gs.c_bs = (uint64_t)T * g.N;
                    gs.C = w.SC; gs.R = nullptr;
                    if ((e = launch_gemm_f16(gs, s)) != hipSuccess) return e;
                    if ((e = launch_sum_slabs(w.SC, best, (uint64_t)T * g.N, g.R, static_cast<float *>(g.C), s)) != hipSuccess) return e;
                    col += g.N;
                    first = last + 1;
                    continue;
                }
            }
            // Long chunks (>= 256 rows), K >= 8192 (Wdown): four K quarters on 256 x 128 tiles + the ordered combine (tools/gemm_bench.py
            // splitk4-proxy: 37.1 against 47.4 us at 3B before the combine).  NFAI_PREFILL_SPLITK_LONG=0 switches it off.
            static const bool split_long = !(getenv("NFAI_PREFILL_SPLITK_LONG") && atoi(getenv("NFAI_PREFILL_SPLITK_LONG")) == 0);
            if (split_long && seg[first]->type == NFAI_F16 && nseg == 1 && T >= 256 && ((T + 127) / 128) % 2 == 0 && K >= 8192 && K % 256 == 0 && g.N % 128 == 0 &&
                C != nullptr && (uint64_t)4 * T * g.N <= (uint64_t)d.H * w.T * w.Spad) {
                GemmArgs gs = g;
                gs.batch = 4; gs.K = K / 4; gs.a_bs = K / 4; gs.b_bs = K / 4; gs.c_bs = (uint64_t)T * g.N;
                gs.C = w.SC; gs.R = nullptr;
                if ((e = launch_gemm_f16(gs, s)) != hipSuccess) return e;
                if (may_defer && fuse_combine && g.R && d.E % 4 == 0 && d.E <= 4096 && g.N == d.E) {
                    pend_ks = 4;          // the next attention norm (or the tail of the chunk) adds residual + slabs into C = w.X
                    pend_R = g.R;
                } else if ((e = launch_sum_slabs(w.SC, 4, (uint64_t)T * g.N, g.R, static_cast<float *>(g.C), s)) != hipSuccess) {
                    return e;
                }
                col += g.N;
                first = last + 1;
                continue;
            }
            if (seg[first]->type == NFAI_F16) {
                e = launch_gemm_f16(g, s);
            } else {
                g.b_type = seg[first]->type;
                e = launch_gemm_kq(g, s);
            }
            if (e != hipSuccess) return e;
            col += g.N;
            first = last + 1;
        }
        return hipSuccess;
    };
    // K-quant blocks, two implementations.  Default: widen the block's matrices into an fp16 scratch (13 us per matrix) and use
    // the direct-to-LDS fp16 GEMMs — 8.7 ms per 512 tokens at 3B Q4_K_M.  NFAI_PREFILL_FUSED=1: the dequant-in-LDS GEMM
    // (k_gemm_kq: quant bytes -> VGPR -> fp16 tile in LDS, no scratch, no extra HBM traffic) — 9.4 ms: its register-staged A
    // operand and ~80 VALU operations of dequantisation per 16 weights cost more than the widening pass saves (measured).
    static const bool widen = !(getenv("NFAI_PREFILL_FUSED") && atoi(getenv("NFAI_PREFILL_FUSED")));
    const uint32_t QKV = HD + 2 * KD;
    // NFAI_PREFILL_READAHEAD=1 (off by default): read-ahead of the next GEMM's fp16 weights on the side stream (kernels_prefill.hip:
    // k_read_ahead), issued when the GEMM in front of it starts, so at most two matrices' worth of bytes (<= 150 MB at 3B) compete for
    // the 256 MB Infinity Cache.  Built because the projections run 15-40 % faster on cache-resident weights (tools/gemm_bench.py);
    // measured in the prefill it LOSES: 6.39-6.44 ms against 5.93 ms per 512 tokens at 3B — beside a GEMM that lives on L2 hits the
    // read-ahead's own HBM stream costs more than the first-use latency it removes (as the side-stream widening did in round 2).
    static const bool read_ahead = getenv("NFAI_PREFILL_READAHEAD") && atoi(getenv("NFAI_PREFILL_READAHEAD")) == 1;
    size_t ra_ev = 0;
    bool ra_used = false;
    auto ahead = [&](std::initializer_list<const Tensor *> ts) -> int {
        if (!read_ahead || !m->s2) return NFAI_OK;
        bool any = false;
        for (const Tensor *t : ts) any = any || (t->ptr && t->type == NFAI_F16);
        if (!any) return NFAI_OK;
        if (ra_ev >= m->pf_events.size()) {
            hipEvent_t e;
            HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            m->pf_events.push_back(e);
        }
        hipEvent_t ev = m->pf_events[ra_ev++];
        HIP_TRY(hipEventRecord(ev, s));              // everything enqueued so far: the read-ahead starts with the GEMM in front of it
        HIP_TRY(hipStreamWaitEvent(m->s2, ev, 0));
        for (const Tensor *t : ts)
            if (t->ptr && t->type == NFAI_F16) {
                hipError_t e = launch_read_ahead(t->ptr, t->rows * t->cols * 2, (uint32_t)m->ctx->prop.multiProcessorCount, m->s2);
                if (e != hipSuccess) return fail(NFAI_ERR_HIP, "prefill: read-ahead launch failed: %s", hipGetErrorString(e));
            }
        ra_used = true;
        return NFAI_OK;
    };
    if (hidden_in) {   // a later pipeline stage: the previous stage's output rows are this chunk's hidden state
        HIP_TRY(hipMemcpyAsync(w.X, hidden_in, (size_t)T * d.E * 4, hipMemcpyDeviceToDevice, s));
    } else {
        HIP_TRY(hipMemcpyAsync(w.toks, tokens, (size_t)T * 4, hipMemcpyHostToDevice, s));
        if (is_kquant(m->token_embd.type))
            P_TRY(launch_embed_rows_kqt(m->token_embd.ptr, m->token_embd.type, m->token_embd.rows, w.toks, w.X, T, d.E, s));
        else
            P_TRY(launch_embed_rows(m->token_embd.ptr, m->token_embd.type, w.toks, w.X, T, d.E, s));
    }
    // RoPE and the q / KV-cache stores in the q | k | v GEMM's epilogue (fp16 weights, also widened ones); NFAI_PREFILL_ROPE_FUSED=0:
    // GEMM -> fp32 q | k | v -> k_rope_store_tiles (bit-identical results, one launch and a 10 MB round trip more per block)
    const char *env_rf = getenv("NFAI_PREFILL_ROPE_FUSED");
    const bool rope_fused_ok = !(env_rf && atoi(env_rf) == 0) && d.D % 16 == 0 && d.rope_dims % 2 == 0;
    if (rope_fused_ok) P_TRY(launch_rope_table(m->d_freqs, pos0, T, d.D, d.rope_dims, w.CS, s));
    for (Layer &Lq : m->layers) {
        Layer L = Lq;
        WideShadow &wd = *w.wide;
        if (wd.ptr) {   // (NFAI_PREFILL_FUSED=1: allocated only for Q8_0 / Q5_K / Q4_0 / Q3_K / IQ4_XS matrices, ensure_wide_shadow)
            const size_t li = (size_t)(&Lq - m->layers.data());
            const bool kept = wd.all && wd.done[li];  // widened by an earlier chunk / prefill and still current
            uint64_t off = wd.all ? li * wd.slot : 0;
            const uint64_t end = off + wd.slot;
            for (Tensor *tq : {&L.wq, &L.wk, &L.wv, &L.wo, &L.wgate, &L.wup, &L.wdown}) {
                if (!prefill_widens(tq->type, !widen)) continue;
                const uint64_t bytes = tq->rows * tq->cols * 2;
                if (off + bytes > end) return fail(NFAI_ERR_STATE, "prefill: fp16 weight scratch too small");
                void *dst = static_cast<uint8_t *>(wd.ptr) + off;
                if (!kept) P_TRY(launch_dequant_t16_f16(tq->ptr, tq->type, tq->rows, tq->cols, dst, s));
                tq->ptr = dst; tq->type = NFAI_F16; tq->owned = false;
                off += (bytes + 255) / 256 * 256;
            }
            if (wd.all) wd.done[li] = 1;
        }
        if (pend_ks) {   // the previous block's Wdown left residual + K-split slabs: combine -> w.X and normalise in one pass
            P_TRY(launch_rmsnorm_rows_combine(w.SC, pend_ks, pend_R, w.X, static_cast<const float *>(L.attn_norm.ptr), w.XN, T, d.E, d.eps, s));
            pend_ks = 0;
        } else {
            P_TRY(launch_rmsnorm_rows(w.X, static_cast<const float *>(L.attn_norm.ptr), w.XN, T, d.E, d.eps, s));
        }
        S_TRY(ahead({&L.wo}));                                                           // while q | k | v computes
        if (rope_fused_ok && L.wq.type == NFAI_F16 && L.wk.type == NFAI_F16 && L.wv.type == NFAI_F16) {
            GemmArgs g;                                                                  // q | k | v + RoPE + q / cache stores in one launch
            g.A = w.XN; g.lda = d.E; g.ldb = d.E; g.M = T; g.N = QKV; g.K = d.E;
            g.B = L.wq.ptr; g.B1 = L.wk.ptr; g.B2 = L.wv.ptr; g.n0 = HD; g.n1 = KD;
            g.epi = 3;
            g.n_cu = (uint32_t)m->ctx->prop.multiProcessorCount;
            g.rope.cs = w.CS; g.rope.qh = w.QH; g.rope.kh = w.KH; g.rope.vt = w.VT; g.rope.kc = L.kcache; g.rope.vc = L.vcache;
            g.rope.pos_stride = m->kv_pos_stride; g.rope.head_stride = m->kv_head_stride;
            g.rope.H = d.H; g.rope.Hkv = d.Hkv; g.rope.D = d.D; g.rope.rope_dims = d.rope_dims; g.rope.pos0 = pos0; g.rope.Spad = Spad;
            g.rope.kv_f16 = (uint32_t)kvf16;
            P_TRY(launch_gemm_f16(g, s));
        } else {
            P_TRY(gemm(w.XN, d.E, L.wq, &L.wk, &L.wv, w.Q, nullptr, QKV, d.E));          // q | k | v in one launch
            P_TRY(launch_rope_store_rows(w.Q, w.Q + HD, w.Q + HD + KD, w.QH, L.kcache, L.vcache, kvf16, m->kv_pos_stride, m->kv_head_stride,
                                         m->d_freqs, d.rope_dims, d.H, d.Hkv, d.D, pos0, T, QKV, w.KH, w.VT, Spad, s));
        }
        // earlier positions (chunked prompts) and the zero padding; the chunk's own rows were written above
        P_TRY(launch_kv_to_f16(L.kcache, L.vcache, kvf16, m->kv_pos_stride, m->kv_head_stride, w.KH, w.VT, d.Hkv, d.D, S, Spad, pos0, S, s));
        // attention of the chunk.  Default: one launch (k_attn_prefill: scores, causal softmax and weighted V with the probabilities
        // kept in registers); NFAI_PREFILL_FLASH=0: Q.K^T GEMM -> row softmax -> P.V GEMM with materialised scores.
        static const bool flash = !(getenv("NFAI_PREFILL_FLASH") && atoi(getenv("NFAI_PREFILL_FLASH")) == 0);
        if (flash) {
            P_TRY(launch_attn_prefill(w.QH, w.KH, w.VT, w.XN, T, d.H, d.Hkv, d.D, Spad, pos0, s));
        } else {
            {   // scores[h][t][s] = q_h[t] . k_kvh[s]   (scaling and the causal limit are applied by the softmax)
                GemmArgs g;
                g.A = w.QH; g.lda = HD; g.a_bs = d.D;
                g.B = w.KH; g.ldb = d.D; g.b_bs = (uint64_t)Spad * d.D; g.b_div = G;
                g.C = w.SC; g.ldc = Spad; g.c_bs = (uint64_t)T * Spad;
                g.M = T; g.N = Spad; g.K = d.D; g.batch = d.H;
                g.causal = 1; g.causal_pos0 = pos0;
                P_TRY(launch_gemm_f16(g, s));
            }
            P_TRY(launch_softmax_causal_rows(w.SC, w.P, d.H, T, Spad, pos0, 1.0f / sqrtf((float)d.D), s));
            {   // att[t][h*D + d] = sum_s P[h][t][s] * V_kvh[s][d]
                GemmArgs g;
                g.A = w.P; g.lda = Spad; g.a_bs = (uint64_t)T * Spad;
                g.B = w.VT; g.ldb = Spad; g.b_bs = (uint64_t)d.D * Spad; g.b_div = G;
                g.C = w.XN; g.epi = 1; g.ldc = HD; g.c_bs = d.D;   // fp16 straight into the Wo GEMM's A operand
                g.M = T; g.N = d.D; g.K = Spad; g.batch = d.H;
                g.causal = 2; g.causal_pos0 = pos0;
                P_TRY(launch_gemm_f16(g, s));
            }
        }
        S_TRY(ahead({&L.wgate, &L.wup}));                                                // while Wo computes
        P_TRY(gemm(w.XN, HD, L.wo, nullptr, nullptr, w.H1, w.X, d.E, HD));                 // + residual (TransformerBlock.cs:153-158)
        P_TRY(launch_rmsnorm_rows(w.H1, static_cast<const float *>(L.ffn_norm.ptr), w.XN, T, d.E, d.eps, s));
        S_TRY(ahead({&L.wdown}));                                                        // while gate | up computes
        {   // gate | up in one launch, act = up * silu(gate) formed in the GEMM epilogue (fp16 [T][F])
            GemmArgs g;
            g.A = w.XN; g.lda = d.E; g.B = L.wgate.ptr; g.B1 = L.wup.ptr; g.n0 = d.F; g.ldb = d.E;
            g.C = w.ACT; g.epi = 2; g.ldc = d.F;
            g.M = T; g.N = 2 * d.F; g.K = d.E;
            g.n_cu = (uint32_t)m->ctx->prop.multiProcessorCount;
            if (L.wgate.type == NFAI_F16) {
                P_TRY(launch_gemm_f16(g, s));
            } else {
                g.b_type = L.wgate.type;  // finalize() guarantees gate and up share an encoding
                P_TRY(launch_gemm_kq(g, s));
            }
        }
        if (&Lq != &m->layers.back()) {                                                  // while Wdown computes: the next block's q, k, v
            const Layer &N = *(&Lq + 1);
            S_TRY(ahead({&N.wq, &N.wk, &N.wv}));
        }
        P_TRY(gemm(w.ACT, d.F, L.wdown, nullptr, nullptr, w.X, w.H1, d.E, d.F, true));     // + residual (:176-181)
    }
    if (pend_ks) {   // the last block of the stage: nobody normalises behind it
        P_TRY(launch_sum_slabs(w.SC, pend_ks, (uint64_t)T * d.E, pend_R, w.X, s));
        pend_ks = 0;
    }
    if (ra_used) {  // the side stream only reads weights; the join keeps destroy / set_tensor from racing with it
        if (ra_ev >= m->pf_events.size()) {
            hipEvent_t e;
            HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            m->pf_events.push_back(e);
        }
        hipEvent_t ev = m->pf_events[ra_ev++];
        HIP_TRY(hipEventRecord(ev, m->s2));
        HIP_TRY(hipStreamWaitEvent(s, ev, 0));
    }
#undef P_TRY
    // a non-last pipeline stage: its output rows (after the tail combine above) are the next stage's input
    if (hidden_out) HIP_TRY(hipMemcpyAsync(hidden_out, w.X, (size_t)T * d.E * 4, hipMemcpyDeviceToDevice, s));
    // the last token's hidden state continues on the M = 1 path (output norm + lm_head + argmax)
    HIP_TRY(hipMemcpyAsync(m->x, w.X + (size_t)(T - 1) * d.E, (size_t)d.E * 4, hipMemcpyDeviceToDevice, s));
    const uint32_t newpos = pos0 + T;
    if (stage)
        HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(m->d_pos), (int)newpos, 1, s));
    else
        HIP_TRY(hipMemcpyAsync(m->d_pos, &newpos, 4, hipMemcpyHostToDevice, s));
    m->pos_host = newpos;
    m->x_last = m->x;
    return NFAI_OK;
}

// The MFMA prefill's type and shape rules for this model's blocks; the token embedding is read only where the prompt enters (embeds).
static bool prefill_mfma_rules(const Model *m, bool embeds)
{
    if (m->pf.T == 0 || m->unfused) return false;
    const nfai_llama_desc &d = m->d;
    if (d.E % 64 || d.F % 64 || (d.H * d.D) % 64 || (d.Hkv * d.D) % 64) return false;
    const int et = m->token_embd.type;
    if (embeds && et != NFAI_F16 && et != NFAI_F32 && !is_t16(et)) return false;
    for (const Layer &L : m->layers)
        for (const Tensor *t : {&L.wq, &L.wk, &L.wv, &L.wo, &L.wgate, &L.wup, &L.wdown})
            if (t->type != NFAI_F16 && !is_t16(t->type)) return false;
    return true;
}

static bool prefill_mfma_ok(const Model *m) { return m->first_stage && m->last_stage && prefill_mfma_rules(m, true); }

// The fp16 copies of a K-quant model's matrices (WideShadow), allocated at the first prefill of any model that shares them.
static int ensure_wide_shadow(Model *m)
{
    WideShadow &wd = *m->pf.wide;
    if (wd.ptr) return NFAI_OK;
    const bool fused = getenv("NFAI_PREFILL_FUSED") && atoi(getenv("NFAI_PREFILL_FUSED"));
    uint64_t need = 0;
    for (const Layer &L : m->layers) {
        uint64_t b = 0;
        for (const Tensor *t : {&L.wq, &L.wk, &L.wv, &L.wo, &L.wgate, &L.wup, &L.wdown})
            if (prefill_widens(t->type, fused)) b += (t->rows * t->cols * 2 + 255) / 256 * 256;
        need = std::max(need, b);
    }
    if (!need) return NFAI_OK;
    // Keep every block's fp16 copy (widened once, at the first prefill) when all of them fit a quarter of the device's memory
    // and leave 4 GB free: the per-block widening is a quarter of a K-quant prefill (64 us of 230 per block at 3B).  The decode
    // path never reads these copies.  NFAI_PREFILL_WIDE_ALL=0 / 1 forces one slot / all slots.
    const uint64_t all = need * m->layers.size();
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const char *env = getenv("NFAI_PREFILL_WIDE_ALL");
    const bool fits = all + (4ull << 30) <= free_b;
    const bool want = env ? atoi(env) != 0 : all <= total_b / 4;
    wd.all = want && fits;
    wd.slot = need;
    wd.bytes = wd.all ? all : need;
    DALLOC(wd.ptr, wd.bytes);
    wd.done.assign(m->layers.size(), 0);
    return NFAI_OK;
}

// Logits of the LAST prompt token: output norm + lm_head + argmax on its hidden state (m->x).  The position was already advanced
// past the prompt, so the head runs without the token bookkeeping.
static int prefill_head(Model *m)
{
    hipStream_t s = m->ctx->stream;
    LaunchTimer *timer = nullptr;
    const Tensor &head = m->output.ptr ? m->output : m->token_embd;
    GemvArgs a = gemv_base(m, head, m->x, m->d.E);
    a.gamma = static_cast<const float *>(m->output_norm.ptr);
    a.y = m->logits;
    const bool am_fused = head.type == NFAI_F16 || head.type == NFAI_F32 || is_t16(head.type);
    if (am_fused) {  // ArgMax in the lm_head launch, as in a decode step; no bookkeeping: the position was set by the last chunk
        a.argmax_part = static_cast<char *>(m->d_argmax_part) + 4096;
        a.argmax_out = m->d_tok;
    }
    K_TRY(KC_LMHEAD, launch_gemv(a, s));
    if (!am_fused) K_TRY(KC_OTHER, launch_argmax(m->logits, m->d.V, m->d_tok, m->d_argmax_part, nullptr, nullptr, 0, s));
    return NFAI_OK;
}

// head = false: only the KV cache is filled (nfai_hip_llama_ingest: prompt tokens whose output the reference's loop discards).
static int prefill_impl(nfai_model_t h, const uint32_t *tokens, uint32_t n, float *logits_last_host, bool head)
{
    MODEL_OR_FAIL(m, h);
    NEED_FINAL(m);
    if (!tokens || n == 0) return fail(NFAI_ERR_INVALID, "prefill: empty prompt");
    if (m->pos_host + n > m->d.C) return fail(NFAI_ERR_KV_FULL, "prefill: %u tokens from position %u exceed KV capacity %u", n, m->pos_host, m->d.C);
    for (uint32_t i = 0; i < n; i++)
        if (tokens[i] >= m->d.V) return fail(NFAI_ERR_INVALID, "prefill: token %u >= vocab %u", tokens[i], m->d.V);
    if (!prefill_mfma_ok(m)) {
        // no MFMA workspace / non-fp16 weights: the prompt goes through the M = 1 path token by token,
        // exactly as the reference feeds it (LlamaModel.cs:103-126)
        for (uint32_t i = 0; i < n; i++) {
            int rc = nfai_hip_llama_decode_step(h, tokens[i], i + 1 == n ? logits_last_host : nullptr, nullptr);
            if (rc) return rc;
        }
        return NFAI_OK;
    }
    hipStream_t s = m->ctx->stream;
    S_TRY(ensure_wide_shadow(m));   // fp16 scratch for the blocks' matrices (K-quant models)
    for (uint32_t done = 0; done < n;) {
        const uint32_t T = std::min(n - done, m->d.max_batch);
        int rc = prefill_chunk(m, tokens + done, T);
        if (rc) return rc;
        done += T;
    }
    if (head) S_TRY(prefill_head(m));
    if (head && logits_last_host) HIP_TRY(hipMemcpyAsync(logits_last_host, m->logits, (size_t)m->d.V * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));  // `tokens` is the caller's (pageable) memory: the copy into the workspace has left it by now
    return NFAI_OK;
}

NFAI_API int32_t nfai_hip_llama_prefill(nfai_model_t h, const uint32_t *tokens, uint32_t n, float *logits_last_host)
{
    return prefill_impl(h, tokens, n, logits_last_host, true);
}

// The prompt phase of LlamaModel.RunAsync (LlamaModel.cs:103-126): every prompt token but the last only has to leave its K and V
// rows behind — the loop overwrites the logits of token i with those of token i + 1 and samples once, after the last one (:128-130).
NFAI_API int32_t nfai_hip_llama_ingest(nfai_model_t h, const uint32_t *tokens, uint32_t n)
{
    if (n == 0) {   // a one-token prompt has nothing in front of the sampled step
        MODEL_OR_FAIL(m, h);
        NEED_FINAL(m);
        return NFAI_OK;
    }
    return prefill_impl(h, tokens, n, nullptr, false);
}

// ---- nfai_hip_llama_score: the log-probabilities of every position (include/nfai_hip.h) ---------------------------------------------
// Vocabulary columns per pass of the head on the MFMA path: the fp32 slab [pf.T][SCORE_NS] is 16.8 MB at max_batch 512, the fp16
// scratch of a quantised head [SCORE_NS][E] 50.3 MB at E = 3072.
constexpr uint32_t SCORE_NS = 8192;

static bool score_mfma_ok(const Model *m)
{
    if (!prefill_mfma_ok(m) || m->d.V % 64) return false;
    const Tensor &head = m->output.ptr ? m->output : m->token_embd;
    return head.type == NFAI_F16 || is_t16(head.type);
}

// The head over the T hidden rows a prefill_chunk left in w.X: output norm of every row, then per slab of the vocabulary the fp16
// GEMM into the slab buffer and the row kernel that folds it into the rows' state; the finish kernel writes rows [at, at + T) of the
// device output arrays.
static int score_chunk_head(Model *m, uint32_t T, const uint32_t *d_tgt, ScoreState *state, uint32_t *d_err, float *d_lp, uint32_t *d_am, float *d_lpm)
{
    const nfai_llama_desc &d = m->d;
    Model::Prefill &w = m->pf;
    hipStream_t s = m->ctx->stream;
    const Tensor &head = m->output.ptr ? m->output : m->token_embd;
    const uint32_t NS = std::min(d.V, SCORE_NS);
    float *slab = static_cast<float *>(m->d_score_slab);
#define SC_TRY(expr)                                                                                             \
    do {                                                                                                         \
        hipError_t _e = (expr);                                                                                  \
        if (_e != hipSuccess)                                                                                    \
            return fail(_e == hipErrorInvalidValue ? NFAI_ERR_INVALID : NFAI_ERR_HIP, "score: %s failed: %s", #expr, \
                        hipGetErrorString(_e));                                                                  \
    } while (0)
    SC_TRY(launch_rmsnorm_rows(w.X, static_cast<const float *>(m->output_norm.ptr), w.XN, T, d.E, d.eps, s));
    for (uint32_t c0 = 0; c0 < d.V; c0 += NS) {
        const uint32_t ns = std::min(NS, d.V - c0);   // V % 64 == 0: the last slab is a multiple of 64 too
        GemmArgs g;
        g.A = w.XN; g.lda = d.E; g.ldb = d.E; g.M = T; g.N = ns; g.K = d.E;
        g.C = slab; g.ldc = NS;
        g.n_cu = (uint32_t)m->ctx->prop.multiProcessorCount;
        if (head.type == NFAI_F16) {
            g.B = static_cast<const uint8_t *>(head.ptr) + (uint64_t)c0 * d.E * 2;
        } else {   // rows c0 .. c0 + ns of the quantised head, widened (64 | c0, ns: whole tiles of 16 rows)
            SC_TRY(launch_dequant_t16_f16(head.ptr, head.type, head.rows, head.cols, c0 / 16, ns / 16, m->d_score_wide, s));
            g.B = m->d_score_wide;
        }
        SC_TRY(launch_gemm_f16(g, s));
        SC_TRY(launch_score_slab(slab, T, NS, c0, ns, d.V, d_tgt, state, d_err, s));
    }
    SC_TRY(launch_score_finish(state, T, d_tgt, d_err, d_lp, d_am, d_lpm, s));
#undef SC_TRY
    return NFAI_OK;
}

NFAI_API int32_t nfai_hip_llama_score(nfai_model_t h, const uint32_t *tokens, uint32_t n, const uint32_t *targets, float *logprob, uint32_t *argmax,
                                      float *logprob_max)
{
    MODEL_OR_FAIL(m, h);
    NEED_FINAL(m);
    const nfai_llama_desc &d = m->d;
    if (!(m->first_stage && m->last_stage)) return fail(NFAI_ERR_UNSUPPORTED, "score: the model is a pipeline stage, not the whole network");
    if (!tokens || n == 0) return fail(NFAI_ERR_INVALID, "score: empty sequence");
    for (uint32_t i = 0; i < n; i++)
        if (tokens[i] >= d.V) return fail(NFAI_ERR_INVALID, "score: token %u >= vocab %u", tokens[i], d.V);
    if (targets)
        for (uint32_t i = 0; i < n; i++)
            if (targets[i] >= d.V && targets[i] != NFAI_SCORE_NO_TARGET) return fail(NFAI_ERR_INVALID, "score: target %u (row %u) >= vocab %u", targets[i], i, d.V);
    if ((uint64_t)m->pos_host + n > d.C) return fail(NFAI_ERR_KV_FULL, "score: %u tokens from position %u exceed KV capacity %u", n, m->pos_host, d.C);
    const bool mfma = score_mfma_ok(m);
    hipStream_t s = m->ctx->stream;
    // the workspace (sizes: include/nfai_hip.h).  n <= C, a chunk has at most max(1, max_batch) rows.
    const uint32_t rows_max = std::max(1u, d.max_batch), NS = std::min(d.V, SCORE_NS);
    const size_t per_pos = (size_t)d.C * 4;
    if (!m->d_score) DALLOC(m->d_score, 4 * per_pos + (size_t)rows_max * sizeof(ScoreState) + 256);
    if (mfma && !m->d_score_slab) DALLOC(m->d_score_slab, (size_t)m->pf.T * NS * 4);
    const Tensor &head = m->output.ptr ? m->output : m->token_embd;
    if (mfma && head.type != NFAI_F16 && !m->d_score_wide) DALLOC(m->d_score_wide, (size_t)NS * d.E * 2);
    char *base = static_cast<char *>(m->d_score);
    uint32_t *d_tgt = reinterpret_cast<uint32_t *>(base);
    float *d_lp = reinterpret_cast<float *>(base + per_pos);   // the three outputs of THIS call side by side, n words each: one download
    uint32_t *d_am = reinterpret_cast<uint32_t *>(d_lp + n);
    float *d_lpm = d_lp + 2 * (size_t)n;
    ScoreState *state = reinterpret_cast<ScoreState *>(base + 4 * per_pos);
    uint32_t *d_err = reinterpret_cast<uint32_t *>(base + 4 * per_pos + (size_t)rows_max * sizeof(ScoreState));
    std::vector<uint32_t> tgt(n);
    for (uint32_t i = 0; i < n; i++) tgt[i] = targets ? targets[i] : (i + 1 < n ? tokens[i + 1] : NFAI_SCORE_NO_TARGET);
    HIP_TRY(hipMemcpyAsync(d_tgt, tgt.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_err, 0, 4, s));
    if (mfma) {
        S_TRY(ensure_wide_shadow(m));
        for (uint32_t done = 0; done < n;) {
            const uint32_t T = std::min(n - done, d.max_batch);
            S_TRY(prefill_chunk(m, tokens + done, T));
            S_TRY(score_chunk_head(m, T, d_tgt + done, state, d_err, d_lp + done, d_am + done, d_lpm + done));
            done += T;
        }
        S_TRY(prefill_head(m));   // the last token's fp32 logits, ArgMax -> token word: where _prefill leaves the model
    } else {
        // the reference-exact form: per token the body of _decode_step (fp32 activations), the row kernels on its logits
        for (uint32_t i = 0; i < n; i++) {
            S_TRY(step_token_blocking(m, tokens[i]));
            hipError_t e = launch_score_slab(m->logits, 1, d.V, 0, d.V, d.V, d_tgt + i, state, d_err, s);
            if (e == hipSuccess) e = launch_score_finish(state, 1, d_tgt + i, d_err, d_lp + i, d_am + i, d_lpm + i, s);
            if (e != hipSuccess) return fail(NFAI_ERR_HIP, "score: row launch failed: %s", hipGetErrorString(e));
        }
    }
    std::vector<uint32_t> out(3 * (size_t)n);   // one download: logprob | argmax | logprob_max of the n rows
    HIP_TRY(hipMemcpyAsync(out.data(), d_lp, 3 * (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (logprob) memcpy(logprob, out.data(), (size_t)n * 4);
    if (argmax) memcpy(argmax, out.data() + n, (size_t)n * 4);
    if (logprob_max) memcpy(logprob_max, out.data() + 2 * (size_t)n, (size_t)n * 4);
    return NFAI_OK;
}

// The prompt phase of one pipeline stage (LlamaModel.cs:103-126 sliced by layer_begin / layer_end): n prompt tokens' K / V rows,
// chunk by chunk on the MFMA prefill, hidden states in and out as [n][E] fp32 device rows.  See include/nfai_hip.h.
NFAI_API int32_t nfai_hip_llama_stage_ingest(nfai_model_t h, const uint32_t *tokens, const void *hidden_in, void *hidden_out, uint32_t n)
{
    MODEL_OR_FAIL(m, h);
    NEED_FINAL(m);
    if (n == 0) return NFAI_OK;
    const nfai_llama_desc &d = m->d;
    if ((uint64_t)m->pos_host + n > d.C)
        return fail(NFAI_ERR_KV_FULL, "stage_ingest: %u tokens from position %u exceed KV capacity %u", n, m->pos_host, d.C);
    if (m->first_stage) {
        if (!tokens) return fail(NFAI_ERR_INVALID, "stage_ingest: tokens are required on the first stage");
        if (hidden_in) return fail(NFAI_ERR_INVALID, "stage_ingest: the first stage embeds its tokens: hidden_in must be NULL");
        for (uint32_t i = 0; i < n; i++)
            if (tokens[i] >= d.V) return fail(NFAI_ERR_INVALID, "stage_ingest: token %u >= vocab %u", tokens[i], d.V);
    } else {
        if (!hidden_in) return fail(NFAI_ERR_INVALID, "stage_ingest: hidden_in is required on a non-first stage");
        if (tokens) return fail(NFAI_ERR_INVALID, "stage_ingest: a non-first stage takes hidden_in: tokens must be NULL");
    }
    if (m->last_stage && hidden_out) return fail(NFAI_ERR_INVALID, "stage_ingest: the last stage forms no output rows: hidden_out must be NULL");
    if (!m->last_stage && !hidden_out) return fail(NFAI_ERR_INVALID, "stage_ingest: hidden_out is required on a non-last stage");
    if (m->first_stage && m->last_stage) return prefill_impl(h, tokens, n, nullptr, false);   // the whole network: nfai_hip_llama_ingest
    if (m->h_pin[1]) return engine_failed(m, m->h_pin[1]);   // as nfai_hip_llama_stage_step
    hipStream_t s = m->ctx->stream;
    const float *in = static_cast<const float *>(hidden_in);
    float *out = static_cast<float *>(hidden_out);
    if (prefill_mfma_rules(m, m->first_stage)) {
        S_TRY(ensure_wide_shadow(m));
        for (uint32_t done = 0; done < n;) {
            const uint32_t T = std::min(n - done, d.max_batch);
            S_TRY(prefill_chunk(m, m->first_stage ? tokens + done : nullptr, T, in ? in + (size_t)done * d.E : nullptr,
                                out ? out + (size_t)done * d.E : nullptr, true));
            done += T;
        }
    } else {
        // no MFMA workspace / rules not met: the body of nfai_hip_llama_stage_step n times, row i in -> row i out (bit-identical to n
        // stage steps; the launches are enqueued directly instead of through the stage graph, which is captured per buffer pair)
        for (uint32_t i = 0; i < n; i++) {
            if (m->first_stage) S_TRY(set_token_async(m, tokens[i]));
            S_TRY(stage_enqueue(m, in ? in + (size_t)i * d.E : nullptr, out ? out + (size_t)i * d.E : nullptr));
            m->pos_host++;
        }
    }
    // `tokens` is the caller's pageable memory: the first stage returns once every copy out of it has run
    if (m->first_stage) HIP_TRY(hipStreamSynchronize(s));
    return NFAI_OK;
}
