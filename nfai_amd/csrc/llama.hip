// llama.hip — model level of the HIP backend: what LlamaModel (graph: LlamaModel.cs:21-68,
// token loop :99-174) and TransformerBlock (wiring TransformerBlock.cs:31-125, op sequence
// :127-184) do in the reference, for a contiguous range of blocks (a pipeline stage).
//
// Per token the fused path issues, per block, five launches (+ the slice merge of attention):
//   [RMSNorm+Wq,Wk,Wv+RoPE+KV write] -> [attention] -> [Wo + residual]
//   -> [RMSNorm+Wgate,Wup+SiLU*up] -> [Wdown + residual]
// then [RMSNorm+lm_head] -> [argmax + token feedback + position advance].  Position and token
// live in device memory, so the whole token is ONE hipGraph that is replayed unchanged for every
// position, with no host round trip inside a greedy loop.  (The reference: 16 fence-waited
// dispatches and two host read-back/add/upload round trips per block)
#include "llama.h"

using namespace nfai;

namespace nfai {

Model *model_of(nfai_model_t h)
{
    if (!handle_live(h)) return nullptr;
    Model *m = reinterpret_cast<Model *>(h);
    return m->magic == 0x4E464D44 ? m : nullptr;
}

int dalloc(void **p, size_t bytes, hipStream_t s)
{
    const size_t padded = (bytes + 255) & ~(size_t)255;
    hipError_t e = hipMalloc(p, padded);
    if (e != hipSuccess) return fail(NFAI_ERR_OOM, "hipMalloc(%zu) failed: %s", padded, hipGetErrorString(e));
    HIP_TRY(hipMemsetAsync(*p, 0, padded, s));
    return NFAI_OK;
}

GemvArgs gemv_base(Model *m, const Tensor &w, const float *x, uint32_t K)
{
    GemvArgs a;
    a.W[0] = w.ptr;
    a.seg_rows[0] = (uint32_t)w.rows;
    a.w_type = w.type;
    a.x = x;
    a.K = K;
    a.eps = m->d.eps;
    a.n_cu = (uint32_t)m->ctx->prop.multiProcessorCount;
    a.pos_dev = m->d_pos;
    a.xcd_shares = m->ctx->xcd_state == 1 ? m->ctx->xcd_shares : nullptr;   // measured by nfai_hip_llama_finalize (gemv_xcd_calibrate)
    return a;
}

int set_token_async(Model *m, uint32_t tok)
{
    // Pageable source: hipMemcpyAsync stages it before returning, so a stack value is safe.
    HIP_TRY(hipMemcpyAsync(m->d_tok, &tok, 4, hipMemcpyHostToDevice, m->ctx->stream));
    return NFAI_OK;
}

uint64_t tensor_bytes(const Tensor &t) { return t.ptr ? weight_row_bytes(t.type, t.cols) * t.rows : 0; }

uint64_t matrix_bytes(const Layer &L)
{
    return tensor_bytes(L.wq) + tensor_bytes(L.wk) + tensor_bytes(L.wv) + tensor_bytes(L.wo) + tensor_bytes(L.wgate) + tensor_bytes(L.wup) + tensor_bytes(L.wdown);
}

// Every weight byte of the model's blocks and (last stage) its head, once: what one pass reads whatever the number of columns
// (SURVEY.md §8d).  quant (a quantised batch or window): every T16 plane once (a tied token_embd is the head's), and the norm gains
// every normed launch reads.
uint64_t weights_once_bytes(const Model *m, bool quant)
{
    uint64_t b = 0;
    for (const Layer &L : m->layers) b += matrix_bytes(L) + (quant ? tensor_bytes(L.attn_norm) + tensor_bytes(L.ffn_norm) : 0);
    if (m->last_stage) b += tensor_bytes(m->output.ptr ? m->output : m->token_embd);   // tied when output.weight is absent
    if (quant) b += tensor_bytes(m->output_norm);
    return b;
}

// A bounded wait inside a launch gave up (a workgroup was not resident, or a producer never published): the results of that
// token are not valid.  The word is sticky until the model is reset.
int engine_failed(Model *m, uint32_t code)
{
    if (code == 0x1000u)
        return fail(NFAI_ERR_HIP, "attention launch gave up waiting for the partial results of a KV slice (code 0x1000): are all its "
                                  "workgroups resident?  NFAI_ATTN_POLL=0 selects the ticket hand-off");
    return fail(NFAI_ERR_HIP, "engine launch gave up waiting (code 0x%x: 0x10 ring slot, 0x20 activation, 0x40 weights, 0x80 gather, "
                              "0x100-0x400 consumers, 0x1000 attention slices): are all %d workgroups resident?  NFAI_ENGINE=0 selects "
                              "the five-launch path", code, m->ctx->prop.multiProcessorCount);
}

}  // namespace nfai

namespace {

Tensor *find_slot(Model *m, const char *name, bool *ignored)
{
    *ignored = false;
    const std::string n(name);
    if (n == "token_embd.weight") return &m->token_embd;
    if (n == "output_norm.weight") return &m->output_norm;
    if (n == "output.weight") return &m->output;
    if (n == "rope_freqs.weight") { *ignored = true; return nullptr; }  // llama3 scaling factors: the reference ignores them (TransformerBlock.cs:33-38)
    unsigned blk = 0;
    char rest[64] = {0};
    if (sscanf(name, "blk.%u.%63s", &blk, rest) == 2) {
        if (blk < m->d.layer_begin || blk >= m->d.layer_end) { *ignored = true; return nullptr; }
        Layer &L = m->layers[blk - m->d.layer_begin];
        const std::string r(rest);
        if (r == "attn_norm.weight") return &L.attn_norm;
        if (r == "attn_q.weight") return &L.wq;
        if (r == "attn_k.weight") return &L.wk;
        if (r == "attn_v.weight") return &L.wv;
        if (r == "attn_output.weight") return &L.wo;
        if (r == "ffn_norm.weight") return &L.ffn_norm;
        if (r == "ffn_gate.weight") return &L.wgate;
        if (r == "ffn_up.weight") return &L.wup;
        if (r == "ffn_down.weight") return &L.wdown;
    }
    return nullptr;
}

int check_shape(const char *what, const Tensor &t, uint64_t rows, uint64_t cols, bool matrix)
{
    if (!t.ptr) return fail(NFAI_ERR_STATE, "finalize: tensor %s was never set", what);
    if (t.rows != rows || t.cols != cols)
        return fail(NFAI_ERR_INVALID, "finalize: tensor %s is %llux%llu, expected %llux%llu", what, (unsigned long long)t.rows,
                    (unsigned long long)t.cols, (unsigned long long)rows, (unsigned long long)cols);
    if (!matrix && t.type != NFAI_F32) return fail(NFAI_ERR_UNSUPPORTED, "finalize: norm gain %s must be F32 (type %d)", what, t.type);
    if (matrix && t.type != NFAI_F16 && t.type != NFAI_F32 && !is_kquant(t.type))
        return fail(NFAI_ERR_UNSUPPORTED, "finalize: matrix %s has ggml type %d; kernels exist for F16/F32/IQ4_XS/Q3_K/Q4_0/Q4_K/Q5_K/Q6_K/Q8_0", what, t.type);
    return NFAI_OK;
}

struct Sched {
    Model *m;
    LaunchTimer *timer;              // null: the step is not profiled
    bool have = false;
    Op pending;
    size_t ev_i = 0;

    int launch_now(const Op &op)
    {
        hipStream_t s = m->ctx->stream;
        if (timer) S_TRY(timer->begin(op.cls));
        hipError_t e = op.kind == 0 ? launch_gemv(op.g, s) : (op.kind == 1 ? launch_attn_decode(op.a, s) : op.f(s));
        if (e != hipSuccess)
            return fail(e == hipErrorInvalidValue ? NFAI_ERR_INVALID : NFAI_ERR_HIP, "launch (class %d) failed: %s", op.cls,
                        hipGetErrorString(e));
        if (timer) S_TRY(timer->end());
        if (timer && m->prof_rep_cls == op.cls) m->prof_ops.push_back(op);  // replayed by profile_kernel
        return NFAI_OK;
    }
    int submit(const Op &op)
    {
        if (have) {
            const bool pf = m->prefetch && !timer && op.kind == 0 && op.g.w_type == NFAI_F16;
            if (pf) {
                if (ev_i >= m->pf_events.size()) {
                    hipEvent_t e;
                    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                    m->pf_events.push_back(e);
                }
                hipEvent_t ev = m->pf_events[ev_i++];
                HIP_TRY(hipEventRecord(ev, m->ctx->stream));       // everything before `pending`
                HIP_TRY(hipStreamWaitEvent(m->s2, ev, 0));
                GemvArgs g = op.g;
                g.prefetch_only = true;
                hipError_t e = launch_gemv(g, m->s2);
                if (e != hipSuccess) return fail(NFAI_ERR_HIP, "prefetch launch failed: %s", hipGetErrorString(e));
                m->s2_used = true;
            }
            int rc = launch_now(pending);
            if (rc) return rc;
        }
        pending = op;
        have = true;
        return NFAI_OK;
    }
    int flush()
    {
        if (have) {
            int rc = launch_now(pending);
            if (rc) return rc;
            have = false;
        }
        if (m->s2_used) {  // join the side stream (required to end a capture; harmless otherwise)
            if (ev_i >= m->pf_events.size()) {
                hipEvent_t e;
                HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                m->pf_events.push_back(e);
            }
            hipEvent_t ev = m->pf_events[ev_i++];
            HIP_TRY(hipEventRecord(ev, m->s2));
            HIP_TRY(hipStreamWaitEvent(m->ctx->stream, ev, 0));
            m->s2_used = false;
        }
        return NFAI_OK;
    }
};

static Op op_gemv(int cls, const GemvArgs &g) { Op o; o.kind = 0; o.cls = cls; o.g = g; return o; }
static Op op_attn(int cls, const AttnArgs &a) { Op o; o.kind = 1; o.cls = cls; o.a = a; return o; }
static Op op_fn(int cls, std::function<hipError_t(hipStream_t)> f) { Op o; o.kind = 2; o.cls = cls; o.f = std::move(f); return o; }

// [RMSNorm + Wq, Wk, Wv + RoPE + KV write] of block L on the activation vector x (TransformerBlock.cs:129-141).
// One launch when q, k, v share an encoding; Q4_K_M files keep attn_v in Q6_K on some blocks: then the segments that differ get
// their own launch (same kernel family, same epilogue).  A Q8_0 segment is never mixed with K-quant segments: it shares a launch only
// with other Q8_0 segments.  Q5_K_M files keep attn_v in Q6_K the same way: Q5_K and Q6_K segments share a launch (NFAI_KQ_MIXED5);
// Q4_K and Q5_K segments never do.  A Q4_0 segment stages its activations as Q4_K does (same A fragments and sums of x', t16.h), but
// its step has another register shape and epilogue than the mixed kernel's Q4_K branch, and no common file type mixes Q4_0 with
// K-quants inside q|k|v: like Q8_0 it shares a launch only with other Q4_0 segments, every other type beside it gets a launch of
// its own.  A Q3_K segment (Q3_K_M files: q and k in Q3_K beside a Q4_K or Q5_K v) stages as Q6_K does, with its own register shape
// and epilogue: the same rule, it shares a launch only with other Q3_K segments.  An IQ4_XS segment stages as
// Q4_K does, as Q4_0, with a register shape and an unpack (the codebook lookup) of its own: the same rule again (an IQ4_XS file keeps
// attn_v in Q5_K when H / Hkv >= 4: two q|k|v launches per block then).  qkv_launch: the launch that starts at segment `first` (-> `last`).
GemvArgs qkv_launch(Model *m, Layer &L, const float *x, int first, int &last)
{
    const nfai_llama_desc &d = m->d;
    const Tensor *seg[3] = {&L.wq, &L.wk, &L.wv};
    auto t16 = [](int ty) { return ty == NFAI_Q4_K_T16 || ty == NFAI_Q6_K_T16; };  // the K-quants of the mixed kernel
    auto t16q5 = [](int ty) { return ty == NFAI_Q5_K_T16 || ty == NFAI_Q6_K_T16; };  // ... of its Q5_K form
    last = first;
    // segments of one encoding share a launch; so do T16 Q4_K and Q6_K segments (mixed kernel, kernels_gemv_kqm.hip), and T16 Q5_K and
    // Q6_K segments.  `fam`: the family the launch has committed to (0 none yet, 4 or 5 once it holds a Q4_K or a Q5_K segment).
    int fam = seg[first]->type == NFAI_Q4_K_T16 ? 4 : (seg[first]->type == NFAI_Q5_K_T16 ? 5 : 0);
    while (last + 1 < 3) {
        const int nt = seg[last + 1]->type, ft = seg[first]->type;
        const int nfam = nt == NFAI_Q4_K_T16 ? 4 : (nt == NFAI_Q5_K_T16 ? 5 : 0);
        const bool joins = nt == ft || (t16(nt) && t16(ft) && fam != 5 && nfam != 5) || (t16q5(nt) && t16q5(ft) && fam != 4 && nfam != 4);
        if (!joins) break;
        if (nfam) fam = nfam;
        last++;
    }
    GemvArgs a = gemv_base(m, *seg[first], x, d.E);
    for (int i = first; i <= last; i++) {
        if (seg[i]->type != seg[first]->type) a.w_type = fam == 5 ? NFAI_KQ_MIXED5 : NFAI_KQ_MIXED;
        if (seg[i]->type == NFAI_Q6_K_T16) a.seg6_mask |= 1u << i;
    }
    for (int i = 0; i < 3; i++) {
        const bool in = i >= first && i <= last;
        a.W[i] = in ? seg[i]->ptr : seg[first]->ptr;
        a.seg_rows[i] = in ? (uint32_t)seg[i]->rows : 0;
    }
    a.gamma = static_cast<const float *>(L.attn_norm.ptr);
    a.mode = GEMV_QKV_ROPE;
    a.y = m->q;
    a.kcache = L.kcache; a.vcache = L.vcache;
    a.kv_type = m->kv_f16 ? NFAI_F16 : NFAI_F32;
    a.kv_pos_stride = m->kv_pos_stride; a.kv_head_stride = m->kv_head_stride;
    a.rope_cs = m->d_ropecs; a.rope_dims = d.rope_dims;
    a.H = d.H; a.Hkv = d.Hkv; a.D = d.D;
    return a;
}

int submit_qkv(Model *m, Layer &L, const float *x, Sched &sch, const GemvArgs::Begin *begin = nullptr)
{
    for (int first = 0; first < 3;) {
        int last;
        GemvArgs a = qkv_launch(m, L, x, first, last);
        if (begin && first == 0) a.begin = *begin;  // the token's first launch also does the per-token prologue
        S_TRY(sch.submit(op_gemv(KC_QKV, a)));
        first = last + 1;
    }
    return NFAI_OK;
}

// scores + softmax + weighted V of block L in one launch (TransformerBlock.cs:144-148)
AttnArgs attn_args(Model *m, Layer &L)
{
    const nfai_llama_desc &d = m->d;
    AttnArgs a;
    a.q = m->q; a.kcache = L.kcache; a.vcache = L.vcache;
    a.kv_type = m->kv_f16 ? NFAI_F16 : NFAI_F32;
    a.kv_pos_stride = m->kv_pos_stride; a.kv_head_stride = m->kv_head_stride;
    a.o = m->att; a.H = d.H; a.Hkv = d.Hkv; a.D = d.D; a.C = d.C;
    a.pos_dev = m->d_pos; a.partials = m->d_attn_part;
    a.n_cu = (uint32_t)m->ctx->prop.multiProcessorCount;
    // slice hand-off by {value, tag} granules: tag = token epoch x blocks + block (never the tag of an earlier launch on this workspace)
    a.epoch = m->attn_ticket ? nullptr : m->d_epoch;
    a.tag_mul = (uint32_t)m->layers.size() + 1; a.tag_add = (uint32_t)(&L - m->layers.data()) + 1; a.err = m->d_engerr;
    a.debug_withhold = m->dbg_withhold;
    return a;
}

int submit_attn(Model *m, Layer &L, Sched &sch) { return sch.submit(op_attn(KC_ATTN, attn_args(m, L))); }

// One block, fused path (TransformerBlock.cs:127-184 in five launches + the attention merge).
int block_fused(Model *m, Layer &L, Sched &sch, const GemvArgs::Begin *begin = nullptr)
{
    const nfai_llama_desc &d = m->d;
    S_TRY(submit_qkv(m, L, m->x, sch, begin));
    {
        GemvArgs a = gemv_base(m, L.wo, m->att, d.H * d.D);
        a.mode = GEMV_RESIDUAL; a.res = m->x; a.y = m->h;
        const AttnArgs at = attn_args(m, L);
        if (attn_wo_ok(at, a)) {  // attention + Wo + residual in one launch (fp16 Wo, the shapes of kernels_attn.hip's table)
            S_TRY(sch.submit(op_fn(KC_ATTN, [at, a](hipStream_t st) { return launch_attn_wo(at, a, st); })));
        } else {
            S_TRY(sch.submit(op_attn(KC_ATTN, at)));
            S_TRY(sch.submit(op_gemv(KC_WO, a)));
        }
    }
    {
        GemvArgs a = gemv_base(m, L.wgate, m->h, d.E);
        a.W[1] = L.wup.ptr; a.seg_rows[1] = (uint32_t)L.wup.rows;
        a.gamma = static_cast<const float *>(L.ffn_norm.ptr);
        a.mode = GEMV_GATEUP; a.y = m->act;
        S_TRY(sch.submit(op_gemv(KC_GATEUP, a)));
    }
    {
        GemvArgs a = gemv_base(m, L.wdown, m->act, d.F);
        a.mode = GEMV_RESIDUAL; a.res = m->h; a.y = m->x;
        S_TRY(sch.submit(op_gemv(KC_DOWN, a)));
    }
    return NFAI_OK;
}

// The engine path (kernels_engine.hip) needs every matrix of every block in fp16 and every K a multiple of 512 (one LDS-DMA
// piece = 512 weights of one row), every gathered vector a multiple of 128 granules, and one workgroup per CU.
bool engine_ok(const Model *m)
{
    if (!m->engine || m->unfused || !m->d_gran) return false;
    const nfai_llama_desc &d = m->d;
    const uint32_t HD = d.H * d.D;
    if (d.E % 512 || d.F % 512 || HD != d.E || (d.Hkv * d.D) % 2 || (d.E != 512 && d.E != 1024 && d.E != 2048 && d.E != 3072 && d.E != 4096)) return false;
    if ((2 * (size_t)d.E + std::max(HD, d.F)) * 4 + 2048 > 160 * 1024 || d.D > 128) return false;  // LDS: the three activation vectors
    for (const Layer &L : m->layers)
        for (const Tensor *t : {&L.wq, &L.wk, &L.wv, &L.wo, &L.wgate, &L.wup, &L.wdown})
            if (t->type != NFAI_F16) return false;
    return true;
}

// One block as the reference's 16-dispatch chain, op for op (parity mode; needs the host copy
// of the position because the 1:1 kernels take it by value).
int block_unfused(Model *m, Layer &L, LaunchTimer *timer)
{
    const nfai_llama_desc &d = m->d;
    hipStream_t s = m->ctx->stream;
    const uint32_t p = m->pos_host, S = p + 1, HD = d.H * d.D, KD = d.Hkv * d.D;
    float *krow = static_cast<float *>(L.kcache) + (uint64_t)p * KD;
    float *vrow = static_cast<float *>(L.vcache) + (uint64_t)p * KD;
    const float *an = static_cast<const float *>(L.attn_norm.ptr), *fn = static_cast<const float *>(L.ffn_norm.ptr);
    K_TRY(KC_OTHER, launch_rmsnorm(m->x, an, m->xn, d.E, d.eps, s));                         // :129
    { GemvArgs a = gemv_base(m, L.wq, m->xn, d.E); a.y = m->qraw; K_TRY(KC_QKV, launch_gemv(a, s)); }   // :131
    { GemvArgs a = gemv_base(m, L.wk, m->xn, d.E); a.y = krow; K_TRY(KC_QKV, launch_gemv(a, s)); }      // :133
    { GemvArgs a = gemv_base(m, L.wv, m->xn, d.E); a.y = vrow; K_TRY(KC_QKV, launch_gemv(a, s)); }      // :135
    K_TRY(KC_OTHER, launch_rope(m->qraw, m->q, m->d_freqs, d.rope_dims, d.H, d.D, p, s));    // :138
    K_TRY(KC_OTHER, launch_rope(krow, krow, m->d_freqs, d.rope_dims, d.Hkv, d.D, p, s));     // :141
    K_TRY(KC_ATTN, launch_attn_scores(m->q, static_cast<const float *>(L.kcache), m->scores, d.H, d.Hkv, d.D, S, s));  // :144
    K_TRY(KC_ATTN, launch_attn_softmax(m->scores, m->wts, d.H, S, d.eps, s));                // :146
    K_TRY(KC_ATTN, launch_attn_wsum(m->wts, static_cast<const float *>(L.vcache), m->att, d.H, d.Hkv, d.D, S, s));     // :148
    { GemvArgs a = gemv_base(m, L.wo, m->att, HD); a.y = m->proj; K_TRY(KC_WO, launch_gemv(a, s)); }    // :150
    K_TRY(KC_OTHER, launch_add(m->x, m->proj, m->h, d.E, s));                                // :153-158
    K_TRY(KC_OTHER, launch_rmsnorm(m->h, fn, m->xn, d.E, d.eps, s));                         // :163
    { GemvArgs a = gemv_base(m, L.wup, m->xn, d.E); a.y = m->up; K_TRY(KC_GATEUP, launch_gemv(a, s)); }     // :165
    { GemvArgs a = gemv_base(m, L.wgate, m->xn, d.E); a.y = m->gate; K_TRY(KC_GATEUP, launch_gemv(a, s)); } // :167
    K_TRY(KC_OTHER, launch_silu(m->gate, m->gate, d.F, s));                                  // :169
    K_TRY(KC_OTHER, launch_mul(m->up, m->gate, m->act, d.F, s));                             // :171
    { GemvArgs a = gemv_base(m, L.wdown, m->act, d.F); a.y = m->proj; K_TRY(KC_DOWN, launch_gemv(a, s)); }  // :173
    K_TRY(KC_OTHER, launch_add(m->h, m->proj, m->x, d.E, s));                                // :176-181
    return NFAI_OK;
}

// Where one token of this model leaves its hidden state: the engine's blocks alternate between m->x and m->h, every other path ends in
// m->x.  A replayed graph does not pass through enqueue_token, so every entry point that runs a token sets m->x_last from here: a
// window or a batch may have pointed it into its own workspace since the graph was captured.
const float *x_after_token(const Model *m)
{
    if (engine_ok(m) && m->eng_plans.size() == m->layers.size()) return ((m->layers.size() - 1) & 1) ? m->x : m->h;
    return m->x;
}

}  // namespace

namespace nfai {

// Everything one token needs on this stage, enqueued on the stream.  Reads token/pos from device.
int enqueue_token(Model *m, bool with_head, LaunchTimer *timer)
{
    const nfai_llama_desc &d = m->d;
    hipStream_t s = m->ctx->stream;
    const uint32_t nfreq = (d.rope_dims < d.D ? d.rope_dims : d.D) / 2;
    const bool emb_kq = is_kquant(m->token_embd.type);
    // The per-token prologue (embedding row -> x, cos/sin table of the position, hand-off epoch: TokenEmbedShader + what
    // RoPEShader.cs:254-256 recomputes per element) rides on the first q|k|v launch of the token when that launch is one of
    // the streaming GEMV kernels and the table is in a layout they read; otherwise it is its own launch.
    GemvArgs::Begin begin;
    {
        auto streams = [](int ty) { return ty == NFAI_F16 || ty == NFAI_F32 || is_t16(ty); };
        const int et = m->token_embd.type;
        static const bool env_off = getenv("NFAI_BEGIN_FUSED") && atoi(getenv("NFAI_BEGIN_FUSED")) == 0;
        const bool engine_path = engine_ok(m) && m->eng_plans.size() == m->layers.size();
        int last0;
        const GemvArgs first_qkv = qkv_launch(m, m->layers[0], m->x, 0, last0);
        begin.on = !env_off && !m->unfused && !engine_path && gemv_begin_ok(first_qkv) && nfreq * 2 <= 128 &&
                   (!m->first_stage || streams(et)) && (!m->first_stage || !is_t16(et) || d.E % 256 == 0);
        if (begin.on) {
            if (m->first_stage) {
                begin.emb = m->token_embd.ptr; begin.emb_type = et; begin.emb_rows = m->token_embd.rows;
                begin.tok = m->d_tok; begin.x_out = m->x;
            }
            begin.freqs = m->d_freqs; begin.cs_out = m->d_ropecs; begin.n_freq = nfreq; begin.epoch = m->d_epoch;
        }
    }
    if (!begin.on) {
        if (m->first_stage && emb_kq)
            K_TRY(KC_OTHER, launch_embed_kq(m->token_embd.ptr, m->token_embd.type, m->token_embd.rows, m->d_tok, m->x, d.E, s));
        K_TRY(KC_OTHER, launch_token_begin(m->first_stage && !emb_kq ? m->token_embd.ptr : nullptr, m->token_embd.type, m->d_tok, m->x, d.E,
                                           m->d_freqs, m->d_ropecs, nfreq, m->d_pos, s, m->d_epoch));
    }
    if (m->unfused) {
        for (Layer &L : m->layers) {
            int rc = block_unfused(m, L, timer);
            if (rc) return rc;
        }
        if (m->last_stage && with_head) {
            const Tensor &head = m->output.ptr ? m->output : m->token_embd;  // tied when output.weight is absent (LlamaModel.cs:64-67)
            K_TRY(KC_OTHER, launch_rmsnorm(m->x, static_cast<const float *>(m->output_norm.ptr), m->xn, d.E, d.eps, s));
            GemvArgs a = gemv_base(m, head, m->xn, d.E);
            a.y = m->logits;
            K_TRY(KC_LMHEAD, launch_gemv(a, s));
            K_TRY(KC_OTHER, launch_argmax(m->logits, d.V, m->d_tok, m->d_argmax_part, m->d_pos, m->d_ring, RING_LEN, s));
        } else {
            K_TRY(KC_OTHER, launch_pos_advance(m->d_pos, s));
        }
        return NFAI_OK;
    }
    Sched sch{m, timer};
    const float *x_final = x_after_token(m);
    if (engine_ok(m) && m->eng_plans.size() == m->layers.size()) {
        // [q|k|v of the first block] then per block [attention] [engine: Wo -> gate|up -> Wdown -> next block's q|k|v].
        // The block input / output alternate between m->x and m->h so that no CU overwrites a vector another CU still reads.
        S_TRY(submit_qkv(m, m->layers[0], m->x, sch));
        for (size_t i = 0; i < m->layers.size(); i++) {
            Layer &L = m->layers[i];
            float *xin = (i & 1) ? m->h : m->x, *xout = (i & 1) ? m->x : m->h;
            S_TRY(submit_attn(m, L, sch));
            const EnginePlan plan = m->eng_plans[i];
            S_TRY(sch.submit(op_fn(KC_ENGINE, [plan](hipStream_t st) { return launch_engine(plan, st); })));
        }
    } else {
        for (Layer &L : m->layers) {
            int rc = block_fused(m, L, sch, (begin.on && &L == &m->layers[0]) ? &begin : nullptr);
            if (rc) return rc;
        }
    }
    m->x_last = x_final;
    if (m->last_stage && with_head) {
        const Tensor &head = m->output.ptr ? m->output : m->token_embd;
        GemvArgs a = gemv_base(m, head, x_final, d.E);
        a.gamma = static_cast<const float *>(m->output_norm.ptr);
        a.y = m->logits;
        // SamplingUtils.ArgMax + the end-of-token bookkeeping ride on the lm_head launch (LlamaModel.cs:125-130 in one launch): the
        // streaming GEMV kernels take it; the fallback kernel for K-quant tensors whose rows are not a multiple of 16 does not
        const bool am_fused = head.type == NFAI_F16 || head.type == NFAI_F32 || is_t16(head.type);
        if (am_fused) {
            a.argmax_part = static_cast<char *>(m->d_argmax_part) + 4096;
            a.argmax_out = m->d_tok; a.argmax_pos_inc = m->d_pos; a.argmax_ring = m->d_ring; a.argmax_ring_len = RING_LEN;
        }
        S_TRY(sch.submit(op_gemv(KC_LMHEAD, a)));
        if (!am_fused)
            S_TRY(sch.submit(op_fn(KC_OTHER, [m](hipStream_t st) {
                return launch_argmax(m->logits, m->d.V, m->d_tok, m->d_argmax_part, m->d_pos, m->d_ring, RING_LEN, st);
            })));
    } else {
        S_TRY(sch.submit(op_fn(KC_OTHER, [m](hipStream_t st) { return launch_pos_advance(m->d_pos, st); })));
    }
    return sch.flush();
}

}  // namespace nfai

namespace {

int ensure_graph(Model *m)
{
    if (m->graph) return NFAI_OK;
    return capture(m->ctx->stream, "token", [&] { return enqueue_token(m, true); }, m->graph);
}

// Enqueue one whole token (graph replay when allowed; launch by launch between the timer's events when profiled).
int run_token(Model *m, LaunchTimer *timer = nullptr)
{
    if (m->pos_host >= m->d.C)
        return fail(NFAI_ERR_KV_FULL, "KV cache full: position %u == capacity %u (the reference would write out of bounds here)",
                    m->pos_host, m->d.C);
    if (m->use_graph && !m->unfused && !timer) {
        S_TRY(ensure_graph(m));
        HIP_TRY(hipGraphLaunch(m->graph.exec, m->ctx->stream));
        m->x_last = x_after_token(m);
    } else {
        S_TRY(enqueue_token(m, true, timer));
    }
    m->pos_host++;
    return NFAI_OK;
}

// The engine launch of every block: parameter blocks written to device memory once (finalize), launched from the token graph.
int build_engine_plans(Model *m)
{
    m->eng_plans.clear();
    if (!engine_ok(m)) return NFAI_OK;
    const nfai_llama_desc &d = m->d;
    const size_t pb = engine_params_bytes();
    if (!m->d_engparams) DALLOC(m->d_engparams, pb * m->layers.size());
    HIP_TRY(hipStreamSynchronize(m->ctx->stream));
    for (size_t i = 0; i < m->layers.size(); i++) {
        Layer &L = m->layers[i];
        float *xin = (i & 1) ? m->h : m->x, *xout = (i & 1) ? m->x : m->h;
        EngineArgs e;
        const bool more = i + 1 < m->layers.size();
        e.n_ops = more ? 4 : 3;
        e.E = d.E; e.F = d.F; e.HD = d.H * d.D;
        e.Wo = L.wo.ptr; e.Wgate = L.wgate.ptr; e.Wup = L.wup.ptr; e.Wdown = L.wdown.ptr;
        e.att = m->att; e.x_in = xin; e.x_out = xout;
        e.gamma_ffn = static_cast<const float *>(L.ffn_norm.ptr);
        e.eps = d.eps;
        uint64_t *gl = m->d_gran + i * (2 * (size_t)d.E + d.F);
        e.g_h = gl; e.g_act = gl + d.E; e.g_x = gl + d.E + d.F;
        e.epoch = m->d_epoch; e.err = m->d_engerr;
        e.n_cu = (uint32_t)m->ctx->prop.multiProcessorCount;
        if (more) {
            Layer &N = m->layers[i + 1];
            e.gamma_next = static_cast<const float *>(N.attn_norm.ptr);
            e.Wqkv[0] = N.wq.ptr; e.Wqkv[1] = N.wk.ptr; e.Wqkv[2] = N.wv.ptr;
            e.qkv_rows[0] = (uint32_t)N.wq.rows; e.qkv_rows[1] = (uint32_t)N.wk.rows; e.qkv_rows[2] = (uint32_t)N.wv.rows;
            e.q_out = m->q; e.kcache = N.kcache; e.vcache = N.vcache;
            e.kv_type = m->kv_f16 ? NFAI_F16 : NFAI_F32;
            e.kv_pos_stride = m->kv_pos_stride; e.kv_head_stride = m->kv_head_stride;
            e.rope_cs = m->d_ropecs; e.rope_dims = d.rope_dims; e.D = d.D; e.pos_dev = m->d_pos;
        }
        EnginePlan plan;
        hipError_t he = engine_plan(e, static_cast<char *>(m->d_engparams) + i * pb, plan);
        if (he == hipErrorInvalidValue) { m->eng_plans.clear(); return NFAI_OK; }  // a shape the engine does not take: five launches
        if (he != hipSuccess) return fail(NFAI_ERR_HIP, "engine_plan failed: %s", hipGetErrorString(he));
        m->eng_plans.push_back(plan);
    }
    return NFAI_OK;
}

}  // namespace


// ---- C ABI -----------------------------------------------------------------------------------
NFAI_API int32_t nfai_hip_llama_create(nfai_ctx_t ch, const nfai_llama_desc *desc, nfai_model_t *out)
{
    Ctx *c = ctx_of(ch);
    if (!c) return fail(NFAI_ERR_INVALID, "llama_create: invalid context handle");
    if (!desc || !out) return fail(NFAI_ERR_INVALID, "llama_create: null argument");
    HIP_TRY(hipSetDevice(c->device));
    const nfai_llama_desc &d = *desc;
    NFAI_REQUIRE(d.E && d.L && d.H && d.Hkv && d.D && d.F && d.V && d.C, "llama_create: zero dimension");
    NFAI_REQUIRE(d.H % d.Hkv == 0 && d.H / d.Hkv <= 8, "llama_create: H=%u must be a multiple (<= 8x) of Hkv=%u", d.H, d.Hkv);
    // the fused decode attention exists for G = H/Hkv in {1, 2, 3, 4, 8}; the 1:1 chain takes any G
    if (!(d.flags & NFAI_LLAMA_UNFUSED) && !attn_group_ok(d.H / d.Hkv))
        return fail(NFAI_ERR_UNSUPPORTED, "llama_create: H/Hkv = %u query heads per kv head (the fused decode takes 1, 2, 3, 4 or 8; "
                                          "NFAI_LLAMA_UNFUSED takes any)", d.H / d.Hkv);
    NFAI_REQUIRE(d.D == 64 || d.D == 128, "llama_create: head_dim %u (kernels exist for 64 and 128)", d.D);
    NFAI_REQUIRE(d.E % 8 == 0 && d.F % 8 == 0 && (d.H * d.D) % 8 == 0, "llama_create: E, F, H*D must be multiples of 8");
    NFAI_REQUIRE(d.layer_begin < d.layer_end && d.layer_end <= d.L, "llama_create: layer range [%u,%u) outside [0,%u)", d.layer_begin,
                 d.layer_end, d.L);
    NFAI_REQUIRE(d.rope_dims % 2 == 0 && d.rope_dims <= d.D, "llama_create: rope_dims %u", d.rope_dims);
    NFAI_REQUIRE(d.rope_n_freqs <= d.rope_dims / 2, "llama_create: rope_n_freqs %u > rope_dims/2", d.rope_n_freqs);
    NFAI_REQUIRE(d.C <= 32768, "llama_create: KV capacity %u > 32768", d.C);
    Model *m = new Model();
    static uint64_t next_serial = 0;
    m->serial = ++next_serial;
    m->ctx = c;
    m->d = d;
    m->first_stage = d.layer_begin == 0;
    m->last_stage = d.layer_end == d.L;
    m->unfused = (d.flags & NFAI_LLAMA_UNFUSED) != 0;
    m->use_graph = (d.flags & NFAI_LLAMA_NO_GRAPH) == 0;
    m->kv_f16 = (d.flags & NFAI_LLAMA_KV_F16) != 0;
    {
        const char *env = getenv("NFAI_PREFETCH");
        m->prefetch = env ? (env[0] == '1') : ((d.flags & NFAI_LLAMA_PREFETCH) != 0);
        if (m->prefetch || d.max_batch > 0) HIP_TRY(hipStreamCreateWithFlags(&m->s2, hipStreamNonBlocking));  // (the prefill reads weights ahead on it)
    }
    {
        const char *env = getenv("NFAI_ENGINE");
        m->engine = !m->unfused && (env ? (env[0] == '1') : ((d.flags & NFAI_LLAMA_ENGINE) != 0));
    }
    if (m->unfused && m->kv_f16) { delete m; return fail(NFAI_ERR_INVALID, "llama_create: the 1:1 chain keeps the reference's fp32 KV cache"); }
    m->layers.resize(d.layer_end - d.layer_begin);
    m->kv_esz = m->kv_f16 ? 2 : 4;
    if (m->unfused) {  // reference layout [C][Hkv*D] (MatrixMultiplyShader.cs:59-65, :286-287)
        m->kv_pos_stride = (uint64_t)d.Hkv * d.D;
        m->kv_head_stride = d.D;
    } else {           // head-major [Hkv][C][D]: each attention block streams one contiguous range
        m->kv_pos_stride = d.D;
        m->kv_head_stride = (uint64_t)d.C * d.D;
    }
    const size_t kvb = (size_t)d.C * d.Hkv * d.D * m->kv_esz;
    for (Layer &L : m->layers) {
        DALLOC(L.kcache, kvb);
        DALLOC(L.vcache, kvb);
    }
    DALLOC(m->d_pos, 256);
    DALLOC(m->d_tok, 256);
    m->d_engerr = m->d_tok + 1;   // the sticky error word sits next to the token word: ONE 8-byte copy takes both to the host after a blocking step
    DALLOC(m->d_ring, RING_LEN * 4);
    DALLOC(m->d_freqs, (d.D / 2 + 8) * 4);
    DALLOC(m->d_ropecs, (d.D + 16) * 4);
    DALLOC(m->d_argmax_part, 4096 + argmax_fused_bytes());  // k_argmax's partials | the fused lm_head + ArgMax launch's
    DALLOC(m->d_epoch, 256);
    if (m->engine) DALLOC(m->d_gran, (size_t)m->layers.size() * (2 * (size_t)d.E + d.F) * 8);
    DALLOC(m->d_attn_part, attn_partials_bytes(d.H, d.Hkv, d.D, true) + attn_wo_extra_bytes(d.H, d.D));
    DALLOC(m->x, d.E * 4);
    DALLOC(m->h, d.E * 4);
    DALLOC(m->q, d.H * d.D * 4);
    DALLOC(m->att, d.H * d.D * 4);
    DALLOC(m->act, d.F * 4);
    if (m->last_stage) DALLOC(m->logits, (size_t)d.V * 4);
    if (m->unfused) {
        DALLOC(m->xn, d.E * 4);
        DALLOC(m->qraw, d.H * d.D * 4);
        DALLOC(m->scores, (size_t)d.H * d.C * 4);
        DALLOC(m->wts, (size_t)d.H * d.C * 4);
        DALLOC(m->proj, d.E * 4);
        DALLOC(m->gate, d.F * 4);
        DALLOC(m->up, d.F * 4);
    }
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&m->h_pin), 4096, hipHostMallocDefault));
    memset(m->h_pin, 0, 4096);
    if (d.max_batch > 0 && !m->unfused) {
        Model::Prefill &w = m->pf;
        w.T = (d.max_batch + 127) / 128 * 128;
        w.Spad = (d.C + 63) / 64 * 64;
        const size_t T = w.T, HD = (size_t)d.H * d.D, KD = (size_t)d.Hkv * d.D;
        DALLOC(w.toks, T * 4);
        DALLOC(w.X, T * d.E * 4);
        DALLOC(w.H1, T * d.E * 4);
        DALLOC(w.Q, T * (HD + 2 * KD) * 4);  // q | k | v columns of one GEMM output
        DALLOC(w.CS, T * d.D * 4);
        DALLOC(w.ATT, T * HD * 4);
        DALLOC(w.G, T * d.F * 2 * 4);        // gate | up columns of one GEMM output
        DALLOC(w.SC, (size_t)d.H * T * w.Spad * 4);
        DALLOC(w.XN, T * std::max<size_t>(d.E, HD) * 2);
        DALLOC(w.QH, T * HD * 2);
        DALLOC(w.KH, KD * w.Spad * 2);
        DALLOC(w.VT, KD * w.Spad * 2);
        DALLOC(w.P, (size_t)d.H * T * w.Spad * 2);
        DALLOC(w.ACT, T * d.F * 2);
    }
    // RoPE frequency table as TransformerBlock.cs:33-38 builds it; entries >= rope_n_freqs are zero
    // (the reference uploads 32 entries only, TransformerBlock.cs:66).
    std::vector<float> fr(d.D / 2 + 8, 0.f);
    for (uint32_t i = 0; i < d.rope_dims / 2; i++) {
        const float f = 1.0f / powf(d.rope_base, (float)i / ((float)d.rope_dims / 2.0f));
        fr[i] = i < d.rope_n_freqs ? f : 0.0f;
    }
    HIP_TRY(hipMemcpyAsync(m->d_freqs, fr.data(), fr.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    handle_register(m);
    *out = reinterpret_cast<nfai_model_t>(m);
    return NFAI_OK;
}

static void drop_graphs(Model *m)
{
    m->g_step.graph.drop();
    m->g_topk.graph.drop();
    m->graph.drop();
    m->stage_graph.drop();
}

NFAI_API int32_t nfai_hip_llama_destroy(nfai_model_t h)
{
    MODEL_OR_FAIL(m, h);
    hipStreamSynchronize(m->ctx->stream);
    drop_graphs(m);
    for (hipEvent_t e : m->pf_events) hipEventDestroy(e);
    if (m->s2) hipStreamDestroy(m->s2);
    for (hipEvent_t e : m->prof_rep_ev) if (e) hipEventDestroy(e);
    auto free_t = [](Tensor &t) { if (t.owned && t.ptr) hipFree(t.ptr); };
    free_t(m->token_embd); free_t(m->output_norm); free_t(m->output);
    for (Layer &L : m->layers) {
        free_t(L.attn_norm); free_t(L.wq); free_t(L.wk); free_t(L.wv); free_t(L.wo);
        free_t(L.ffn_norm); free_t(L.wgate); free_t(L.wup); free_t(L.wdown);
        hipFree(L.kcache); hipFree(L.vcache);
    }
    void *ptrs[] = {m->d_score, m->d_score_slab, m->d_score_wide, m->d_topk, m->d_engparams, m->d_gran, m->d_epoch, m->d_pos, m->d_tok, m->d_ring, m->d_freqs, m->d_ropecs, m->d_argmax_part, m->d_attn_part, m->x, m->h,
                    m->q, m->att, m->act, m->logits, m->xn, m->qraw, m->scores, m->wts, m->proj, m->gate, m->up};
    for (void *p : ptrs) if (p) hipFree(p);
    void *pfp[] = {m->pf.CS, m->pf.toks, m->pf.X, m->pf.H1, m->pf.Q, m->pf.K, m->pf.V, m->pf.ATT, m->pf.G, m->pf.U, m->pf.SC,
                   m->pf.XN, m->pf.QH, m->pf.KH, m->pf.VT, m->pf.P, m->pf.ACT};
    for (void *p : pfp) if (p) hipFree(p);
    if (m->h_pin) hipHostFree(m->h_pin);
    m->magic = 0;
    handle_unregister(m);
    delete m;
    return NFAI_OK;
}

static int set_tensor_impl(Model *m, const char *name, int type, uint64_t rows, uint64_t cols, const void *host, void *dev)
{
    if (!name) return fail(NFAI_ERR_INVALID, "set_tensor: null name");
    bool ignored = false;
    Tensor *t = find_slot(m, name, &ignored);
    if (ignored) return NFAI_OK;
    if (!t) return fail(NFAI_ERR_INVALID, "set_tensor: unknown tensor name '%s'", name);
    const uint64_t rb = weight_row_bytes(type, cols);
    if (rb == 0) return fail(NFAI_ERR_UNSUPPORTED, "set_tensor(%s): ggml type %d with %llu columns is not supported (the reference "
                             "throws \"Unsupported data type\" for everything but F32/F16, Parser.cs:111-114)", name, type,
                             (unsigned long long)cols);
    if (!dev && !host) return fail(NFAI_ERR_INVALID, "set_tensor(%s): null data", name);
    if (dev && (reinterpret_cast<uintptr_t>(dev) & 15)) return fail(NFAI_ERR_INVALID, "set_tensor_device(%s): pointer not 16-byte aligned", name);
    // The new storage is built completely before the slot is touched: a failing re-set (allocation, copy, repack) leaves the
    // previous tensor in place and valid.  Only then is the old owned storage freed and the slot swapped.
    Tensor nt;
    nt.type = type; nt.rows = rows; nt.cols = cols; nt.bytes = rb * rows;
    hipStream_t s = m->ctx->stream;
    if ((type == NFAI_Q8_0 || type == NFAI_Q5_K || type == NFAI_Q4_0 || type == NFAI_Q3_K || type == NFAI_IQ4_XS) && (rows == 0 || rows % 16))
        return fail(NFAI_ERR_UNSUPPORTED, "set_tensor(%s): %s needs rows %% 16 == 0, cols %% 256 == 0 and cols <= 32768 (%llu x %llu)", name,
                    type == NFAI_Q8_0 ? "Q8_0" : (type == NFAI_Q4_0 ? "Q4_0" : (type == NFAI_Q3_K ? "Q3_K" : (type == NFAI_IQ4_XS ? "IQ4_XS" : "Q5_K"))), (unsigned long long)rows, (unsigned long long)cols);
    const bool q4_t16 = type == NFAI_Q4_K && rows > 0 && rows % 16 == 0, q6_t16 = type == NFAI_Q6_K && rows > 0 && rows % 16 == 0;
    const bool q8_t16 = type == NFAI_Q8_0, q5_t16 = type == NFAI_Q5_K, q40_t16 = type == NFAI_Q4_0, q3_t16 = type == NFAI_Q3_K, iq4_t16 = type == NFAI_IQ4_XS;
    auto fail_free = [&](void *a, void *b, int rc) { if (a) hipFree(a); if (b) hipFree(b); return rc; };
    if (type == NFAI_Q6_K || q4_t16 || q8_t16 || q5_t16 || q40_t16 || q3_t16 || iq4_t16) {
        // native blocks (host or device) -> owned repacked copy: Q6_K planes (common.h), IQ4_XS / Q3_K / Q4_0 / Q4_K / Q5_K / Q6_K / Q8_0 T16 tiles (kernels_gemv_kqm.hip)
        void *native = dev, *staged = nullptr;
        if (!dev) {
            int rc = dalloc(&staged, nt.bytes, s);
            if (rc) return rc;
            hipError_t e = hipMemcpyAsync(staged, host, nt.bytes, hipMemcpyHostToDevice, s);
            if (e != hipSuccess) return fail_free(staged, nullptr, fail(NFAI_ERR_HIP, "set_tensor(%s): upload failed: %s", name, hipGetErrorString(e)));
            native = staged;
        }
        int rc = dalloc(&nt.ptr, nt.bytes, s);
        if (rc) return fail_free(staged, nullptr, rc);
        nt.owned = true;
        hipError_t e = q4_t16 ? launch_repack_q4k_t16(native, nt.ptr, rows, cols, s)
                     : q6_t16 ? launch_repack_q6k_t16(native, nt.ptr, rows, cols, s)
                     : q8_t16 ? launch_repack_q80_t16(native, nt.ptr, rows, cols, s)
                     : q5_t16 ? launch_repack_q5k_t16(native, nt.ptr, rows, cols, s)
                     : q40_t16 ? launch_repack_q40_t16(native, nt.ptr, rows, cols, s)
                     : q3_t16 ? launch_repack_q3k_t16(native, nt.ptr, rows, cols, s)
                     : iq4_t16 ? launch_repack_iq4xs_t16(native, nt.ptr, rows, cols, s)
                              : launch_repack_q6k(native, nt.ptr, rows * cols / 256, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail_free(staged, nt.ptr, fail(NFAI_ERR_HIP, "set_tensor(%s): K-quant repack failed: %s", name, hipGetErrorString(e)));
        if (q4_t16) nt.type = NFAI_Q4_K_T16;
        if (q6_t16) nt.type = NFAI_Q6_K_T16;
        if (q8_t16) nt.type = NFAI_Q8_0_T16;
        if (q5_t16) nt.type = NFAI_Q5_K_T16;
        if (q40_t16) nt.type = NFAI_Q4_0_T16;
        if (q3_t16) nt.type = NFAI_Q3_K_T16;
        if (iq4_t16) nt.type = NFAI_IQ4_XS_T16;
        if (staged) hipFree(staged);
    } else if (dev) {
        nt.ptr = dev;
        nt.owned = false;
    } else {
        int rc = dalloc(&nt.ptr, nt.bytes, s);
        if (rc) return rc;
        nt.owned = true;
        hipError_t e = hipMemcpyAsync(nt.ptr, host, nt.bytes, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail_free(nt.ptr, nullptr, fail(NFAI_ERR_HIP, "set_tensor(%s): upload failed: %s", name, hipGetErrorString(e)));
    }
    // the kept fp16 copies of the K-quant prefill are of the old weights; a copy other slots still read stays theirs
    if (m->pf.wide.use_count() > 1) m->pf.wide = std::make_shared<WideShadow>();
    else std::fill(m->pf.wide->done.begin(), m->pf.wide->done.end(), 0);
    m->finalized = false;  // graphs captured over the old pointer are dropped by the next finalize
    m->weights_gen++;
    if (t->owned && t->ptr) {
        hipStreamSynchronize(s);  // nothing enqueued may still read the old storage
        hipFree(t->ptr);
    }
    *t = nt;
    return NFAI_OK;
}

// The slots of a pipeline stage: separate models (KV cache, position, graph) over the donor's weights.
NFAI_API int32_t nfai_hip_llama_share_tensors(nfai_model_t h, nfai_model_t donor_h)
{
    MODEL_OR_FAIL(m, h);
    Model *src = model_of(donor_h);
    if (!src || src == m) return fail(NFAI_ERR_INVALID, "share_tensors: invalid donor handle");
    if (src->ctx->device != m->ctx->device) return fail(NFAI_ERR_INVALID, "share_tensors: donor lives on another device");
    const nfai_llama_desc &a = m->d, &b = src->d;
    if (a.E != b.E || a.L != b.L || a.H != b.H || a.Hkv != b.Hkv || a.D != b.D || a.F != b.F || a.V != b.V ||
        a.layer_begin != b.layer_begin || a.layer_end != b.layer_end)
        return fail(NFAI_ERR_INVALID, "share_tensors: donor has different dimensions or layer range");
    auto share = [](Tensor &dst, const Tensor &s2) {
        if (dst.owned && dst.ptr) hipFree(dst.ptr);
        dst = s2;
        dst.owned = false;
    };
    hipStreamSynchronize(m->ctx->stream);
    share(m->token_embd, src->token_embd);
    share(m->output_norm, src->output_norm);
    share(m->output, src->output);
    for (size_t i = 0; i < m->layers.size(); i++) {
        Layer &L = m->layers[i];
        const Layer &S = src->layers[i];
        share(L.attn_norm, S.attn_norm); share(L.wq, S.wq); share(L.wk, S.wk); share(L.wv, S.wv); share(L.wo, S.wo);
        share(L.ffn_norm, S.ffn_norm); share(L.wgate, S.wgate); share(L.wup, S.wup); share(L.wdown, S.wdown);
    }
    // the donor's fp16 copies of the K-quant matrices too (prefill, stage ingest): same weights, same stream, so a slot finds them
    // widened by whichever model ran first, in stream order.  Another context's stream would race the re-widened single slot.
    m->pf.wide = src->ctx == m->ctx ? src->pf.wide : std::make_shared<WideShadow>();
    m->finalized = false;
    m->weights_gen++;
    return NFAI_OK;
}

NFAI_API int32_t nfai_hip_llama_set_tensor(nfai_model_t h, const char *name, int32_t type, uint64_t rows, uint64_t cols, const void *host)
{
    MODEL_OR_FAIL(m, h);
    return set_tensor_impl(m, name, type, rows, cols, host, nullptr);
}

NFAI_API int32_t nfai_hip_llama_set_tensor_device(nfai_model_t h, const char *name, int32_t type, uint64_t rows, uint64_t cols, void *dev)
{
    MODEL_OR_FAIL(m, h);
    if (!dev) return fail(NFAI_ERR_INVALID, "set_tensor_device: null pointer");
    return set_tensor_impl(m, name, type, rows, cols, nullptr, dev);
}

NFAI_API int32_t nfai_hip_llama_finalize(nfai_model_t h)
{
    MODEL_OR_FAIL(m, h);
    const nfai_llama_desc &d = m->d;
    int rc;
    if (m->first_stage || (m->last_stage && !m->output.ptr))
        if ((rc = check_shape("token_embd.weight", m->token_embd, d.V, d.E, true))) return rc;
    if (m->last_stage) {
        if ((rc = check_shape("output_norm.weight", m->output_norm, 1, d.E, false))) return rc;
        if (m->output.ptr && (rc = check_shape("output.weight", m->output, d.V, d.E, true))) return rc;
    }
    for (size_t i = 0; i < m->layers.size(); i++) {
        Layer &L = m->layers[i];
        char nm[64];
#define CHK(field, suffix, r, c_, mat)                                         \
    snprintf(nm, sizeof(nm), "blk.%zu." suffix, i + d.layer_begin);            \
    if ((rc = check_shape(nm, L.field, r, c_, mat))) return rc;
        CHK(attn_norm, "attn_norm.weight", 1, d.E, false)
        CHK(wq, "attn_q.weight", d.H * d.D, d.E, true)
        CHK(wk, "attn_k.weight", d.Hkv * d.D, d.E, true)
        CHK(wv, "attn_v.weight", d.Hkv * d.D, d.E, true)
        CHK(wo, "attn_output.weight", d.E, d.H * d.D, true)
        CHK(ffn_norm, "ffn_norm.weight", 1, d.E, false)
        CHK(wgate, "ffn_gate.weight", d.F, d.E, true)
        CHK(wup, "ffn_up.weight", d.F, d.E, true)
        CHK(wdown, "ffn_down.weight", d.E, d.F, true)
#undef CHK
        if (!m->unfused && L.wgate.type != L.wup.type)
            return fail(NFAI_ERR_UNSUPPORTED, "finalize: blk.%zu ffn_gate and ffn_up have different tensor types", i + d.layer_begin);
    }
    drop_graphs(m);
    (void)gemv_xcd_calibrate(m->ctx);   // once per context: how fast each XCD streams (rows of the lm_head / gate | up launches are dealt by it)
    if ((rc = build_engine_plans(m))) return rc;
    m->finalized = true;
    return NFAI_OK;
}

// (TopkOut, common.h: the head of the top-k workspace, topk_out_offset())
static_assert(sizeof(TopkOut) + 16 <= 4096, "pinned staging: words 0..3 (argmax, error word, token in, spare), then the candidates");

// Capture [token word H2D] -> the token -> [top-k launch] -> [argmax, error word(, candidates) D2H].  Errors inside the capture end
// it before they are reported (a stream left in capture mode would poison every later call).
static int ensure_sync_graph(Model *m, Model::SyncGraph &sg, bool topk, float temperature, uint32_t k)
{
    if (sg.graph && (!topk || (sg.temperature == temperature && sg.k == k))) return NFAI_OK;
    sg.graph.drop();
    hipStream_t s = m->ctx->stream;
    S_TRY(capture(s, "blocking-step", [&]() -> int {
        HIP_TRY(hipMemcpyAsync(m->d_tok, m->h_pin + 2, 4, hipMemcpyHostToDevice, s));
        S_TRY(enqueue_token(m, true));
        if (topk) {
            const hipError_t e = launch_topk(m->logits, m->d.V, temperature, k, m->d_topk, s);
            if (e != hipSuccess) return fail(NFAI_ERR_HIP, "decode_topk: launch failed: %s", hipGetErrorString(e));
        }
        HIP_TRY(hipMemcpyAsync(m->h_pin, m->d_tok, 8, hipMemcpyDeviceToHost, s));   // token word + error word (adjacent)
        if (topk)
            HIP_TRY(hipMemcpyAsync(m->h_pin + 4, static_cast<const char *>(m->d_topk) + topk_out_offset(), sizeof(TopkOut), hipMemcpyDeviceToHost, s));
        return NFAI_OK;
    }, sg.graph));
    sg.temperature = temperature;
    sg.k = k;
    return NFAI_OK;
}

// One token, blocking; the argmax and the sticky error word of the in-kernel waits land in m->h_pin[0..1] (with topk: the candidates
// in m->h_pin[4..]).  The slices' workgroups of the attention launch wait for each other (granule hand-off): when one of those
// bounded waits gives up (codes 0x1000-0x4000: a workgroup was not resident, e.g. another process shares the device), the token's
// results are not valid — the model switches to the ticket form, which never waits, for good, says so once on stderr, and the SAME
// token is run again from the same position.
static int step_blocking(Model *m, uint32_t token, bool topk = false, float temperature = 0.f, uint32_t k = 0)
{
    hipStream_t s = m->ctx->stream;
    for (int attempt = 0;; attempt++) {
        const uint32_t pos = m->pos_host;
        int rc;
        if (m->use_graph && !m->unfused) {
            if (m->pos_host >= m->d.C)
                return fail(NFAI_ERR_KV_FULL, "KV cache full: position %u == capacity %u (the reference would write out of bounds here)",
                            m->pos_host, m->d.C);
            Model::SyncGraph &sg = topk ? m->g_topk : m->g_step;
            if ((rc = ensure_sync_graph(m, sg, topk, temperature, k))) return rc;
            m->h_pin[2] = token;
            HIP_TRY(hipGraphLaunch(sg.graph.exec, s));
            m->x_last = x_after_token(m);
            m->pos_host++;
        } else {
            if ((rc = set_token_async(m, token))) return rc;
            if ((rc = run_token(m))) return rc;
            if (topk) {
                const hipError_t e = launch_topk(m->logits, m->d.V, temperature, k, m->d_topk, s);
                if (e != hipSuccess) return fail(NFAI_ERR_HIP, "decode_topk: launch failed: %s", hipGetErrorString(e));
                HIP_TRY(hipMemcpyAsync(m->h_pin + 4, static_cast<const char *>(m->d_topk) + topk_out_offset(), sizeof(TopkOut), hipMemcpyDeviceToHost, s));
            }
            HIP_TRY(hipMemcpyAsync(m->h_pin, m->d_tok, 8, hipMemcpyDeviceToHost, s));   // token word + error word (adjacent)
        }
        HIP_TRY(hipStreamSynchronize(s));
        const uint32_t code = m->h_pin[1];
        if (code == 0) return NFAI_OK;
        if (attempt > 0 || m->attn_ticket || (code & ~0x7000u) != 0) return engine_failed(m, code);
        fprintf(stderr, "nfai_hip: an attention launch gave up waiting for a KV slice's partial results (code 0x%x) at position %u — are all its "
                        "workgroups resident?  Re-running the token on the ticket hand-off; this model keeps it from now on.\n", code, pos);
        m->attn_ticket = true;
        drop_graphs(m);  // captured with the granule form
        HIP_TRY(hipMemsetAsync(m->d_engerr, 0, 4, s));
        HIP_TRY(hipMemcpyAsync(m->d_pos, &pos, 4, hipMemcpyHostToDevice, s));  // the failed token may have advanced it
        HIP_TRY(hipStreamSynchronize(s));
        m->h_pin[1] = 0;
        m->pos_host = pos;
    }
}

namespace nfai {
int step_token_blocking(Model *m, uint32_t token) { return step_blocking(m, token); }
}  // namespace nfai

NFAI_API int32_t nfai_hip_llama_decode_step(nfai_model_t h, uint32_t token, float *logits_host, uint32_t *argmax)
{
    MODEL_OR_FAIL(m, h);
    NEED_FINAL(m);
    if (!(m->first_stage && m->last_stage)) return fail(NFAI_ERR_STATE, "decode_step: model is a pipeline stage; use nfai_hip_llama_stage_step");
    if (token >= m->d.V) return fail(NFAI_ERR_INVALID, "decode_step: token %u >= vocab %u", token, m->d.V);
    int rc = step_blocking(m, token);
    if (rc) return rc;
    if (argmax) *argmax = m->h_pin[0];
    if (logits_host) {
        hipStream_t s = m->ctx->stream;
        HIP_TRY(hipMemcpyAsync(logits_host, m->logits, (size_t)m->d.V * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return NFAI_OK;
}

// One token, then the candidates of the reference's DEFAULT sampler on the device (LlamaModel.cs:128-130,165: TopP over V logits
// read back to the host; here 8k + 8 bytes come back instead of 513 KB).
NFAI_API int32_t nfai_hip_llama_decode_topk(nfai_model_t h, uint32_t token, float temperature, uint32_t k, uint32_t *ids_out, float *probs_out)
{
    MODEL_OR_FAIL(m, h);
    NEED_FINAL(m);
    if (!(m->first_stage && m->last_stage)) return fail(NFAI_ERR_STATE, "decode_topk: model is a pipeline stage");
    if (token >= m->d.V) return fail(NFAI_ERR_INVALID, "decode_topk: token %u >= vocab %u", token, m->d.V);
    // every argument is checked BEFORE the token runs (topk_run's own predicates): a rejected call leaves the position where it was
    if (!ids_out || !probs_out) return fail(NFAI_ERR_INVALID, "decode_topk: null output");
    if (k == 0 || k > TOPK_MAX || k > m->d.V) return fail(NFAI_ERR_INVALID, "decode_topk: k=%u outside [1, min(%u, V=%u)]", k, TOPK_MAX, m->d.V);
    if (!(temperature > 0.f)) return fail(NFAI_ERR_INVALID, "decode_topk: temperature %g (the reference divides by it, SamplingUtils.cs:7)", temperature);
    if (!m->d_topk) DALLOC(m->d_topk, topk_work_bytes(m->d.V));
    // the token's kernels, the candidate launch and the read-back (error word + 8 * TOPK_MAX + 8 bytes) are ONE graph: one launch
    // and one host synchronisation per sampled token
    int rc = step_blocking(m, token, true, temperature, k);
    if (rc) return rc;
    const TopkOut *out = reinterpret_cast<const TopkOut *>(m->h_pin + 4);
    topk_finish(out->v, out->i, out->M, out->S, temperature, k, ids_out, probs_out);
    return NFAI_OK;
}

NFAI_API int32_t nfai_hip_llama_set_token(nfai_model_t h, uint32_t token)
{
    MODEL_OR_FAIL(m, h);
    if (token >= m->d.V) return fail(NFAI_ERR_INVALID, "set_token: token %u >= vocab %u", token, m->d.V);
    return set_token_async(m, token);
}

NFAI_API int32_t nfai_hip_llama_decode_enqueue(nfai_model_t h, uint32_t n_steps)
{
    MODEL_OR_FAIL(m, h);
    NEED_FINAL(m);
    if (!(m->first_stage && m->last_stage)) return fail(NFAI_ERR_STATE, "decode_enqueue: model is a pipeline stage");
    if (m->pos_host + n_steps > m->d.C)
        return fail(NFAI_ERR_KV_FULL, "decode_enqueue: %u steps from position %u exceed KV capacity %u", n_steps, m->pos_host, m->d.C);
    for (uint32_t i = 0; i < n_steps; i++) {
        int rc = run_token(m);
        if (rc) return rc;
    }
    return NFAI_OK;
}

NFAI_API int32_t nfai_hip_llama_fetch_tokens(nfai_model_t h, uint32_t n, uint32_t *tokens_out)
{
    MODEL_OR_FAIL(m, h);
    if (!tokens_out || n == 0 || n > RING_LEN || n > m->pos_host) return fail(NFAI_ERR_INVALID, "fetch_tokens: n=%u (pos %u, ring %u)", n, m->pos_host, RING_LEN);
    hipStream_t s = m->ctx->stream;
    std::vector<uint32_t> ring(RING_LEN);
    HIP_TRY(hipMemcpyAsync(ring.data(), m->d_ring, RING_LEN * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(m->h_pin + 1, m->d_engerr, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (m->h_pin[1]) return engine_failed(m, m->h_pin[1]);
    for (uint32_t i = 0; i < n; i++) tokens_out[i] = ring[(m->pos_host - n + i) % RING_LEN];
    return NFAI_OK;
}

NFAI_API int32_t nfai_hip_llama_decode_greedy(nfai_model_t h, uint32_t first_token, uint32_t n_steps, uint32_t *tokens_out)
{
    int rc = nfai_hip_llama_set_token(h, first_token);
    if (rc) return rc;
    if ((rc = nfai_hip_llama_decode_enqueue(h, n_steps))) return rc;
    return nfai_hip_llama_fetch_tokens(h, n_steps, tokens_out);
}

namespace nfai {

// The stage's work for one token: hidden state in -> this stage's blocks -> hidden state out
// (or lm_head + argmax on the last stage).  Captured once per (hidden_in, hidden_out) pair.
int stage_enqueue(Model *m, const void *hidden_in, void *hidden_out)
{
    hipStream_t s = m->ctx->stream;
    if (!m->first_stage) HIP_TRY(hipMemcpyAsync(m->x, hidden_in, (size_t)m->d.E * 4, hipMemcpyDeviceToDevice, s));
    int rc = enqueue_token(m, true);
    if (rc) return rc;
    if (!m->last_stage) HIP_TRY(hipMemcpyAsync(hidden_out, m->x_last ? m->x_last : m->x, (size_t)m->d.E * 4, hipMemcpyDeviceToDevice, s));
    // the sticky error word of the launches that wait inside the kernel (attention slices, engine) travels to pinned host memory
    // with every step; nfai_hip_llama_stage_step looks at it on entry, so a stage that never synchronises still reports a
    // hand-off that gave up — one step late
    HIP_TRY(hipMemcpyAsync(m->h_pin + 1, m->d_engerr, 4, hipMemcpyDeviceToHost, s));
    return NFAI_OK;
}

}  // namespace nfai

NFAI_API int32_t nfai_hip_llama_stage_step(nfai_model_t h, uint32_t token, const void *hidden_in, void *hidden_out,
                                           float *logits_host, uint32_t *argmax)
{
    MODEL_OR_FAIL(m, h);
    NEED_FINAL(m);
    hipStream_t s = m->ctx->stream;
    if (m->pos_host >= m->d.C) return fail(NFAI_ERR_KV_FULL, "stage_step: KV cache full at position %u", m->pos_host);
    if (m->h_pin[1]) return engine_failed(m, m->h_pin[1]);  // written by an earlier step of this stage (see stage_enqueue)
    if (m->first_stage) {
        if (token != NFAI_TOKEN_ON_DEVICE) {
            if (token >= m->d.V) return fail(NFAI_ERR_INVALID, "stage_step: token %u >= vocab %u", token, m->d.V);
            int rc = set_token_async(m, token);
            if (rc) return rc;
        }
    } else if (!hidden_in) {
        return fail(NFAI_ERR_INVALID, "stage_step: hidden_in is required on a non-first stage");
    }
    if (!m->last_stage && !hidden_out) return fail(NFAI_ERR_INVALID, "stage_step: hidden_out is required on a non-last stage");
    if (m->use_graph && !m->unfused) {
        if (!m->stage_graph || m->stage_in != hidden_in || m->stage_out != hidden_out) {
            m->stage_graph.drop();
            S_TRY(capture(s, "stage", [&] { return stage_enqueue(m, hidden_in, hidden_out); }, m->stage_graph));
            m->stage_in = hidden_in;
            m->stage_out = hidden_out;
        }
        HIP_TRY(hipGraphLaunch(m->stage_graph.exec, s));
        m->x_last = x_after_token(m);
    } else {
        int rc = stage_enqueue(m, hidden_in, hidden_out);
        if (rc) return rc;
    }
    m->pos_host++;
    if (m->last_stage && (logits_host || argmax)) {
        if (logits_host) HIP_TRY(hipMemcpyAsync(logits_host, m->logits, (size_t)m->d.V * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(m->h_pin, m->d_tok, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (argmax) *argmax = m->h_pin[0];
    }
    return NFAI_OK;
}

// Token hand-over between pipeline ends without a host round trip: 4-byte device-to-device copies
// on the context stream (the last stage's argmax -> a buffer RCCL sends; the received buffer ->
// the first stage's token word).
NFAI_API int32_t nfai_hip_llama_token_to_device(nfai_model_t h, void *dst_dev)
{
    MODEL_OR_FAIL(m, h);
    if (!dst_dev) return fail(NFAI_ERR_INVALID, "token_to_device: null pointer");
    HIP_TRY(hipMemcpyAsync(dst_dev, m->d_tok, 4, hipMemcpyDeviceToDevice, m->ctx->stream));
    return NFAI_OK;
}

NFAI_API int32_t nfai_hip_llama_token_from_device(nfai_model_t h, const void *src_dev)
{
    MODEL_OR_FAIL(m, h);
    if (!src_dev) return fail(NFAI_ERR_INVALID, "token_from_device: null pointer");
    HIP_TRY(hipMemcpyAsync(m->d_tok, src_dev, 4, hipMemcpyDeviceToDevice, m->ctx->stream));
    return NFAI_OK;
}

NFAI_API int32_t nfai_hip_llama_set_pos(nfai_model_t h, uint32_t pos)
{
    MODEL_OR_FAIL(m, h);
    if (pos > m->d.C) return fail(NFAI_ERR_INVALID, "set_pos: %u > capacity %u", pos, m->d.C);
    HIP_TRY(hipMemcpyAsync(m->d_pos, &pos, 4, hipMemcpyHostToDevice, m->ctx->stream));
    HIP_TRY(hipMemsetAsync(m->d_engerr, 0, 4, m->ctx->stream));
    HIP_TRY(hipStreamSynchronize(m->ctx->stream));
    m->h_pin[1] = 0;  // the host mirror of the error word (after the stream is idle: no copy into it is pending)
    m->pos_host = pos;
    return NFAI_OK;
}

NFAI_API int32_t nfai_hip_llama_reset(nfai_model_t h) { return nfai_hip_llama_set_pos(h, 0); }

NFAI_API int32_t nfai_hip_llama_pos(nfai_model_t h, uint32_t *pos)
{
    MODEL_OR_FAIL(m, h);
    if (pos) *pos = m->pos_host;
    return NFAI_OK;
}

NFAI_API int32_t nfai_hip_llama_read(nfai_model_t h, int32_t which, float *host, uint64_t n)
{
    MODEL_OR_FAIL(m, h);
    const nfai_llama_desc &d = m->d;
    const float *src = nullptr;
    uint64_t cap = 0;
    switch (which) {
        case 0: src = m->x_last ? m->x_last : m->x; cap = d.E; break;
        case 1: src = m->q; cap = (uint64_t)d.H * d.D; break;
        case 2: src = m->att; cap = (uint64_t)d.H * d.D; break;
        case 3: src = m->act; cap = d.F; break;
        case 4: src = m->logits; cap = d.V; break;
    }
    if (!src || !host || n > cap) return fail(NFAI_ERR_INVALID, "llama_read: which=%d n=%llu", which, (unsigned long long)n);
    HIP_TRY(hipMemcpyAsync(host, src, n * 4, hipMemcpyDeviceToHost, m->ctx->stream));
    HIP_TRY(hipStreamSynchronize(m->ctx->stream));
    return NFAI_OK;
}

NFAI_API int32_t nfai_hip_llama_read_kv(nfai_model_t h, uint32_t layer, int32_t is_v, uint32_t pos, float *host)
{
    MODEL_OR_FAIL(m, h);
    const nfai_llama_desc &d = m->d;
    if (layer < d.layer_begin || layer >= d.layer_end || pos >= d.C || !host) return fail(NFAI_ERR_INVALID, "read_kv: layer %u pos %u", layer, pos);
    Layer &L = m->layers[layer - d.layer_begin];
    const char *base = static_cast<const char *>(is_v ? L.vcache : L.kcache);
    hipStream_t s = m->ctx->stream;
    std::vector<uint16_t> tmp16;
    if (m->kv_f16) tmp16.resize((size_t)d.Hkv * d.D);
    for (uint32_t kh = 0; kh < d.Hkv; kh++) {
        const uint64_t idx = (uint64_t)pos * m->kv_pos_stride + (uint64_t)kh * m->kv_head_stride;
        void *dst = m->kv_f16 ? static_cast<void *>(tmp16.data() + (size_t)kh * d.D) : static_cast<void *>(host + (size_t)kh * d.D);
        HIP_TRY(hipMemcpyAsync(dst, base + idx * m->kv_esz, (size_t)d.D * m->kv_esz, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    if (m->kv_f16)
        for (size_t i = 0; i < tmp16.size(); i++) {
            _Float16 hv;
            memcpy(&hv, &tmp16[i], 2);
            host[i] = (float)hv;
        }
    return NFAI_OK;
}

NFAI_API int32_t nfai_hip_llama_bytes_per_token(nfai_model_t h, uint32_t pos, uint64_t *total, uint64_t *dominant)
{
    MODEL_OR_FAIL(m, h);
    const nfai_llama_desc &d = m->d;
    // KV per block: read p+1 positions, write 1
    uint64_t t = weights_once_bytes(m, false) + m->layers.size() * (2ull * d.Hkv * d.D * m->kv_esz * ((uint64_t)pos + 2));
    if (m->first_stage) t += weight_row_bytes(m->token_embd.type, d.E);
    uint64_t dom = 0;
    for (const Layer &L : m->layers)
        dom = std::max({dom, tensor_bytes(L.wq) + tensor_bytes(L.wk) + tensor_bytes(L.wv), tensor_bytes(L.wgate) + tensor_bytes(L.wup)});
    if (total) *total = t;
    if (dominant) *dominant = dom;
    return NFAI_OK;
}

NFAI_API int32_t nfai_hip_llama_profile_kernel(nfai_model_t h, uint32_t token, int32_t cls, uint32_t reps, float *us_avg)
{
    MODEL_OR_FAIL(m, h);
    NEED_FINAL(m);
    if (!us_avg || reps == 0 || cls < 0 || cls >= KC_N) return fail(NFAI_ERR_INVALID, "profile_kernel: bad arguments");
    if (!(m->first_stage && m->last_stage)) return fail(NFAI_ERR_STATE, "profile_kernel: whole-model contexts only");
    if (m->unfused) return fail(NFAI_ERR_STATE, "profile_kernel: fused path only");
    if (token >= m->d.V) return fail(NFAI_ERR_INVALID, "profile_kernel: token %u >= vocab %u", token, m->d.V);
    // The replayed launches read the position word AFTER the token advanced it: a replayed q|k|v stores its K / V rows at pos + 1 and
    // a replayed attention reads rows 0 .. pos + 1.  Row pos + 1 must exist: refused before anything runs, like every capacity error.
    if ((uint64_t)m->pos_host + 2 > m->d.C)
        return fail(NFAI_ERR_KV_FULL, "profile_kernel: the token at position %u and the replay behind it need positions up to %u; the KV "
                                      "capacity is %u", m->pos_host, m->pos_host + 1, m->d.C);
    int rc = set_token_async(m, token);
    if (rc) return rc;
    for (hipEvent_t &e : m->prof_rep_ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    m->prof_rep_cls = cls;
    m->prof_ops.clear();
    LaunchTimer timer(m->ctx->stream);   // the step runs launch by launch, as a profiled one does; its times are not read
    rc = run_token(m, &timer);
    m->prof_rep_cls = -1;
    if (rc) return rc;
    if (m->prof_ops.empty()) return fail(NFAI_ERR_STATE, "profile_kernel: no launch of class %d in a step", cls);
    // Replay: every launch of the class in a step (one per block: 28 different weight sets at 3B, far beyond the 256 MB
    // Infinity Cache, so nothing is re-read from cache), `reps` rounds, back to back between ONE pair of events.  The replay runs at
    // the ADVANCED position word: it leaves the position, the token word, the ring, the logits and every K / V row at or below the
    // token's own as the step left them; it overwrites the K / V rows at position + 1 (which the next token writes before anyone
    // reads them) and the activation vectors (a replayed first q|k|v launch also redoes the token prologue: the embedding row of
    // the ArgMax lands in the hidden-state vector).
    hipStream_t s = m->ctx->stream;
    // Engine launches hand vectors over under a per-token tag: a replay with the tag unchanged would find every hand-off already
    // complete and never wait.  So each replayed engine launch is preceded by the one-block kernel that advances the tag (as in
    // a real token), and the same number of those kernels alone is timed and subtracted.
    const bool bump = cls == KC_ENGINE;
    auto bump_launch = [&]() { return launch_token_begin(nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, m->d_pos, s, m->d_epoch); };
    HIP_TRY(hipEventRecord(m->prof_rep_ev[0], s));
    for (uint32_t r = 0; r < reps; r++)
        for (const Op &op : m->prof_ops) {
            if (bump && bump_launch() != hipSuccess) return fail(NFAI_ERR_HIP, "profile_kernel: tag launch failed");
            GemvArgs g = op.g;
            g.argmax_part = nullptr;  // a replayed lm_head must not advance the position again (the GEMV itself is idempotent)
            hipError_t e = op.kind == 0 ? launch_gemv(g, s) : (op.kind == 1 ? launch_attn_decode(op.a, s) : op.f(s));
            if (e != hipSuccess) return fail(NFAI_ERR_HIP, "profile_kernel: replay launch failed: %s", hipGetErrorString(e));
        }
    HIP_TRY(hipEventRecord(m->prof_rep_ev[1], s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, m->prof_rep_ev[0], m->prof_rep_ev[1]));
    if (bump) {
        HIP_TRY(hipEventRecord(m->prof_rep_ev[0], s));
        for (size_t i = 0; i < (size_t)reps * m->prof_ops.size(); i++)
            if (bump_launch() != hipSuccess) return fail(NFAI_ERR_HIP, "profile_kernel: tag launch failed");
        HIP_TRY(hipEventRecord(m->prof_rep_ev[1], s));
        HIP_TRY(hipStreamSynchronize(s));
        float ms0 = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms0, m->prof_rep_ev[0], m->prof_rep_ev[1]));
        ms -= ms0;
    }
    *us_avg = ms * 1e3f / (float)((size_t)reps * m->prof_ops.size());
    m->prof_ops.clear();
    return NFAI_OK;
}

NFAI_API int32_t nfai_hip_llama_profile_step(nfai_model_t h, uint32_t token, float *ms_by_class, uint32_t *launches_by_class)
{
    MODEL_OR_FAIL(m, h);
    NEED_FINAL(m);
    if (!ms_by_class || !launches_by_class) return fail(NFAI_ERR_INVALID, "profile_step: null output");
    if (!(m->first_stage && m->last_stage)) return fail(NFAI_ERR_STATE, "profile_step: whole-model contexts only");
    S_TRY(set_token_async(m, token));
    LaunchTimer timer(m->ctx->stream);
    S_TRY(run_token(m, &timer));
    return timer.collect(ms_by_class, launches_by_class);
}

// Test hook (not in nfai_hip.h): where the model's fp16 copies of its K-quant matrices live and how many bytes they take (0 / NULL
// before the first prefill); slots that share a donor's tensors report the donor's (tests/test_gpu_pipeline_ingest.py).
NFAI_API int32_t nfai_hip_debug_prefill_shadow(nfai_model_t h, void **ptr, uint64_t *bytes)
{
    MODEL_OR_FAIL(m, h);
    if (ptr) *ptr = m->pf.wide->ptr;
    if (bytes) *bytes = m->pf.wide->bytes;
    return NFAI_OK;
}

// Test hook (not in nfai_hip.h): slice `slice_plus_1 - 1` of kv head 0 of every attention launch publishes nothing, so the bounded
// waits of the granule hand-off give up and the fall-back to the ticket form can be exercised (tests/test_gpu_model.py).  0: off.
NFAI_API int32_t nfai_hip_debug_attn_withhold(nfai_model_t h, uint32_t slice_plus_1)
{
    MODEL_OR_FAIL(m, h);
    HIP_TRY(hipStreamSynchronize(m->ctx->stream));
    m->dbg_withhold = slice_plus_1;
    drop_graphs(m);
    return NFAI_OK;
}

// Test hook (not in nfai_hip.h): K or V rows [pos, pos + n) of one block as fp32 [n][Hkv*D] (fp16 caches widened) with one
// synchronisation, where nfai_hip_llama_read_kv takes one per row (tests/test_gpu_attention_depth.py reads up to 32768 rows).
NFAI_API int32_t nfai_hip_debug_read_kv_rows(nfai_model_t h, uint32_t layer, int32_t is_v, uint32_t pos, uint32_t n, float *host)
{
    MODEL_OR_FAIL(m, h);
    const nfai_llama_desc &d = m->d;
    if (layer < d.layer_begin || layer >= d.layer_end || n == 0 || (uint64_t)pos + n > d.C || !host)
        return fail(NFAI_ERR_INVALID, "read_kv_rows: layer %u rows [%u, %u + %u)", layer, pos, pos, n);
    Layer &L = m->layers[layer - d.layer_begin];
    const char *base = static_cast<const char *>(is_v ? L.vcache : L.kcache);
    hipStream_t s = m->ctx->stream;
    const size_t row = (size_t)d.Hkv * d.D, esz = m->kv_esz;
    std::vector<uint16_t> tmp16;
    if (m->kv_f16) tmp16.resize(row * n);
    char *dst = m->kv_f16 ? reinterpret_cast<char *>(tmp16.data()) : reinterpret_cast<char *>(host);
    for (uint32_t kh = 0; kh < d.Hkv; kh++) {  // one strided copy per kv head: D elements of each of the n positions
        const uint64_t idx = (uint64_t)pos * m->kv_pos_stride + (uint64_t)kh * m->kv_head_stride;
        HIP_TRY(hipMemcpy2DAsync(dst + (size_t)kh * d.D * esz, row * esz, base + idx * esz, m->kv_pos_stride * esz, (size_t)d.D * esz, n,
                                 hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    if (m->kv_f16)
        for (size_t i = 0; i < tmp16.size(); i++) {
            _Float16 hv;
            memcpy(&hv, &tmp16[i], 2);
            host[i] = (float)hv;
        }
    return NFAI_OK;
}
