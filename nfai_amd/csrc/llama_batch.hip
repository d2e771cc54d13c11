// llama_batch.hip — batches and windows: several columns (sequences, or consecutive positions of one) per pass over the weights.
#include "llama.h"

using namespace nfai;

// ---- batched decode: n models ("slots" over one set of weights) advance one token each in ONE pass over the weights ---------------
// What N concurrent token loops of the reference do N times over (LlamaModel.cs:116-125 per sequence), with every weight row read
// once per step (kernels_gemv_batch.hip).  A batch owns a workspace and two graphs, no weights and no KV cache: column i of every
// launch reads and writes member i's own activation vectors, cache, token word, ring and position word, so after a batch step each
// member is in the state its own nfai_hip_llama_decode_step would have left.  Launches per token: 1 (embedding rows) + 5 per block
// (q|k|v, attention, Wo, gate|up, Wdown) + 1 (lm_head + ArgMax + bookkeeping), a linear chain on the context's stream.
namespace {

// The words a step exchanges with the device, in the layout the kernels see: am_tok_batch = out (every column's ArgMax; a batch reads
// its tokens from the same words, so a greedy step finds the last one's ArgMax there), err = out + BATCH_MAX (the q|k|v launches'
// error word), out[WIN_NOUT] = n_out, win_ctl = draft | k behind a window's token words.  The pinned host mirror has the same layout.
constexpr uint32_t WIN_MAGIC = 0x4E46574E, WIN_IN = 32;
struct StepWords {
    uint32_t out[BATCH_MAX];
    uint32_t err;
    uint32_t n_out;                         // a window: the count of emitted tokens
    uint32_t pad[WIN_IN - BATCH_MAX - 2];
    uint32_t in[BATCH_MAX];                 // the step's tokens (on the device a window's only: a batch's go to `out`)
    uint32_t draft[BATCH_MAX];
    uint32_t k;                             // the draft count; WIN_ALL: a multi-token step
};
static_assert(offsetof(StepWords, err) == BATCH_MAX * 4 && offsetof(StepWords, n_out) == WIN_NOUT * 4, "am_tok_batch[BATCH_MAX] / [WIN_NOUT]");
static_assert(offsetof(StepWords, in) == WIN_IN * 4 && offsetof(StepWords, draft) == (WIN_IN + BATCH_MAX) * 4 &&
              offsetof(StepWords, k) == (WIN_IN + 2 * BATCH_MAX) * 4, "win_ctl: BATCH_MAX drafts, then their count, behind the token words");
static_assert(sizeof(StepWords) == offsetof(StepWords, k) + 4 && sizeof(StepWords) <= 256, "k is the last word; one 256-byte allocation");
// A wide batch's view of the same allocation: sixteen ArgMax / token words, the error word behind them, the step's tokens at WIN_IN.
struct WideWords {
    uint32_t out[WIDE_MAX];
    uint32_t err;
    uint32_t pad[WIN_IN - WIDE_MAX - 1];
    uint32_t in[WIDE_MAX];
};
static_assert(offsetof(WideWords, in) == offsetof(StepWords, in) && sizeof(WideWords) <= sizeof(StepWords), "one allocation, the tokens where a batch's are");

struct Batch {
    uint32_t magic = 0x4E464254;  // 'NFBT'
    Ctx *ctx = nullptr;
    uint32_t n = 0;
    nfai_model_t handles[WIDE_MAX] = {};
    Model *mem[WIDE_MAX] = {};
    uint64_t serial[WIDE_MAX] = {};
    uint32_t gen[WIDE_MAX] = {};
    bool wide = false;             // nfai_hip_llama_batch_create_wide: up to WIDE_MAX fp16 members on kernels_gemv_wide.hip (WideWords, WideOps)
    bool quant = false;            // the members' matrices are quantised, in the T16 layout (nfai_hip_llama_batch_create_ex, NFAI_BATCH_QUANT[_ANY])
    StepWords *d_w = nullptr, *h_w = nullptr;   // the step's words on the device | their pinned mirror
    void *d_am = nullptr, *d_attn = nullptr;
    Graph g_io[WIDE_MAX + 1];      // by column count (a batch: its n), captured on first use: [tokens H2D] -> the token -> [results D2H]
    Graph g_body;                  // a batch: the token alone (greedy)
    // nfai_hip_llama_batch_step_topk (allocated by its first call): n workspace slices with the members' TopkOut array behind them |
    // that array's pinned mirror | [tokens H2D] -> the token -> the two row launches -> [results + candidates D2H], captured for
    // (topk_t, topk_k) and re-captured when they change
    void *d_topk = nullptr;
    TopkOut *h_topk = nullptr;
    Graph g_topk;
    float topk_t = 0.f;
    uint32_t topk_k = 0;
    // column i's activation vectors: member i's own (a batch), or the window's (every column is mem[0])
    float *cx[WIDE_MAX] = {}, *ch[WIDE_MAX] = {}, *cq[WIDE_MAX] = {}, *catt[WIDE_MAX] = {}, *cact[WIDE_MAX] = {}, *clog[WIDE_MAX] = {};
    const uint32_t *d_in = nullptr;   // the step's token words (a batch: d_w->out, where the tail leaves the next step's)
    // A window (nfai_hip_llama_window_create, magic 'NFWN'): up to max_tokens columns at consecutive positions of mem[0]; n is the
    // column count of the call at hand.
    bool window = false;
    uint32_t max_tokens = 0;
    float *w_act = nullptr;                       // the columns' activation vectors, w_act_floats in all
    size_t w_act_floats = 0;
    uint32_t models() const { return window ? 1u : n; }   // the distinct models behind the columns
    // the step's words in either view (w: d_w or h_w)
    uint32_t *out_of(StepWords *w) const { return wide ? reinterpret_cast<WideWords *>(w)->out : w->out; }
    uint32_t *in_of(StepWords *w) const { return wide ? reinterpret_cast<WideWords *>(w)->in : w->in; }
    uint32_t *err_of(StepWords *w) const { return wide ? &reinterpret_cast<WideWords *>(w)->err : &w->err; }
    size_t out_bytes() const { return window ? offsetof(StepWords, pad) : (wide ? offsetof(WideWords, pad) : offsetof(StepWords, n_out)); }
};

Batch *batch_of(nfai_batch_t h)
{
    if (!handle_live(h)) return nullptr;
    Batch *b = reinterpret_cast<Batch *>(h);
    return b->magic == 0x4E464254 ? b : nullptr;
}

#define BATCH_OR_FAIL(bt, h)                                                      \
    Batch *bt = batch_of(h);                                                      \
    if (!bt) return fail(NFAI_ERR_INVALID, "%s: invalid batch handle", __func__); \
    HIP_TRY(hipSetDevice(bt->ctx->device))

// every model is still the one the batch or window was created over (a destroyed model is an error, not a crash)
int columns_live(Batch *bt, const char *fn)
{
    for (uint32_t i = 0; i < bt->models(); i++) {
        Model *m = model_of(bt->handles[i]);
        if (!m || m != bt->mem[i] || m->serial != bt->serial[i])
            return bt->window ? fail(NFAI_ERR_INVALID, "%s: invalid window: its model was destroyed while the window held it", fn)
                              : fail(NFAI_ERR_INVALID, "%s: invalid member %u: the model was destroyed while the batch held it", fn, i);
        if (!m->finalized || m->weights_gen != bt->gen[i])
            return bt->window
                       ? fail(NFAI_ERR_INVALID, "%s: invalid window: the model's tensors changed after the window was created (make a new window)", fn)
                       : fail(NFAI_ERR_INVALID, "%s: invalid member %u: its tensors changed after the batch was created (make a new batch)", fn, i);
    }
    return NFAI_OK;
}

// the first of the step's n tokens that is no token of the vocabulary
int tokens_ok(Batch *bt, const uint32_t *tokens, uint32_t n, const char *fn)
{
    const uint32_t V = bt->mem[0]->d.V;
    for (uint32_t i = 0; i < n; i++)
        if (tokens[i] >= V) return fail(NFAI_ERR_INVALID, "%s: %s %u: token %u >= vocab %u", fn, bt->window ? "column" : "member", i, tokens[i], V);
    return NFAI_OK;
}

// the existing capacity error, for the first model that has no room for `steps` more positions; nothing is enqueued
int columns_capacity(Batch *bt, uint32_t steps, const char *fn)
{
    for (uint32_t i = 0; i < bt->models(); i++) {
        Model *m = bt->mem[i];
        if ((uint64_t)m->pos_host + steps <= m->d.C) continue;
        if (bt->window)
            return fail(NFAI_ERR_KV_FULL, "%s: KV cache full: %u position(s) from position %u exceed capacity %u (the reference would write out of "
                                          "bounds here)", fn, steps, m->pos_host, m->d.C);
        return fail(NFAI_ERR_KV_FULL, "%s: member %u: KV cache full: %u step(s) from position %u exceed capacity %u (the reference would write out "
                                      "of bounds here)", fn, i, steps, m->pos_host, m->d.C);
    }
    return NFAI_OK;
}

// The five launch forms of a block + the head, for the members of `bt` (also used, with nothing launched, to check the shapes).
struct BatchOps {
    Batch *bt;
    BatchGemvArgs base() const
    {
        BatchGemvArgs a;
        Model *m0 = bt->mem[0];
        a.n = bt->n; a.eps = m0->d.eps; a.n_cu = (uint32_t)bt->ctx->prop.multiProcessorCount;
        return a;
    }
    BatchGemvArgs qkv(size_t l) const
    {
        BatchGemvArgs a = base();
        Model *m0 = bt->mem[0];
        const nfai_llama_desc &d = m0->d;
        const Layer &L = m0->layers[l];
        a.W[0] = L.wq.ptr; a.W[1] = L.wk.ptr; a.W[2] = L.wv.ptr;
        a.seg_rows[0] = (uint32_t)L.wq.rows; a.seg_rows[1] = (uint32_t)L.wk.rows; a.seg_rows[2] = (uint32_t)L.wv.rows;
        a.K = d.E; a.mode = GEMV_QKV_ROPE; a.gamma = static_cast<const float *>(L.attn_norm.ptr);
        for (uint32_t i = 0; i < bt->n; i++) {
            Model *m = bt->mem[i];
            a.x[i] = bt->cx[i]; a.y[i] = bt->cq[i]; a.pos_off[i] = bt->window ? i : 0u;
            a.kc[i] = m->layers[l].kcache; a.vc[i] = m->layers[l].vcache;
            a.kv_head_stride[i] = m->kv_head_stride; a.cap[i] = m->d.C; a.pos[i] = m->d_pos;
        }
        a.kv_pos_stride = m0->kv_pos_stride; a.kv_type = m0->kv_f16 ? NFAI_F16 : NFAI_F32;
        a.freqs = m0->d_freqs; a.rope_dims = d.rope_dims; a.H = d.H; a.Hkv = d.Hkv; a.D = d.D;
        a.err = &bt->d_w->err;
        return a;
    }
    BatchAttnArgs attn(size_t l) const
    {
        BatchAttnArgs a;
        Model *m0 = bt->mem[0];
        a.n = bt->n;
        for (uint32_t i = 0; i < bt->n; i++) {
            Model *m = bt->mem[i];
            a.q[i] = bt->cq[i]; a.o[i] = bt->catt[i]; a.kc[i] = m->layers[l].kcache; a.vc[i] = m->layers[l].vcache;
            a.kv_head_stride[i] = m->kv_head_stride; a.cap[i] = m->d.C; a.pos[i] = m->d_pos;
        }
        a.kv_pos_stride = m0->kv_pos_stride; a.kv_type = m0->kv_f16 ? NFAI_F16 : NFAI_F32;
        a.H = m0->d.H; a.Hkv = m0->d.Hkv; a.D = m0->d.D; a.work = bt->d_attn;
        return a;
    }
    BatchGemvArgs wo(size_t l) const
    {
        BatchGemvArgs a = base();
        Model *m0 = bt->mem[0];
        const Layer &L = m0->layers[l];
        a.W[0] = L.wo.ptr; a.seg_rows[0] = (uint32_t)L.wo.rows; a.K = m0->d.H * m0->d.D; a.mode = GEMV_RESIDUAL;
        for (uint32_t i = 0; i < bt->n; i++) { a.x[i] = bt->catt[i]; a.res[i] = bt->cx[i]; a.y[i] = bt->ch[i]; }
        return a;
    }
    BatchGemvArgs gateup(size_t l) const
    {
        BatchGemvArgs a = base();
        Model *m0 = bt->mem[0];
        const Layer &L = m0->layers[l];
        a.W[0] = L.wgate.ptr; a.W[1] = L.wup.ptr; a.seg_rows[0] = (uint32_t)L.wgate.rows; a.seg_rows[1] = (uint32_t)L.wup.rows;
        a.K = m0->d.E; a.mode = GEMV_GATEUP; a.gamma = static_cast<const float *>(L.ffn_norm.ptr);
        for (uint32_t i = 0; i < bt->n; i++) { a.x[i] = bt->ch[i]; a.y[i] = bt->cact[i]; }
        return a;
    }
    BatchGemvArgs down(size_t l) const
    {
        BatchGemvArgs a = base();
        Model *m0 = bt->mem[0];
        const Layer &L = m0->layers[l];
        a.W[0] = L.wdown.ptr; a.seg_rows[0] = (uint32_t)L.wdown.rows; a.K = m0->d.F; a.mode = GEMV_RESIDUAL;
        for (uint32_t i = 0; i < bt->n; i++) { a.x[i] = bt->cact[i]; a.res[i] = bt->ch[i]; a.y[i] = bt->cx[i]; }
        return a;
    }
    BatchGemvArgs head() const
    {
        BatchGemvArgs a = base();
        Model *m0 = bt->mem[0];
        const Tensor &hd = m0->output.ptr ? m0->output : m0->token_embd;  // tied when output.weight is absent (LlamaModel.cs:64-67)
        a.W[0] = hd.ptr; a.seg_rows[0] = (uint32_t)hd.rows; a.K = m0->d.E; a.mode = GEMV_PLAIN;
        a.gamma = static_cast<const float *>(m0->output_norm.ptr);
        for (uint32_t i = 0; i < bt->n; i++) {
            Model *m = bt->mem[i];
            a.x[i] = bt->cx[i]; a.y[i] = bt->clog[i];
            a.am_tok[i] = m->d_tok; a.am_pos[i] = m->d_pos; a.am_ring[i] = m->d_ring;
        }
        a.am_work = bt->d_am; a.am_tok_batch = bt->d_w->out; a.am_ring_len = RING_LEN;
        if (bt->window && bt->d_in) a.win_ctl = bt->d_w->draft;   // drafts and their count, behind the token words
        return a;
    }
    WindowAttnArgs wattn(size_t l) const
    {
        WindowAttnArgs a;
        Model *m = bt->mem[0];
        a.n = bt->n;
        for (uint32_t i = 0; i < bt->n; i++) { a.q[i] = bt->cq[i]; a.o[i] = bt->catt[i]; }
        a.kc = m->layers[l].kcache; a.vc = m->layers[l].vcache;
        a.kv_head_stride = m->kv_head_stride; a.kv_pos_stride = m->kv_pos_stride; a.cap = m->d.C; a.pos = m->d_pos;
        a.kv_type = m->kv_f16 ? NFAI_F16 : NFAI_F32;
        a.H = m->d.H; a.Hkv = m->d.Hkv; a.D = m->d.D; a.work = bt->d_attn;
        return a;
    }
};

// A GEMV's arguments with the type of its weights: what the quantised kernels take (kernels_gemv_batch_kqm.hip); the fp16 ones take
// the base.
BatchKqArgs batch_kq(const BatchGemvArgs &a, int type)
{
    BatchKqArgs k;
    static_cast<BatchGemvArgs &>(k) = a;
    k.w_type = type;
    return k;
}

// q|k|v of block l: one launch for fp16 members; for quantised ones by weight type, in the fixed order Q4_K, Q5_K, Q6_K, Q8_0, Q4_0, Q3_K, IQ4_XS: one
// launch when the three matrices agree, one per type when they differ (Q4_K_M and Q5_K_M files keep attn_v in Q6_K on half of the
// blocks), so that a launch stages the activations in ONE fragment layout.  Returns the number of launches, three at the most.
int batch_qkv(const BatchOps &ops, size_t l, BatchKqArgs (&out)[3])
{
    const BatchGemvArgs base = ops.qkv(l);
    if (!ops.bt->quant) {
        out[0] = batch_kq(base, NFAI_F16);
        return 1;
    }
    const Layer &L = ops.bt->mem[0]->layers[l];
    const Tensor *t[3] = {&L.wq, &L.wk, &L.wv};
    int n = 0;
    for (int type : {NFAI_Q4_K_T16, NFAI_Q5_K_T16, NFAI_Q6_K_T16, NFAI_Q8_0_T16, NFAI_Q4_0_T16, NFAI_Q3_K_T16, NFAI_IQ4_XS_T16}) {
        BatchKqArgs k = batch_kq(base, type);
        int j = 0;
        for (int i = 0; i < 3; i++) { k.W[i] = nullptr; k.seg_rows[i] = 0; }
        for (int i = 0; i < 3; i++)
            if (t[i]->type == type) { k.W[j] = t[i]->ptr; k.seg_rows[j] = (uint32_t)t[i]->rows; k.seg_role[j] = (uint32_t)i; j++; }
        if (j) out[n++] = k;
    }
    return n;
}

// The launches of one token of every column, in order: the embedding rows, per block q|k|v, attention, Wo, gate|up, Wdown, then the
// head.  enqueue_batch launches them; shapes_ok asks the kernels' predicates about the same sequence.  gemv(class, arguments) takes
// the GEMVs, other(class, block) the embedding (KC_OTHER) and attention launches; a non-zero return ends the walk.
template <class Gemv, class Other>
int batch_token(const BatchOps &ops, Gemv gemv, Other other)
{
    Model *m0 = ops.bt->mem[0];
    S_TRY(other(KC_OTHER, (size_t)0));
    for (size_t l = 0; l < m0->layers.size(); l++) {
        const Layer &L = m0->layers[l];
        BatchKqArgs qkv[3];
        const int nq = batch_qkv(ops, l, qkv);
        for (int j = 0; j < nq; j++) S_TRY(gemv(KC_QKV, qkv[j]));
        S_TRY(other(KC_ATTN, l));
        S_TRY(gemv(KC_WO, batch_kq(ops.wo(l), L.wo.type)));
        S_TRY(gemv(KC_GATEUP, batch_kq(ops.gateup(l), L.wgate.type)));
        S_TRY(gemv(KC_DOWN, batch_kq(ops.down(l), L.wdown.type)));
    }
    return gemv(KC_LMHEAD, batch_kq(ops.head(), (m0->output.ptr ? m0->output : m0->token_embd).type));
}

// The launch forms of a wide batch (kernels_gemv_wide.hip): BatchOps' five GEMVs with sixteen columns, and the existing attention
// kernel once per 8 members (`half`), each launch with its own slice of the workspace.
struct WideOps {
    Batch *bt;
    WideGemvArgs base() const
    {
        WideGemvArgs a;
        a.n = bt->n; a.eps = bt->mem[0]->d.eps; a.n_cu = (uint32_t)bt->ctx->prop.multiProcessorCount;
        return a;
    }
    WideGemvArgs qkv(size_t l) const
    {
        WideGemvArgs a = base();
        Model *m0 = bt->mem[0];
        const nfai_llama_desc &d = m0->d;
        const Layer &L = m0->layers[l];
        a.W[0] = L.wq.ptr; a.W[1] = L.wk.ptr; a.W[2] = L.wv.ptr;
        a.seg_rows[0] = (uint32_t)L.wq.rows; a.seg_rows[1] = (uint32_t)L.wk.rows; a.seg_rows[2] = (uint32_t)L.wv.rows;
        a.K = d.E; a.mode = GEMV_QKV_ROPE; a.gamma = static_cast<const float *>(L.attn_norm.ptr);
        for (uint32_t i = 0; i < bt->n; i++) {
            Model *m = bt->mem[i];
            a.x[i] = bt->cx[i]; a.y[i] = bt->cq[i];
            a.kc[i] = m->layers[l].kcache; a.vc[i] = m->layers[l].vcache;
            a.kv_head_stride[i] = m->kv_head_stride; a.cap[i] = m->d.C; a.pos[i] = m->d_pos;
        }
        a.kv_pos_stride = m0->kv_pos_stride; a.kv_type = m0->kv_f16 ? NFAI_F16 : NFAI_F32;
        a.freqs = m0->d_freqs; a.rope_dims = d.rope_dims; a.H = d.H; a.Hkv = d.Hkv; a.D = d.D;
        a.err = bt->err_of(bt->d_w);
        return a;
    }
    BatchAttnArgs attn(size_t l, uint32_t half) const
    {
        BatchAttnArgs a;
        Model *m0 = bt->mem[0];
        const uint32_t first = half * BATCH_MAX;
        a.n = std::min(BATCH_MAX, bt->n - first);
        for (uint32_t i = 0; i < a.n; i++) {
            Model *m = bt->mem[first + i];
            a.q[i] = bt->cq[first + i]; a.o[i] = bt->catt[first + i]; a.kc[i] = m->layers[l].kcache; a.vc[i] = m->layers[l].vcache;
            a.kv_head_stride[i] = m->kv_head_stride; a.cap[i] = m->d.C; a.pos[i] = m->d_pos;
        }
        a.kv_pos_stride = m0->kv_pos_stride; a.kv_type = m0->kv_f16 ? NFAI_F16 : NFAI_F32;
        a.H = m0->d.H; a.Hkv = m0->d.Hkv; a.D = m0->d.D;
        a.work = static_cast<char *>(bt->d_attn) + half * batch_attn_bytes(m0->d.H, m0->d.D);
        return a;
    }
    WideGemvArgs wo(size_t l) const
    {
        WideGemvArgs a = base();
        Model *m0 = bt->mem[0];
        const Layer &L = m0->layers[l];
        a.W[0] = L.wo.ptr; a.seg_rows[0] = (uint32_t)L.wo.rows; a.K = m0->d.H * m0->d.D; a.mode = GEMV_RESIDUAL;
        for (uint32_t i = 0; i < bt->n; i++) { a.x[i] = bt->catt[i]; a.res[i] = bt->cx[i]; a.y[i] = bt->ch[i]; }
        return a;
    }
    WideGemvArgs gateup(size_t l) const
    {
        WideGemvArgs a = base();
        Model *m0 = bt->mem[0];
        const Layer &L = m0->layers[l];
        a.W[0] = L.wgate.ptr; a.W[1] = L.wup.ptr; a.seg_rows[0] = (uint32_t)L.wgate.rows; a.seg_rows[1] = (uint32_t)L.wup.rows;
        a.K = m0->d.E; a.mode = GEMV_GATEUP; a.gamma = static_cast<const float *>(L.ffn_norm.ptr);
        for (uint32_t i = 0; i < bt->n; i++) { a.x[i] = bt->ch[i]; a.y[i] = bt->cact[i]; }
        return a;
    }
    WideGemvArgs down(size_t l) const
    {
        WideGemvArgs a = base();
        Model *m0 = bt->mem[0];
        const Layer &L = m0->layers[l];
        a.W[0] = L.wdown.ptr; a.seg_rows[0] = (uint32_t)L.wdown.rows; a.K = m0->d.F; a.mode = GEMV_RESIDUAL;
        for (uint32_t i = 0; i < bt->n; i++) { a.x[i] = bt->cact[i]; a.res[i] = bt->ch[i]; a.y[i] = bt->cx[i]; }
        return a;
    }
    WideGemvArgs head() const
    {
        WideGemvArgs a = base();
        Model *m0 = bt->mem[0];
        const Tensor &hd = m0->output.ptr ? m0->output : m0->token_embd;  // tied when output.weight is absent (LlamaModel.cs:64-67)
        a.W[0] = hd.ptr; a.seg_rows[0] = (uint32_t)hd.rows; a.K = m0->d.E; a.mode = GEMV_PLAIN;
        a.gamma = static_cast<const float *>(m0->output_norm.ptr);
        for (uint32_t i = 0; i < bt->n; i++) {
            Model *m = bt->mem[i];
            a.x[i] = bt->cx[i]; a.y[i] = bt->clog[i];
            a.am_tok[i] = m->d_tok; a.am_pos[i] = m->d_pos; a.am_ring[i] = m->d_ring;
        }
        a.am_work = bt->d_am; a.am_tok_batch = bt->out_of(bt->d_w); a.am_ring_len = RING_LEN;
        return a;
    }
};

// batch_token for a wide batch: the same sequence; other(class, block, half) takes the embedding and attention launches of members
// 8 half .. (one launch per 8 members).
template <class Gemv, class Other>
int wide_token(const WideOps &ops, Gemv gemv, Other other)
{
    Model *m0 = ops.bt->mem[0];
    const uint32_t halves = (ops.bt->n + BATCH_MAX - 1) / BATCH_MAX;
    for (uint32_t h = 0; h < halves; h++) S_TRY(other(KC_OTHER, (size_t)0, h));
    for (size_t l = 0; l < m0->layers.size(); l++) {
        S_TRY(gemv(KC_QKV, ops.qkv(l)));
        for (uint32_t h = 0; h < halves; h++) S_TRY(other(KC_ATTN, l, h));
        S_TRY(gemv(KC_WO, ops.wo(l)));
        S_TRY(gemv(KC_GATEUP, ops.gateup(l)));
        S_TRY(gemv(KC_DOWN, ops.down(l)));
    }
    return gemv(KC_LMHEAD, ops.head());
}

// One launch of a token, between the timer's events when the step is profiled.
int timed_launch(LaunchTimer *timer, int c, const std::function<hipError_t()> &f)
{
    if (timer) S_TRY(timer->begin(c));
    const hipError_t e = f();
    if (e != hipSuccess)
        return fail(e == hipErrorInvalidValue ? NFAI_ERR_INVALID : NFAI_ERR_HIP, "batch launch (class %d) failed: %s", c, hipGetErrorString(e));
    if (timer) S_TRY(timer->end());
    return NFAI_OK;
}

int enqueue_wide(Batch *bt, LaunchTimer *timer)
{
    hipStream_t s = bt->ctx->stream;
    Model *m0 = bt->mem[0];
    WideOps ops{bt};
    auto gemv = [&](int c, const WideGemvArgs &a) { return timed_launch(timer, c, [&] { return launch_wide_gemv(a, s); }); };
    auto other = [&](int c, size_t l, uint32_t half) {
        return timed_launch(timer, c, [&] {
            if (c == KC_ATTN) return launch_batch_attn(ops.attn(l, half), s);
            const uint32_t first = half * BATCH_MAX;
            return launch_batch_embed(m0->token_embd.ptr, m0->token_embd.rows, m0->d.E, bt->d_in + first, bt->cx + first,
                                      std::min(BATCH_MAX, bt->n - first), s);
        });
    };
    return wide_token(ops, gemv, other);
}

// One token of every column, enqueued on the stream.  timer (a profiled step): hipEvents around every launch, by class.
int enqueue_batch(Batch *bt, LaunchTimer *timer = nullptr)
{
    if (bt->wide) return enqueue_wide(bt, timer);
    hipStream_t s = bt->ctx->stream;
    Model *m0 = bt->mem[0];
    BatchOps ops{bt};
    auto run = [&](int c, const std::function<hipError_t()> &f) { return timed_launch(timer, c, f); };
    float *xs[BATCH_MAX] = {};
    for (uint32_t i = 0; i < bt->n; i++) xs[i] = bt->cx[i];
    auto gemv = [&](int c, const BatchKqArgs &k) { return run(c, [&] { return bt->quant ? launch_batch_gemv_kq(k, s) : launch_batch_gemv(k, s); }); };
    auto other = [&](int c, size_t l) {
        return run(c, [&] {
            if (c == KC_ATTN) return bt->window ? launch_window_attn(ops.wattn(l), s) : launch_batch_attn(ops.attn(l), s);
            return bt->quant ? launch_batch_embed_kq(m0->token_embd.ptr, m0->token_embd.type, m0->token_embd.rows, m0->d.E, bt->d_in, xs, bt->n, s)
                             : launch_batch_embed(m0->token_embd.ptr, m0->token_embd.rows, m0->d.E, bt->d_in, xs, bt->n, s);
        });
    };
    return batch_token(ops, gemv, other);
}

// The step's words between the pinned mirror and the device: the tokens (a window: with the drafts and their count) in, the ArgMax
// words and the error word (a window: and the emitted count) out.
int words_in(Batch *bt, hipStream_t s)
{
    if (bt->window) HIP_TRY(hipMemcpyAsync(bt->d_w->in, bt->h_w->in, sizeof(StepWords) - offsetof(StepWords, in), hipMemcpyHostToDevice, s));
    else HIP_TRY(hipMemcpyAsync(bt->out_of(bt->d_w), bt->in_of(bt->h_w), bt->n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    return NFAI_OK;
}

int words_out(Batch *bt, hipStream_t s)
{
    HIP_TRY(hipMemcpyAsync(bt->h_w, bt->d_w, bt->out_bytes(), hipMemcpyDeviceToHost, s));
    return NFAI_OK;
}

// with_io: [words_in] -> the token -> [words_out]; otherwise the token alone (greedy).
int columns_capture(Batch *bt, bool with_io, Graph &g)
{
    if (g) return NFAI_OK;
    hipStream_t s = bt->ctx->stream;
    return capture(s, bt->window ? "window" : "batch", [&]() -> int {
        if (with_io) S_TRY(words_in(bt, s));
        S_TRY(enqueue_batch(bt));
        if (with_io) S_TRY(words_out(bt, s));
        return NFAI_OK;
    }, g);
}

void batch_free(Batch *bt)
{
    for (Graph &g : bt->g_io) g.drop();
    bt->g_body.drop();
    bt->g_topk.drop();
    if (bt->d_topk) hipFree(bt->d_topk);
    if (bt->h_topk) hipHostFree(bt->h_topk);
    if (bt->w_act) hipFree(bt->w_act);
    if (bt->d_w) hipFree(bt->d_w);
    if (bt->d_am) hipFree(bt->d_am);
    if (bt->d_attn) hipFree(bt->d_attn);
    if (bt->h_w) hipHostFree(bt->h_w);
    bt->magic = 0;
    delete bt;
}

// A step failed on the device (the error word names the column: a position word at or past the capacity, nothing was written): the
// token's results are not valid.  Every model's position word goes back to the host's view, which did not move; the word is cleared
// for the next step.
int columns_device_failed(Batch *bt, uint32_t code, const char *fn)
{
    hipStream_t s = bt->ctx->stream;
    for (uint32_t i = 0; i < bt->models(); i++) HIP_TRY(hipMemcpyAsync(bt->mem[i]->d_pos, &bt->mem[i]->pos_host, 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(bt->err_of(bt->d_w), 0, 4, s));
    HIP_TRY(hipStreamSynchronize(s));
    *bt->err_of(bt->h_w) = 0;
    const uint32_t i = code & 0xFFu;
    if (bt->window)
        return fail(NFAI_ERR_KV_FULL, "%s: column %u: the position word on the device put it at or past the KV capacity %u (code 0x%x); the "
                                      "position did not move", fn, i, bt->mem[0]->d.C, code);
    return fail(NFAI_ERR_KV_FULL, "%s: member %u: its position word on the device was at or past its KV capacity %u (code 0x%x); no "
                                  "member's position moved", fn, i, i < bt->n ? bt->mem[i]->d.C : 0u, code);
}

// After the synchronisation of one step: the device-side bound, or the host's view of the positions follows the device's (a batch:
// one token per member; a window: the emitted count, *n_out).
int columns_finish(Batch *bt, uint32_t *n_out, const char *fn)
{
    if (*bt->err_of(bt->h_w)) return columns_device_failed(bt, *bt->err_of(bt->h_w), fn);
    if (!bt->window) {
        for (uint32_t i = 0; i < bt->n; i++) { bt->mem[i]->pos_host++; bt->mem[i]->x_last = bt->mem[i]->x; }
        return NFAI_OK;
    }
    Model *m = bt->mem[0];
    const uint32_t n = bt->h_w->n_out;
    if (n < 1 || n > bt->n) return fail(NFAI_ERR_HIP, "%s: the device reported %u emitted tokens of %u columns", fn, n, bt->n);
    m->pos_host += n;
    m->x_last = bt->cx[n - 1];
    *n_out = n;
    return NFAI_OK;
}

// One step launch by launch between hipEvents (the pinned words are filled): device time and launch count by kernel class.
int profile_columns(Batch *bt, float *ms_by_class, uint32_t *launches_by_class, const char *fn)
{
    hipStream_t s = bt->ctx->stream;
    LaunchTimer timer(s);
    S_TRY(words_in(bt, s));
    S_TRY(enqueue_batch(bt, &timer));
    S_TRY(words_out(bt, s));
    S_TRY(timer.collect(ms_by_class, launches_by_class));
    uint32_t n = 0;
    return columns_finish(bt, &n, fn);
}

// One model of a batch or window: what a batch admits as a member (i; the window's model is i = 0), in this order: finalized, a whole
// model, the fused five-launch path, member 0's KV element type, matrix types (fp16 throughout, or with NFAI_BATCH_QUANT Q4_K / Q6_K
// in the T16 layout throughout, with NFAI_BATCH_QUANT_ANY besides it Q5_K / Q8_0 / Q4_0 / Q3_K / IQ4_XS too, in any per-tensor mix), member 0's tensors.
// quant: the model's matrices are quantised.
int admit_member(Model *m, Model *m0, uint32_t i, uint32_t flags, bool window, const char *fn, bool &quant)
{
    const char *obj = window ? "window" : "batch";
    char who[24];   // in messages: "member i" of a batch, "the model" of a window
    if (window) snprintf(who, sizeof who, "the model");
    else snprintf(who, sizeof who, "member %u", i);
    if (!m->finalized) return fail(NFAI_ERR_INVALID, "%s: invalid %s: call nfai_hip_llama_finalize first", fn, who);
    if (!(m->first_stage && m->last_stage))
        return fail(NFAI_ERR_UNSUPPORTED, "%s: %s is a pipeline stage (blocks [%u, %u) of %u); a %s takes whole models", fn, who,
                    m->d.layer_begin, m->d.layer_end, m->d.L, obj);
    if (m->unfused || m->engine)
        return fail(NFAI_ERR_UNSUPPORTED, "%s: %s runs the %s path; a %s takes models of the fused five-launch path", fn, who,
                    m->unfused ? "1:1 (NFAI_LLAMA_UNFUSED)" : "engine", obj);
    if (m->kv_f16 != m0->kv_f16)
        return fail(NFAI_ERR_UNSUPPORTED, "%s: %s keeps an %s KV cache, member 0 an %s one; one element type per batch", fn, who,
                    m->kv_f16 ? "fp16" : "fp32", m0->kv_f16 ? "fp16" : "fp32");
    const bool allow_q = (flags & NFAI_BATCH_QUANT) != 0, allow_any = (flags & NFAI_BATCH_QUANT_ANY) != 0;
    const char *first16 = nullptr, *firstq = nullptr;
    size_t first16_blk = 0, firstq_blk = 0;
    int firstq_type = 0;
    auto mat = [&](const Tensor &t, const char *what, size_t blk) -> int {
        if (!t.ptr) return NFAI_OK;
        if (t.type == NFAI_F16) {
            if (!first16) { first16 = what; first16_blk = blk; }
            return NFAI_OK;
        }
        if (!allow_q)
            return fail(NFAI_ERR_UNSUPPORTED, "%s: %s: %s of block %zu has ggml type %d; the batched kernels take fp16 matrices "
                                              "(K-quant and Q8_0 weights decode through nfai_hip_llama_decode_step)", fn, who, what, blk, ggml_type_of(t.type));
        if (t.type == NFAI_Q4_K || t.type == NFAI_Q6_K)
            return fail(NFAI_ERR_UNSUPPORTED, "%s: %s: %s of block %zu (ggml type %d, %llu rows) runs the VALU fallback (rows %% 16 != 0); the batched "
                                              "int8-MFMA kernels take 16-row tiles", fn, who, what, blk, ggml_type_of(t.type), (unsigned long long)t.rows);
        if (allow_any && (t.type == NFAI_Q5_K || t.type == NFAI_Q8_0 || t.type == NFAI_Q4_0 || t.type == NFAI_Q3_K || t.type == NFAI_IQ4_XS))
            return fail(NFAI_ERR_UNSUPPORTED, "%s: %s: %s of block %zu has ggml type %d in its native layout (the VALU fallback); the batched "
                                              "int8-MFMA kernels take the T16 layout", fn, who, what, blk, ggml_type_of(t.type));
        if (!allow_any && t.type != NFAI_Q4_K_T16 && t.type != NFAI_Q6_K_T16)
            return fail(NFAI_ERR_UNSUPPORTED, "%s: %s: %s of block %zu has ggml type %d; a quantised %s takes Q4_K and Q6_K matrices "
                                              "(Q5_K, Q8_0, Q4_0 and Q3_K weights decode through nfai_hip_llama_decode_step, or in a %s made with "
                                              "NFAI_BATCH_QUANT | NFAI_BATCH_QUANT_ANY)", fn, who, what, blk, ggml_type_of(t.type), obj, obj);
        if (!is_t16(t.type)) return fail(NFAI_ERR_UNSUPPORTED, "%s: %s: %s of block %zu has ggml type %d; a quantised %s takes IQ4_XS, Q3_K, Q4_0, Q4_K, "
                                                               "Q5_K, Q6_K and Q8_0 matrices", fn, who, what, blk, ggml_type_of(t.type), obj);
        if (!firstq) { firstq = what; firstq_blk = blk; firstq_type = ggml_type_of(t.type); }
        return NFAI_OK;
    };
    S_TRY(mat(m->token_embd, "token_embd", 0));
    S_TRY(mat(m->output, "output", 0));
    for (size_t l = 0; l < m->layers.size(); l++) {
        const Layer &L = m->layers[l];
        S_TRY(mat(L.wq, "attn_q", l)); S_TRY(mat(L.wk, "attn_k", l)); S_TRY(mat(L.wv, "attn_v", l)); S_TRY(mat(L.wo, "attn_output", l));
        S_TRY(mat(L.wgate, "ffn_gate", l)); S_TRY(mat(L.wup, "ffn_up", l)); S_TRY(mat(L.wdown, "ffn_down", l));
    }
    if (first16 && firstq)
        return fail(NFAI_ERR_UNSUPPORTED, "%s: %s mixes fp16 and quantised matrices (%s of block %zu is fp16, %s of block %zu has ggml type %d); "
                                          "a %s runs one kernel family", fn, who, first16, first16_blk, firstq, firstq_blk, firstq_type, obj);
    quant = firstq != nullptr;   // (every member reads member 0's tensors, checked next)
    // the same tensors as member 0: a donor and models that called nfai_hip_llama_share_tensors on it, in any order
    bool same = m->layers.size() == m0->layers.size() && m->token_embd.ptr == m0->token_embd.ptr && m->output.ptr == m0->output.ptr &&
                m->output_norm.ptr == m0->output_norm.ptr && m->d.E == m0->d.E && m->d.H == m0->d.H && m->d.Hkv == m0->d.Hkv &&
                m->d.D == m0->d.D && m->d.F == m0->d.F && m->d.V == m0->d.V && m->d.eps == m0->d.eps && m->d.rope_dims == m0->d.rope_dims &&
                m->d.rope_base == m0->d.rope_base && m->d.rope_n_freqs == m0->d.rope_n_freqs;
    for (size_t l = 0; same && l < m->layers.size(); l++) {
        const Layer &A = m->layers[l], &B = m0->layers[l];
        same = A.attn_norm.ptr == B.attn_norm.ptr && A.wq.ptr == B.wq.ptr && A.wk.ptr == B.wk.ptr && A.wv.ptr == B.wv.ptr && A.wo.ptr == B.wo.ptr &&
               A.ffn_norm.ptr == B.ffn_norm.ptr && A.wgate.ptr == B.wgate.ptr && A.wup.ptr == B.wup.ptr && A.wdown.ptr == B.wdown.ptr;
    }
    if (!same)
        return fail(NFAI_ERR_UNSUPPORTED, "%s: %s does not read the same tensors as member 0 (one copy of the weights per batch: "
                                          "nfai_hip_llama_share_tensors)", fn, who);
    return NFAI_OK;
}

// Do the batched kernels take the members' shapes?  Asked before anything is allocated, at every column count the object may be called
// with (a batch: its n; a window: 1 .. win_tokens); t_bad: the count they refuse.
bool shapes_ok(Batch *bt, uint32_t win_tokens, uint32_t &t_bad)
{
    Model *m0 = bt->mem[0];
    BatchOps ops{bt};
    StepWords words;
    uint32_t dummy = 0;
    bt->d_w = &words; bt->d_am = &dummy; bt->d_attn = &dummy;   // placeholders for the argument checks only
    const uint32_t n = bt->n;
    bool ok = attn_group_ok(m0->d.H / m0->d.Hkv);
    if (bt->wide) {
        ok = ok && wide_token(WideOps{bt}, [](int, const WideGemvArgs &a) { return wide_gemv_ok(a) ? 0 : 1; }, [](int, size_t, uint32_t) { return 0; }) == 0;
        bt->d_w = nullptr; bt->d_am = nullptr; bt->d_attn = nullptr;
        t_bad = n;
        return ok;
    }
    t_bad = n;
    for (uint32_t t = win_tokens ? 1 : n; ok && t <= (win_tokens ? win_tokens : n); t++) {
        bt->n = t_bad = t;
        ok = batch_token(ops, [&](int, const BatchKqArgs &k) { return (bt->quant ? batch_gemv_kq_ok(k) : batch_gemv_ok(k)) ? 0 : 1; },
                         [](int, size_t) { return 0; }) == 0;
        if (bt->quant) {   // the quantised embedding rows, and gate | up of one type per block
            ok = ok && m0->d.E % 256 == 0;
            for (const Layer &L : m0->layers) ok = ok && L.wgate.type == L.wup.type;
        }
    }
    bt->d_w = nullptr; bt->d_am = nullptr; bt->d_attn = nullptr;
    return ok;
}

// The object's own device memory: the step's words and their pinned mirror, the ArgMax and attention workspaces, and a window's
// activation vectors (the model's stay what its last own token left).
int columns_alloc(Batch *bt, uint32_t win_tokens, const char *fn)
{
    Model *m0 = bt->mem[0];
    hipStream_t s = bt->ctx->stream;
    S_TRY(dalloc(reinterpret_cast<void **>(&bt->d_w), sizeof(StepWords), s));
    S_TRY(dalloc(&bt->d_am, bt->wide ? wide_argmax_bytes() : batch_argmax_bytes(), s));
    // (a wide batch: one workspace slice per attention launch of 8 members)
    S_TRY(dalloc(&bt->d_attn, win_tokens ? window_attn_bytes(m0->d.H, m0->d.D) : (bt->wide ? 2 : 1) * batch_attn_bytes(m0->d.H, m0->d.D), s));
    if (win_tokens) {
        const nfai_llama_desc &d = m0->d;
        auto r64 = [](size_t v) { return (v + 63) & ~(size_t)63; };   // every vector on a 256-byte boundary
        const size_t E = r64(d.E), HD = r64((size_t)d.H * d.D), F = r64(d.F), per = 2 * E + 2 * HD + F + r64(d.V);
        S_TRY(dalloc(reinterpret_cast<void **>(&bt->w_act), per * win_tokens * 4, s));
        bt->w_act_floats = per * win_tokens;
        for (uint32_t i = 0; i < win_tokens; i++) {
            float *b = bt->w_act + per * i;
            bt->cx[i] = b; bt->ch[i] = b + E; bt->cq[i] = b + 2 * E; bt->catt[i] = b + 2 * E + HD; bt->cact[i] = b + 2 * E + 2 * HD;
            bt->clog[i] = b + 2 * E + 2 * HD + F;
        }
    }
    if (hipHostMalloc(reinterpret_cast<void **>(&bt->h_w), sizeof(StepWords), hipHostMallocDefault) != hipSuccess) return fail(NFAI_ERR_OOM, "%s: pinned staging", fn);
    memset(bt->h_w, 0, sizeof(StepWords));
    bt->d_in = win_tokens ? bt->d_w->in : bt->out_of(bt->d_w);
    if (hipStreamSynchronize(s) != hipSuccess) return fail(NFAI_ERR_HIP, "%s: stream synchronisation failed", fn);
    return NFAI_OK;
}

}  // namespace

// fn: the entry point's name in messages.  flags: NFAI_BATCH_* (0 = the fp16 batch of nfai_hip_llama_batch_create).
// win_tokens > 0 (nfai_hip_llama_window_create, n = 1): the one model is admitted as a batch admits a member, and the object made is a
// window of win_tokens columns over it.
// wide (nfai_hip_llama_batch_create_wide): up to WIDE_MAX fp16 members on the MFMA kernels; flags must be 0.
static int batch_create_impl(const nfai_model_t *models, uint32_t n, uint32_t flags, nfai_batch_t *out, const char *fn, uint32_t win_tokens = 0,
                             bool wide = false)
{
    if (!models || !out) return fail(NFAI_ERR_INVALID, "%s: null argument", fn);
    if (wide && flags) return fail(NFAI_ERR_INVALID, "%s: invalid flags 0x%x (a wide batch takes none: fp16 matrices only)", fn, flags);
    if (wide && (n < 1 || n > WIDE_MAX)) return fail(NFAI_ERR_INVALID, "%s: invalid n = %u (a wide batch holds 1 to %u models)", fn, n, WIDE_MAX);
    if (flags & ~(uint32_t)(NFAI_BATCH_QUANT | NFAI_BATCH_QUANT_ANY))
        return fail(NFAI_ERR_INVALID, "%s: invalid flags 0x%x (known: NFAI_BATCH_QUANT = 0x%x, NFAI_BATCH_QUANT_ANY = 0x%x)", fn, flags,
                    NFAI_BATCH_QUANT, NFAI_BATCH_QUANT_ANY);
    if ((flags & NFAI_BATCH_QUANT_ANY) && !(flags & NFAI_BATCH_QUANT))
        return fail(NFAI_ERR_INVALID, "%s: flags 0x%x: NFAI_BATCH_QUANT_ANY widens NFAI_BATCH_QUANT and is only valid together with it", fn, flags);
    if (!wide && (n < 1 || n > BATCH_MAX)) return fail(NFAI_ERR_INVALID, "%s: invalid n = %u (a batch holds 1 to %u models)", fn, n, BATCH_MAX);
    Model *mem[WIDE_MAX] = {};
    for (uint32_t i = 0; i < n; i++) {
        mem[i] = model_of(models[i]);
        if (!mem[i]) return fail(NFAI_ERR_INVALID, "%s: member %u: invalid model handle", fn, i);
        for (uint32_t j = 0; j < i; j++)
            if (mem[j] == mem[i]) return fail(NFAI_ERR_INVALID, "%s: invalid member %u: the same model as member %u", fn, i, j);
    }
    Model *m0 = mem[0];
    for (uint32_t i = 0; i < n; i++)
        if (mem[i]->ctx != m0->ctx) return fail(NFAI_ERR_INVALID, "%s: invalid member %u: it lives on another context than member 0", fn, i);
    HIP_TRY(hipSetDevice(m0->ctx->device));
    bool quant = false;
    for (uint32_t i = 0; i < n; i++) S_TRY(admit_member(mem[i], m0, i, flags, win_tokens != 0, fn, quant));
    if (!m0->token_embd.ptr) return fail(NFAI_ERR_UNSUPPORTED, "%s: member 0 has no token embedding", fn);
    Batch *bt = new Batch();
    bt->ctx = m0->ctx;
    bt->n = n;
    bt->quant = quant;
    bt->wide = wide;
    for (uint32_t i = 0; i < n; i++) {
        Model *m = mem[i];
        bt->handles[i] = models[i]; bt->mem[i] = m; bt->serial[i] = m->serial; bt->gen[i] = m->weights_gen;
        bt->cx[i] = m->x; bt->ch[i] = m->h; bt->cq[i] = m->q; bt->catt[i] = m->att; bt->cact[i] = m->act; bt->clog[i] = m->logits;
    }
    if (win_tokens) {
        bt->magic = WIN_MAGIC; bt->window = true; bt->max_tokens = win_tokens;
        for (uint32_t i = 0; i < BATCH_MAX; i++) { bt->handles[i] = models[0]; bt->mem[i] = m0; bt->serial[i] = m0->serial; bt->gen[i] = m0->weights_gen; }
    }
    uint32_t t_bad = n;
    if (!shapes_ok(bt, win_tokens, t_bad)) {
        const nfai_llama_desc &d = m0->d;
        delete bt;
        if (win_tokens)
            return fail(NFAI_ERR_UNSUPPORTED, "%s: the batched kernels do not take this shape at %u of the window's %u columns (E %u, F %u, H %u, "
                                              "Hkv %u, D %u, V %u)", fn, t_bad, win_tokens, d.E, d.F, d.H, d.Hkv, d.D, d.V);
        return fail(NFAI_ERR_UNSUPPORTED, "%s: the batched kernels do not take this shape at n = %u (E %u, F %u, H %u, Hkv %u, D %u, V %u)", fn, n,
                    d.E, d.F, d.H, d.Hkv, d.D, d.V);
    }
    const int rc = columns_alloc(bt, win_tokens, fn);
    if (rc) {
        batch_free(bt);
        return rc;
    }
    handle_register(bt);
    *out = reinterpret_cast<nfai_batch_t>(bt);
    return NFAI_OK;
}

NFAI_API int32_t nfai_hip_llama_batch_create(const nfai_model_t *models, uint32_t n, nfai_batch_t *out)
{
    return batch_create_impl(models, n, 0, out, "batch_create");
}

NFAI_API int32_t nfai_hip_llama_batch_create_ex(const nfai_model_t *models, uint32_t n, uint32_t flags, nfai_batch_t *out)
{
    return batch_create_impl(models, n, flags, out, "batch_create_ex");
}

NFAI_API int32_t nfai_hip_llama_batch_create_wide(const nfai_model_t *models, uint32_t n, uint32_t flags, nfai_batch_t *out)
{
    return batch_create_impl(models, n, flags, out, "batch_create_wide", 0, true);
}

NFAI_API int32_t nfai_hip_llama_batch_destroy(nfai_batch_t h)
{
    BATCH_OR_FAIL(bt, h);
    hipStreamSynchronize(bt->ctx->stream);
    handle_unregister(bt);
    batch_free(bt);
    return NFAI_OK;
}

NFAI_API int32_t nfai_hip_llama_batch_step(nfai_batch_t h, const uint32_t *tokens, float *logits_host, uint32_t *argmax)
{
    BATCH_OR_FAIL(bt, h);
    S_TRY(columns_live(bt, "batch_step"));
    if (!tokens) return fail(NFAI_ERR_INVALID, "batch_step: null tokens");
    S_TRY(tokens_ok(bt, tokens, bt->n, "batch_step"));
    S_TRY(columns_capacity(bt, 1, "batch_step"));
    S_TRY(columns_capture(bt, true, bt->g_io[bt->n]));
    hipStream_t s = bt->ctx->stream;
    for (uint32_t i = 0; i < bt->n; i++) bt->in_of(bt->h_w)[i] = tokens[i];
    HIP_TRY(hipGraphLaunch(bt->g_io[bt->n].exec, s));
    HIP_TRY(hipStreamSynchronize(s));
    S_TRY(columns_finish(bt, nullptr, "batch_step"));
    if (argmax)
        for (uint32_t i = 0; i < bt->n; i++) argmax[i] = bt->out_of(bt->h_w)[i];
    if (logits_host) {
        const uint32_t V = bt->mem[0]->d.V;
        for (uint32_t i = 0; i < bt->n; i++)
            HIP_TRY(hipMemcpyAsync(logits_host + (size_t)i * V, bt->mem[i]->logits, (size_t)V * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return NFAI_OK;
}

// ---- a step that returns every member's TopP candidates (the reference's DEFAULT sampler, LlamaModel.cs:128-130,165) ----------------
namespace {

TopkOut *topk_out_dev(Batch *bt) { return reinterpret_cast<TopkOut *>(static_cast<char *>(bt->d_topk) + bt->n * topk_rows_stride(bt->mem[0]->d.V)); }

// [words_in] -> the token -> candidates of every member's logits (ONE pair of launches) -> [words_out + all candidates in one copy],
// a linear chain; kept until (temperature, k) change (ensure_sync_graph in llama.hip is the single model's form).
int ensure_topk_graph(Batch *bt, float temperature, uint32_t k)
{
    if (bt->g_topk && bt->topk_t == temperature && bt->topk_k == k) return NFAI_OK;
    bt->g_topk.drop();
    hipStream_t s = bt->ctx->stream;
    S_TRY(capture(s, "batch top-k", [&]() -> int {
        S_TRY(words_in(bt, s));
        S_TRY(enqueue_batch(bt));
        const uint32_t V = bt->mem[0]->d.V;
        for (uint32_t first = 0; first < bt->n; first += BATCH_MAX) {   // one pair of launches per 8 rows (a wide batch: two)
            TopkRowsArgs rows;
            const uint32_t r = std::min(BATCH_MAX, bt->n - first);
            for (uint32_t i = 0; i < r; i++) rows.x[i] = bt->clog[first + i];   // fp32 logits whatever the weights are
            const hipError_t e = launch_topk_rows(rows, r, V, temperature, k, static_cast<char *>(bt->d_topk) + first * topk_rows_stride(V),
                                                  topk_out_dev(bt) + first, s);
            if (e != hipSuccess)
                return fail(e == hipErrorInvalidValue ? NFAI_ERR_INVALID : NFAI_ERR_HIP, "batch_step_topk: launch failed: %s", hipGetErrorString(e));
        }
        S_TRY(words_out(bt, s));
        HIP_TRY(hipMemcpyAsync(bt->h_topk, topk_out_dev(bt), bt->n * sizeof(TopkOut), hipMemcpyDeviceToHost, s));
        return NFAI_OK;
    }, bt->g_topk));
    bt->topk_t = temperature;
    bt->topk_k = k;
    return NFAI_OK;
}

}  // namespace

NFAI_API int32_t nfai_hip_llama_batch_step_topk(nfai_batch_t h, const uint32_t *tokens, float temperature, uint32_t k, uint32_t *ids_out,
                                                float *probs_out)
{
    BATCH_OR_FAIL(bt, h);
    S_TRY(columns_live(bt, "batch_step_topk"));
    // every argument is checked BEFORE anything is enqueued: a refused call leaves every member's position where it was
    if (!tokens || !ids_out || !probs_out) return fail(NFAI_ERR_INVALID, "batch_step_topk: null argument");
    const uint32_t V = bt->mem[0]->d.V;
    S_TRY(tokens_ok(bt, tokens, bt->n, "batch_step_topk"));
    if (k == 0 || k > TOPK_MAX || k > V) return fail(NFAI_ERR_INVALID, "batch_step_topk: k=%u outside [1, min(%u, V=%u)]", k, TOPK_MAX, V);
    if (!(temperature > 0.f))
        return fail(NFAI_ERR_INVALID, "batch_step_topk: temperature %g (the reference divides by it, SamplingUtils.cs:7)", temperature);
    S_TRY(columns_capacity(bt, 1, "batch_step_topk"));
    hipStream_t s = bt->ctx->stream;
    if (!bt->d_topk) {   // (before the capture: an allocation is no stream operation)  Both or neither: a half-made pair is undone
        void *work = nullptr;
        TopkOut *pin = nullptr;
        int rc = dalloc(&work, bt->n * topk_rows_stride(V) + bt->n * sizeof(TopkOut), s);
        if (!rc && hipHostMalloc(reinterpret_cast<void **>(&pin), bt->n * sizeof(TopkOut), hipHostMallocDefault) != hipSuccess)
            rc = fail(NFAI_ERR_OOM, "batch_step_topk: pinned staging");
        if (rc) {
            hipStreamSynchronize(s);
            if (work) hipFree(work);
            return rc;
        }
        bt->d_topk = work;
        bt->h_topk = pin;
    }
    S_TRY(ensure_topk_graph(bt, temperature, k));
    for (uint32_t i = 0; i < bt->n; i++) bt->in_of(bt->h_w)[i] = tokens[i];
    HIP_TRY(hipGraphLaunch(bt->g_topk.exec, s));
    HIP_TRY(hipStreamSynchronize(s));
    S_TRY(columns_finish(bt, nullptr, "batch_step_topk"));
    for (uint32_t i = 0; i < bt->n; i++) {
        const TopkOut &o = bt->h_topk[i];
        topk_finish(o.v, o.i, o.M, o.S, temperature, k, ids_out + (size_t)i * k, probs_out + (size_t)i * k);
    }
    return NFAI_OK;
}

NFAI_API int32_t nfai_hip_llama_batch_greedy(nfai_batch_t h, const uint32_t *first_tokens, uint32_t n_steps, uint32_t *tokens_out)
{
    BATCH_OR_FAIL(bt, h);
    S_TRY(columns_live(bt, "batch_greedy"));
    if (!first_tokens || !tokens_out) return fail(NFAI_ERR_INVALID, "batch_greedy: null argument");
    if (n_steps == 0 || n_steps > RING_LEN) return fail(NFAI_ERR_INVALID, "batch_greedy: n_steps = %u outside [1, %u]", n_steps, RING_LEN);
    S_TRY(tokens_ok(bt, first_tokens, bt->n, "batch_greedy"));
    S_TRY(columns_capacity(bt, n_steps, "batch_greedy"));
    S_TRY(columns_capture(bt, false, bt->g_body));
    hipStream_t s = bt->ctx->stream;
    for (uint32_t i = 0; i < bt->n; i++) bt->in_of(bt->h_w)[i] = first_tokens[i];
    S_TRY(words_in(bt, s));
    // the feedback stays on the device: the lm_head launch leaves every member's ArgMax in the batch's token words
    for (uint32_t st = 0; st < n_steps; st++) HIP_TRY(hipGraphLaunch(bt->g_body.exec, s));
    std::vector<uint32_t> ring((size_t)bt->n * RING_LEN);
    for (uint32_t i = 0; i < bt->n; i++)
        HIP_TRY(hipMemcpyAsync(ring.data() + (size_t)i * RING_LEN, bt->mem[i]->d_ring, RING_LEN * 4, hipMemcpyDeviceToHost, s));
    S_TRY(words_out(bt, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (*bt->err_of(bt->h_w)) return columns_device_failed(bt, *bt->err_of(bt->h_w), "batch_greedy");
    for (uint32_t i = 0; i < bt->n; i++) {
        Model *m = bt->mem[i];
        for (uint32_t st = 0; st < n_steps; st++) tokens_out[(size_t)st * bt->n + i] = ring[(size_t)i * RING_LEN + (m->pos_host + st) % RING_LEN];
        m->pos_host += n_steps;
        m->x_last = m->x;
    }
    return NFAI_OK;
}

NFAI_API int32_t nfai_hip_llama_batch_bytes_per_token(nfai_batch_t h, uint64_t *total)
{
    BATCH_OR_FAIL(bt, h);
    S_TRY(columns_live(bt, "batch_bytes_per_token"));
    Model *m0 = bt->mem[0];
    const nfai_llama_desc &d = m0->d;
    uint64_t t = weights_once_bytes(m0, bt->quant);   // (W + n KV(p))
    for (uint32_t i = 0; i < bt->n; i++) {   // per member: its embedding row, its KV rows read (p + 1 positions) and written (1)
        Model *m = bt->mem[i];
        if (!bt->quant || m0->output.ptr) t += weight_row_bytes(m0->token_embd.type, d.E);   // (a tied quantised table is the head's)
        t += (uint64_t)m0->layers.size() * (2ull * d.Hkv * d.D * m->kv_esz * ((uint64_t)m->pos_host + 1) + 2ull * d.Hkv * d.D * m->kv_esz);
    }
    if (total) *total = t;
    return NFAI_OK;
}

// One batch step launch by launch between hipEvents (slow path, for tools/batch_decode_bench.py): device time and launch count by
// kernel class (the ids of nfai_hip_llama_profile_step).  It IS a step: every member advances by one token.
NFAI_API int32_t nfai_hip_llama_batch_profile_step(nfai_batch_t h, const uint32_t *tokens, float *ms_by_class, uint32_t *launches_by_class)
{
    BATCH_OR_FAIL(bt, h);
    S_TRY(columns_live(bt, "batch_profile_step"));
    if (!tokens || !ms_by_class || !launches_by_class) return fail(NFAI_ERR_INVALID, "batch_profile_step: null argument");
    S_TRY(tokens_ok(bt, tokens, bt->n, "batch_profile_step"));
    S_TRY(columns_capacity(bt, 1, "batch_profile_step"));
    for (uint32_t i = 0; i < bt->n; i++) bt->in_of(bt->h_w)[i] = tokens[i];
    return profile_columns(bt, ms_by_class, launches_by_class, "batch_profile_step");
}

// ---- window: up to 8 CONSECUTIVE positions of one sequence per pass over the weights (greedy speculative decoding) ------------------
// The batched launches with every column bound to the same model at positions p, p + 1, ... (BatchGemvArgs::pos_off), the window
// attention (kernels_attn_window.hip) in place of k_battn, and the accept rule in the lm_head tail (win_tail, common.h).  A window
// is a Batch with `window` set: it owns the columns' activation vectors, workspaces, token / draft / result words, pinned staging
// and one graph per column count; the weights, the KV cache, the position word, the token word and the ring are the model's.
namespace {

Batch *window_of(nfai_window_t h)
{
    if (!handle_live(h)) return nullptr;
    Batch *b = reinterpret_cast<Batch *>(h);
    return b->magic == WIN_MAGIC ? b : nullptr;
}

#define WINDOW_OR_FAIL(bt, h)                                                      \
    Batch *bt = window_of(h);                                                      \
    if (!bt) return fail(NFAI_ERR_INVALID, "%s: invalid window handle", __func__); \
    HIP_TRY(hipSetDevice(bt->ctx->device))

// The arguments every stepping entry point checks before anything is enqueued; sets the column count and fills the pinned words.
// k = WIN_ALL: a multi-token step (every column is kept).
int window_prepare(Batch *bt, const uint32_t *tokens, uint32_t t, const uint32_t *draft, uint32_t k, const char *fn)
{
    S_TRY(columns_live(bt, fn));
    if (t < 1 || t > bt->max_tokens) return fail(NFAI_ERR_INVALID, "%s: invalid token count %u (this window takes 1 to %u per step)", fn, t, bt->max_tokens);
    S_TRY(tokens_ok(bt, tokens, t, fn));
    S_TRY(columns_capacity(bt, t, fn));
    bt->n = t;
    for (uint32_t i = 0; i < BATCH_MAX; i++) {
        bt->h_w->in[i] = i < t ? tokens[i] : 0u;
        bt->h_w->draft[i] = (k != WIN_ALL && i < k) ? draft[i] : 0u;
    }
    bt->h_w->k = k;
    return NFAI_OK;
}

int window_run(Batch *bt, float *logits_host, uint32_t *n_out, const char *fn)
{
    S_TRY(columns_capture(bt, true, bt->g_io[bt->n]));
    hipStream_t s = bt->ctx->stream;
    HIP_TRY(hipGraphLaunch(bt->g_io[bt->n].exec, s));
    if (logits_host) {   // the columns' logits behind the graph, in front of the ONE synchronisation
        const size_t V = bt->mem[0]->d.V;
        for (uint32_t i = 0; i < bt->n; i++) HIP_TRY(hipMemcpyAsync(logits_host + i * V, bt->clog[i], V * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return columns_finish(bt, n_out, fn);
}

}  // namespace

NFAI_API int32_t nfai_hip_llama_window_create(nfai_model_t model, uint32_t max_tokens, uint32_t flags, nfai_window_t *out)
{
    if (!out) return fail(NFAI_ERR_INVALID, "window_create: null argument");
    if (max_tokens < 2 || max_tokens > BATCH_MAX)
        return fail(NFAI_ERR_INVALID, "window_create: invalid max_tokens = %u (a window takes 2 to %u tokens per step)", max_tokens, BATCH_MAX);
    return batch_create_impl(&model, 1, flags, out, "window_create", max_tokens);
}

NFAI_API int32_t nfai_hip_llama_window_destroy(nfai_window_t h)
{
    WINDOW_OR_FAIL(bt, h);
    hipStreamSynchronize(bt->ctx->stream);
    Model *m = model_of(bt->handles[0]);
    // the hidden state of the last token is where that token left it (columns_finish); a model whose last token went through THIS
    // window falls back to its own vector, one that went through another window or its own path since keeps what it has
    if (m && m == bt->mem[0] && m->serial == bt->serial[0] && bt->w_act && m->x_last >= bt->w_act && m->x_last < bt->w_act + bt->w_act_floats)
        m->x_last = m->x;
    handle_unregister(bt);
    batch_free(bt);
    return NFAI_OK;
}

NFAI_API int32_t nfai_hip_llama_window_step(nfai_window_t h, const uint32_t *tokens, uint32_t t, float *logits_host, uint32_t *argmax)
{
    WINDOW_OR_FAIL(bt, h);
    if (!tokens) return fail(NFAI_ERR_INVALID, "window_step: null tokens");
    S_TRY(window_prepare(bt, tokens, t, nullptr, WIN_ALL, "window_step"));
    uint32_t n = 0;
    S_TRY(window_run(bt, logits_host, &n, "window_step"));
    if (argmax)
        for (uint32_t i = 0; i < t; i++) argmax[i] = bt->h_w->out[i];
    return NFAI_OK;
}

NFAI_API int32_t nfai_hip_llama_window_verify(nfai_window_t h, uint32_t token, const uint32_t *draft, uint32_t k, float *logits_host,
                                              uint32_t *tokens_out, uint32_t *n_out)
{
    WINDOW_OR_FAIL(bt, h);
    if (!tokens_out || !n_out || (k && !draft)) return fail(NFAI_ERR_INVALID, "window_verify: null argument");
    if (k + 1 > bt->max_tokens || k >= BATCH_MAX)
        return fail(NFAI_ERR_INVALID, "window_verify: invalid draft count %u (this window verifies 0 to %u drafts per step)", k, bt->max_tokens - 1);
    uint32_t cols[BATCH_MAX] = {token};
    for (uint32_t i = 0; i < k; i++) cols[1 + i] = draft[i];
    S_TRY(window_prepare(bt, cols, k + 1, draft, k, "window_verify"));
    uint32_t n = 0;
    S_TRY(window_run(bt, logits_host, &n, "window_verify"));
    for (uint32_t i = 0; i < n; i++) tokens_out[i] = bt->h_w->out[i];
    *n_out = n;
    return NFAI_OK;
}

NFAI_API int32_t nfai_hip_llama_window_bytes_per_step(nfai_window_t h, uint32_t t, uint64_t *total)
{
    WINDOW_OR_FAIL(bt, h);
    S_TRY(columns_live(bt, "window_bytes_per_step"));
    if (t < 1 || t > bt->max_tokens) return fail(NFAI_ERR_INVALID, "window_bytes_per_step: invalid token count %u (1 to %u)", t, bt->max_tokens);
    Model *m = bt->mem[0];
    const nfai_llama_desc &d = m->d;
    uint64_t b = weights_once_bytes(m, bt->quant);   // as a batch step (nfai_hip_llama_batch_bytes_per_token)
    if (!bt->quant || m->output.ptr) b += (uint64_t)t * weight_row_bytes(m->token_embd.type, d.E);
    // KV: the p prefix rows ONCE for all columns, column i's i + 1 window rows, t rows written
    const uint64_t row = 2ull * d.Hkv * d.D * m->kv_esz;
    b += (uint64_t)m->layers.size() * row * ((uint64_t)m->pos_host + (uint64_t)t * (t + 1) / 2 + t);
    if (total) *total = b;
    return NFAI_OK;
}

// One window step of t tokens (as _window_step without results: the position advances by t) launch by launch between hipEvents.
NFAI_API int32_t nfai_hip_llama_window_profile_step(nfai_window_t h, const uint32_t *tokens, uint32_t t, float *ms_by_class, uint32_t *launches_by_class)
{
    WINDOW_OR_FAIL(bt, h);
    if (!tokens || !ms_by_class || !launches_by_class) return fail(NFAI_ERR_INVALID, "window_profile_step: null argument");
    S_TRY(window_prepare(bt, tokens, t, nullptr, WIN_ALL, "window_profile_step"));
    return profile_columns(bt, ms_by_class, launches_by_class, "window_profile_step");
}

// Test hook (not in nfai_hip.h, like nfai_hip_debug_read_kv_rows): column `col`'s vector of the last window call — which 1 = q of the
// last block (after RoPE), 2 = that block's attention output — for tests that check the window attention launch on its own.
NFAI_API int32_t nfai_hip_debug_window_read(nfai_window_t h, uint32_t col, int32_t which, float *host, uint64_t n)
{
    WINDOW_OR_FAIL(bt, h);
    S_TRY(columns_live(bt, "debug_window_read"));
    Model *m = bt->mem[0];
    if (!host || col >= bt->max_tokens || (which != 1 && which != 2) || n > (uint64_t)m->d.H * m->d.D)
        return fail(NFAI_ERR_INVALID, "debug_window_read: invalid argument");
    HIP_TRY(hipMemcpyAsync(host, which == 1 ? bt->cq[col] : bt->catt[col], n * 4, hipMemcpyDeviceToHost, bt->ctx->stream));
    HIP_TRY(hipStreamSynchronize(bt->ctx->stream));
    return NFAI_OK;
}
