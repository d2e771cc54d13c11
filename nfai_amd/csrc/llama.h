// llama.h — what the model-layer translation units share (llama.hip: the model and its token path; llama_prefill.hip: the MFMA
// prompt path; llama_batch.hip: batches and windows).  Private to the library: nothing here is exported.
#pragma once
#include <string.h>

#include <algorithm>
#include <functional>

#include <map>
#include <memory>
#include <string>
#include <vector>

#include "common.h"

namespace nfai {

struct Tensor {
    int type = -1;
    uint64_t rows = 0, cols = 0;
    void *ptr = nullptr;
    bool owned = false;
    uint64_t bytes = 0;
};

struct Layer {
    Tensor attn_norm, wq, wk, wv, wo, ffn_norm, wgate, wup, wdown;
    void *kcache = nullptr, *vcache = nullptr;
};

// K-quant models: the blocks' matrices widened to fp16 for the MFMA GEMMs (allocated on first use) — one slot per block, each
// widened ONCE and kept, when that fits the memory budget (288 GB of HBM: 6.4 GB at 3B, 16 GB at 8B); otherwise one slot, re-widened
// for every block of every chunk.  Shared by the slots of a pipeline stage (nfai_hip_llama_share_tensors on the same context): one
// copy per set of weights, not one per in-flight sequence.
struct WideShadow {
    void *ptr = nullptr;
    uint64_t bytes = 0;
    bool all = false;
    uint64_t slot = 0;               // bytes per block slot
    std::vector<uint8_t> done;       // per block: slot holds the current weights
    ~WideShadow() { if (ptr) hipFree(ptr); }
};

// A captured graph and its executable form.
struct Graph {
    hipGraph_t g = nullptr;
    hipGraphExec_t exec = nullptr;
    explicit operator bool() const { return exec != nullptr; }
    void drop()
    {
        if (exec) { hipGraphExecDestroy(exec); exec = nullptr; }
        if (g) { hipGraphDestroy(g); g = nullptr; }
    }
};

// What `body` enqueues on `s`, as a graph: synchronise, capture, instantiate.  The capture is ALWAYS ended before an error is reported
// (a stream left in capture mode would poison every later call); the partial graph is destroyed and the body's own code comes first.
template <class Body>
int capture(hipStream_t s, const char *what, Body body, Graph &out)
{
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = body();
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(s, &g);
    if (rc || e != hipSuccess) {
        if (g) hipGraphDestroy(g);
        if (rc) return rc;
        return fail(NFAI_ERR_HIP, "capturing the %s graph failed: %s", what, hipGetErrorString(e));
    }
    out.g = g;
    HIP_TRY(hipGraphInstantiate(&out.exec, g, nullptr, nullptr, 0));
    return NFAI_OK;
}

enum KClass { KC_QKV = 0, KC_ATTN = 1, KC_WO = 2, KC_GATEUP = 3, KC_DOWN = 4, KC_LMHEAD = 5, KC_OTHER = 6, KC_ENGINE = 7, KC_N = 8 };

constexpr uint32_t RING_LEN = 8192;

// A hipEvent pair around every launch of a profiled step, summed by kernel class.  The events are the timer's own: whatever it
// created goes with it, also when a launch failed between begin() and end().
struct LaunchTimer {
    hipStream_t s;
    std::vector<hipEvent_t> ev;   // two per launch
    std::vector<int> cls;
    explicit LaunchTimer(hipStream_t stream) : s(stream) {}
    LaunchTimer(const LaunchTimer &) = delete;
    LaunchTimer &operator=(const LaunchTimer &) = delete;
    ~LaunchTimer() { for (hipEvent_t e : ev) hipEventDestroy(e); }
    int begin(int c)
    {
        for (int i = 0; i < 2; i++) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            ev.push_back(e);
        }
        cls.push_back(c);
        HIP_TRY(hipEventRecord(ev[ev.size() - 2], s));
        return NFAI_OK;
    }
    int end()
    {
        HIP_TRY(hipEventRecord(ev.back(), s));
        return NFAI_OK;
    }
    int collect(float *ms_by_class, uint32_t *launches_by_class)
    {
        HIP_TRY(hipStreamSynchronize(s));
        for (int i = 0; i < KC_N; i++) { ms_by_class[i] = 0.f; launches_by_class[i] = 0; }
        for (size_t i = 0; i < cls.size(); i++) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]));
            ms_by_class[cls[i]] += ms;
            launches_by_class[cls[i]]++;
        }
        return NFAI_OK;
    }
};

// ---- launch scheduler with a one-op look-ahead ------------------------------------------------------
// Every short GEMV pays ~3 us of dispatch + first-byte latency + drain during which HBM idles.  With
// NFAI_LLAMA_PREFETCH, when op i+1 is an fp16 GEMV its "prefetch-only" twin (the same grid touching
// exactly the bytes each wave requests first, default cache policy) is launched on a side stream as
// soon as op i-1 has finished, i.e. concurrently with op i: the requests straddle the i -> i+1
// boundary and op i+1 finds its first two steps in L2 / Infinity Cache.  Pure performance hint: no
// result depends on it (the side stream writes nothing).
struct Op {
    int kind = 2;  // 0 gemv, 1 attention, 2 generic
    int cls = KC_OTHER;
    GemvArgs g;
    AttnArgs a;
    std::function<hipError_t(hipStream_t)> f;
};


struct Model {
    uint32_t magic = 0x4E464D44;  // 'NFMD'
    Ctx *ctx = nullptr;
    nfai_llama_desc d{};
    bool finalized = false;
    bool first_stage = false, last_stage = false;
    bool unfused = false, use_graph = true, kv_f16 = false;
    bool engine = false;             // requested: one engine launch per block where the tensors allow it
    bool attn_ticket = false;        // a bounded wait of the granule hand-off gave up once: this model stays on the ticket form, which never waits
    uint32_t dbg_withhold = 0;       // test hook (nfai_hip_debug_attn_withhold)
    uint64_t *d_gran = nullptr;      // engine hand-off granules: per block h (E) | act (F) | x (E)
    uint32_t *d_epoch = nullptr, *d_engerr = nullptr;
    void *d_engparams = nullptr;     // one parameter block per block's engine launch
    std::vector<EnginePlan> eng_plans;  // built by finalize when engine_ok
    Tensor token_embd, output_norm, output;
    std::vector<Layer> layers;  // index = block - layer_begin
    uint64_t kv_pos_stride = 0, kv_head_stride = 0;
    uint32_t kv_esz = 4;
    // device state
    uint32_t *d_pos = nullptr, *d_tok = nullptr, *d_ring = nullptr;
    float *d_freqs = nullptr, *d_ropecs = nullptr;
    void *d_argmax_part = nullptr;
    void *d_topk = nullptr;          // workspace of the top-k candidate launch (allocated by the first nfai_hip_llama_decode_topk)
    float *d_attn_part = nullptr;
    // workspace of nfai_hip_llama_score (allocated by its first call): per KV position targets | logprob | argmax | logprob_max, then
    // one ScoreState per chunk row and the error word; MFMA path: the fp32 logit slab [pf.T][min(V, 8192)] and, for a quantised head,
    // the fp16 scratch [min(V, 8192)][E] one slab of it is widened into
    void *d_score = nullptr, *d_score_slab = nullptr, *d_score_wide = nullptr;
    // activations
    float *x = nullptr, *h = nullptr, *q = nullptr, *att = nullptr, *act = nullptr, *logits = nullptr;
    // extra activations of the unfused 1:1 chain
    float *xn = nullptr, *qraw = nullptr, *scores = nullptr, *wts = nullptr, *proj = nullptr, *gate = nullptr, *up = nullptr;
    uint32_t *h_pin = nullptr;  // pinned staging for token / pos
    // prefill workspace (allocated when desc.max_batch > 0); T = max_batch rounded up to 128
    struct Prefill {
        uint32_t T = 0, Spad = 0;
        uint32_t *toks = nullptr;
        float *CS = nullptr;       // cos / sin of the chunk's positions [T][D/2][2] (the q | k | v epilogue)
        float *X = nullptr, *H1 = nullptr, *Q = nullptr, *K = nullptr, *V = nullptr, *ATT = nullptr, *G = nullptr, *U = nullptr, *SC = nullptr;
        void *XN = nullptr, *QH = nullptr, *KH = nullptr, *VT = nullptr, *P = nullptr, *ACT = nullptr;  // fp16
        std::shared_ptr<WideShadow> wide = std::make_shared<WideShadow>();
    } pf;
    uint32_t pos_host = 0;
    uint64_t serial = 0;             // never reused: a batch (nfai_hip_llama_batch_create) tells a member from a later model at the same address
    uint32_t weights_gen = 0;        // advanced whenever a tensor slot changes: a batch holds the pointers it was created over
    const float *x_last = nullptr;   // where the last enqueued token left the hidden state (m->x, or m->h on the engine path)
    Graph graph;                     // one token (enqueue_token)
    // the BLOCKING calls (nfai_hip_llama_decode_step / _decode_topk) as one graph each: token word in (from pinned host memory),
    // the token, [the top-k candidate launch,] argmax + error word [+ candidates] out to pinned host memory — the host's share of a
    // sampled token is one hipGraphLaunch and one hipStreamSynchronize
    struct SyncGraph {
        Graph graph;
        float temperature = 0.f;
        uint32_t k = 0;
    } g_step, g_topk;
    bool prefetch = false, s2_used = false;  // side-stream weight prefetch (NFAI_LLAMA_PREFETCH)
    hipStream_t s2 = nullptr;
    std::vector<hipEvent_t> pf_events;
    Graph stage_graph;               // pipeline-stage graph, captured per (hidden_in, hidden_out)
    const void *stage_in = nullptr;
    void *stage_out = nullptr;
    // profiling
    int prof_rep_cls = -1;           // profile_kernel: class whose launches are collected and replayed back to back
    std::vector<struct Op> prof_ops;
    hipEvent_t prof_rep_ev[2] = {nullptr, nullptr};
};

#define MODEL_OR_FAIL(m, h)                                                      \
    Model *m = model_of(h);                                                      \
    if (!m) return fail(NFAI_ERR_INVALID, "%s: invalid model handle", __func__); \
    HIP_TRY(hipSetDevice(m->ctx->device))

#define DALLOC(ptr, bytes)                                                          \
    do {                                                                            \
        int _rc = dalloc(reinterpret_cast<void **>(&(ptr)), (bytes), m->ctx->stream); \
        if (_rc) return _rc;                                                        \
    } while (0)

#define S_TRY(expr)            \
    do {                       \
        int _rc = (expr);      \
        if (_rc) return _rc;   \
    } while (0)

// One launch; `timer` (a LaunchTimer *, null when the step is not profiled) in scope.
#define K_TRY(cls, expr)                                                                                        \
    do {                                                                                                        \
        if (timer) S_TRY(timer->begin(cls));                                                                    \
        hipError_t _e = (expr);                                                                                 \
        if (_e != hipSuccess)                                                                                   \
            return fail(_e == hipErrorInvalidValue ? NFAI_ERR_INVALID : NFAI_ERR_HIP, "%s: %s failed: %s", __func__, #expr, \
                        hipGetErrorString(_e));                                                                 \
        if (timer) S_TRY(timer->end());                                                                         \
    } while (0)

#define NEED_FINAL(m) \
    if (!(m)->finalized) return fail(NFAI_ERR_STATE, "%s: call nfai_hip_llama_finalize first", __func__)

// ---- defined in llama.hip ---------------------------------------------------------------------------
Model *model_of(nfai_model_t h);
int dalloc(void **p, size_t bytes, hipStream_t s);
GemvArgs gemv_base(Model *m, const Tensor &w, const float *x, uint32_t K);
uint64_t tensor_bytes(const Tensor &t);
uint64_t weights_once_bytes(const Model *m, bool quant);
int set_token_async(Model *m, uint32_t tok);
int engine_failed(Model *m, uint32_t code);
int enqueue_token(Model *m, bool with_head, LaunchTimer *timer = nullptr);
int stage_enqueue(Model *m, const void *hidden_in, void *hidden_out);
int step_token_blocking(Model *m, uint32_t token);   // the body of nfai_hip_llama_decode_step: one token, blocking, nothing downloaded

}  // namespace nfai
