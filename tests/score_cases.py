"""Scoring a token sequence (nfai_hip_score_rows, nfai_hip_llama_score): the fp64 reference, the model cases and their bars, shared by
tests/test_score.py (CPU), tests/test_gpu_score_rows.py and tests/test_gpu_score.py.

A case is a model (dimensions, weight encoding, KV type), a path (max_batch 0 = the M = 1 path, otherwise the MFMA path in chunks of
max_batch rows), a lead-in of `lead` Step calls and n scored tokens.  ONE oracle walk per (model, token seed) over LEAD_MAX + N_MAX
tokens serves every case of that model: a case scores rows lead .. lead + n - 1 of it.

Bars.  Logits: 5e-4 * max(1, max|logit|) on the M = 1 path with an fp32 cache, 2e-2 * max(1, max|logit|) on the MFMA path or with an
fp16 cache (the project's bars).  A log-probability is a logit minus a convex mean of logits: twice the logit bar.  tests/test_score.py
re-measures, on every run, what the MFMA head alone costs (normalised row rounded to fp16 x fp16 weights, fp32 accumulation) and holds it
under half of that.

Pinned rows: the oracle's top-2 logit gap exceeds two logit bars of the case; only there must the ArgMax equal the oracle's.  At least
PIN_TIGHT of the rows of every case at the 5e-4 bar and PIN_LOOSE of every case at the 2e-2 bar must be pinned (asserted on the oracle
alone, tests/test_score.py); a case that falls short starts from a later token seed (RESEED), never from other weights or bars.
"""
import functools
from dataclasses import dataclass

import numpy as np

from nfai_amd import synth

NO_TARGET = 0xFFFFFFFF
N_MAX, LEAD_MAX = 48, 5
TIGHT, LOOSE = 5e-4, 2e-2
PIN_TIGHT, PIN_LOOSE = 0.90, 0.50
REAL_VOCAB = synth.LlamaDims("score-v128256", 256, 1, 4, 2, 64, 512, 128256, True)   # 15.7 slabs of 8192 columns
ENCODINGS = ("f16", "q4_k_m", "q5_k_m", "all_q8_0", "q4_0")


def score_rows_ref(logits, targets):
    """fp64: (logprob[T], argmax[T], logprob_max[T]) of logits [T][V]; targets[r] == NO_TARGET gives logprob 0.  The ArgMax is the
    first index of the maximum (SamplingUtils.cs:55-56), the log-probabilities the log of SamplingUtils.Softmax (:35-41)."""
    lg = np.asarray(logits, np.float64)
    lg = lg.reshape(-1, lg.shape[-1])
    m = lg.max(axis=1)
    lse = m + np.log(np.exp(lg - m[:, None]).sum(axis=1))
    am = np.argmax(lg, axis=1).astype(np.uint32)
    t = np.asarray(targets, np.int64).reshape(-1)
    has = t != NO_TARGET
    lp = np.zeros(lg.shape[0])
    lp[has] = lg[np.nonzero(has)[0], t[has]] - lse[has]
    return lp, am, m - lse


# ---- models ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights(dims, enc):
    """(what the model loads, what the oracle computes on): the default synth weights, quantised by the helpers of the encoding's tests."""
    if enc == "f16":
        w = synth.make_weights(dims)
        return w, w
    if enc == "q4_k_m":
        from test_gpu_batch_quant import quant_weights
        return quant_weights(synth.make_weights(dims))[:2]
    if enc == "q4_0":
        from test_gpu_q4_0 import quant_weights
        return quant_weights(dims, 1234, "q4_0", std=0.02)[:2]
    from test_gpu_batch_quant_any import quant_weights
    return quant_weights(dims, enc, seed=1234, std=0.02)[:2]


def ddict(d):
    return dict(E=d.E, L=d.L, H=d.H, Hkv=d.Hkv, D=d.D, F=d.F, V=d.V, eps=1e-5, rope_dims=d.D, rope_base=500000.0)


@dataclass(frozen=True)
class Case:
    dims: synth.LlamaDims
    enc: str
    kv_f16: bool
    max_batch: int
    n: int
    lead: int = 0
    explicit: bool = False      # targets given (ArgMax rows, NO_TARGET rows, random rows) instead of NULL

    @property
    def id(self):
        return (f"{self.dims.name}-{self.enc}-{'kv16' if self.kv_f16 else 'kv32'}-mb{self.max_batch}-n{self.n}-at{self.lead}"
                + ("-targets" if self.explicit else ""))

    @property
    def scale(self):
        return LOOSE if (self.max_batch > 0 or self.kv_f16) else TIGHT

    @property
    def pin_share(self):
        return PIN_LOOSE if self.scale == LOOSE else PIN_TIGHT


def _cases():
    out = []
    for dims in (synth.TINY, synth.TINY_D128):
        for enc in ENCODINGS:
            out.append(Case(dims, enc, False, 0, N_MAX))            # M = 1
            out.append(Case(dims, enc, False, 128, N_MAX))          # one MFMA chunk
    for dims, enc in ((synth.TINY, "f16"), (synth.TINY_D128, "q4_k_m")):   # chunk edges of max_batch 16, from position 0 and behind a lead-in
        for n in (1, 15, 16, 17, 35):
            for lead in (0, LEAD_MAX):
                out.append(Case(dims, enc, False, 16, n, lead))
    for enc in ("f16", "q4_0"):                                      # fp16 KV cache
        out.append(Case(synth.TINY_D128, enc, True, 0, N_MAX))
        out.append(Case(synth.TINY_D128, enc, True, 128, N_MAX))
    out.append(Case(synth.TINY, "f16", False, 16, 35, 0, True))
    out.append(Case(synth.TINY_D128, "q5_k_m", False, 0, 17, LEAD_MAX, True))
    out.append(Case(REAL_VOCAB, "f16", False, 16, 20))              # the model path across slab boundaries (two chunks)
    return out


CASES = _cases()
# (dims name, enc): the token seed its walk starts from where seed 99 leaves a case short of its pinned share (found by
# tests/test_score.py::test_pinned_share, which names the case that falls short)
RESEED = {
    ("tiny-llama", "f16"): 100,            # seed 99 (and 7): a short case of max_batch 16 falls under half at the prefill bar
    ("tiny-llama-d128", "q4_k_m"): 107,    # seed 99: 42 % of the 48 rows pinned at the prefill bar
}


def token_seed(dims, enc):
    return RESEED.get((dims.name, enc), 99)


@dataclass
class Walk:
    toks: np.ndarray            # LEAD_MAX + N_MAX tokens
    logits: np.ndarray          # [len][V] fp32: the oracle's
    hidden: np.ndarray          # [len][E]: the hidden state in front of the output norm
    K: list
    V: list


@functools.lru_cache(maxsize=None)
def walk(dims, enc):
    import oracle as orc
    n = LEAD_MAX + (N_MAX if dims is not REAL_VOCAB else 20)
    toks = synth.make_tokens(dims, n, seed=token_seed(dims, enc))
    ref = orc.OracleLlama(orc.LlamaDesc(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, C=n), weights(dims, enc)[1])
    logits, hidden = [], []
    for t in toks:
        logits.append(np.array(ref.step(int(t)), np.float32))
        hidden.append(np.array(ref.hidden(), np.float32))
    K = [np.array(ref.kcache(l)[:n], np.float32) for l in range(dims.L)]
    V = [np.array(ref.vcache(l)[:n], np.float32) for l in range(dims.L)]
    ref.close()
    return Walk(np.asarray(toks, np.uint32), np.stack(logits), np.stack(hidden), K, V)


def case_rows(c):
    """(lead-in tokens, scored tokens, targets as the entry point is given them (None = NULL), targets as scored [n], oracle logits [n][V])."""
    w = walk(c.dims, c.enc)
    lead, toks, lg = w.toks[:c.lead], w.toks[c.lead:c.lead + c.n], w.logits[c.lead:c.lead + c.n]
    if not c.explicit:
        scored = np.append(toks[1:], np.uint32(NO_TARGET)).astype(np.uint32)
        return lead, toks, None, scored, lg
    r = np.random.Generator(np.random.PCG64(c.n + c.lead))
    tg = r.integers(0, c.dims.V, c.n).astype(np.uint32)
    tg[::3] = np.argmax(lg[::3], axis=1)      # the target is the ArgMax
    tg[1::5] = NO_TARGET
    return lead, toks, tg, tg, lg


def logit_bars(c, lg):
    """[n]: the case's logit bar on every row."""
    return c.scale * np.maximum(1.0, np.abs(lg).max(axis=1))


def pinned(c, lg):
    """[n] bool: the oracle's top-2 gap exceeds two logit bars."""
    top = np.partition(lg.astype(np.float64), -2, axis=1)[:, -2:]
    return (top[:, 1] - top[:, 0]) > 2 * logit_bars(c, lg)


def head_restated(dims, enc):
    """(fp64 log-probabilities at the next token and of the maximum, the same of the MFMA head restated: output norm in fp32, row
    rounded to fp16, weights rounded to fp16, fp32 accumulation, fp64 softmax; the fp64 logits) on the walk's hidden rows."""
    w = walk(dims, enc)
    wref = weights(dims, enc)[1]
    head = np.asarray(wref.get("output.weight", wref["token_embd.weight"]))
    g = np.asarray(wref["output_norm.weight"])
    h64 = w.hidden.astype(np.float64)
    xn64 = h64 / np.sqrt(np.mean(h64 * h64, axis=1, keepdims=True) + 1e-5) * g.astype(np.float64)
    l64 = xn64 @ head.astype(np.float64).T
    h32 = w.hidden.astype(np.float32)
    xn32 = (h32 / np.sqrt(np.mean(h32 * h32, axis=1, keepdims=True, dtype=np.float32) + np.float32(1e-5)) * g.astype(np.float32)).astype(np.float32)
    l32 = xn32.astype(np.float16).astype(np.float32) @ head.astype(np.float16).astype(np.float32).T
    tg = np.append(w.toks[1:], np.uint32(NO_TARGET))
    return score_rows_ref(l64, tg), score_rows_ref(l32, tg), l64
