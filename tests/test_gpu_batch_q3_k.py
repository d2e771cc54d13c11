"""Batches (nfai_hip_llama_batch_*) and windows (nfai_hip_llama_window_*) on Q3_K_M weights (NFAI_BATCH_QUANT | NFAI_BATCH_QUANT_ANY,
k_bgemv_kq on the Q3_K T16 layout beside Q4_K / Q5_K / Q6_K) on the GPU.  It follows tests/test_gpu_batch_q4_0.py, whose helpers and
bars it uses: 5e-4 * max(1, max|logit|) with an fp32 KV cache.  Here a batch member or a window column is held against the SAME model
state advanced by nfai_hip_llama_decode_step (a twin over the same weights), and the batch that mixes all six quantised types against
the CPU oracle on the dequantised weights.  The reference throws for every quantised type (NFAI.GGUF/Parser.cs:111-114): parity is
unpinned by it, the format is synth.dequantize_q3_k's restatement (tests/test_q3_k.py)."""
import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth
from test_gpu_batch_quant import CAP, check_step, ddict, dispose, make_members, odesc, seq_tokens
from test_gpu_batch_quant_any import quantize as quantize_other
from test_gpu_q3_k import quant_weights, quantize as quantize_q3
from test_gpu_q4_0 import quantize as quantize_q4

pytestmark = pytest.mark.gpu

Q4_0, Q8_0, Q3_K, Q4_K, Q5_K, Q6_K = 2, 8, 11, 12, 13, 14
DIMS = synth.TINY_D128
BAR = 5e-4


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


def any_batch(ms):
    from nfai_amd.llama_model import LlamaBatch
    return LlamaBatch(ms, quantized=True, any_quant=True)


def any_window(m, max_tokens=8):
    from nfai_amd.llama_model import LlamaWindow
    return LlamaWindow(m, max_tokens, quantized=True, any_quant=True)


def stagger(ms, toks, n):
    """Member s (and its twin n + s) takes its first 5 + 7 s tokens alone: unequal positions."""
    for s in range(n):
        for t in toks[s][:5 + 7 * s]:
            ms[s].Step(int(t), want_logits=False)
            ms[n + s].Step(int(t), want_logits=False)


@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_staggered_q3_k_m_batch_matches_every_members_own_decode_step(mgr, n):
    """n members at positions 5, 12, 19, ... then 12 batch steps; a twin of every member takes the same tokens through
    nfai_hip_llama_decode_step: logits within 5e-4 * max(1, max|logit|), every ArgMax equal."""
    wq, _ = quant_weights(DIMS, 61, "q3_k_m")
    ms = make_members(mgr, DIMS, wq, 2 * n, CAP)           # members 0 .. n-1 in the batch, n .. 2n-1 their twins
    toks = [seq_tokens(DIMS, s) for s in range(n)]
    stagger(ms, toks, n)
    batch = any_batch(ms[:n])
    for i in range(12):
        st = [int(toks[s][5 + 7 * s + i]) for s in range(n)]
        lg, am = batch.Step(st)
        for s in range(n):
            want, wam = ms[n + s].Step(st[s])
            err, bar = float(np.abs(lg[s] - want).max()), BAR * max(1.0, float(np.abs(want).max()))
            assert err <= bar, (i, s, err, bar)
            assert int(am[s]) == wam == int(np.argmax(lg[s])), (i, s)
    for s in range(n):
        assert ms[s].Pos == ms[n + s].Pos == 5 + 7 * s + 12
    prof = batch.ProfileStep([int(toks[s][5 + 7 * s + 12]) for s in range(n)])
    assert prof["qkv"][1] == 2 * DIMS.L, prof              # q and k (Q3_K) in one launch, v (Q5_K / Q4_K) in another
    dispose(batch, ms)


def test_q3_k_m_members_are_refused_without_batch_quant_any(mgr):
    from nfai_amd import _lib
    from nfai_amd._lib import NfaiHipError
    from nfai_amd.llama_model import LlamaBatch, LlamaWindow
    wq, _ = quant_weights(DIMS, 61, "q3_k_m")
    ms = make_members(mgr, DIMS, wq, 2, 8)

    def refused(make, pattern):
        with pytest.raises(NfaiHipError, match=pattern) as e:
            make()
        assert e.value.code == _lib.ERR_UNSUPPORTED, e.value.args

    any_batch(ms).Dispose()                                # admitted with both flags
    any_window(ms[0], 4).Dispose()
    refused(lambda: LlamaBatch(ms, quantized=True), r"member 0: token_embd of block 0 has ggml type 11\b")   # (untied: the table is Q3_K)
    refused(lambda: LlamaBatch(ms, quantized=True), r"has ggml type 11; a quantised batch takes Q4_K and Q6_K matrices "
                                                    r"\(Q5_K, Q8_0, Q4_0 and Q3_K weights decode through nfai_hip_llama_decode_step")
    refused(lambda: LlamaWindow(ms[0], 4, quantized=True), r"has ggml type 11; a quantised window takes Q4_K and Q6_K matrices")
    refused(lambda: LlamaBatch(ms), r"has ggml type 11; the batched kernels take fp16")
    dispose(None, ms)


def test_window_steps_match_token_by_token_decode(mgr):
    """5 tokens alone, then windows of T = 1, 2, 5, 8 tokens: every column's logits and ArgMax against a twin that takes the same
    tokens one by one through nfai_hip_llama_decode_step, and the K / V rows the window wrote against the twin's."""
    wq, _ = quant_weights(DIMS, 61, "q3_k_m")
    m, twin = make_members(mgr, DIMS, wq, 2, CAP)
    toks = [int(t) for t in synth.make_tokens(DIMS, 32, seed=131)]
    for t in toks[:5]:
        m.Step(t, want_logits=False)
        twin.Step(t, want_logits=False)
    win = any_window(m)
    cur = 5
    try:
        for T in (1, 2, 5, 8):
            lg, am = win.Step(toks[cur:cur + T])
            assert lg.shape == (T, DIMS.V) and am.shape == (T,)
            for i in range(T):
                want, wam = twin.Step(toks[cur + i])
                err, bar = float(np.abs(lg[i] - want).max()), BAR * max(1.0, float(np.abs(want).max()))
                assert err <= bar, (T, i, err, bar)
                assert int(am[i]) == wam == int(np.argmax(lg[i])), (T, i)
                for l in range(DIMS.L):    # the bar of the batched tests for K / V rows with an fp32 cache
                    np.testing.assert_allclose(m.ReadKV(l, False, cur + i), twin.ReadKV(l, False, cur + i), rtol=0, atol=1e-3)
                    np.testing.assert_allclose(m.ReadKV(l, True, cur + i), twin.ReadKV(l, True, cur + i), rtol=0, atol=1e-3)
            cur += T
            assert m.Pos == twin.Pos == cur
    finally:
        win.Dispose()
        dispose(None, [m, twin])


def test_window_verify_accepts_all_none_and_a_prefix_of_a_draft(mgr):
    """g = the twin's plain greedy continuation.  Drafts g[:k] are all kept (T = 1, 2, 5, 8 columns); a draft wrong at its first token
    keeps none; wrong at column j keeps the prefix g[:j]."""
    wq, _ = quant_weights(DIMS, 61, "q3_k_m")
    m, twin = make_members(mgr, DIMS, wq, 2, CAP)
    prompt = [int(t) for t in synth.make_tokens(DIMS, 9, seed=302)]
    p = len(prompt) - 1
    for t in prompt[:-1]:
        twin.Step(t, want_logits=False)
    g, tok = [], prompt[-1]
    for _ in range(9):
        tok = twin.Step(tok, want_logits=False)[1]
        g.append(tok)
    win = any_window(m)

    def bring():
        m.Reset()
        for t in prompt[:-1]:
            m.Step(t, want_logits=False)

    try:
        for k in (0, 1, 4, 7):                             # every draft right
            bring()
            lg, out = win.Verify(prompt[-1], g[:k], want_logits=True)
            assert [int(t) for t in out] == g[:k + 1], (k, out, g)
            assert lg.shape == (k + 1, DIMS.V) and m.Pos == p + k + 1
        for j in (0, 2, 6):                                # the first error at column j: none (j = 0) or the prefix g[:j] is kept
            bring()
            draft = list(g[:7])
            draft[j] = (draft[j] + 1) % DIMS.V
            _, out = win.Verify(prompt[-1], draft)
            assert [int(t) for t in out] == g[:j + 1], (j, out, g)
            assert m.Pos == p + j + 1
    finally:
        win.Dispose()
        dispose(None, [m, twin])


@pytest.mark.parametrize("n", [2, 5])
def test_step_topk_candidates_are_the_single_models_decode_topk(mgr, n):
    """StepTopK(tokens, 0.5, 40) of a staggered Q3_K_M batch: bit-equal to the device's top-k on every member's own logits
    (tests/test_gpu_batch_sampling.py's rule), and equal to what nfai_hip_llama_decode_topk gives a twin of the member: the same
    candidate ids in the same order wherever the twin's neighbouring candidates are further apart than the logit bar allows the two
    paths to differ, probabilities within exp(2 b / T) - 1 relative (b = 5e-4 * max(1, max|logit|) on every logit, T = 0.5)."""
    from test_gpu_batch_sampling import check_candidates
    wq, _ = quant_weights(DIMS, 61, "q3_k_m")
    ms = make_members(mgr, DIMS, wq, 2 * n, CAP)
    toks = [seq_tokens(DIMS, s) for s in range(n)]
    stagger(ms, toks, n)
    batch = any_batch(ms[:n])
    feed = [int(toks[s][5 + 7 * s]) for s in range(n)]
    for i in range(6):
        ids, probs = batch.StepTopK(feed, 0.5, 40)
        assert ids.shape == (n, 40) and probs.shape == (n, 40)
        own = check_candidates(mgr, ms[:n], DIMS.V, ids, probs, 0.5, 40, f"step {i}")
        for s in range(n):
            ids1, probs1 = ms[n + s].StepTopK(feed[s], 0.5, 40)
            rel = float(np.expm1(2 * BAR * max(1.0, float(np.abs(own[s]).max())) / 0.5))   # numerator e^(b/T), normaliser e^(b/T)
            for c in range(40):
                if ids[s][c] == ids1[c]:
                    assert abs(probs[s][c] - probs1[c]) <= rel * probs1[c], (i, s, c)
                else:   # a swap (or, at the 40th place, a replacement) is allowed only between candidates the bar cannot tell apart
                    at = np.flatnonzero(ids1 == ids[s][c])
                    j = int(at[0]) if at.size else 39
                    assert at.size or c == 39, (i, s, c)
                    assert abs(probs1[j] - probs1[c]) <= rel * max(probs1[j], probs1[c]), (i, s, c)
            feed[s] = int(ids[s][0])
    dispose(batch, ms)


SIX = [Q3_K, Q4_0, Q4_K, Q5_K, Q6_K, Q8_0]
KINDS = ["attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_down"]


def six_type(name):
    """A per-tensor mix of all six quantised types: kind k of block l takes SIX[(k + l) % 6] (ffn_up follows ffn_gate: one launch),
    the table is Q3_K and the head Q6_K.  Every block holds all six types; every q|k|v has three types: three launches."""
    if name == "token_embd.weight":
        return Q3_K
    if name == "output.weight":
        return Q6_K
    _, l, kind, _ = name.split(".")
    return SIX[(KINDS.index("ffn_gate" if kind == "ffn_up" else kind) + int(l)) % 6]


def test_one_batch_mixing_all_six_quantised_types(mgr):
    from nfai_amd.llama_model import QuantTensor
    n = 3
    w = synth.make_weights(DIMS, seed=23, std=0.05)
    wq, wref, seen = {}, {}, set()
    for name, a in w.items():
        if a.ndim == 1:
            wq[name] = wref[name] = a
            continue
        qt = six_type(name)
        seen.add(qt)
        a32 = a.astype(np.float32)
        raw, deq = quantize_q3(a32, Q3_K) if qt == Q3_K else (quantize_q4(a32, Q4_0) if qt == Q4_0 else quantize_other(a32, qt))
        wq[name], wref[name] = QuantTensor(raw, qt, a.shape), deq
    assert seen == set(SIX)
    ms = make_members(mgr, DIMS, wq, n, CAP)
    refs = [orc.OracleLlama(odesc(DIMS, CAP), wref) for _ in range(n)]
    toks = [seq_tokens(DIMS, s) for s in range(n)]
    for s in range(n):
        for t in toks[s][:2 + 3 * s]:
            ms[s].Step(int(t), want_logits=False)
            refs[s].step(int(t))
    batch = any_batch(ms)
    for i in range(8):
        st = [int(toks[s][2 + 3 * s + i]) for s in range(n)]
        lg, am = batch.Step(st)
        check_step(lg, am, [refs[s].step(st[s]) for s in range(n)], BAR, f"step {i}")
    prof = batch.ProfileStep([int(toks[s][2 + 3 * s + 8]) for s in range(n)])
    assert prof["qkv"][1] == 3 * DIMS.L, prof
    assert prof["wo"][1] == prof["gateup"][1] == prof["down"][1] == DIMS.L and prof["lmhead"][1] == 1, prof
    dispose(batch, ms)
