"""Batches (nfai_hip_llama_batch_*) and windows (nfai_hip_llama_window_*) on IQ4_XS weights (NFAI_BATCH_QUANT | NFAI_BATCH_QUANT_ANY,
k_bgemv_kq on the IQ4_XS T16 layout beside Q5_K / Q6_K) on the GPU.  It follows tests/test_gpu_batch_q3_k.py, whose helpers and bars
it uses: 5e-4 * max(1, max|logit|) with an fp32 KV cache.  A batch member or a window column is held against the SAME model state
advanced by nfai_hip_llama_decode_step (a twin over the same weights) and against the CPU oracle on the dequantised weights; the
batch that mixes all seven quantised types against the oracle.  The reference throws for every quantised type
(NFAI.GGUF/Parser.cs:111-114): parity is unpinned by it, the format is synth.dequantize_iq4_xs's restatement (tests/test_iq4_xs.py)."""
import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth
from test_gpu_batch_quant import CAP, check_step, dispose, make_members, odesc, seq_tokens
from test_gpu_batch_quant_any import quantize as quantize_other
from test_gpu_batch_q3_k import any_batch, any_window, stagger
from test_gpu_iq4_xs import GQA4, quant_weights, quantize as quantize_iq4
from test_gpu_q3_k import quantize as quantize_q3

pytestmark = pytest.mark.gpu

Q4_0, Q8_0, Q3_K, Q4_K, Q5_K, Q6_K, IQ4_XS = 2, 8, 11, 12, 13, 14, 23
DIMS = synth.TINY_D128
BAR = 5e-4


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


@pytest.mark.parametrize("dims,mix", [(DIMS, "all_iq4_xs"), (GQA4, "iq4_xs")], ids=["d128-all", "gqa4-mix"])
@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_staggered_iq4_xs_batch_matches_every_members_own_decode_step_and_the_oracle(mgr, n, dims, mix):
    """n members at positions 5, 12, 19, ... then 12 batch steps; a twin of every member takes the same tokens through
    nfai_hip_llama_decode_step, and member 0 and the last member also walk the oracle: logits within 5e-4 * max(1, max|logit|) of
    both, every ArgMax equal.  all_iq4_xs: the IQ4_XS table and head in the batch; GQA4 in the iq4_xs mix: a Q5_K v beside IQ4_XS
    q and k (two q|k|v launches per block), a Q5_K ffn_down in block 0, the Q6_K head."""
    wq, wref = quant_weights(dims, 61, mix)
    ms = make_members(mgr, dims, wq, 2 * n, CAP)           # members 0 .. n-1 in the batch, n .. 2n-1 their twins
    toks = [seq_tokens(dims, s) for s in range(n)]
    stagger(ms, toks, n)
    walked = sorted({0, n - 1})
    refs = {s: orc.OracleLlama(odesc(dims, CAP), wref) for s in walked}
    for s in walked:
        for t in toks[s][:5 + 7 * s]:
            refs[s].step(int(t))
    batch = any_batch(ms[:n])
    for i in range(12):
        st = [int(toks[s][5 + 7 * s + i]) for s in range(n)]
        lg, am = batch.Step(st)
        for s in range(n):
            want, wam = ms[n + s].Step(st[s])
            err, bar = float(np.abs(lg[s] - want).max()), BAR * max(1.0, float(np.abs(want).max()))
            assert err <= bar, (i, s, err, bar)
            assert int(am[s]) == wam == int(np.argmax(lg[s])), (i, s)
        check_step([lg[s] for s in walked], [am[s] for s in walked], [refs[s].step(st[s]) for s in walked], BAR, f"step {i}")
    for s in range(n):
        assert ms[s].Pos == ms[n + s].Pos == 5 + 7 * s + 12
    prof = batch.ProfileStep([int(toks[s][5 + 7 * s + 12]) for s in range(n)])
    assert prof["qkv"][1] == (2 if dims is GQA4 else 1) * dims.L, prof
    dispose(batch, ms)


@pytest.mark.parametrize("n", [2, 5])
def test_batch_greedy_on_the_device(mgr, n):
    wq, _ = quant_weights(DIMS, 61, "all_iq4_xs")
    ms = make_members(mgr, DIMS, wq, n, CAP)
    toks = [seq_tokens(DIMS, s) for s in range(n)]
    batch = any_batch(ms)

    def prime():
        for s in range(n):
            ms[s].Reset()
            for t in toks[s][:3 + 4 * s]:
                ms[s].Step(int(t), want_logits=False)

    prime()
    first = [int(toks[s][3 + 4 * s]) for s in range(n)]
    got = batch.Greedy(first, 16)
    assert [m.Pos for m in ms] == [3 + 4 * s + 16 for s in range(n)]
    prime()
    cur, host = list(first), []
    for _ in range(16):
        _, am = batch.Step(cur, want_logits=False)
        cur = [int(a) for a in am]
        host.append(cur)
    assert got.tolist() == host
    dispose(batch, ms)


def test_iq4_xs_members_are_refused_without_batch_quant_any(mgr):
    from nfai_amd import _lib
    from nfai_amd._lib import NfaiHipError
    from nfai_amd.llama_model import LlamaBatch, LlamaWindow
    wq, _ = quant_weights(DIMS, 61, "iq4_xs")
    ms = make_members(mgr, DIMS, wq, 2, 8)

    def refused(make, pattern):
        with pytest.raises(NfaiHipError, match=pattern) as e:
            make()
        assert e.value.code == _lib.ERR_UNSUPPORTED, e.value.args

    any_batch(ms).Dispose()                                # admitted with both flags
    any_window(ms[0], 4).Dispose()
    refused(lambda: LlamaBatch(ms, quantized=True), r"member 0: token_embd of block 0 has ggml type 23\b")   # (untied: the table is IQ4_XS)
    refused(lambda: LlamaBatch(ms, quantized=True), r"has ggml type 23; a quantised batch takes Q4_K and Q6_K matrices "
                                                    r"\(Q5_K, Q8_0, Q4_0 and Q3_K weights decode through nfai_hip_llama_decode_step")   # (the existing message; the type is named by its id)
    refused(lambda: LlamaWindow(ms[0], 4, quantized=True), r"has ggml type 23; a quantised window takes Q4_K and Q6_K matrices")
    refused(lambda: LlamaBatch(ms), r"has ggml type 23; the batched kernels take fp16")
    dispose(None, ms)


@pytest.mark.parametrize("dims,mix", [(DIMS, "all_iq4_xs"), (GQA4, "iq4_xs")], ids=["d128-all", "gqa4-mix"])
def test_window_steps_match_token_by_token_decode(mgr, dims, mix):
    """5 tokens alone, then windows of T = 1, 2, 5, 8 tokens: every column's logits and ArgMax against a twin that takes the same
    tokens one by one through nfai_hip_llama_decode_step, and the K / V rows the window wrote against the twin's."""
    wq, _ = quant_weights(dims, 61, mix)
    m, twin = make_members(mgr, dims, wq, 2, CAP)
    toks = [int(t) for t in synth.make_tokens(dims, 32, seed=131)]
    for t in toks[:5]:
        m.Step(t, want_logits=False)
        twin.Step(t, want_logits=False)
    win = any_window(m)
    cur = 5
    try:
        for T in (1, 2, 5, 8):
            lg, am = win.Step(toks[cur:cur + T])
            assert lg.shape == (T, dims.V) and am.shape == (T,)
            for i in range(T):
                want, wam = twin.Step(toks[cur + i])
                err, bar = float(np.abs(lg[i] - want).max()), BAR * max(1.0, float(np.abs(want).max()))
                assert err <= bar, (T, i, err, bar)
                assert int(am[i]) == wam == int(np.argmax(lg[i])), (T, i)
                for l in (0, dims.L - 1):    # the bar of the batched tests for K / V rows with an fp32 cache
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
    wq, _ = quant_weights(DIMS, 61, "all_iq4_xs")
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
    """StepTopK(tokens, 0.5, 40) of a staggered IQ4_XS batch: bit-equal to the device's top-k on every member's own logits
    (tests/test_gpu_batch_sampling.py's rule), and equal to what nfai_hip_llama_decode_topk gives a twin of the member: the same
    candidate ids in the same order wherever the twin's neighbouring candidates are further apart than the logit bar allows the two
    paths to differ, probabilities within exp(2 b / T) - 1 relative (b = 5e-4 * max(1, max|logit|) on every logit, T = 0.5)."""
    from test_gpu_batch_sampling import check_candidates
    wq, _ = quant_weights(DIMS, 61, "all_iq4_xs")
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


SEVEN = [IQ4_XS, Q3_K, Q4_0, Q4_K, Q5_K, Q6_K, Q8_0]
KINDS = ["attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_down"]
SEVEN_DIMS = synth.LlamaDims("seven-types", 256, 7, 4, 2, 64, 512, 512, False)


def seven_type(name):
    """A per-tensor mix of all seven quantised types: kind k of block l takes SEVEN[(k + l) % 7] (ffn_up follows ffn_gate: one
    launch), the table is IQ4_XS and the head Q6_K.  Over seven blocks every kind meets every type; every q|k|v has three types:
    three launches."""
    if name == "token_embd.weight":
        return IQ4_XS
    if name == "output.weight":
        return Q6_K
    _, l, kind, _ = name.split(".")
    return SEVEN[(KINDS.index("ffn_gate" if kind == "ffn_up" else kind) + int(l)) % 7]


def quantize_any(a32, qt):
    if qt == IQ4_XS or qt == Q4_0:
        return quantize_iq4(a32, qt)
    if qt == Q3_K:
        return quantize_q3(a32, Q3_K)
    return quantize_other(a32, qt)


def test_one_batch_mixing_all_seven_quantised_types(mgr):
    from nfai_amd.llama_model import QuantTensor
    n, dims = 3, SEVEN_DIMS
    w = synth.make_weights(dims, seed=23, std=0.05)
    wq, wref, seen = {}, {}, {}
    for name, a in w.items():
        if a.ndim == 1:
            wq[name] = wref[name] = a
            continue
        qt = seven_type(name)
        if name.startswith("blk."):
            seen.setdefault(name.split(".")[2], set()).add(qt)
        raw, deq = quantize_any(a.astype(np.float32), qt)
        wq[name], wref[name] = QuantTensor(raw, qt, a.shape), deq
    assert all(seen[k] == set(SEVEN) for k in KINDS), seen
    ms = make_members(mgr, dims, wq, n, CAP)
    refs = [orc.OracleLlama(odesc(dims, CAP), wref) for _ in range(n)]
    toks = [seq_tokens(dims, s) for s in range(n)]
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
    assert prof["qkv"][1] == 3 * dims.L, prof
    assert prof["wo"][1] == prof["gateup"][1] == prof["down"][1] == dims.L and prof["lmhead"][1] == 1, prof
    win = any_window(ms[0], 4)                             # the same mix is admitted as a window: three columns against the oracle
    ms[0].Reset()
    ref = orc.OracleLlama(odesc(dims, CAP), wref)
    lg, am = win.Step([int(t) for t in toks[0][:3]])
    check_step(lg, am, [ref.step(int(t)) for t in toks[0][:3]], BAR, "window")
    win.Dispose()
    dispose(batch, ms)
