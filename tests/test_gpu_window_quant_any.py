"""The window (nfai_hip_llama_window_*) on Q5_K / Q8_0 weights (NFAI_BATCH_QUANT | NFAI_BATCH_QUANT_ANY) on the GPU: up to 8
consecutive positions of one model per pass over the weights against the CPU oracle on the DEQUANTISED weights fed the same tokens one
by one, the bit-exact invariants of a window, Verify, and RunAsync(greedy=True, speculative=k) on such models.  The mirror of
tests/test_gpu_window_decode.py on the mixes "q5_k_m" and "all_q8_0" of tests/test_gpu_batch_quant_any.py.

Tolerances are the project's: 5e-4 * max(1, max|logit|) with an fp32 KV cache, 2e-2 with an fp16 one; K / V rows 1e-3 / 2e-2 absolute.

Verify is checked against the model's OWN greedy continuation, taken on a twin (a model sharing the tensors) by Verify with no draft:
a window's column does not depend on the columns beside it by a bit, so the kept tokens are exactly the twin's, with no near-tie
rule.  RunAsync compares the window path with the batch-1 path, which are different kernels: there the oracle's greedy continuation
of the prompt (token 7, weights of seed 21, tiny-llama, fp32 KV) must have its two largest logits more than twice the tolerance
apart at every recorded step (asserted from the oracle alone), so both paths must emit the oracle's tokens."""
import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth
from test_gpu_batch_quant_any import quant_weights
from test_gpu_window_decode import CAP, N_REC, Recording, _IdTokenizer, check_column, ddict, odesc

pytestmark = pytest.mark.gpu

MIXES = ["q5_k_m", "all_q8_0"]
CONFIGS = [pytest.param(d, x, k, id=f"{d.name}-{x}-{'kv16' if k else 'kv32'}")
           for d in (synth.TINY, synth.TINY_D128) for x in MIXES for k in (False, True)]


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


def make_model(mgr, dims, mix, cap=CAP, **kw):
    from nfai_amd.llama_model import LlamaModel
    return LlamaModel(mgr, synth.make_metadata(dims), quant_weights(dims, mix)[0], cap, dims=ddict(dims), **kw)


def any_window(m, max_tokens=8):
    from nfai_amd.llama_model import LlamaWindow
    return LlamaWindow(m, max_tokens, quantized=True, any_quant=True)


# ---- 1: Step against the oracle --------------------------------------------------------------------------------------------------------
STEP_TOKENS = 5 + 36   # 5 alone, then windows of 1 .. 8
_ORACLE = {}


def oracle_steps(dims, mix):
    """The oracle fed the test's tokens one by one, once per (shape, mix): every step's logits, and the K / V caches at the end."""
    key = (dims.name, mix)
    if key not in _ORACLE:
        ref = orc.OracleLlama(odesc(dims, CAP), quant_weights(dims, mix)[1])
        toks = [int(t) for t in synth.make_tokens(dims, 64, seed=131)]
        lg = [ref.step(t).copy() for t in toks[:STEP_TOKENS]]
        _ORACLE[key] = (toks, lg, [ref.kcache(l)[:STEP_TOKENS].copy() for l in range(dims.L)], [ref.vcache(l)[:STEP_TOKENS].copy() for l in range(dims.L)])
    return _ORACLE[key]


@pytest.mark.parametrize("dims,mix,kv_f16", CONFIGS)
def test_window_steps_match_the_oracle(mgr, dims, mix, kv_f16):
    """5 tokens through _decode_step, then windows of t = 1 .. 8 tokens: every column's logits, ArgMax, the position and the K / V
    rows of every window position against the oracle fed the same tokens one by one."""
    toks, want, kc, vc = oracle_steps(dims, mix)
    m = make_model(mgr, dims, mix, kv_f16=kv_f16)
    scale = 2e-2 if kv_f16 else 5e-4
    atol = 2e-2 if kv_f16 else 1e-3
    for t in toks[:5]:
        m.Step(t, want_logits=False)
    cur = 5
    win = any_window(m)
    try:
        for t in range(1, 9):
            tk = toks[cur:cur + t]
            lg, am = win.Step(tk)
            assert lg.shape == (t, dims.V) and am.shape == (t,)
            for i in range(t):
                check_column(lg[i], am[i], want[cur + i], scale, f"t={t} pos {cur + i} column {i}")
            for l in range(dims.L):
                for i in range(t):
                    np.testing.assert_allclose(m.ReadKV(l, False, cur + i), kc[l][cur + i], rtol=0, atol=atol)
                    np.testing.assert_allclose(m.ReadKV(l, True, cur + i), vc[l][cur + i], rtol=0, atol=atol)
            cur += t
            assert m.Pos == cur
        assert cur == STEP_TOKENS
        assert win.BytesPerStep(4) > win.BytesPerStep(2) > 0
    finally:
        win.Dispose()
        m.Dispose()


# ---- 2: bit-exact invariants -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,mix,kv_f16", CONFIGS)
def test_a_column_depends_neither_on_the_window_size_nor_on_later_columns(mgr, dims, mix, kv_f16):
    """Column i's logits are BIT-IDENTICAL for every T > i, and when the tokens of the columns behind it are replaced."""
    m = make_model(mgr, dims, mix, kv_f16=kv_f16)
    toks = [int(t) for t in synth.make_tokens(dims, 64, seed=133)]
    win = any_window(m)
    depth = 37   # two prefix slices and the window's own

    def bring():
        m.Reset()
        for t in toks[:depth]:
            m.Step(t, want_logits=False)

    try:
        bring()
        cols = toks[depth:depth + 8]
        lg8, am8 = win.Step(cols)
        for i in range(8):
            bring()
            lg, am = win.Step(cols[:i + 1])
            np.testing.assert_array_equal(lg, lg8[:i + 1])
            np.testing.assert_array_equal(am, am8[:i + 1])
        for i in range(7):
            other = cols[:i + 1] + [(t + 1 + j) % dims.V for j, t in enumerate(cols[i + 1:])]
            bring()
            lg, am = win.Step(other)
            np.testing.assert_array_equal(lg[:i + 1], lg8[:i + 1])
            assert not np.array_equal(lg[i + 1], lg8[i + 1])   # (the replaced column did change)
    finally:
        win.Dispose()
        m.Dispose()


@pytest.mark.parametrize("dims,mix,kv_f16", CONFIGS)
def test_rows_of_rejected_drafts_are_never_read(mgr, dims, mix, kv_f16):
    """A model whose Verify rejected drafts and went on decoding, against a twin that was fed only the accepted tokens through
    windows at the same base positions: BIT-IDENTICAL logits at every later step."""
    a = make_model(mgr, dims, mix, kv_f16=kv_f16)
    b = make_model(mgr, dims, mix, kv_f16=kv_f16, share_from=a)
    wa, wb = any_window(a), any_window(b)
    toks = [int(t) for t in synth.make_tokens(dims, 64, seed=135)]
    depth = 33
    try:
        for mdl in (a, b):
            for t in toks[:depth]:
                mdl.Step(t, want_logits=False)
        _, g = wb.Verify(toks[depth], [])            # the model's own two next tokens (from the twin, then put back)
        g0 = int(g[0])
        _, g = wb.Verify(g0, [])
        g1 = int(g[0])
        b.SetPos(depth)
        wrong = [(g1 + 1) % dims.V, (g1 + 2) % dims.V, (g1 + 3) % dims.V, 5, 6, 7]
        lga, out = wa.Verify(toks[depth], [g0] + wrong, want_logits=True)   # draft 0 right, draft 1 wrong: rows depth + 2 .. + 7 are stale
        assert [int(t) for t in out] == [g0, g1]
        lgb, amb = wb.Step([toks[depth], g0])        # the twin: the accepted tokens only, same base position
        assert int(amb[1]) == g1 and a.Pos == b.Pos == depth + 2
        np.testing.assert_array_equal(lga[:2], lgb)
        assert not np.array_equal(a.ReadKV(0, False, depth + 3), b.ReadKV(0, False, depth + 3))   # (the rejected rows ARE there)
        nxt = g1
        for k in (0, 0, 2, 0, 1):                    # single columns first: the stale rows stay above the position
            draft = [(nxt + 3 + j) % dims.V for j in range(k)]
            la, oa = wa.Verify(nxt, draft, want_logits=True)
            lb, ob = wb.Verify(nxt, draft, want_logits=True)
            np.testing.assert_array_equal(la, lb)
            np.testing.assert_array_equal(oa, ob)
            assert a.Pos == b.Pos
            nxt = int(oa[-1])
        la, _ = a.Step(nxt)
        lb, _ = b.Step(nxt)
        np.testing.assert_array_equal(la, lb)
    finally:
        wa.Dispose()
        wb.Dispose()
        b.Dispose()
        a.Dispose()


# ---- 3: Verify -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,mix,kv_f16", CONFIGS)
def test_verify_keeps_right_drafts_and_stops_at_the_first_wrong_one(mgr, dims, mix, kv_f16):
    """The twin's Verify with k = 0, repeated, is the model's greedy continuation g.  Drafts g[:k] are all kept (k + 1 tokens, g[:k + 1]);
    with draft j spoiled, j + 1 tokens come out: the kept drafts and the model's own token in place of the wrong one."""
    a = make_model(mgr, dims, mix, kv_f16=kv_f16)
    b = make_model(mgr, dims, mix, kv_f16=kv_f16, share_from=a)
    wa, wb = any_window(a), any_window(b)
    prompt = [int(t) for t in synth.make_tokens(dims, 9, seed=302)]
    p = len(prompt) - 1

    def bring(m):
        m.Reset()
        for t in prompt[:-1]:
            m.Step(t, want_logits=False)

    try:
        bring(b)
        g, tok = [], prompt[-1]
        for _ in range(9):
            _, out = wb.Verify(tok, [])
            assert len(out) == 1
            tok = int(out[0])
            g.append(tok)
        for k in range(8):                            # every draft right
            bring(a)
            lg, out = wa.Verify(prompt[-1], g[:k], want_logits=True)
            assert [int(t) for t in out] == g[:k + 1], (k, out, g)
            assert lg.shape == (k + 1, dims.V) and [int(np.argmax(r)) for r in lg] == g[:k + 1]
            assert a.Pos == p + k + 1
            a.Enqueue(1)                              # the token word: a greedy step on the device continues from the last kept token
            nxt = a.FetchTokens(1)
            assert len(nxt) == 1 and a.Pos == p + k + 2
        for j in range(7):                            # the first error at column j, for every j
            bring(a)
            draft = list(g[:7])
            draft[j] = (draft[j] + 1) % dims.V
            _, out = wa.Verify(prompt[-1], draft)
            assert [int(t) for t in out] == g[:j + 1], (j, out, g)
            assert a.Pos == p + j + 1
    finally:
        wa.Dispose()
        wb.Dispose()
        b.Dispose()
        a.Dispose()


@pytest.mark.parametrize("mix", MIXES)
def test_speculative_run_async_equals_the_plain_greedy_generation(mgr, mix):
    """24 tokens through RunAsync(greedy=True, speculative=3) on a Q5_K_M and on a Q8_0 model, with no new argument: the model
    recorded what it was given and opens the window with both flags.  The drafter is sometimes right (it knows the oracle's recording
    and spoils every third proposal at its second token, every fifth at its first).  The text is that of speculative=0."""
    dims = synth.TINY
    wref = quant_weights(dims, mix)[1]
    prompt = [7]
    rec = Recording(dims, wref, prompt, 5e-4)
    print(f"recording {rec.tokens[:N_REC]}")
    assert all(rec.ok[:N_REC]), rec.ok   # from the oracle alone: no step of the continuation is a near tie
    m = make_model(mgr, dims, mix)
    assert m._any_quant and m._quantized
    m.tokenizer = _IdTokenizer()
    m.promptPrefill = False
    calls = []

    class Drafter:
        def Propose(self, history, k):
            done = len(history) - len(prompt)
            d = list(rec.tokens[done:done + k])
            calls.append(len(d))
            if len(calls) % 3 == 0 and len(d) > 1:
                d[1] = (d[1] + 1) % dims.V
            if len(calls) % 5 == 0 and d:
                d[0] = (d[0] + 1) % dims.V
            return d

    try:
        plain = [int(t) for t in "".join(m.RunAsync("7", greedy=True, max_tokens=N_REC)).split()]
        assert plain == rec.tokens[:N_REC]
        pos_plain = m.Pos
        m.Reset()
        spec = [int(t) for t in "".join(m.RunAsync("7", greedy=True, max_tokens=N_REC, speculative=3, drafter=Drafter())).split()]
        assert spec == plain
        assert len(calls) < N_REC          # some drafts were kept: fewer passes than tokens
        assert m.Pos == pos_plain          # every emitted token but the last was fed, as in the plain loop
    finally:
        m.Dispose()


# ---- 4: bounds and refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", MIXES)
def test_a_window_past_the_capacity_is_kv_full_and_moves_nothing(mgr, mix):
    from nfai_amd import _lib
    dims, cap = synth.TINY_D128, 16
    m = make_model(mgr, dims, mix, cap=cap)
    win = any_window(m)
    toks = [int(t) for t in synth.make_tokens(dims, 32, seed=137)]
    try:
        for t in toks[:12]:
            m.Step(t, want_logits=False)
        before = [(m.ReadKV(l, False, p), m.ReadKV(l, True, p)) for l in range(dims.L) for p in range(cap)]
        with pytest.raises(_lib.KVCacheFull, match="capacity 16"):
            win.Step(toks[12:17])                                   # 12 + 5 > 16
        with pytest.raises(_lib.KVCacheFull):
            win.Verify(toks[12], toks[13:17])
        assert m.Pos == 12
        after = [(m.ReadKV(l, False, p), m.ReadKV(l, True, p)) for l in range(dims.L) for p in range(cap)]
        for (k0, v0), (k1, v1) in zip(before, after):
            np.testing.assert_array_equal(k0, k1)
            np.testing.assert_array_equal(v0, v1)
        lg, am = win.Step(toks[12:16])                               # 12 + 4 == 16 fits
        assert m.Pos == 16 and np.isfinite(lg).all()
        with pytest.raises(_lib.KVCacheFull):
            win.Verify(toks[16], [])
    finally:
        win.Dispose()
        m.Dispose()


@pytest.mark.parametrize("mix,ggml", [("q5_k_m", 13), ("all_q8_0", 8)])
def test_without_the_new_flag_creation_is_refused_as_before(mgr, mix, ggml):
    from nfai_amd import _lib
    from nfai_amd.llama_model import LlamaWindow
    m = make_model(mgr, synth.TINY, mix)
    try:
        with pytest.raises(_lib.NfaiHipError, match=rf"has ggml type {ggml}; a quantised window takes Q4_K and Q6_K matrices") as e:
            LlamaWindow(m, 4, quantized=True)
        assert e.value.code == _lib.ERR_UNSUPPORTED
        with pytest.raises(_lib.NfaiHipError, match=r"the batched kernels take fp16") as e:
            LlamaWindow(m, 4)
        assert e.value.code == _lib.ERR_UNSUPPORTED
        any_window(m, 4).Dispose()
    finally:
        m.Dispose()
