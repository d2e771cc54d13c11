"""The window (nfai_hip_llama_window_*, kernels_attn_window.hip) on the GPU: up to 8 consecutive positions of ONE model per pass over
the weights, against the CPU oracle fed the same tokens one by one, and its use as lossless greedy speculative decoding (Verify).

Weights: fp16, or the Q4_K_M-like mix of tests/test_gpu_batch_quant.py (Q6_K for token_embd, output and attn_v / ffn_down of even
blocks, Q4_K elsewhere) against the oracle on the DEQUANTISED weights.

Tolerances are the project's: 5e-4 * max(1, max|logit|) with an fp32 KV cache, 2e-2 with an fp16 one, for both weight kinds (the
bound tests/test_gpu_batch_quant.py uses on the same weights); K / V rows 1e-3 / 2e-2 absolute as tests/test_gpu_batch_decode.py;
the attention launch alone 3e-5 * max(1, max|V|) against float64 (tests/test_gpu_attention_depth.py).

Verify is checked against a greedy continuation RECORDED BY THE ORACLE ALONE.  Seeds and prompts (VERIFY_SEEDS) were chosen on the
CPU so that the oracle's two largest logits are more than twice the tolerance apart at all but at most one of the 24 recorded steps
(asserted); at such a step either of the two is accepted and the oracle continues on the token the GPU emitted.  With the fp32-cache
tolerance every configuration has a varied recording without such a step.  Twice the fp16-cache tolerance is 4 % of the largest
logit, which random weights rarely clear 24 times running: three of the four fp16-cache recordings found settle on one or two
repeated tokens (strongly preferred ones), which still exercises every accept / reject path.  That DIFFERENT tokens are kept is shown
by the fp32-cache ones and, for an fp16 cache, by tiny-llama with the Q4_K_M mix (260 75 225 483 225 483 225 228 ...)."""
import ctypes as C
import re

import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth

pytestmark = pytest.mark.gpu

CAP = 96
Q4_K, Q5_K, Q6_K, Q8_0 = 12, 13, 14, 8
ATTN_BAR = 3e-5
MIN_CHUNK, MAX_SPLIT = 32, 32   # kernels_attn_window.hip: WA_MIN_CHUNK, WA_NSPLIT (the slicing of the cached prefix)

CONFIGS = [pytest.param(d, q, k, id=f"{d.name}-{'q4km' if q else 'f16'}-{'kv16' if k else 'kv32'}")
           for d in (synth.TINY, synth.TINY_D128) for q in (False, True) for k in (False, True)]


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


def odesc(d, cap):
    return orc.LlamaDesc(E=d.E, L=d.L, H=d.H, Hkv=d.Hkv, D=d.D, F=d.F, V=d.V, C=cap)


def ddict(d):
    return dict(E=d.E, L=d.L, H=d.H, Hkv=d.Hkv, D=d.D, F=d.F, V=d.V, eps=1e-5, rope_dims=d.D, rope_base=500000.0)


def logit_tol(want, scale):
    return scale * max(1.0, float(np.abs(want).max()))


def mix_type(name):
    if name.startswith(("token_embd", "output.")):
        return Q6_K
    m = re.match(r"blk\.(\d+)\.(attn_v|ffn_down)\.weight$", name)
    return Q6_K if m and int(m.group(1)) % 2 == 0 else Q4_K


def quant_weights(w):
    """synth weights -> ({name: QuantTensor | gains}, {name: dequantised fp32 | gains}) in the mix of test_gpu_batch_quant.py."""
    from nfai_amd.llama_model import QuantTensor
    wq, wref = {}, {}
    for name, a in w.items():
        if a.ndim == 1:
            wq[name] = wref[name] = a
            continue
        a32 = np.ascontiguousarray(a, np.float32)
        if mix_type(name) == Q4_K:
            raw = orc.quantize_q4k(a32)
            deq = orc.dequant_q4k(raw, a32.size)
        else:
            raw = orc.quantize_q6k(a32)
            deq = orc.dequant_q6k(raw, a32.size)
        wq[name] = QuantTensor(raw, mix_type(name), a.shape)
        wref[name] = deq.reshape(a.shape)
    return wq, wref


_WEIGHTS = {}


def weights(dims, quant, seed=21):
    """(what the model loads, what the oracle computes on)."""
    key = (dims.name, quant, seed)
    if key not in _WEIGHTS:
        w = synth.make_weights(dims, seed=seed, std=0.05)
        _WEIGHTS[key] = quant_weights(w) if quant else (w, w)
    return _WEIGHTS[key]


def make_model(mgr, dims, wdev, quant, cap=CAP, **kw):
    from nfai_amd.llama_model import LlamaModel
    if quant:
        kw.setdefault("dims", ddict(dims))
    return LlamaModel(mgr, synth.make_metadata(dims), wdev, cap, **kw)


def check_column(lg, am, want, scale, where):
    tol = logit_tol(want, scale)
    err = float(np.abs(lg - want).max())
    print(f"{where}: max|dlogit| {err:.3e} tol {tol:.3e}")
    assert err <= tol, (where, err, tol)
    assert int(am) == int(np.argmax(lg)), (where, int(am), int(np.argmax(lg)))   # first index of the maximum


# ---- 1: Step against the oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,quant,kv_f16", CONFIGS)
def test_window_steps_match_the_oracle(mgr, dims, quant, kv_f16):
    """5 tokens through _decode_step, then windows of t = 1 .. 8 tokens, a plain _decode_step, and another window: every column's
    logits, ArgMax, the position and the K / V rows of every window position against the oracle fed the same tokens one by one."""
    from nfai_amd.llama_model import LlamaWindow
    wdev, wref = weights(dims, quant)
    m = make_model(mgr, dims, wdev, quant, kv_f16=kv_f16)
    ref = orc.OracleLlama(odesc(dims, CAP), wref)
    toks = [int(t) for t in synth.make_tokens(dims, 64, seed=131)]
    scale = 2e-2 if kv_f16 else 5e-4
    atol = 2e-2 if kv_f16 else 1e-3
    cur = 0
    for t in toks[:5]:
        m.Step(t, want_logits=False)
        ref.step(t)
        cur += 1
    win = LlamaWindow(m, 8, quantized=quant)

    def window(t):
        nonlocal cur
        tk = toks[cur:cur + t]
        lg, am = win.Step(tk)
        assert lg.shape == (t, dims.V) and am.shape == (t,)
        for i in range(t):
            check_column(lg[i], am[i], ref.step(tk[i]), scale, f"t={t} pos {cur + i} column {i}")
        for l in range(dims.L):
            for i in range(t):
                np.testing.assert_allclose(m.ReadKV(l, False, cur + i), ref.kcache(l)[cur + i], rtol=0, atol=atol)
                np.testing.assert_allclose(m.ReadKV(l, True, cur + i), ref.vcache(l)[cur + i], rtol=0, atol=atol)
        cur += t
        assert m.Pos == cur

    try:
        for t in range(1, 9):
            window(t)
        lg, am = m.Step(toks[cur])                    # the model alone, behind the windows
        check_column(lg, am, ref.step(toks[cur]), scale, f"decode_step pos {cur}")
        cur += 1
        assert m.Pos == cur
        window(3)                                      # and a window behind it
        window(8)
        assert win.BytesPerStep(4) > win.BytesPerStep(2) > 0
    finally:
        win.Dispose()
        m.Dispose()


# ---- 2: bit-exact invariants -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,quant,kv_f16", CONFIGS)
def test_a_column_depends_neither_on_the_window_size_nor_on_later_columns(mgr, dims, quant, kv_f16):
    """Column i's logits are BIT-IDENTICAL for T = i + 1 and T = 8, and when the tokens of the columns behind it are replaced: the
    GEMV sums are per column (tests/test_gpu_batch_decode.py::test_a_column_does_not_depend_on_its_neighbours), the attention slices
    the prefix by the position alone and column i's own rows p .. p + i are its fixed last piece."""
    from nfai_amd.llama_model import LlamaWindow
    wdev, _ = weights(dims, quant)
    m = make_model(mgr, dims, wdev, quant, kv_f16=kv_f16)
    toks = [int(t) for t in synth.make_tokens(dims, 64, seed=133)]
    win = LlamaWindow(m, 8, quantized=quant)
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


@pytest.mark.parametrize("dims,quant,kv_f16", CONFIGS)
def test_rows_of_rejected_drafts_are_never_read(mgr, dims, quant, kv_f16):
    """A model whose Verify rejected drafts and went on decoding, against a twin that was fed only the accepted tokens through
    windows at the same base positions: BIT-IDENTICAL logits at every later step, though the first one's cache holds the rejected
    drafts' rows above its position."""
    from nfai_amd.llama_model import LlamaWindow
    wdev, _ = weights(dims, quant)
    a = make_model(mgr, dims, wdev, quant, kv_f16=kv_f16)
    b = make_model(mgr, dims, wdev, quant, kv_f16=kv_f16, share_from=a)
    wa, wb = LlamaWindow(a, 8, quantized=quant), LlamaWindow(b, 8, quantized=quant)
    toks = [int(t) for t in synth.make_tokens(dims, 64, seed=135)]
    depth = 33
    try:
        for mdl in (a, b):
            for t in toks[:depth]:
                mdl.Step(t, want_logits=False)
        # the model's own two next tokens (from the twin, then put back)
        _, g = wb.Verify(toks[depth], [])
        g0 = int(g[0])
        _, g = wb.Verify(g0, [])
        g1 = int(g[0])
        b.SetPos(depth)
        wrong = [(g1 + 1) % dims.V, (g1 + 2) % dims.V, (g1 + 3) % dims.V, 5, 6, 7]
        lga, out = wa.Verify(toks[depth], [g0] + wrong, want_logits=True)   # 8 columns: draft 0 right, draft 1 wrong -> rows depth + 2 .. + 7 are stale
        assert [int(t) for t in out] == [g0, g1]
        lgb, amb = wb.Step([toks[depth], g0])                   # the twin: the accepted tokens only, same base position
        assert int(amb[1]) == g1 and a.Pos == b.Pos == depth + 2
        np.testing.assert_array_equal(lga[:2], lgb)
        # (the rejected rows ARE there and differ from the twin's)
        assert not np.array_equal(a.ReadKV(0, False, depth + 3), b.ReadKV(0, False, depth + 3))
        nxt = g1
        for step, k in enumerate((0, 0, 2, 0, 1)):             # single columns first: the stale rows stay above the position
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
N_REC = 24
# (dims, quantised, fp16 KV) -> (weight seed, prompt seed): chosen on the CPU with the oracle alone, see the module docstring
VERIFY_SEEDS = {
    ("tiny-llama", False, False): (23, 302), ("tiny-llama", True, False): (23, 302),
    ("tiny-llama-d128", False, False): (21, 307), ("tiny-llama-d128", True, False): (21, 312),
    ("tiny-llama", False, True): (26, 311), ("tiny-llama", True, True): (28, 306),
    ("tiny-llama-d128", False, True): (194, 305), ("tiny-llama-d128", True, True): (194, 305),
}


class Recording:
    """The oracle's greedy continuation of a prompt: tokens[i] is the token emitted after i fed-back tokens.  ok[i]: the two largest
    logits of step i are more than twice the tolerance apart.  At a step that is not, settle() accepts the runner-up too and
    re-records from there on the token the GPU emitted."""

    def __init__(self, dims, wref, prompt, scale, n=N_REC + 2):
        self.dims, self.wref, self.prompt, self.scale, self.n = dims, wref, list(prompt), scale, n
        self.tokens, self.second, self.ok = [], [], []
        self._extend([])

    def _extend(self, forced):
        ref = orc.OracleLlama(odesc(self.dims, CAP), self.wref)
        for t in self.prompt[:-1]:
            ref.step(int(t))
        lg = ref.step(int(self.prompt[-1]))
        toks, second, ok = [], [], []
        for i in range(self.n):
            order = np.argsort(-lg, kind="stable")
            tol = logit_tol(lg, self.scale)
            ok.append(float(lg[order[0]] - lg[order[1]]) > 2 * tol)
            second.append(int(order[1]))
            t = forced[i] if i < len(forced) else int(order[0])
            toks.append(t)
            lg = ref.step(t)
        self.tokens, self.second, self.ok = toks, second, ok

    def settle(self, i, tok):
        """The GPU emitted `tok` as token i."""
        tok = int(tok)
        if tok == self.tokens[i]:
            return
        assert not self.ok[i], (i, tok, self.tokens[i])                    # a clear step: the oracle's token, nothing else
        alternatives = {self.tokens[i], self.second[i]}
        assert tok in alternatives, (i, tok, alternatives)                  # a near tie: either of the two largest
        self._extend(self.tokens[:i] + [tok])

    def expect(self, start, got):
        for j, t in enumerate(got):
            self.settle(start + j, t)


def verify_setup(mgr, dims, quant, kv_f16):
    from nfai_amd.llama_model import LlamaWindow
    wseed, pseed = VERIFY_SEEDS[(dims.name, quant, kv_f16)]
    wdev, wref = weights(dims, quant, seed=wseed)
    prompt = [int(t) for t in synth.make_tokens(dims, 9, seed=pseed)]
    rec = Recording(dims, wref, prompt, 2e-2 if kv_f16 else 5e-4)
    excluded = sum(1 for v in rec.ok[:N_REC] if not v)
    print(f"recording {rec.tokens[:N_REC]}; steps within twice the tolerance: {excluded}")
    assert excluded <= 1, (excluded, rec.ok)
    m = make_model(mgr, dims, wdev, quant, kv_f16=kv_f16)
    return m, LlamaWindow(m, 8, quantized=quant), prompt, rec


def bring_to_prompt(m, prompt):
    m.Reset()
    for t in prompt[:-1]:
        m.Step(t, want_logits=False)


@pytest.mark.parametrize("dims,quant,kv_f16", CONFIGS)
def test_verify_keeps_right_drafts_and_stops_at_the_first_wrong_one(mgr, dims, quant, kv_f16):
    m, win, prompt, rec = verify_setup(mgr, dims, quant, kv_f16)
    p = len(prompt) - 1
    try:
        # every draft right: k + 1 tokens for k = 0 .. 7
        for k in range(8):
            bring_to_prompt(m, prompt)
            lg, out = win.Verify(prompt[-1], rec.tokens[:k], want_logits=True)
            rec.expect(0, out)
            assert len(out) == k + 1, (k, out)
            assert lg.shape == (k + 1, dims.V) and [int(np.argmax(r)) for r in lg] == [int(t) for t in out]
            assert m.Pos == p + k + 1
            m.Enqueue(1)                                  # the token word: a greedy step on the device continues the recording
            rec.expect(k + 1, m.FetchTokens(1))
            assert m.Pos == p + k + 2
        # the first error at column j, for every j
        for j in range(7):
            bring_to_prompt(m, prompt)
            draft = list(rec.tokens[:7])
            draft[j] = (draft[j] + 1) % dims.V
            if not rec.ok[j] and draft[j] == rec.second[j]:
                draft[j] = (draft[j] + 1) % dims.V        # (wrong under the near-tie rule too)
            _, out = win.Verify(prompt[-1], draft)
            rec.expect(0, out)
            assert len(out) == j + 1, (j, out)
            assert m.Pos == p + j + 1
            m.Enqueue(1)
            rec.expect(j + 1, m.FetchTokens(1))
        # NULL outputs are an error code, and nothing moved
        from nfai_amd import _lib
        bring_to_prompt(m, prompt)
        n = C.c_uint32()
        d = (C.c_uint32 * 2)(1, 2)
        with pytest.raises(_lib.NfaiHipError, match="null argument"):
            _lib.call("nfai_hip_llama_window_verify", win.handle, prompt[-1], d, 2, None, None, C.byref(n))
        with pytest.raises(_lib.NfaiHipError, match="null tokens"):
            _lib.call("nfai_hip_llama_window_step", win.handle, None, 2, None, None)
        with pytest.raises(_lib.NfaiHipError, match="draft count"):
            win.Verify(prompt[-1], [1] * 8)
        assert m.Pos == p
    finally:
        win.Dispose()
        m.Dispose()


class _IdTokenizer:
    """Prompts are space-separated token ids; a token's text is its id."""
    EosTokenId = 1 << 30

    def Tokenize(self, prompt, addBos=False):
        return [int(t) for t in prompt.split()]

    def Detokenize(self, ids):
        return "".join(f"{int(t)} " for t in ids)


@pytest.mark.parametrize("dims,quant,kv_f16", CONFIGS)
def test_speculative_run_async_equals_the_plain_greedy_generation(mgr, dims, quant, kv_f16):
    """24 tokens through RunAsync(greedy=True, speculative=4) with a drafter that is sometimes right (it knows the recording and
    spoils every third proposal at its second token, every fifth at its first) against the oracle's recording, and against the
    plain greedy RunAsync."""
    m, win, prompt, rec = verify_setup(mgr, dims, quant, kv_f16)
    win.Dispose()
    m.tokenizer = _IdTokenizer()
    m.promptPrefill = False
    text = " ".join(str(t) for t in prompt)
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
        m.Reset()
        plain = [int(t) for t in "".join(m.RunAsync(text, greedy=True, max_tokens=N_REC)).split()]
        assert len(plain) == N_REC
        rec.expect(0, plain)
        pos_plain = m.Pos
        m.Reset()
        spec = [int(t) for t in "".join(m.RunAsync(text, greedy=True, max_tokens=N_REC, speculative=4, drafter=Drafter())).split()]
        assert len(spec) == N_REC
        rec.expect(0, spec)
        assert len(calls) < N_REC          # some drafts were kept: fewer passes than tokens
        assert m.Pos == pos_plain          # every emitted token but the last was fed, as in the plain loop
        if all(rec.ok[:N_REC]):
            assert spec == plain
    finally:
        m.Dispose()


class _EosTokenizer(_IdTokenizer):
    def __init__(self, eos):
        self.EosTokenId = int(eos)


@pytest.mark.parametrize("dims,quant,kv_f16", CONFIGS)
def test_speculative_run_async_stops_at_eos_where_the_plain_loop_stops(mgr, dims, quant, kv_f16):
    """The end of a turn.  EOS is a token of the recording (the first from the fourth on that is new there, else the third or second; a
    recording of one repeated token makes the FIRST emitted token EOS), and the drafter proposes the recording as it goes on: the EOS the model will
    emit with further right tokens behind it.  The plain loop never feeds an emitted EOS, so the speculative loop must leave the
    position in front of it too, and a second turn continues from the same state: it is checked against the oracle fed
    prompt + the tokens in front of EOS + the second prompt (near ties as in Recording.settle), and against the plain loop."""
    m, win, prompt, rec = verify_setup(mgr, dims, quant, kv_f16)
    win.Dispose()
    e = next((j for j in (*range(3, N_REC - 8), 2, 1) if rec.tokens[j] not in rec.tokens[:j] and all(rec.ok[:j + 1])), 0)
    assert all(rec.ok[:e + 1]), rec.ok      # the turn ends where the oracle says, with no near tie in front of it
    m.tokenizer = _EosTokenizer(rec.tokens[e])
    m.promptPrefill = False
    text = " ".join(str(t) for t in prompt)
    prompt2 = [int(t) for t in synth.make_tokens(dims, 5, seed=77)]
    text2 = " ".join(str(t) for t in prompt2)
    N2 = 8
    rec2 = [Recording(dims, rec.wref, prompt + rec.tokens[:e] + prompt2, rec.scale, n=N2 + 1) for _ in range(2)]   # one per loop
    k = next(k for k in (4, 5, 6, 7) if e % (k + 1) <= k - 2)   # every draft in front of EOS is kept: EOS is not the last of its proposal
    proposals = []

    class Drafter:
        def Propose(self, history, k):
            done = len(history) - len(prompt)
            d = list(rec.tokens[done:done + k])
            proposals.append(d)
            return d

    def two_turns(**kw):
        m.Reset()
        m.tokenizer.EosTokenId = rec.tokens[e]
        first = [int(t) for t in "".join(m.RunAsync(text, greedy=True, max_tokens=N_REC, **kw)).split()]
        pos1 = m.Pos
        m.tokenizer.EosTokenId = 1 << 30           # the second turn runs its N2 tokens whatever they are
        second = [int(t) for t in "".join(m.RunAsync(text2, greedy=True, max_tokens=N2, **kw)).split()]
        return first, pos1, second, m.Pos

    try:
        want_first = rec.tokens[:e] if e else rec.tokens[:1]     # (the first token is yielded whatever it is)
        want_pos1 = len(prompt) + e                               # the prompt and the e tokens in front of EOS were fed
        plain = two_turns()
        spec = two_turns(speculative=k, drafter=Drafter())
        print(f"eos = token {e} of the recording; proposals {proposals[:4]}; plain {plain}; speculative {spec}")
        assert any(rec.tokens[e] in d and d.index(rec.tokens[e]) < len(d) - 1 for d in proposals)   # EOS with right tokens behind it
        for r2, (first, pos1, second, pos2) in zip(rec2, (plain, spec)):
            assert first == want_first, (first, want_first)
            assert pos1 == want_pos1, (pos1, want_pos1)
            assert len(second) == N2
            r2.expect(0, second)
            assert pos2 == want_pos1 + len(prompt2) + N2 - 1
        if all(rec2[0].ok[:N2]):
            assert spec[2] == plain[2]
    finally:
        m.Dispose()


# ---- 4: bounds and refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quant", [False, True], ids=["f16", "q4km"])
def test_a_window_past_the_capacity_is_kv_full_and_moves_nothing(mgr, quant):
    from nfai_amd import _lib
    from nfai_amd.llama_model import LlamaWindow
    dims, cap = synth.TINY_D128, 16
    wdev, _ = weights(dims, quant)
    m = make_model(mgr, dims, wdev, quant, cap=cap)
    win = LlamaWindow(m, 8, quantized=quant)
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


def test_a_model_destroyed_under_its_window_is_invalid(mgr):
    from nfai_amd import _lib
    from nfai_amd.llama_model import LlamaWindow
    dims = synth.TINY
    wdev, _ = weights(dims, False)
    keep = make_model(mgr, dims, wdev, False)
    m = make_model(mgr, dims, wdev, False, share_from=keep)
    win = LlamaWindow(m, 4)
    try:
        win.Step([1, 2])
        m.Dispose()
        for call in (lambda: win.Step([3, 4]), lambda: win.Verify(3, [4]), lambda: win.BytesPerStep(2), lambda: win.ProfileStep([3, 4]),
                     lambda: window_vec(win, 0, 1, 8)):
            with pytest.raises(_lib.NfaiHipError, match="destroyed") as e:
                call()
            assert e.value.code == _lib.ERR_INVALID
    finally:
        win.Dispose()
        keep.Dispose()


def test_create_refuses_what_a_batch_refuses_by_name(mgr):
    from nfai_amd import _lib
    from nfai_amd.llama_model import LlamaWindow, QuantTensor
    dims = synth.TINY
    w = synth.make_weights(dims, seed=21, std=0.05)

    def typed(qt, quantize):
        return {k: (a if a.ndim == 1 else QuantTensor(np.frombuffer(quantize(a.astype(np.float32)), np.uint8).copy(), qt, a.shape))
                for k, a in w.items()}

    def refused(m, pattern, quantized):
        try:
            with pytest.raises(_lib.NfaiHipError, match=pattern) as e:
                LlamaWindow(m, 4, quantized=quantized)
            assert e.value.code == _lib.ERR_UNSUPPORTED
        finally:
            m.Dispose()

    refused(make_model(mgr, dims, typed(Q5_K, synth.quantize_q5_k), True), r"token_embd of block 0 has ggml type 13", True)
    refused(make_model(mgr, dims, typed(Q8_0, synth.quantize_q8_0), True), r"token_embd of block 0 has ggml type 8", True)
    wq, _ = weights(dims, True)
    refused(make_model(mgr, dims, wq, True), r"token_embd of block 0 has ggml type 14; the batched kernels take fp16", False)
    refused(make_model(mgr, dims, w, False, layer_range=(0, 1)), r"the model is a pipeline stage \(blocks \[0, 1\) of 2\); a window takes whole models", False)
    refused(make_model(mgr, dims, w, False, unfused=True), r"1:1 \(NFAI_LLAMA_UNFUSED\) path", False)
    m = make_model(mgr, dims, w, False)
    try:
        for bad in (1, 9):
            with pytest.raises(_lib.NfaiHipError, match=f"max_tokens = {bad}") as e:
                LlamaWindow(m, bad)
            assert e.value.code == _lib.ERR_INVALID
        win = LlamaWindow(m, 2)
        with pytest.raises(_lib.NfaiHipError, match="token count 3"):
            win.Step([1, 2, 3])
        with pytest.raises(_lib.NfaiHipError, match="vocab"):
            win.Step([1, dims.V])
        win.Dispose()
    finally:
        m.Dispose()


# ---- 5: the attention launch at full-width head shapes and depth ----------------------------------------------------------------------
def attn_split(S):
    ns = min(-(-S // MIN_CHUNK), MAX_SPLIT)
    ch = -(-S // ns)
    return -(-S // ch), ch


def decode_positions(cap, D):
    """The depths tests/test_gpu_attention_depth.py::decode_positions checks the decode attention at (one key, one and two slices,
    32 full slices of 32 and one more key, a last slice of one row, the shortest last slice in the upper half, exactly full slices,
    several tiles per slice, the last row)."""
    step = (256 // (D // 4)) * 4

    def last(S):
        ns, ch = attn_split(S)
        return S - (ns - 1) * ch

    short = min(range(cap // 2, cap + 1), key=lambda S: (last(S), -S))
    full = (cap - 1) // MAX_SPLIT * MAX_SPLIT
    multi = min(cap - 1, MAX_SPLIT * step * 3 + 7)
    return sorted({S for S in (1, 32, 33, 993, 1024, 1025, short, full, multi, cap) if 1 <= S <= cap})


def kv_rows(m, layer, is_v, pos, n):
    from nfai_amd import _lib
    lib = _lib.load()
    lib.nfai_hip_debug_read_kv_rows.argtypes = [_lib.H, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
    lib.nfai_hip_debug_read_kv_rows.restype = C.c_int32
    out = np.empty((n, m.dims["Hkv"] * m.dims["D"]), np.float32)
    _lib.call("nfai_hip_debug_read_kv_rows", m.handle, layer, int(is_v), pos, n, out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


def window_vec(win, col, which, n):
    from nfai_amd import _lib
    lib = _lib.load()
    lib.nfai_hip_debug_window_read.argtypes = [_lib.H, C.c_uint32, C.c_int32, C.POINTER(C.c_float), C.c_uint64]
    lib.nfai_hip_debug_window_read.restype = C.c_int32
    out = np.empty(n, np.float32)
    _lib.call("nfai_hip_debug_window_read", win.handle, col, which, out.ctypes.data_as(C.POINTER(C.c_float)), n)
    return out


# the 3B and 8B head shapes (G = 3 and 4, D = 128), and narrow models for the instantiations no other test reaches: G = 1 and 8 at both
# head sizes (G = 8, D = 128 is the largest LDS plan)
@pytest.mark.parametrize("name,H,Hkv,D,E,kv16", [("3b", 24, 8, 128, 3072, False), ("3b", 24, 8, 128, 3072, True),
                                                  ("8b", 32, 8, 128, 4096, False), ("8b", 32, 8, 128, 4096, True),
                                                  ("g8-d64", 8, 1, 64, 512, False), ("g8-d64", 8, 1, 64, 512, True),
                                                  ("g1-d64", 8, 8, 64, 512, False), ("g8-d128", 8, 1, 128, 1024, False),
                                                  ("g1-d128", 4, 4, 128, 512, True)],
                         ids=["3b-kv32", "3b-kv16", "8b-kv32", "8b-kv16", "g8-d64-kv32", "g8-d64-kv16", "g1-d64-kv32", "g8-d128-kv32",
                              "g1-d128-kv16"])
def test_window_attention_against_fp64_at_depth(mgr, name, H, Hkv, D, E, kv16):
    """The last block's window attention output of all 8 columns against float64 NumPy on the cache rows read back, at base positions
    p = S - 1 for the depths S the decode attention is checked at (p >= 1024: 32 prefix slices), capacity 2048."""
    from nfai_amd.llama_model import LlamaModel, LlamaWindow
    cap, T = 2048, 8
    dims = synth.LlamaDims(f"window-attn-{name}", E, 2, H, Hkv, D, 512, 1024, True)
    w = synth.make_weights(dims, seed=61, std=0.05 * np.sqrt(512.0 / E))
    m = LlamaModel(mgr, synth.make_metadata(dims), w, cap, kv_f16=kv16, max_batch=512)
    win = LlamaWindow(m, T)
    G, layer = H // Hkv, dims.L - 1
    try:
        toks = [int(t) for t in synth.make_tokens(dims, cap + T, seed=cap + H)]
        m.Ingest(toks[:cap - 1])
        K = np.zeros((cap, Hkv, D), np.float32)
        V = np.zeros((cap, Hkv, D), np.float32)
        K[:cap - 1] = kv_rows(m, layer, False, 0, cap - 1).reshape(cap - 1, Hkv, D)
        V[:cap - 1] = kv_rows(m, layer, True, 0, cap - 1).reshape(cap - 1, Hkv, D)
        worst = 0.0
        for S in decode_positions(cap, D):
            p = min(S - 1, cap - T)
            away = p // 2 if p > 16 else p + 40
            for base in (away, p):      # a window at a distant position first: a stale output cannot pass
                m.SetPos(base)
                win.Step(toks[base:base + T], want_logits=False)
                K[base:base + T] = kv_rows(m, layer, False, base, T).reshape(T, Hkv, D)
                V[base:base + T] = kv_rows(m, layer, True, base, T).reshape(T, Hkv, D)
            assert attn_split(p)[0] == 32 if p >= 1024 else True
            for c in range(T):
                q = window_vec(win, c, 1, H * D).astype(np.float64).reshape(Hkv, G, D)
                got = window_vec(win, c, 2, H * D).astype(np.float64).reshape(Hkv, G, D)
                n = p + c + 1
                for h in range(Hkv):
                    k64, v64 = K[:n, h].astype(np.float64), V[:n, h].astype(np.float64)
                    sc = q[h] @ k64.T / np.sqrt(D)
                    pr = np.exp(sc - sc.max(axis=1, keepdims=True))
                    want = (pr / pr.sum(axis=1, keepdims=True)) @ v64
                    err, bar = float(np.abs(got[h] - want).max()), ATTN_BAR * max(1.0, float(np.abs(v64).max()))
                    assert err <= bar, (name, S, p, c, h, err, bar)
                    worst = max(worst, err / bar)
        print(f"window attention {name} kv16={kv16}: worst err / bar = {worst:.3g}")
    finally:
        win.Dispose()
        m.Dispose()
