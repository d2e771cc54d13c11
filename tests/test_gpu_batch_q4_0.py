"""Batches (nfai_hip_llama_batch_*) and windows (nfai_hip_llama_window_*) on Q4_0 weights (NFAI_BATCH_QUANT | NFAI_BATCH_QUANT_ANY,
k_bgemv_kq on the Q4_0 T16 layout) on the GPU, against the CPU oracle on the DEQUANTISED weights.  It follows
tests/test_gpu_batch_quant_any.py and tests/test_gpu_window_quant_any.py, whose helpers, token sequences and bars it uses, on the
mixes "all_q4_0" (every matrix, the head and the embedding table too) and "q4_0" (synth.q4_0_type: the head in Q6_K).

Tolerances are the project's: 5e-4 * max(1, max|logit|) with an fp32 KV cache, 2e-2 with an fp16 one; hidden state and K / V rows
1e-3 / 2e-2 absolute.  In the fp32-cache runs of the staggered batch the ArgMax also equals the oracle's wherever the oracle's two
largest logits are more than twice the tolerance apart (a rule of the oracle alone; it may leave out at most one of a member's 24
steps, asserted)."""
from dataclasses import replace

import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth
from test_gpu_batch_quant import CAP, check_step, ddict, dispose, make_members, odesc, seq_tokens
from test_gpu_batch_quant_any import quantize as quantize_other
from test_gpu_q4_0 import Q4_0, mix_type, quantize as quantize_q4
from test_gpu_window_decode import N_REC, Recording, _IdTokenizer, check_column

pytestmark = pytest.mark.gpu

Q8_0, Q4_K, Q5_K, Q6_K = 8, 12, 13, 14
MIXES = ["all_q4_0", "q4_0"]


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


_WEIGHTS = {}


def quant_weights(dims, mix, seed=21, std=0.05):
    """({name: QuantTensor | gains}, {name: dequantised fp32 | gains}), quantised once per module.  mix: all_q4_0, q4_0, or a
    (q, k, v) tuple of ggml types for the three attention inputs (the rest Q4_0)."""
    from nfai_amd.llama_model import QuantTensor
    key = (dims.name, mix, seed, std)
    if key not in _WEIGHTS:
        w = synth.make_weights(dims, seed=seed, std=std)
        wq, wref = {}, {}
        for name, a in w.items():
            if a.ndim == 1:
                wq[name] = wref[name] = a
                continue
            qt = mix_type(name, mix, dims)
            raw, deq = quantize_q4(a.astype(np.float32), qt) if qt == Q4_0 else quantize_other(a.astype(np.float32), qt)
            wq[name] = QuantTensor(raw, qt, a.shape)
            wref[name] = deq
        _WEIGHTS[key] = (wq, wref)
    return _WEIGHTS[key]


def any_batch(ms):
    from nfai_amd.llama_model import LlamaBatch
    return LlamaBatch(ms, quantized=True, any_quant=True)


def any_window(m, max_tokens=8):
    from nfai_amd.llama_model import LlamaWindow
    return LlamaWindow(m, max_tokens, quantized=True, any_quant=True)


def make_model(mgr, dims, mix, cap=CAP, **kw):
    from nfai_amd.llama_model import LlamaModel
    return LlamaModel(mgr, synth.make_metadata(dims), quant_weights(dims, mix)[0], cap, dims=ddict(dims), **kw)


# ---- batches -------------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_member(dims, mix, s):
    """Member s of the staggered batch through the oracle alone, once per (shape, mix, member): the logits of its 24 batch steps,
    then its hidden state and last K / V rows."""
    key = (dims.name, mix, s)
    if key not in _ORACLE:
        ref = orc.OracleLlama(odesc(dims, CAP), quant_weights(dims, mix)[1])
        toks = seq_tokens(dims, s)
        for t in toks[:5 + 7 * s]:
            ref.step(int(t))
        wants = [ref.step(int(toks[5 + 7 * s + i])).copy() for i in range(24)]
        last = 5 + 7 * s + 24
        _ORACLE[key] = (wants, ref.hidden().copy(), [ref.kcache(l)[last - 1].copy() for l in range(dims.L)],
                        [ref.vcache(l)[last - 1].copy() for l in range(dims.L)])
    return _ORACLE[key]


@pytest.mark.parametrize("n,kv_f16", [(1, False), (2, False), (5, False), (8, False), (5, True)], ids=lambda v: str(v))
@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("dims", [synth.TINY, synth.TINY_D128], ids=lambda d: d.name)
def test_staggered_batch_matches_the_oracle(mgr, dims, mix, n, kv_f16):
    """Member s takes its first 5 + 7 s tokens alone through _decode_step (unequal positions), then 24 batch steps."""
    wq, _ = quant_weights(dims, mix)
    ms = make_members(mgr, dims, wq, n, CAP, kv_f16=kv_f16)
    refs = [oracle_member(dims, mix, s) for s in range(n)]
    toks = [seq_tokens(dims, s) for s in range(n)]
    scale = 2e-2 if kv_f16 else 5e-4
    for s in range(n):
        for t in toks[s][:5 + 7 * s]:
            ms[s].Step(int(t), want_logits=False)
    batch = any_batch(ms)
    excluded = [0] * n
    for i in range(24):
        step_toks = [int(toks[s][5 + 7 * s + i]) for s in range(n)]
        lg, am = batch.Step(step_toks)
        check_step(lg, am, [refs[s][0][i] for s in range(n)], scale, f"step {i}", oracle_argmax=not kv_f16, excluded=excluded)
    print(f"steps left out per member: {excluded}")
    assert max(excluded) <= 1, excluded
    for s in range(n):
        last = 5 + 7 * s + 24
        assert ms[s].Pos == last
        atol = 1e-3 if not kv_f16 else 2e-2
        np.testing.assert_allclose(ms[s].Read(0, dims.E), refs[s][1], rtol=0, atol=atol)
        for l in range(dims.L):
            np.testing.assert_allclose(ms[s].ReadKV(l, False, last - 1), refs[s][2][l], rtol=0, atol=atol)
            np.testing.assert_allclose(ms[s].ReadKV(l, True, last - 1), refs[s][3][l], rtol=0, atol=atol)
    dispose(batch, ms)


@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("dims", [synth.TINY, synth.TINY_D128], ids=lambda d: d.name)
def test_a_column_does_not_depend_on_its_neighbours(mgr, dims, mix):
    """The same member state and token in column 0 of a batch of 2, alone in a batch of 1, in column 4 of a batch of 5 and in column
    7 of a batch of 8 whose other members sit at other depths: BIT-IDENTICAL logits; a permutation of the members changes no
    member's logits by a bit."""
    wq, _ = quant_weights(dims, mix)
    ms = make_members(mgr, dims, wq, 8, CAP)
    toks = [seq_tokens(dims, s) for s in range(8)]

    def bring(s, count):
        ms[s].Reset()
        for t in toks[s][:count]:
            ms[s].Step(int(t), want_logits=False)

    probe, depth, tok = 3, 17, int(toks[3][17])
    bring(probe, depth)
    b1 = any_batch([ms[probe]])
    lg_1, am_1 = b1.Step([tok])
    b1.Dispose()
    bring(probe, depth)
    bring(0, 9)
    b2 = any_batch([ms[probe], ms[0]])
    lg_a, am_a = b2.Step([tok, int(toks[0][9])])
    b2.Dispose()
    np.testing.assert_array_equal(lg_1[0], lg_a[0])
    for s in range(8):
        bring(s, depth if s == probe else 4 + 5 * s)
    five = [0, 1, 2, 4, probe]
    b5 = any_batch([ms[s] for s in five])
    lg_5, am_5 = b5.Step([tok if s == probe else int(toks[s][4 + 5 * s]) for s in five])
    b5.Dispose()
    np.testing.assert_array_equal(lg_a[0], lg_5[4])
    for s in range(8):
        bring(s, depth if s == probe else 4 + 5 * s)
    order = [s for s in range(8) if s != probe] + [probe]
    b8 = any_batch([ms[s] for s in order])
    lg_b, am_b = b8.Step([tok if s == probe else int(toks[s][4 + 5 * s]) for s in order])
    b8.Dispose()
    np.testing.assert_array_equal(lg_a[0], lg_b[7])
    assert am_1[0] == am_a[0] == am_5[4] == am_b[7]
    first = {s: lg_b[i].copy() for i, s in enumerate(order)}
    for s in range(8):
        bring(s, depth if s == probe else 4 + 5 * s)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    bp = any_batch([ms[s] for s in perm])
    lg_p, _ = bp.Step([tok if s == probe else int(toks[s][4 + 5 * s]) for s in perm])
    for i, s in enumerate(perm):
        np.testing.assert_array_equal(lg_p[i], first[s])
    dispose(bp, ms)


@pytest.mark.parametrize("qkv", [(Q4_0, Q8_0, Q6_K), (Q4_K, Q4_0, Q5_K)], ids=["q4_0-q8_0-q6_k", "q4_k-q4_0-q5_k"])
def test_q4_0_beside_the_other_types_in_one_qkv(mgr, qkv):
    """Q4_0 beside the other admitted types inside a q|k|v: one launch per type, three here; both in the batch and in the model's
    own decode step (which gives a Q4_0 segment a launch of its own)."""
    dims, n = synth.TINY_D128, 3
    wq, wref = quant_weights(dims, qkv)
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
        check_step(lg, am, [refs[s].step(st[s]) for s in range(n)], 5e-4, f"step {i}")
    prof = batch.ProfileStep([int(toks[s][2 + 3 * s + 8]) for s in range(n)])
    assert prof["qkv"][1] == 3 * dims.L, prof
    assert prof["wo"][1] == prof["gateup"][1] == prof["down"][1] == dims.L and prof["lmhead"][1] == 1, prof
    dispose(batch, ms)


WIDE = replace(synth.LLAMA_32_3B, L=1, V=2048, F=4352, name="llama-3.2-3b-1blk-f4352")


@pytest.mark.parametrize("n", [8, 3])
def test_tiled_k_two_slots_per_wave_and_the_ragged_last_tile(mgr, n):
    """The smallest shape that reaches them (tests/test_gpu_batch_quant_any.py): E = 3072 is 12 super-blocks (two slots per wave);
    F = 4352 is 17: Wdown runs as two K tiles of 9 on 5 waves, the last wave's second slot is empty and the second tile ends one
    super-block past K."""
    wq, wref = quant_weights(WIDE, "all_q4_0", seed=31, std=0.02)
    C = 32
    ms = make_members(mgr, WIDE, wq, n, C)
    refs = [orc.OracleLlama(odesc(WIDE, C), wref) for _ in range(n)]
    toks = [synth.make_tokens(WIDE, 32, seed=200 + s) for s in range(n)]
    for s in range(n):
        for t in toks[s][:1 + 2 * s]:
            ms[s].Step(int(t), want_logits=False)
            refs[s].step(int(t))
    batch = any_batch(ms)
    for i in range(12):
        st = [int(toks[s][1 + 2 * s + i]) for s in range(n)]
        lg, am = batch.Step(st)
        check_step(lg, am, [refs[s].step(st[s]) for s in range(n)], 5e-4, f"step {i}")
    dispose(batch, ms)


@pytest.mark.parametrize("n", [2, 5])
def test_step_topk_rows_are_those_of_the_members_own_logits(mgr, n):
    """StepTopK on a staggered Q4_0 batch: every member's candidates are bit-equal to the device's top-k on the member's own logits
    of that step (nfai_hip_topk, the launch nfai_hip_llama_decode_topk runs behind one model's step), as
    tests/test_gpu_batch_sampling.py checks it for the other types; the drawn tokens are fed back."""
    from test_gpu_batch_sampling import check_candidates, staggered
    dims = synth.TINY_D128
    wq, _ = quant_weights(dims, "all_q4_0")
    ms = make_members(mgr, dims, wq, n, CAP)
    toks = staggered(ms, dims, n)
    batch = any_batch(ms)
    feed = [int(toks[s][5 + 7 * s]) for s in range(n)]
    for i in range(6):
        ids, probs = batch.StepTopK(feed, 0.5, 40)
        assert ids.shape == (n, 40) and probs.shape == (n, 40)
        own = check_candidates(mgr, ms, dims.V, ids, probs, 0.5, 40, f"step {i}")
        for s in range(n):
            assert int(ids[s][0]) == int(np.argmax(own[s])) and ms[s].Pos == 5 + 7 * s + i + 1
            feed[s] = int(ids[s][0])
    dispose(batch, ms)


# ---- windows -------------------------------------------------------------------------------------------------------------------------
CONFIGS = [pytest.param(d, x, k, id=f"{d.name}-{x}-{'kv16' if k else 'kv32'}")
           for d, x, k in ((synth.TINY, "all_q4_0", False), (synth.TINY_D128, "q4_0", False), (synth.TINY_D128, "all_q4_0", True))]
STEP_TOKENS = 5 + 36   # 5 alone, then windows of 1 .. 8


@pytest.mark.parametrize("dims,mix,kv_f16", CONFIGS)
def test_window_steps_match_the_oracle(mgr, dims, mix, kv_f16):
    """5 tokens through _decode_step, then windows of t = 1 .. 8 tokens: every column's logits, ArgMax, the position and the K / V
    rows of every window position against the oracle fed the same tokens one by one."""
    ref = orc.OracleLlama(odesc(dims, CAP), quant_weights(dims, mix)[1])
    toks = [int(t) for t in synth.make_tokens(dims, 64, seed=131)]
    want = [ref.step(t).copy() for t in toks[:STEP_TOKENS]]
    m = make_model(mgr, dims, mix, kv_f16=kv_f16)
    scale = 2e-2 if kv_f16 else 5e-4
    atol = 2e-2 if kv_f16 else 1e-3
    for t in toks[:5]:
        m.Step(t, want_logits=False)
    cur = 5
    win = any_window(m)
    try:
        for t in range(1, 9):
            lg, am = win.Step(toks[cur:cur + t])
            assert lg.shape == (t, dims.V) and am.shape == (t,)
            for i in range(t):
                check_column(lg[i], am[i], want[cur + i], scale, f"t={t} pos {cur + i} column {i}")
            for l in range(dims.L):
                for i in range(t):
                    np.testing.assert_allclose(m.ReadKV(l, False, cur + i), ref.kcache(l)[cur + i], rtol=0, atol=atol)
                    np.testing.assert_allclose(m.ReadKV(l, True, cur + i), ref.vcache(l)[cur + i], rtol=0, atol=atol)
            cur += t
            assert m.Pos == cur
        assert cur == STEP_TOKENS
    finally:
        win.Dispose()
        m.Dispose()


@pytest.mark.parametrize("dims,mix,kv_f16", CONFIGS)
def test_a_column_depends_neither_on_the_window_size_nor_on_later_columns(mgr, dims, mix, kv_f16):
    """Column i's logits are BIT-IDENTICAL for every T > i, and when the tokens of the columns behind it are replaced."""
    m = make_model(mgr, dims, mix, kv_f16=kv_f16)
    toks = [int(t) for t in synth.make_tokens(dims, 64, seed=133)]
    win = any_window(m)
    depth = 37

    def bring():
        m.Reset()
        for t in toks[:depth]:
            m.Step(t, want_logits=False)

    try:
        bring()
        cols = toks[depth:depth + 8]
        lg8, am8 = win.Step(cols)
        for i in (0, 1, 4, 6):   # T = 1, 2, 5, 7 against T = 8
            bring()
            lg, am = win.Step(cols[:i + 1])
            np.testing.assert_array_equal(lg, lg8[:i + 1])
            np.testing.assert_array_equal(am, am8[:i + 1])
        for i in (0, 3, 6):
            other = cols[:i + 1] + [(t + 1 + j) % dims.V for j, t in enumerate(cols[i + 1:])]
            bring()
            lg, am = win.Step(other)
            np.testing.assert_array_equal(lg[:i + 1], lg8[:i + 1])
            assert not np.array_equal(lg[i + 1], lg8[i + 1])   # (the replaced column did change)
    finally:
        win.Dispose()
        m.Dispose()


@pytest.mark.parametrize("dims,mix,kv_f16", CONFIGS)
def test_verify_and_the_rows_of_rejected_drafts(mgr, dims, mix, kv_f16):
    """The twin's Verify with no draft, repeated, is the model's greedy continuation g (a window's column does not depend on the
    columns beside it by a bit, so no near-tie rule is needed).  Drafts g[:k] are all kept; with draft j spoiled, j + 1 tokens come
    out; and a model whose Verify rejected drafts goes on BIT-IDENTICAL to a twin that was fed only the accepted tokens: the rows
    of rejected drafts are never read."""
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
        for k in (0, 1, 4, 7):                        # every draft right: T = 1, 2, 5, 8
            bring(a)
            lg, out = wa.Verify(prompt[-1], g[:k], want_logits=True)
            assert [int(t) for t in out] == g[:k + 1], (k, out, g)
            assert lg.shape == (k + 1, dims.V) and [int(np.argmax(r)) for r in lg] == g[:k + 1]
            assert a.Pos == p + k + 1
        for j in (0, 2, 6):                           # the first error at column j
            bring(a)
            draft = list(g[:7])
            draft[j] = (draft[j] + 1) % dims.V
            _, out = wa.Verify(prompt[-1], draft)
            assert [int(t) for t in out] == g[:j + 1], (j, out, g)
            assert a.Pos == p + j + 1
        # a: draft 0 right, draft 1 wrong (rows p + 2 .. are stale); b: the accepted tokens only, from the same base position
        bring(a)
        bring(b)
        wrong = [g[0], (g[1] + 1) % dims.V, (g[1] + 2) % dims.V, 5, 6, 7]
        lga, out = wa.Verify(prompt[-1], wrong, want_logits=True)
        assert [int(t) for t in out] == g[:2]
        lgb, amb = wb.Step([prompt[-1], g[0]])
        assert int(amb[1]) == g[1] and a.Pos == b.Pos == p + 2
        np.testing.assert_array_equal(lga[:2], lgb)
        assert not np.array_equal(a.ReadKV(0, False, p + 3), b.ReadKV(0, False, p + 3))   # (the rejected rows ARE there)
        nxt = g[1]
        for k in (0, 0, 2, 1):
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


SPEC_SEEDS = {"all_q4_0": 21, "q4_0": 21}   # weight seeds whose greedy continuation of token 7 has no near tie (asserted below)


@pytest.mark.parametrize("mix", MIXES)
def test_speculative_run_async_equals_the_plain_greedy_generation(mgr, mix):
    """24 tokens through RunAsync(greedy=True, speculative=4) on a Q4_0 model, with no new argument: the model recorded what it was
    given and opens the window with both flags.  The drafter is sometimes right (it knows the oracle's recording and spoils every
    third proposal at its second token, every fifth at its first).  The text is that of speculative=0, and the oracle's: its two
    largest logits are more than twice the tolerance apart at every recorded step (asserted from the oracle alone)."""
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY
    wq, wref = quant_weights(dims, mix, seed=SPEC_SEEDS[mix])
    prompt = [7]
    rec = Recording(dims, wref, prompt, 5e-4)
    print(f"recording {rec.tokens[:N_REC]}")
    assert all(rec.ok[:N_REC]), rec.ok
    m = LlamaModel(mgr, synth.make_metadata(dims), wq, CAP, dims=ddict(dims))
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
        spec = [int(t) for t in "".join(m.RunAsync("7", greedy=True, max_tokens=N_REC, speculative=4, drafter=Drafter())).split()]
        assert spec == plain
        assert len(calls) < N_REC          # some drafts were kept: fewer passes than tokens
        assert m.Pos == pos_plain
    finally:
        m.Dispose()


# ---- admissions ------------------------------------------------------------------------------------------------------------------------
def test_admissions_and_refusals(mgr):
    from nfai_amd import _lib
    from nfai_amd._lib import NfaiHipError
    from nfai_amd.llama_model import LlamaBatch, LlamaWindow
    from test_gpu_batch_quant_any import quant_weights as other_weights
    dims = synth.TINY_D128

    def refused(make, pattern):
        with pytest.raises(NfaiHipError, match=pattern) as e:
            make()
        assert e.value.code == _lib.ERR_UNSUPPORTED, e.value.args

    made = []
    ms = make_members(mgr, dims, quant_weights(dims, "all_q4_0")[0], 2, 8)
    made += reversed(ms)
    any_batch(ms).Dispose()                                                                  # admitted with both flags
    any_window(ms[0], 4).Dispose()
    refused(lambda: LlamaBatch(ms, quantized=True), r"member 0: token_embd of block 0 has ggml type 2\b")
    refused(lambda: LlamaBatch(ms, quantized=True), r"has ggml type 2; a quantised batch takes Q4_K and Q6_K matrices")
    refused(lambda: LlamaBatch(ms), r"member 0: token_embd of block 0 has ggml type 2; the batched kernels take fp16")
    refused(lambda: LlamaWindow(ms[0], 4, quantized=True), r"has ggml type 2; a quantised window takes Q4_K and Q6_K matrices")
    refused(lambda: LlamaWindow(ms[0], 4), r"has ggml type 2; the batched kernels take fp16")
    with pytest.raises(NfaiHipError) as e:                                                   # a wide batch takes fp16 only
        LlamaBatch(ms, wide=True)
    assert e.value.code == _lib.ERR_UNSUPPORTED and "ggml type 2" in str(e.value), e.value.args
    # the file mix (head in Q6_K): the first matrix that is not Q4_K / Q6_K is named
    mq = make_members(mgr, dims, quant_weights(dims, "q4_0")[0], 2, 8)
    made += reversed(mq)
    any_batch(mq).Dispose()
    refused(lambda: LlamaBatch(mq, quantized=True), r"member 0: token_embd of block 0 has ggml type 2\b")   # (untied: the table is Q4_0)
    # the other four types' mixes stay admitted under both flags
    for mix in ("q5_k_m", "all_q8_0", "q8_0_v_q4k"):
        mo = make_members(mgr, dims, other_weights(dims, mix)[0], 2, 8)
        made += reversed(mo)
        any_batch(mo).Dispose()
    for m in made:
        m.Dispose()
