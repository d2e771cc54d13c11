"""The wide batch (nfai_hip_llama_batch_create_wide, kernels_gemv_wide.hip) on the GPU: up to 16 models over one set of fp16 weights
advance one token each per step on the fp16 MFMA, every member at its own position in its own KV cache, against one CPU oracle per
sequence.

Tolerance: the decode path's own, 5e-4 * max(1, max|logit|) (fp16 weights, activations as two fp16 planes hi + 2^-11 lo, fp32 sums:
tests/test_batch_wide_bar.py holds a restatement of that arithmetic under half of it and shows a lost plane over it); 2e-2 with an fp16
KV cache; K / V rows and the hidden state 1e-3 / 2e-2.  The returned argmax is always the first index of the maximum of the returned
logits; in the fp32-cache runs of test 1 it also equals the oracle's argmax wherever the oracle's two largest logits are more than
twice the tolerance apart — a rule that depends on the oracle alone and leaves out at most ONE of a member's 16 steps (asserted; with
these inputs: TINY member 1, TINY_D128 members 10 and 14)."""
from dataclasses import replace

import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth

from test_batch_vocab import V_REAL, ragged_vocabs, vocab_dims
from test_batch_wide import WIDE_MAX, wide_ties
from test_gpu_batch_decode import CAP, check_step, dispose, logit_tol, make_members, odesc
from test_gpu_batch_sampling import bit_equal, topk_single

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


def wide(ms):
    from nfai_amd.llama_model import LlamaBatch
    return LlamaBatch(ms, wide=True)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
ALONE, STEPS = (lambda s: 3 + 4 * s), 16
_REF = {}


def member_tokens(dims, s):
    return synth.make_tokens(dims, ALONE(s) + STEPS, seed=100 + s)


def member_reference(dims, w, s):
    """Member s's oracle, walked once per model and shared by every case: (logits of the 16 wide steps, hidden state, last K / V rows)."""
    key = (dims.name, s)
    if key not in _REF:
        ref = orc.OracleLlama(odesc(dims, CAP), w)
        toks = member_tokens(dims, s)
        for t in toks[:ALONE(s)]:
            ref.step(int(t), want_logits=False)
        logits = [ref.step(int(t)).copy() for t in toks[ALONE(s):]]
        last = ALONE(s) + STEPS - 1
        _REF[key] = (logits, ref.hidden().copy(), [ref.kcache(l)[last].copy() for l in range(dims.L)],
                     [ref.vcache(l)[last].copy() for l in range(dims.L)])
        ref.close()
    return _REF[key]


@pytest.mark.parametrize("kv_f16", [False, True], ids=["kv-f32", "kv-f16"])
@pytest.mark.parametrize("n", [1, 5, 9, 12, 16])
@pytest.mark.parametrize("dims", [synth.TINY, synth.TINY_D128], ids=lambda d: d.name)
def test_staggered_wide_batch_matches_the_oracle(mgr, dims, n, kv_f16):
    """Member s takes its first 3 + 4 s tokens alone through _decode_step (positions 3 ... 63), then 16 wide steps."""
    w = synth.make_weights(dims, seed=21, std=0.05)
    ms = make_members(mgr, dims, w, n, CAP, kv_f16=kv_f16)
    refs = [member_reference(dims, w, s) for s in range(n)]
    toks = [member_tokens(dims, s) for s in range(n)]
    scale = 2e-2 if kv_f16 else 5e-4
    for s in range(n):
        for t in toks[s][:ALONE(s)]:
            ms[s].Step(int(t), want_logits=False)
    batch = wide(ms)
    excluded = [0] * n
    for i in range(STEPS):
        lg, am = batch.Step([int(toks[s][ALONE(s) + i]) for s in range(n)])
        check_step(lg, am, [refs[s][0][i] for s in range(n)], scale, f"step {i}", oracle_argmax=not kv_f16, excluded=excluded)
    assert max(excluded) <= 1, excluded   # the near-tie rule may leave out at most one of a member's 16 steps
    atol = 2e-2 if kv_f16 else 1e-3
    for s in range(n):
        last = ALONE(s) + STEPS
        assert ms[s].Pos == last
        np.testing.assert_allclose(ms[s].Read(0, dims.E), refs[s][1], rtol=0, atol=atol)
        for l in range(dims.L):
            np.testing.assert_allclose(ms[s].ReadKV(l, False, last - 1), refs[s][2][l], rtol=0, atol=atol)
            np.testing.assert_allclose(ms[s].ReadKV(l, True, last - 1), refs[s][3][l], rtol=0, atol=atol)
    dispose(batch, ms)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [synth.TINY, synth.TINY_D128], ids=lambda d: d.name)
def test_a_column_does_not_depend_on_its_neighbours(mgr, dims):
    """The same member state and token (a) in column 0 of a wide batch of 9 and (b) in column 15 of one of 16 whose other members hold
    other sequences at other positions: BIT-IDENTICAL logits (the kernel always runs 16 columns; a (row, column) sum is a function of
    the matrix shape alone).  A permutation of the 16 members changes no member's logits by a bit."""
    w = synth.make_weights(dims, seed=21, std=0.05)
    ms = make_members(mgr, dims, w, 16, CAP)
    toks = [member_tokens(dims, s) for s in range(16)]
    depth = lambda s: 17 if s == 3 else 2 + 3 * s

    def bring(members):
        for s in members:
            ms[s].Reset()
            for t in toks[s][:depth(s)]:
                ms[s].Step(int(t), want_logits=False)

    feed = lambda order: [int(toks[s][depth(s)]) for s in order]
    probe = 3
    nine = [probe] + [s for s in range(16) if s != probe][:8]
    bring(nine)
    b = wide([ms[s] for s in nine])
    lg_a, am_a = b.Step(feed(nine))
    b.Dispose()
    order = [s for s in range(16) if s != probe] + [probe]
    bring(range(16))
    b = wide([ms[s] for s in order])
    lg_b, am_b = b.Step(feed(order))
    b.Dispose()
    np.testing.assert_array_equal(bits(lg_a[0]), bits(lg_b[15]))
    assert am_a[0] == am_b[15]
    first = {s: lg_b[i].copy() for i, s in enumerate(order)}
    perm = [5, 12, 2, 15, 7, 0, 9, 3, 14, 6, 11, 1, 13, 4, 10, 8]
    bring(range(16))
    b = wide([ms[s] for s in perm])
    lg_p, _ = b.Step(feed(perm))
    for i, s in enumerate(perm):
        np.testing.assert_array_equal(bits(lg_p[i]), bits(first[s]))
    dispose(b, ms)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def test_wide_and_single_steps_interleave(mgr):
    dims, n = synth.TINY_D128, 10
    w = synth.make_weights(dims, seed=21, std=0.05)
    ms = make_members(mgr, dims, w, n, CAP)
    refs = [orc.OracleLlama(odesc(dims, CAP), w) for _ in range(n)]
    toks = [synth.make_tokens(dims, 40, seed=100 + s) for s in range(n)]
    cur = [0] * n

    def batch_step(batch, where):
        st = [int(toks[s][cur[s]]) for s in range(n)]
        lg, am = batch.Step(st)
        wants = []
        for s in range(n):
            wants.append(refs[s].step(st[s]))
            cur[s] += 1
        check_step(lg, am, wants, 5e-4, where)

    for s in range(n):   # staggered start
        for t in toks[s][:2 + 2 * s]:
            ms[s].Step(int(t), want_logits=False)
            refs[s].step(int(t), want_logits=False)
            cur[s] += 1
    batch = wide(ms)
    batch_step(batch, "wide 0")
    for s in (1, 9):   # members of both halves alone
        lg, am = ms[s].Step(int(toks[s][cur[s]]))
        want = refs[s].step(int(toks[s][cur[s]]))
        cur[s] += 1
        assert np.abs(lg - want).max() <= logit_tol(want)
    batch_step(batch, "wide 1")
    batch_step(batch, "wide 2")
    back = cur[8] - 3   # member 8 goes back by 3 and the batch re-feeds those tokens
    ms[8].SetPos(back)
    refs[8].close()
    refs[8] = orc.OracleLlama(odesc(dims, CAP), w)
    for t in toks[8][:back]:
        refs[8].step(int(t), want_logits=False)
    cur[8] = back
    for i in range(3):
        batch_step(batch, f"re-feed {i}")
    assert [m.Pos for m in ms] == cur
    for s in range(n):
        for l in range(dims.L):
            np.testing.assert_allclose(ms[s].ReadKV(l, False, cur[s] - 1), refs[s].kcache(l)[cur[s] - 1], rtol=0, atol=1e-3)
            np.testing.assert_allclose(ms[s].ReadKV(l, True, cur[s] - 1), refs[s].vcache(l)[cur[s] - 1], rtol=0, atol=1e-3)
        refs[s].close()
    dispose(batch, ms)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
def test_greedy_on_the_device(mgr):
    dims, n = synth.TINY_D128, 11
    w = synth.make_weights(dims, seed=21, std=0.05)
    ms = make_members(mgr, dims, w, n, CAP)
    toks = [member_tokens(dims, s) for s in range(n)]
    batch = wide(ms)

    def prime():
        for s in range(n):
            ms[s].Reset()
            for t in toks[s][:ALONE(s)]:
                ms[s].Step(int(t), want_logits=False)

    prime()
    first = [int(toks[s][ALONE(s)]) for s in range(n)]
    got = batch.Greedy(first, 16)
    assert [m.Pos for m in ms] == [ALONE(s) + 16 for s in range(n)]
    prime()
    cur, host = list(first), []
    for _ in range(16):
        _, am = batch.Step(cur, want_logits=False)
        cur = [int(a) for a in am]
        host.append(cur)
    assert got.tolist() == host
    dispose(batch, ms)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
def run_against_oracles(mgr, dims, w, n, alone, steps, cap, scale=5e-4, tok_seed=200, kv_atol=1e-3):
    """Member s is fed alone[s] tokens through its own path, then `steps` wide steps: logits, ArgMax, positions, the last K / V rows."""
    ms = make_members(mgr, dims, w, n, cap)
    refs = [orc.OracleLlama(odesc(dims, cap), w) for _ in range(n)]
    toks = [synth.make_tokens(dims, alone[s] + steps, seed=tok_seed + s) for s in range(n)]
    batch = None
    try:
        for s in range(n):
            for t in toks[s][:alone[s]]:
                ms[s].Step(int(t), want_logits=False)
                refs[s].step(int(t), want_logits=False)
        batch = wide(ms)
        worst = 0.0
        for i in range(steps):
            st = [int(toks[s][alone[s] + i]) for s in range(n)]
            lg, am = batch.Step(st)
            wants = [refs[s].step(st[s]) for s in range(n)]
            worst = max(worst, max(float(np.abs(lg[s] - wants[s]).max()) / logit_tol(wants[s], scale) for s in range(n)))
            check_step(lg, am, wants, scale, f"step {i}")
        print(f"{dims.name} n {n}: worst err / tol = {worst:.3f}")
        assert [m.Pos for m in ms] == [alone[s] + steps for s in range(n)]
        for s in range(n):
            p = alone[s] + steps - 1
            for l in range(dims.L):
                np.testing.assert_allclose(ms[s].ReadKV(l, False, p), refs[s].kcache(l)[p], rtol=0, atol=kv_atol)
                np.testing.assert_allclose(ms[s].ReadKV(l, True, p), refs[s].vcache(l)[p], rtol=0, atol=kv_atol)
    finally:
        dispose(batch, ms)
        for r in refs:
            r.close()


TILE_EDGES = [synth.THIN_E3072, synth.THIN_E4096, replace(synth.THIN_F8192, L=1, name="thin-f8192-1blk"), synth.THIN_F14336]


@pytest.mark.parametrize("dims", TILE_EDGES, ids=lambda d: d.name)
def test_panel_edges(mgr, dims):
    """One block, V = 512, n = 16, 8 steps.  E = 3072: a ragged second x panel (2048 + 1024) under one RMSNorm; E = 4096: two whole
    panels; F = 8192 / 14336: Wdown carries its accumulators across four / seven panels, with the K split among the waves inside each."""
    assert dims.L == 1 and dims.V == 512
    w = synth.make_weights(dims, seed=31)
    run_against_oracles(mgr, dims, w, 16, [1 + s for s in range(16)], 8, 32)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
def test_attention_through_the_second_launch(mgr):
    """Two blocks at the 1B head shape (32 query heads over 8 kv heads of 64, as tests/test_gpu_batch_decode.py::test_attention_at_depth)
    with V = 1024, thin in E and F so that the oracles' 2100 steps stay cheap: members 8 - 11, which the second attention launch serves
    from its own workspace slice, at depths 1, 300, 700 and 1100 (1 to 32 KV slices), members 0 - 7 shallow; 4 steps."""
    b1 = synth.LLAMA_32_1B
    d2 = synth.LlamaDims("thin-1b-heads-2blk", 512, 2, b1.H, b1.Hkv, b1.D, 1024, 1024, True)
    w = synth.make_weights(d2, seed=37)
    run_against_oracles(mgr, d2, w, 12, [2 + s for s in range(8)] + [1, 300, 700, 1100], 4, 1108, tok_seed=300)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", ["real", "f16+4", "f16+5"])
def test_head_at_large_and_ragged_vocabularies(mgr, V):
    """V = 128256 at E = 256 (tied): every workgroup of the lm_head walks one or two groups of 16 tiles and carries each column's best.
    32 n_cu + 4 (tests/test_batch_vocab.py::ragged_vocabs: exactly one wave of the ≤ 8 batch's head has a second unit) ends in a tile
    with 4 live rows; 32 n_cu + 5 is no multiple of 4: the scalar stores."""
    n_cu = int(mgr.info.compute_units)
    dims = vocab_dims(synth.TINY, V_REAL if V == "real" else ragged_vocabs(n_cu)[V], tied=True)
    w = synth.make_weights(dims, seed=21, std=0.05)
    run_against_oracles(mgr, dims, w, 16, [1 + s for s in range(16)], 3, CAP, tok_seed=600)


def test_equal_maxima_the_lowest_index_wins(mgr):
    """Sixteen columns of one wide step at V = 128256, each with its winning row copied to one other row placed by the launch's own
    dealing (tests/test_batch_wide.py::WIDE_TIE_KINDS): the two logits are bit-equal, they are the column's maximum, and the token is
    the lower index."""
    n_cu = int(mgr.info.compute_units)
    dims, wdev, alone, step, winners, sets, expect, wants = wide_ties(n_cu)
    ms = make_members(mgr, dims, wdev, WIDE_MAX, 48)
    batch = None
    try:
        for s in range(WIDE_MAX):
            for t in alone[s]:
                ms[s].Step(t, want_logits=False)
        batch = wide(ms)
        lg, am = batch.Step(step)
        check_step(lg, am, wants, 5e-4, "ties")
        for b in range(WIDE_MAX):
            r, (x, what) = winners[b], sets[b]
            assert bits(lg[b][x]) == bits(lg[b][r]), (b, what, lg[b][x], lg[b][r])
            assert lg[b][r] == lg[b].max(), (b, what)
            assert int(am[b]) == expect[b], (b, what, int(am[b]), expect[b])
    finally:
        dispose(batch, ms)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------
def test_step_topk_rows_are_those_of_the_members_own_logits(mgr):
    """StepTopK at n = 13 (two candidate launches: 8 + 5 rows): each row is bit-identical to nfai_hip_topk of that member's logits."""
    dims, n = synth.TINY_D128, 13
    w = synth.make_weights(dims, seed=21, std=0.05)
    ms = make_members(mgr, dims, w, n, CAP)
    toks = [member_tokens(dims, s) for s in range(n)]
    for s in range(n):
        for t in toks[s][:ALONE(s)]:
            ms[s].Step(int(t), want_logits=False)
    batch = wide(ms)
    for i in range(3):
        ids, probs = batch.StepTopK([int(toks[s][ALONE(s) + i]) for s in range(n)], 0.5, 40)
        assert ids.shape == (n, 40) and probs.shape == (n, 40)
        for s in range(n):
            ids1, probs1 = topk_single(mgr, ms[s].Read(4, dims.V), 0.5, 40)
            assert np.array_equal(ids[s], ids1) and bit_equal(probs[s], probs1), (i, s)
            assert ms[s].Pos == ALONE(s) + i + 1
    dispose(batch, ms)


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------
def test_run_tokens_wide_streams_are_the_members_own(mgr):
    """RunTokens(wide=True, greedy=True) over 12 conversations: each member's stream is the one it yields alone in a wide batch of 1
    (a column does not depend on its neighbours), and the batches re-formed on retirement are wide ones."""
    from nfai_amd.llama_model import LlamaBatch
    dims, n, limit = synth.TINY_D128, 12, 8
    w = synth.make_weights(dims, seed=21, std=0.05)
    ms = make_members(mgr, dims, w, n, CAP)
    lists = [[int(t) for t in synth.make_tokens(dims, 2 + s, seed=900 + s)] for s in range(n)]
    batch = wide(ms)

    def streams_of(pairs, count):
        return [[tk for j, tk in pairs if j == i] for i in range(count)]

    # an EOS that ends some streams early: the third token member 5 yields when nothing ends a stream but the limit
    free = streams_of(list(batch.RunTokens(lists, -1, greedy=True, max_tokens=limit, wide=True)), n)
    assert all(len(v) == limit for v in free)
    k = next(k for k in (3, 2, 1) if free[5][k] not in free[5][1:k])   # (a greedy stream may repeat itself)
    eos = free[5][k]
    made, orig = [], LlamaBatch.__init__

    def spy(self, models, **kw):
        made.append((len(list(models)), kw.get("wide")))
        orig(self, models, **kw)

    for m in ms:
        m.Reset()
    LlamaBatch.__init__ = spy
    try:
        got = streams_of(list(batch.RunTokens(lists, eos, greedy=True, max_tokens=limit, wide=True)), n)
    finally:
        LlamaBatch.__init__ = orig
    batch.Dispose()
    print(f"eos {eos}: stream lengths {[len(v) for v in got]}, re-formed batches (members, wide) {made}")
    assert len(got[5]) == k and made and all(wd is True for _, wd in made), (got[5], made)   # retired early; the smaller batches are wide
    for s in range(n):
        ms[s].Reset()
        one = wide([ms[s]])
        alone = [tk for _, tk in one.RunTokens([lists[s]], eos, greedy=True, max_tokens=limit, wide=True)]
        one.Dispose()
        assert alone == got[s], (s, alone, got[s])
    dispose(None, ms)


# ---- 10 -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(mgr):
    from nfai_amd import _lib
    from nfai_amd._lib import KVCacheFull, NfaiHipError
    from nfai_amd.llama_model import LlamaBatch, LlamaModel, QuantTensor
    dims = synth.TINY_D128
    w = synth.make_weights(dims, seed=21, std=0.05)
    md = synth.make_metadata(dims)
    caps = [40] * 12 + [6] + [40] * 3
    ms = make_members(mgr, dims, w, 16, caps)

    def refused(models, code, pattern):
        with pytest.raises(NfaiHipError, match=pattern) as e:
            LlamaBatch(models, wide=True)
        assert e.value.code == code, e.value.args

    # a quantised member: the tensor is named
    wq = {name: a if a.ndim == 1 else QuantTensor(orc.quantize_q4k(a.astype(np.float32)), _lib.Q4_K, a.shape) for name, a in w.items()}
    dd = dict(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, eps=1e-5, rope_dims=dims.D, rope_base=500000.0)
    q = LlamaModel(mgr, md, wq, 8, dims=dd)
    refused([q], _lib.ERR_UNSUPPORTED, "member 0: token_embd of block 0 has ggml type 12")
    # mixed shapes: a model of other widths does not read member 0's tensors
    other = LlamaModel(mgr, synth.make_metadata(synth.TINY), synth.make_weights(synth.TINY, seed=21, std=0.05), 8)
    refused(ms[:9] + [other], _lib.ERR_UNSUPPORTED, "member 9")
    # mixed KV element types, a duplicate
    k16 = LlamaModel(mgr, md, w, 8, share_from=ms[0], kv_f16=True)
    refused(ms[:10] + [k16], _lib.ERR_UNSUPPORTED, "member 10")
    refused(ms[:12] + [ms[3]], _lib.ERR_INVALID, "member 12")
    # the narrow creators keep their limit
    with pytest.raises(NfaiHipError, match="a batch holds 1 to 8 models"):
        LlamaBatch(ms[:9])
    # KV_FULL names member 12 before anything is enqueued: nothing moves
    batch = wide(ms)
    toks = [member_tokens(dims, s) for s in range(16)]
    for i in range(6):
        batch.Step([int(toks[s][i]) for s in range(16)], want_logits=False)
    assert [m.Pos for m in ms] == [6] * 16
    rows = [ms[s].ReadKV(0, False, 5).copy() for s in (0, 12, 15)]
    with pytest.raises(KVCacheFull, match="member 12"):
        batch.Step([1] * 16)
    with pytest.raises(KVCacheFull, match="member 12"):
        batch.Greedy([1] * 16, 1)
    with pytest.raises(KVCacheFull, match="member 12"):
        batch.StepTopK([1] * 16)
    assert [m.Pos for m in ms] == [6] * 16
    for r, s in zip(rows, (0, 12, 15)):
        np.testing.assert_array_equal(ms[s].ReadKV(0, False, 5), r)
    ms[12].SetPos(2)
    batch.Step([int(toks[s][6 if s != 12 else 2]) for s in range(16)], want_logits=False)
    assert [m.Pos for m in ms] == [7] * 12 + [3] + [7] * 3
    # a member destroyed while the batch holds it: an error, not a crash
    ms[13].Dispose()
    with pytest.raises(NfaiHipError, match="member 13"):
        batch.Step([1] * 16)
    batch.Dispose()
    for m in [q, other, k16] + [m for i, m in enumerate(ms) if i != 13][::-1]:
        m.Dispose()
