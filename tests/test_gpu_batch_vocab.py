"""The lm_head launch of the batched decode and of the window (k_bgemv / k_bgemv_kq in GEMV_PLAIN: logits, per-column ArgMax merged
over lanes, waves and workgroups, win_tail) at the vocabulary of the real models, V = 128256, and on EQUAL maxima.

Why: with V <= 32 n_cu (fp16) / 16 n_cu (K-quant) every wave / workgroup of that launch owns ONE row unit, so the carry of the best
(value, index) from one unit to the next, the ragged deal and the odd tails of the weight ping-pong do not execute; tests/
test_gpu_batch_decode.py, test_gpu_batch_quant.py and test_gpu_window_decode.py stop at V = 4096.  And on random weights no two
logits are equal, so nothing there depends on the rule "the LOWEST index among equal maxima" (SamplingUtils.cs:55-56).

1. every logit of every column against one CPU oracle per sequence (the K-quant mix: on the dequantised weights) at V = 128256
   (E = 256 and 512), at vocabularies derived from the CU count in which exactly one wave / workgroup has a second unit
   (tests/test_batch_vocab.py::ragged_vocabs; 32 n_cu + 5 also ends in a group with one live row) and on one Llama-3.2-3B block with
   V = 32 n_cu + 2064; batches of 2, 3 and 8 (the three compiled widths) at staggered positions; tokens 0, V - 1, V - 16 and one id
   above 65536 go through the embedding and are checked through the K / V rows; a window of 8 and a device-side Greedy at V = 128256.
2. eight columns whose maximum is shared by two rows with bit-identical weights, the copy placed by the kernel's own row dealing
   (tests/test_batch_vocab.py): the logits are bit-equal, they are the maximum, and the token is the lower index, at n = 8 and n = 3.
3. a window over a greedy chain of such columns: Verify keeps a draft that is the lower index and stops at one that is the higher
   index of the same maximum, exactly where the plain one-token loop goes.

Tolerances are the project's: 5e-4 * max(1, max|logit|) with an fp32 KV cache, 2e-2 with an fp16 one, K / V rows 1e-3 / 2e-2
(tests/test_gpu_batch_decode.py).  Every test prints V, E, n, the CU count, the units per wave / workgroup and its worst error / bar."""
from dataclasses import replace

import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth

from test_batch_vocab import CAP, Deal, V_REAL, batch_ties, chain_ties, chain_wrong, odesc, ragged_vocabs, vocab_dims, weights
from test_gpu_batch_decode import check_step, dispose, logit_tol
from test_gpu_batch_decode import make_members as make_members_f16
from test_gpu_batch_quant import ddict
from test_gpu_batch_quant import make_members as make_members_q

pytestmark = pytest.mark.gpu

KINDS = [pytest.param(False, id="f16"), pytest.param(True, id="mix")]


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


@pytest.fixture(scope="module")
def n_cu(mgr):
    n = int(mgr.info.compute_units)
    assert n > 64, n   # (the final merge reads the partials of more than 64 workgroups: a lane has more than one)
    return n


def make_members(mgr, dims, wdev, quant, n, cap, **kw):
    return (make_members_q if quant else make_members_f16)(mgr, dims, wdev, n, cap, **kw)


def make_model(mgr, dims, wdev, quant, cap=CAP, **kw):
    from nfai_amd.llama_model import LlamaModel
    if quant:
        kw.setdefault("dims", ddict(dims))
    return LlamaModel(mgr, synth.make_metadata(dims), wdev, cap, **kw)


def describe(dims, quant, n, deal):
    lo, hi, many = deal.passes()
    per = "units per workgroup" if quant else "groups per wave"
    return f"V {dims.V} E {dims.E} n {n} CUs {deal.n_cu} {'mix' if quant else 'f16'} {per} {lo}..{hi} ({many} with {hi})"


def edge_tokens(V):
    """Ids the embedding kernels must reach in a table of V rows: the first and the last row, the last 16-row tile's first row, and a
    row whose index needs more than 16 bits."""
    return [0, V - 1, V - 16, 70001 if V > 70001 else V // 2 + 1]


def worst_ratio(lg, wants, scale):
    return max(float(np.abs(lg[s] - w).max()) / logit_tol(w, scale) for s, w in enumerate(wants))


def run_batch(mgr, n_cu, dims, quant, n, kv_f16=False, steps=7, seed=21, std=0.05, cap=CAP):
    """Member s is fed 1 + 2 s tokens alone, then `steps` batch steps: every logit, the ArgMax, and the K / V rows of every batch position."""
    from nfai_amd.llama_model import LlamaBatch
    deal = Deal(dims.V, n_cu, quant)
    assert deal.nonvacuous(), (dims.V, n_cu)   # some wave (fp16) / workgroup (K-quant) of the lm_head launch owns more than one unit
    wdev, wref = weights(dims, quant, seed, std)
    ms = make_members(mgr, dims, wdev, quant, n, cap, kv_f16=kv_f16)
    refs = [orc.OracleLlama(odesc(dims, cap), wref) for _ in range(n)]
    toks = [[int(t) for t in synth.make_tokens(dims, 1 + 2 * s + steps, seed=600 + s)] for s in range(n)]
    e = edge_tokens(dims.V)
    toks[0][1], toks[1][3], toks[0][2], toks[1][4] = e   # the first two batch steps of members 0 and 1
    scale, atol = (2e-2, 2e-2) if kv_f16 else (5e-4, 1e-3)
    batch = None
    try:
        for s in range(n):
            for t in toks[s][:1 + 2 * s]:
                ms[s].Step(t, want_logits=False)
                refs[s].step(t, want_logits=False)
        batch = LlamaBatch(ms, quantized=quant)
        worst = 0.0
        for i in range(steps):
            st = [toks[s][1 + 2 * s + i] for s in range(n)]
            lg, am = batch.Step(st)
            wants = [refs[s].step(st[s]) for s in range(n)]
            worst = max(worst, worst_ratio(lg, wants, scale))
            check_step(lg, am, wants, scale, f"step {i}")
        print(f"{describe(dims, quant, n, deal)} kv_f16 {kv_f16}: worst err / tol = {worst:.3f}")
        for s in range(n):
            assert ms[s].Pos == 1 + 2 * s + steps
            for l in range(dims.L):
                for p in range(1 + 2 * s, 1 + 2 * s + steps):
                    np.testing.assert_allclose(ms[s].ReadKV(l, False, p), refs[s].kcache(l)[p], rtol=0, atol=atol)
                    np.testing.assert_allclose(ms[s].ReadKV(l, True, p), refs[s].vcache(l)[p], rtol=0, atol=atol)
    finally:
        dispose(batch, ms)
        for r in refs:
            r.close()


# ---- 1: every logit ---------------------------------------------------------------------------------------------------------------------
def real_dims(E):
    return vocab_dims(synth.TINY if E == 256 else synth.TINY_D128, V_REAL, tied=True)


@pytest.mark.parametrize("E,n,kv_f16", [(256, 2, False), (256, 3, False), (256, 8, False), (512, 8, False), (512, 2, False), (512, 3, True)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("quant", KINDS)
def test_batch_at_the_real_vocabulary(mgr, n_cu, quant, E, n, kv_f16):
    """V = 128256 (tied: the table the embedding reads is the head).  fp16: each wave walks 15 or 16 row groups on 256 CUs; B = 2 and
    4 take two 512-element chunks per step, B = 8 one, so their ping-pong tails differ.  K-quant: 31 or 32 units per workgroup; E = 512
    gives the launch two waves, so columns are finished by different waves."""
    run_batch(mgr, n_cu, real_dims(E), quant, n, kv_f16)


@pytest.mark.parametrize("n", [2, 3, 8])
@pytest.mark.parametrize("which", ["f16+4", "f16+5", "mix+16"])
def test_batch_at_the_first_ragged_vocabularies(mgr, n_cu, which, n):
    """32 n_cu + 4: one wave has two groups, every other one.  32 n_cu + 5: two waves have two, and the last group has ONE live row
    (the three others are clamped loads whose sums are dropped): a vocabulary that is no multiple of 4 is admitted and exact.
    16 n_cu + 16 (K-quant): one workgroup has two units."""
    quant = which.startswith("mix")
    run_batch(mgr, n_cu, vocab_dims(synth.TINY, ragged_vocabs(n_cu)[which]), quant, n)


@pytest.mark.parametrize("n", [8, 3])
@pytest.mark.parametrize("quant", KINDS)
def test_wide_row_block_with_several_units_per_wave(mgr, n_cu, quant, n):
    """tests/test_gpu_batch_decode.py::test_full_width_block's construction (one Llama-3.2-3B block, weights seed 31) with
    V = 32 n_cu + 2064: one or two groups per wave (two or three units per workgroup) together with several K steps per group;
    E = 3072 gives the K-quant launch six waves, so columns 6 and 7 share waves with 0 and 1."""
    V = ragged_vocabs(n_cu)["mix-wide" if quant else "f16-wide"]
    d1 = replace(synth.LLAMA_32_3B, L=1, V=V, name=f"{synth.LLAMA_32_3B.name}-1blk-v{V}")
    run_batch(mgr, n_cu, d1, quant, n, steps=6, seed=31, std=0.02, cap=32)


@pytest.mark.parametrize("quant", KINDS)
def test_window_at_the_real_vocabulary(mgr, n_cu, quant):
    """5 plain steps, a window of 8, a plain step behind it (tests/test_gpu_window_decode.py::test_window_steps_match_the_oracle)."""
    from nfai_amd.llama_model import LlamaWindow
    dims = real_dims(256)
    deal = Deal(dims.V, n_cu, quant)
    assert deal.nonvacuous()
    wdev, wref = weights(dims, quant)
    m = make_model(mgr, dims, wdev, quant)
    win = LlamaWindow(m, 8, quantized=quant)
    ref = orc.OracleLlama(odesc(dims, CAP), wref)
    toks = [int(t) for t in synth.make_tokens(dims, 14, seed=131)]
    toks[5], toks[6], toks[12], toks[13] = edge_tokens(dims.V)
    try:
        for t in toks[:5]:
            m.Step(t, want_logits=False)
            ref.step(t, want_logits=False)
        lg, am = win.Step(toks[5:13])
        assert lg.shape == (8, dims.V) and m.Pos == 13
        wants = [ref.step(t) for t in toks[5:13]]
        check_step(lg, am, wants, 5e-4, "window")
        worst = worst_ratio(lg, wants, 5e-4)
        for l in range(dims.L):
            for p in range(5, 13):
                np.testing.assert_allclose(m.ReadKV(l, False, p), ref.kcache(l)[p], rtol=0, atol=1e-3)
                np.testing.assert_allclose(m.ReadKV(l, True, p), ref.vcache(l)[p], rtol=0, atol=1e-3)
        lg1, am1 = m.Step(toks[13])
        want = ref.step(toks[13])
        check_step(lg1[None], [am1], [want], 5e-4, "plain step behind the window")
        worst = max(worst, worst_ratio(lg1[None], [want], 5e-4))
        assert m.Pos == 14
        print(f"window of 8: {describe(dims, quant, 8, deal)}: worst err / tol = {worst:.3f}")
    finally:
        win.Dispose()
        m.Dispose()
        ref.close()


@pytest.mark.parametrize("n", [8, 3])
@pytest.mark.parametrize("quant", KINDS)
def test_greedy_on_the_device_at_the_real_vocabulary(mgr, n_cu, quant, n):
    """12 steps with the ArgMax fed back on the device equal 12 host-driven steps (tests/test_gpu_batch_decode.py::
    test_greedy_on_the_device): the ticket of the merge is re-armed across launches at the full grid."""
    from nfai_amd.llama_model import LlamaBatch
    dims = real_dims(256)
    assert Deal(dims.V, n_cu, quant).nonvacuous()
    wdev, _ = weights(dims, quant)
    ms = make_members(mgr, dims, wdev, quant, n, CAP)
    toks = [[int(t) for t in synth.make_tokens(dims, 2 + 2 * s, seed=700 + s)] for s in range(n)]
    batch = LlamaBatch(ms, quantized=quant)

    def prime():
        for s in range(n):
            ms[s].Reset()
            for t in toks[s][:-1]:
                ms[s].Step(t, want_logits=False)

    try:
        prime()
        first = [toks[s][-1] for s in range(n)]
        got = batch.Greedy(first, 12)
        assert [m.Pos for m in ms] == [1 + 2 * s + 12 for s in range(n)]
        prime()
        cur, host = list(first), []
        for _ in range(12):
            _, am = batch.Step(cur, want_logits=False)
            cur = [int(a) for a in am]
            host.append(cur)
        assert got.tolist() == host
        assert len({t for row in host for t in row}) > n   # (not one repeated token)
    finally:
        dispose(batch, ms)


# ---- 2: equal maxima ----------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("quant", KINDS)
def test_equal_maxima_the_lowest_index_wins(mgr, n_cu, quant):
    """Eight columns of one batch step at V = 128256, each with its winning row copied to one other row placed by the launch's own
    dealing (tests/test_batch_vocab.py::TIE_KINDS: the same unit, a later and an earlier pass of the same lane, another wave, other
    workgroups on both sides, row 0, row V - 1).  Then the first three members as a batch of 3: a column's choice does not move
    with the batch size."""
    from nfai_amd.llama_model import LlamaBatch
    dims, wdev, wref, alone, step, winners, sets, expect, wants = batch_ties(quant, n_cu)
    deal = Deal(dims.V, n_cu, quant)
    assert deal.nonvacuous()
    ms = make_members(mgr, dims, wdev, quant, 8, CAP)
    batch, seen = None, {}
    try:
        for n in (8, 3):
            for s in range(n):
                ms[s].Reset()
                for t in alone[s]:
                    ms[s].Step(t, want_logits=False)
            batch = LlamaBatch(ms[:n], quantized=quant)
            lg, am = batch.Step(step[:n])
            batch.Dispose()
            batch = None
            check_step(lg, am, wants[:n], 5e-4, f"n = {n}")
            print(f"ties: {describe(dims, quant, n, deal)}: worst err / tol = {worst_ratio(lg, wants[:n], 5e-4):.3f}")
            for b in range(n):
                r, (x, what) = winners[b], sets[b]
                assert bits(lg[b][x]) == bits(lg[b][r]), (n, b, what, lg[b][x], lg[b][r])        # bit-identical weights, bit-equal logits
                assert lg[b][r] == lg[b].max(), (n, b, what)                                      # ... which are the column's maximum
                assert int(am[b]) == expect[b], (n, b, what, int(am[b]), expect[b], deal.place(r), deal.place(x))
            seen[n] = (lg, am)
        np.testing.assert_array_equal(seen[3][1], seen[8][1][:3])
        np.testing.assert_array_equal(bits(seen[3][0]), bits(seen[8][0][:3]))
    finally:
        dispose(batch, ms)


# ---- 3: the window's accept rule on a tie -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quant,V", [(False, 512), (False, V_REAL), (True, V_REAL)], ids=["f16-512", "f16-128256", "mix-128256"])
def test_verify_accepts_the_lower_and_rejects_the_higher_index_of_a_tie(mgr, n_cu, quant, V):
    """A greedy chain t0 -> a_0 -> ... -> a_7 in which every column's maximum is shared by two rows and a_i is the lower one
    (tests/test_batch_vocab.py::chain_ties).  All seven right drafts are kept; a draft replaced by the HIGHER row of its column's tie
    (the same logit bit for bit, the wrong index) ends the window there; the plain loop emits the same eight tokens."""
    from nfai_amd.llama_model import LlamaWindow
    dims, wdev, wref, prompt, t0, winners, sets, a = chain_ties(quant, V, n_cu)
    deal = Deal(dims.V, n_cu, quant)
    assert deal.nonvacuous() or V != V_REAL
    m = make_model(mgr, dims, wdev, quant)
    twin = make_model(mgr, dims, wdev, quant, share_from=m)
    win = LlamaWindow(m, 8, quantized=quant)
    p = len(prompt)

    def bring(mdl):
        mdl.Reset()
        for t in prompt:
            mdl.Step(t, want_logits=False)

    try:
        bring(m)
        lg, out = win.Verify(t0, a[:7], want_logits=True)
        assert [int(t) for t in out] == a, (out, a)
        assert m.Pos == p + 8
        for i in range(8):
            r, (x, what) = winners[i], sets[i]
            assert bits(lg[i][x]) == bits(lg[i][r]) and lg[i][r] == lg[i].max(), (i, what)
        for i in (1, 4, 6):
            bring(m)
            draft = list(a[:7])
            draft[i] = chain_wrong(winners, sets, i)
            assert draft[i] != a[i] and bits(lg[i][draft[i]]) == bits(lg[i][a[i]])
            _, out = win.Verify(t0, draft)
            assert [int(t) for t in out] == a[:i + 1], (i, out, a)
            assert m.Pos == p + i + 1
        bring(twin)
        tok, plain = t0, []
        for _ in range(8):
            _, tok = twin.Step(tok, want_logits=False)
            plain.append(int(tok))
        assert plain == a, (plain, a)
        print(f"accept rule: {describe(dims, quant, 8, deal)}: chain {a}")
    finally:
        win.Dispose()
        twin.Dispose()
        m.Dispose()
