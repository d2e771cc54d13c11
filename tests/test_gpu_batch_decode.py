"""The batched decode step (nfai_hip_llama_batch_*, kernels_gemv_batch.hip) on the GPU: n models over one set of fp16 weights
advance one token each per step, every member at its own position in its own KV cache, against one CPU oracle per sequence.

Tolerance: the decode path's own, 5e-4 * max(1, max|logit|) (tests/test_gpu_model.py::logit_tol: fp16 weights, fp32 activations and
sums, the same class of arithmetic); 2e-2 with an fp16 KV cache (test_kv_f16_option).  The returned argmax is always the first
index of the maximum of the returned logits; in the fp32-cache runs of test 1 it also equals the oracle's argmax wherever the
oracle's two largest logits are more than twice the tolerance apart — a rule that depends on the oracle alone and may leave out
at most ONE of a member's 24 batch steps (asserted)."""
from dataclasses import replace

import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth

pytestmark = pytest.mark.gpu

CAP = 96


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


def odesc(d, C):
    return orc.LlamaDesc(E=d.E, L=d.L, H=d.H, Hkv=d.Hkv, D=d.D, F=d.F, V=d.V, C=C)


def logit_tol(want, scale=5e-4):
    return scale * max(1.0, float(np.abs(want).max()))


def seq_tokens(dims, s):
    return synth.make_tokens(dims, 29 + 7 * s, seed=100 + s)


def make_members(mgr, dims, w, n, caps, **kw):
    """n models over one copy of the weights: member 0 is the donor, the others share its tensors."""
    from nfai_amd.llama_model import LlamaModel
    md = synth.make_metadata(dims)
    caps = [caps] * n if isinstance(caps, int) else list(caps)
    ms = [LlamaModel(mgr, md, w, caps[0], **kw)]
    for i in range(1, n):
        ms.append(LlamaModel(mgr, md, w, caps[i], share_from=ms[0], **kw))
    return ms


def check_step(lg, am, wants, scale, where, oracle_argmax=False, excluded=None):
    """Every member of one batch step against its oracle logits `wants`."""
    for s, want in enumerate(wants):
        tol = logit_tol(want, scale)
        err = float(np.abs(lg[s] - want).max())
        print(f"{where} member {s}: max|dlogit| {err:.3e} tol {tol:.3e}")
        assert err <= tol, (where, s, err, tol)
        assert int(am[s]) == int(np.argmax(lg[s])), (where, s, int(am[s]), int(np.argmax(lg[s])))   # first index of the maximum
        if oracle_argmax:
            top2 = np.partition(want, -2)[-2:]
            if float(top2[1] - top2[0]) > 2 * tol:
                assert int(am[s]) == orc.argmax(want), (where, s)
            else:
                excluded[s] += 1


def dispose(batch, members):
    if batch is not None:
        batch.Dispose()
    for m in reversed(members):   # the donor last
        m.Dispose()


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv_f16", [False, True], ids=["kv-f32", "kv-f16"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("dims", [synth.TINY, synth.TINY_D128], ids=lambda d: d.name)
def test_staggered_batch_matches_the_oracle(mgr, dims, n, kv_f16):
    """Member s takes its first 5 + 7 s tokens alone through _decode_step (positions 5 ... 54), then 24 batch steps."""
    from nfai_amd.llama_model import LlamaBatch
    w = synth.make_weights(dims, seed=21, std=0.05)
    ms = make_members(mgr, dims, w, n, CAP, kv_f16=kv_f16)
    refs = [orc.OracleLlama(odesc(dims, CAP), w) for _ in range(n)]
    toks = [seq_tokens(dims, s) for s in range(n)]
    scale = 2e-2 if kv_f16 else 5e-4
    for s in range(n):
        for t in toks[s][:5 + 7 * s]:
            ms[s].Step(int(t), want_logits=False)
            refs[s].step(int(t))
    batch = LlamaBatch(ms)
    excluded = [0] * n
    for i in range(24):
        step_toks = [int(toks[s][5 + 7 * s + i]) for s in range(n)]
        lg, am = batch.Step(step_toks)
        wants = [refs[s].step(step_toks[s]) for s in range(n)]
        check_step(lg, am, wants, scale, f"step {i}", oracle_argmax=not kv_f16, excluded=excluded)
    assert max(excluded) <= 1, excluded   # the near-tie rule may leave out at most one of a member's 24 steps
    for s in range(n):
        last = 5 + 7 * s + 24
        assert ms[s].Pos == last
        atol = 1e-3 if not kv_f16 else 2e-2   # fp32 cache: test_decode_matches_oracle's bound; fp16 cache: its own stated scale
        np.testing.assert_allclose(ms[s].Read(0, dims.E), refs[s].hidden(), rtol=0, atol=atol)
        for l in range(dims.L):
            np.testing.assert_allclose(ms[s].ReadKV(l, False, last - 1), refs[s].kcache(l)[last - 1], rtol=0, atol=atol)
            np.testing.assert_allclose(ms[s].ReadKV(l, True, last - 1), refs[s].vcache(l)[last - 1], rtol=0, atol=atol)
    dispose(batch, ms)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [synth.TINY, synth.TINY_D128], ids=lambda d: d.name)
def test_a_column_does_not_depend_on_its_neighbours(mgr, dims):
    """The same member state and token (a) in column 0 of a batch of 2 and (b) in column 7 of a batch of 8 whose other members hold
    other sequences at other positions: BIT-IDENTICAL logits.  The B = 2, 4 and 8 kernels share one summation order: a (row,
    column) sum is one fp32 chain per lane over k = 512 c + 8 lane .. + 7, c ascending, then the wave sum; neither the batch size,
    nor the K tiling, nor the grid, nor the other columns enter it, and the attention works per sequence (its slicing depends on
    that sequence's depth alone).  Within one batch size, permuting the members changes no member's logits by a bit either."""
    from nfai_amd.llama_model import LlamaBatch
    w = synth.make_weights(dims, seed=21, std=0.05)
    ms = make_members(mgr, dims, w, 8, CAP)
    toks = [seq_tokens(dims, s) for s in range(8)]

    def bring(s, count):
        ms[s].Reset()
        for t in toks[s][:count]:
            ms[s].Step(int(t), want_logits=False)

    probe, depth, tok = 3, 17, int(toks[3][17])
    # (a) column 0 of a batch of 2
    bring(probe, depth)
    bring(0, 9)
    b2 = LlamaBatch([ms[probe], ms[0]])
    lg_a, am_a = b2.Step([tok, int(toks[0][9])])
    b2.Dispose()
    # (b) column 7 of a batch of 8, other sequences at other positions
    for s in range(8):
        bring(s, depth if s == probe else 4 + 5 * s)
    order = [s for s in range(8) if s != probe] + [probe]
    b8 = LlamaBatch([ms[s] for s in order])
    lg_b, am_b = b8.Step([tok if s == probe else int(toks[s][4 + 5 * s]) for s in order])
    b8.Dispose()
    np.testing.assert_array_equal(lg_a[0], lg_b[7])
    assert am_a[0] == am_b[7]
    # permutation within one batch size
    first = {s: lg_b[i].copy() for i, s in enumerate(order)}
    for s in range(8):
        bring(s, depth if s == probe else 4 + 5 * s)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    bp = LlamaBatch([ms[s] for s in perm])
    lg_p, _ = bp.Step([tok if s == probe else int(toks[s][4 + 5 * s]) for s in perm])
    for i, s in enumerate(perm):
        np.testing.assert_array_equal(lg_p[i], first[s])
    dispose(bp, ms)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def test_batch_and_single_steps_interleave(mgr):
    from nfai_amd.llama_model import LlamaBatch
    dims, n = synth.TINY_D128, 3
    w = synth.make_weights(dims, seed=21, std=0.05)
    ms = make_members(mgr, dims, w, n, CAP)
    refs = [orc.OracleLlama(odesc(dims, CAP), w) for _ in range(n)]
    toks = [seq_tokens(dims, s) for s in range(n)]
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
        for t in toks[s][:2 + 3 * s]:
            ms[s].Step(int(t), want_logits=False)
            refs[s].step(int(t))
            cur[s] += 1
    batch = LlamaBatch(ms)
    batch_step(batch, "batch 0")
    lg, am = ms[1].Step(int(toks[1][cur[1]]))   # one member alone
    want = refs[1].step(int(toks[1][cur[1]]))
    cur[1] += 1
    assert np.abs(lg - want).max() <= logit_tol(want)
    batch_step(batch, "batch 1")
    batch_step(batch, "batch 2")
    # member 2 goes back by 3 and the batch re-feeds those tokens
    back = cur[2] - 3
    ms[2].SetPos(back)
    refs[2] = orc.OracleLlama(odesc(dims, CAP), w)
    for t in toks[2][:back]:
        refs[2].step(int(t))
    cur[2] = back
    for i in range(3):
        batch_step(batch, f"re-feed {i}")
    assert [m.Pos for m in ms] == cur
    dispose(batch, ms)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 5])
def test_greedy_on_the_device(mgr, n):
    from nfai_amd.llama_model import LlamaBatch
    dims = synth.TINY_D128
    w = synth.make_weights(dims, seed=21, std=0.05)
    ms = make_members(mgr, dims, w, n, CAP)
    toks = [seq_tokens(dims, s) for s in range(n)]
    batch = LlamaBatch(ms)

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


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 3])
@pytest.mark.parametrize("dims", [synth.LLAMA_32_1B, synth.LLAMA_32_3B, synth.LLAMA_31_8B], ids=lambda d: d.name)
def test_full_width_block(mgr, dims, n):
    """One block at the published widths (test_one_full_width_block's construction, V = 4096): K = 8192 and 14336 at B = 8 do not fit
    the LDS in one piece (the K tiles of Wdown), and the head runs at full row length."""
    from nfai_amd.llama_model import LlamaBatch
    d1 = replace(dims, L=1, V=4096, name=dims.name + "-1blk")
    w = synth.make_weights(d1, seed=31)
    C = 32
    ms = make_members(mgr, d1, w, n, C)
    refs = [orc.OracleLlama(odesc(d1, C), w) for _ in range(n)]
    toks = [synth.make_tokens(d1, 32, seed=200 + s) for s in range(n)]
    for s in range(n):
        for t in toks[s][:1 + 2 * s]:
            ms[s].Step(int(t), want_logits=False)
            refs[s].step(int(t))
    batch = LlamaBatch(ms)
    for i in range(12):
        st = [int(toks[s][1 + 2 * s + i]) for s in range(n)]
        lg, am = batch.Step(st)
        check_step(lg, am, [refs[s].step(st[s]) for s in range(n)], 5e-4, f"step {i}")
    dispose(batch, ms)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,positions,caps", [(synth.LLAMA_32_1B, [1, 300, 700, 1100], 1108), (synth.LLAMA_32_3B, [5, 400, 700], 2304)],
                         ids=["1b-to-1100", "3b-capacity-2304"])
def test_attention_at_depth(mgr, dims, positions, caps):
    """test_attention_slices_full_width's construction (two blocks at the published head shape, V = 1024, weights seed 37): members
    brought alone to very different depths, then 4 batch steps — 1 to 32 KV slices live in one attention launch.  A capacity above
    2048 selects the one-pass form of the batch-1 attention for the members' own steps; the batch must agree with it too."""
    from nfai_amd.llama_model import LlamaBatch
    n = len(positions)
    d2 = replace(dims, L=2, V=1024, name=dims.name + "-2blk")
    w = synth.make_weights(d2, seed=37)
    ms = make_members(mgr, d2, w, n, caps)
    refs = [orc.OracleLlama(odesc(d2, caps), w) for _ in range(n)]
    toks = [synth.make_tokens(d2, positions[s] + 4, seed=300 + s) for s in range(n)]
    for s in range(n):
        for t in toks[s][:positions[s]]:
            ms[s].Step(int(t), want_logits=False)
            refs[s].step(int(t))
    batch = LlamaBatch(ms)
    for i in range(4):
        st = [int(toks[s][positions[s] + i]) for s in range(n)]
        lg, am = batch.Step(st)
        check_step(lg, am, [refs[s].step(st[s]) for s in range(n)], 5e-4, f"step {i}")
    assert [m.Pos for m in ms] == [p + 4 for p in positions]
    dispose(batch, ms)


def test_members_of_one_batch_may_have_different_capacities(mgr):
    from nfai_amd.llama_model import LlamaBatch
    dims, caps = synth.TINY_D128, [40, 96, 64]
    w = synth.make_weights(dims, seed=21, std=0.05)
    ms = make_members(mgr, dims, w, 3, caps)
    refs = [orc.OracleLlama(odesc(dims, caps[s]), w) for s in range(3)]
    toks = [seq_tokens(dims, s) for s in range(3)]
    batch = LlamaBatch(ms)
    for i in range(20):
        st = [int(toks[s][i]) for s in range(3)]
        lg, am = batch.Step(st)
        check_step(lg, am, [refs[s].step(st[s]) for s in range(3)], 5e-4, f"step {i}")
    dispose(batch, ms)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(mgr):
    from nfai_amd import _lib
    from nfai_amd._lib import KVCacheFull, NfaiHipError
    from nfai_amd.llama_model import LlamaBatch, LlamaModel, QuantTensor
    dims = synth.TINY_D128
    w = synth.make_weights(dims, seed=21, std=0.05)
    md = synth.make_metadata(dims)
    ms = make_members(mgr, dims, w, 2, 8)

    def refused(models, code, pattern):
        with pytest.raises(NfaiHipError, match=pattern) as e:
            LlamaBatch(models)
        assert e.value.code == code, e.value.args

    # K-quant weights
    wq = {}
    for name, a in w.items():
        wq[name] = a if a.ndim == 1 else QuantTensor(orc.quantize_q4k(a.astype(np.float32)), _lib.Q4_K, a.shape)
    dd = dict(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, eps=1e-5, rope_dims=dims.D, rope_base=500000.0)
    q = LlamaModel(mgr, md, wq, 8, dims=dd)
    refused([q], _lib.ERR_UNSUPPORTED, "member 0")
    # a stage of a two-stage model
    stage = LlamaModel(mgr, md, w, 8, layer_range=(0, 2))
    refused([stage], _lib.ERR_UNSUPPORTED, "pipeline stage")
    # two models with their own separate weights
    own = LlamaModel(mgr, md, w, 8)
    refused([ms[0], own], _lib.ERR_UNSUPPORTED, "member 1")
    # mixed KV element types
    k16 = LlamaModel(mgr, md, w, 8, share_from=ms[0], kv_f16=True)
    refused([ms[0], k16], _lib.ERR_UNSUPPORTED, "member 1")
    # a duplicate member
    refused([ms[0], ms[1], ms[0]], _lib.ERR_INVALID, "member 2")
    # a valid batch on the same context still works
    batch = LlamaBatch(ms)
    refs = [orc.OracleLlama(odesc(dims, 8), w) for _ in range(2)]
    toks = [seq_tokens(dims, s) for s in range(2)]
    ms[1].Step(int(toks[1][0]), want_logits=False)
    refs[1].step(int(toks[1][0]))
    for i in range(7):   # member 1 reaches its capacity of 8 after 7 batch steps
        st = [int(toks[0][i]), int(toks[1][1 + i])]
        lg, am = batch.Step(st)
        check_step(lg, am, [refs[s].step(st[s]) for s in range(2)], 5e-4, f"step {i}")
    assert [m.Pos for m in ms] == [7, 8]
    with pytest.raises(KVCacheFull, match="member 1"):
        batch.Step([1, 2])
    assert [m.Pos for m in ms] == [7, 8]   # no member moved
    with pytest.raises(KVCacheFull):
        batch.Greedy([1, 2], 1)
    assert [m.Pos for m in ms] == [7, 8]
    ms[1].SetPos(3)
    refs[1] = orc.OracleLlama(odesc(dims, 8), w)
    for t in toks[1][:3]:
        refs[1].step(int(t))
    st = [int(toks[0][7]), int(toks[1][3])]
    lg, am = batch.Step(st)
    check_step(lg, am, [refs[s].step(st[s]) for s in range(2)], 5e-4, "after set_pos")
    assert [m.Pos for m in ms] == [8, 4]
    # a member destroyed while the batch holds it: an error, not a crash
    ms[1].Dispose()
    with pytest.raises(NfaiHipError, match="member 1"):
        batch.Step([1, 2])
    batch.Dispose()
    for m in (q, stage, own, k16, ms[0]):
        m.Dispose()


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------
def test_holding_a_model_in_a_batch_changes_nothing_about_its_own_path(mgr):
    from nfai_amd.llama_model import LlamaBatch
    dims = synth.TINY_D128
    w = synth.make_weights(dims, seed=21, std=0.05)
    ms = make_members(mgr, dims, w, 2, 48)
    toks = synth.make_tokens(dims, 30, seed=77)
    for i, t in enumerate(toks):
        if i == 11:
            LlamaBatch([ms[1]]).Dispose()   # created and destroyed without a step
        la, aa = ms[0].Step(int(t))
        if i == 19:
            b = LlamaBatch([ms[1]])         # ... and held across a step of the member's own path
        lb, ab = ms[1].Step(int(t))
        if i == 19:
            b.Dispose()
        np.testing.assert_array_equal(la, lb)
        assert aa == ab
    dispose(None, ms)
