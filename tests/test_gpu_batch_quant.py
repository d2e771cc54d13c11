"""The batched decode step on Q4_K / Q6_K members (nfai_hip_llama_batch_create_ex with NFAI_BATCH_QUANT, kernels_gemv_batch_kqm.hip)
on the GPU: n models over one set of quantised weights advance one token each per step, every member at its own position in its own
KV cache, against one CPU oracle per sequence on the DEQUANTISED weights.  The mirror of tests/test_gpu_batch_decode.py.

Tensor mix ("q4_k_m" below, so that both the uniform and the split q|k|v launch run): Q6_K for token_embd, output and for attn_v /
ffn_down of blocks with an even index; Q4_K everywhere else.  "all_q4_k": every matrix Q4_K.

Tolerance: 5e-4 * max(1, max|logit|), what the project states for the K-quant model path
(tests/test_gpu_kquant.py::test_qkv_rope_kquant_mixed_v) and for the fp16 batch (tests/test_gpu_batch_decode.py::logit_tol); 2e-2 with
an fp16 KV cache, as there.  The returned argmax is always the first index of the maximum of the returned logits; in the fp32-cache
runs of test 1 it also equals the oracle's argmax wherever the oracle's two largest logits are more than twice the tolerance apart —
a rule that depends on the oracle alone and may leave out at most ONE of a member's 24 batch steps (asserted)."""
import re
from dataclasses import replace

import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth

pytestmark = pytest.mark.gpu

CAP = 96
Q4_K, Q6_K = 12, 14


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


def odesc(d, C):
    return orc.LlamaDesc(E=d.E, L=d.L, H=d.H, Hkv=d.Hkv, D=d.D, F=d.F, V=d.V, C=C)


def ddict(d):
    return dict(E=d.E, L=d.L, H=d.H, Hkv=d.Hkv, D=d.D, F=d.F, V=d.V, eps=1e-5, rope_dims=d.D, rope_base=500000.0)


def logit_tol(want, scale=5e-4):
    return scale * max(1.0, float(np.abs(want).max()))


def seq_tokens(dims, s):
    return synth.make_tokens(dims, 29 + 7 * s, seed=100 + s)


def mix_type(name, mix):
    if mix == "all_q4_k":
        return Q4_K
    if name.startswith(("token_embd", "output.")):
        return Q6_K
    m = re.match(r"blk\.(\d+)\.(attn_v|ffn_down)\.weight$", name)
    return Q6_K if m and int(m.group(1)) % 2 == 0 else Q4_K


def quantize(a, qt):
    a = np.ascontiguousarray(a, np.float32)
    if qt == Q4_K:
        b = orc.quantize_q4k(a)
        return b, orc.dequant_q4k(b, a.size).reshape(a.shape)
    b = orc.quantize_q6k(a)
    return b, orc.dequant_q6k(b, a.size).reshape(a.shape)


def quant_weights(w, mix="q4_k_m"):
    """synth weights -> ({name: QuantTensor | gains}, {name: dequantised fp32 | gains})."""
    from nfai_amd.llama_model import QuantTensor
    wq, wref = {}, {}
    for name, a in w.items():
        if a.ndim == 1:
            wq[name] = a
            wref[name] = a
            continue
        qt = mix_type(name, mix)
        raw, deq = quantize(a.astype(np.float32), qt)
        wq[name] = QuantTensor(raw, qt, a.shape)
        wref[name] = deq
    return wq, wref


def make_members(mgr, dims, wq, n, caps, **kw):
    """n models over one copy of the quantised weights: member 0 is the donor, the others share its tensors."""
    from nfai_amd.llama_model import LlamaModel
    md = synth.make_metadata(dims)
    caps = [caps] * n if isinstance(caps, int) else list(caps)
    ms = [LlamaModel(mgr, md, wq, caps[0], dims=ddict(dims), **kw)]
    for i in range(1, n):
        ms.append(LlamaModel(mgr, md, wq, caps[i], dims=ddict(dims), share_from=ms[0], **kw))
    return ms


def check_step(lg, am, wants, scale, where, oracle_argmax=False, excluded=None):
    """Every member of one batch step against its oracle logits `wants` (the rule of tests/test_gpu_batch_decode.py::check_step)."""
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
@pytest.mark.parametrize("n,kv_f16", [(1, False), (2, False), (3, False), (4, False), (5, False), (8, False), (2, True), (8, True)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("dims", [synth.TINY, synth.TINY_D128], ids=lambda d: d.name)
def test_staggered_batch_matches_the_oracle(mgr, dims, n, kv_f16):
    """Member s takes its first 5 + 7 s tokens alone through _decode_step (positions 5 ... 54), then 24 batch steps.  The oracle alone
    leaves out 0 or 1 step of every member on both shapes for these inputs and this mix (TINY: members 0, 3, 4, 7 one step each;
    TINY_D128: members 1, 3)."""
    from nfai_amd.llama_model import LlamaBatch
    w = synth.make_weights(dims, seed=21, std=0.05)
    wq, wref = quant_weights(w)
    ms = make_members(mgr, dims, wq, n, CAP, kv_f16=kv_f16)
    refs = [orc.OracleLlama(odesc(dims, CAP), wref) for _ in range(n)]
    toks = [seq_tokens(dims, s) for s in range(n)]
    scale = 2e-2 if kv_f16 else 5e-4
    for s in range(n):
        for t in toks[s][:5 + 7 * s]:
            ms[s].Step(int(t), want_logits=False)
            refs[s].step(int(t))
    batch = LlamaBatch(ms, quantized=True)
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
        atol = 1e-3 if not kv_f16 else 2e-2
        np.testing.assert_allclose(ms[s].Read(0, dims.E), refs[s].hidden(), rtol=0, atol=atol)
        for l in range(dims.L):
            np.testing.assert_allclose(ms[s].ReadKV(l, False, last - 1), refs[s].kcache(l)[last - 1], rtol=0, atol=atol)
            np.testing.assert_allclose(ms[s].ReadKV(l, True, last - 1), refs[s].vcache(l)[last - 1], rtol=0, atol=atol)
    dispose(batch, ms)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [synth.TINY, synth.TINY_D128], ids=lambda d: d.name)
def test_a_column_does_not_depend_on_its_neighbours(mgr, dims):
    """The same member state and token (a) in column 0 of a batch of 2 and (b) in column 7 of a batch of 8 whose other members hold
    other sequences at other depths: BIT-IDENTICAL logits.  The B = 2, 4 and 8 kernels share one summation order (per slot of a K
    tile in tile order, the four lane groups by rows4_sum, the slots in slot order); neither the batch size, nor the K tiling (a
    function of K alone), nor the grid, nor the other columns enter it.  Permuting the members changes no member's logits by a bit."""
    from nfai_amd.llama_model import LlamaBatch
    w = synth.make_weights(dims, seed=21, std=0.05)
    wq, _ = quant_weights(w)
    ms = make_members(mgr, dims, wq, 8, CAP)
    toks = [seq_tokens(dims, s) for s in range(8)]

    def bring(s, count):
        ms[s].Reset()
        for t in toks[s][:count]:
            ms[s].Step(int(t), want_logits=False)

    probe, depth, tok = 3, 17, int(toks[3][17])
    bring(probe, depth)
    bring(0, 9)
    b2 = LlamaBatch([ms[probe], ms[0]], quantized=True)
    lg_a, am_a = b2.Step([tok, int(toks[0][9])])
    b2.Dispose()
    for s in range(8):
        bring(s, depth if s == probe else 4 + 5 * s)
    order = [s for s in range(8) if s != probe] + [probe]
    b8 = LlamaBatch([ms[s] for s in order], quantized=True)
    lg_b, am_b = b8.Step([tok if s == probe else int(toks[s][4 + 5 * s]) for s in order])
    b8.Dispose()
    np.testing.assert_array_equal(lg_a[0], lg_b[7])
    assert am_a[0] == am_b[7]
    first = {s: lg_b[i].copy() for i, s in enumerate(order)}
    for s in range(8):
        bring(s, depth if s == probe else 4 + 5 * s)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    bp = LlamaBatch([ms[s] for s in perm], quantized=True)
    lg_p, _ = bp.Step([tok if s == probe else int(toks[s][4 + 5 * s]) for s in perm])
    for i, s in enumerate(perm):
        np.testing.assert_array_equal(lg_p[i], first[s])
    dispose(bp, ms)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def test_batch_and_single_steps_interleave(mgr):
    """Step, SetPos and Ingest (the MFMA prefill: the members have a prefill workspace) on members between batch steps."""
    from nfai_amd.llama_model import LlamaBatch
    dims, n = synth.TINY_D128, 3
    w = synth.make_weights(dims, seed=21, std=0.05)
    wq, wref = quant_weights(w)
    ms = make_members(mgr, dims, wq, n, CAP, max_batch=16)
    refs = [orc.OracleLlama(odesc(dims, CAP), wref) for _ in range(n)]
    toks = [seq_tokens(dims, s) for s in range(n)]
    cur = [0] * n

    def batch_step(batch, where, scale=5e-4):
        st = [int(toks[s][cur[s]]) for s in range(n)]
        lg, am = batch.Step(st)
        wants = []
        for s in range(n):
            wants.append(refs[s].step(st[s]))
            cur[s] += 1
        check_step(lg, am, wants, scale, where)

    for s in range(n):   # staggered start
        for t in toks[s][:2 + 3 * s]:
            ms[s].Step(int(t), want_logits=False)
            refs[s].step(int(t))
            cur[s] += 1
    batch = LlamaBatch(ms, quantized=True)
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
    refs[2] = orc.OracleLlama(odesc(dims, CAP), wref)
    for t in toks[2][:back]:
        refs[2].step(int(t))
    cur[2] = back
    for i in range(3):
        batch_step(batch, f"re-feed {i}")
    assert [m.Pos for m in ms] == cur
    # member 0 ingests 5 tokens through the prefill (fp16 operands: the K / V rows it leaves carry the prefill's stated 2e-2 scale)
    chunk = [int(t) for t in toks[0][cur[0]:cur[0] + 5]]
    ms[0].Ingest(chunk)
    for t in chunk:
        refs[0].step(t)
    cur[0] += 5
    for i in range(2):
        batch_step(batch, f"after ingest {i}", scale=2e-2)
    assert [m.Pos for m in ms] == cur
    dispose(batch, ms)


def test_holding_a_model_in_a_quantised_batch_changes_nothing_about_its_own_path(mgr):
    from nfai_amd.llama_model import LlamaBatch
    dims = synth.TINY_D128
    w = synth.make_weights(dims, seed=21, std=0.05)
    wq, _ = quant_weights(w)
    ms = make_members(mgr, dims, wq, 2, 48)
    toks = synth.make_tokens(dims, 30, seed=77)
    for i, t in enumerate(toks):
        if i == 11:
            LlamaBatch([ms[1]], quantized=True).Dispose()   # created and destroyed without a step
        la, aa = ms[0].Step(int(t))
        if i == 19:
            b = LlamaBatch([ms[1]], quantized=True)         # ... and held across a step of the member's own path
        lb, ab = ms[1].Step(int(t))
        if i == 19:
            b.Dispose()
        np.testing.assert_array_equal(la, lb)
        assert aa == ab
    dispose(None, ms)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 5])
def test_greedy_on_the_device(mgr, n):
    from nfai_amd.llama_model import LlamaBatch
    dims = synth.TINY_D128
    w = synth.make_weights(dims, seed=21, std=0.05)
    wq, _ = quant_weights(w)
    ms = make_members(mgr, dims, wq, n, CAP)
    toks = [seq_tokens(dims, s) for s in range(n)]
    batch = LlamaBatch(ms, quantized=True)

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
@pytest.mark.parametrize("mix", ["q4_k_m", "all_q4_k"])
@pytest.mark.parametrize("n", [8, 3])
@pytest.mark.parametrize("dims", [synth.LLAMA_32_1B, synth.LLAMA_32_3B, synth.LLAMA_31_8B], ids=lambda d: d.name)
def test_full_width_block(mgr, dims, n, mix):
    """One block at the published widths (tests/test_gpu_batch_decode.py::test_full_width_block's construction, V = 4096): the test
    that meets the LDS budgets — K = 8192 and 14336 at B = 8 (the K tiles of Wdown), the q|k|v of mixed types at E = 3072 / 4096
    (block 0 is even: v and Wdown are Q6_K in the mix), the head at full row length."""
    from nfai_amd.llama_model import LlamaBatch
    d1 = replace(dims, L=1, V=4096, name=dims.name + "-1blk")
    w = synth.make_weights(d1, seed=31)
    wq, wref = quant_weights(w, mix)
    C = 32
    ms = make_members(mgr, d1, wq, n, C)
    refs = [orc.OracleLlama(odesc(d1, C), wref) for _ in range(n)]
    toks = [synth.make_tokens(d1, 32, seed=200 + s) for s in range(n)]
    for s in range(n):
        for t in toks[s][:1 + 2 * s]:
            ms[s].Step(int(t), want_logits=False)
            refs[s].step(int(t))
    batch = LlamaBatch(ms, quantized=True)
    for i in range(12):
        st = [int(toks[s][1 + 2 * s + i]) for s in range(n)]
        lg, am = batch.Step(st)
        check_step(lg, am, [refs[s].step(st[s]) for s in range(n)], 5e-4, f"step {i}")
    dispose(batch, ms)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_admissions(mgr):
    from nfai_amd import _lib
    from nfai_amd._lib import KVCacheFull, NfaiHipError
    from nfai_amd.llama_model import LlamaBatch, LlamaModel, QuantTensor
    dims = synth.TINY_D128
    w = synth.make_weights(dims, seed=21, std=0.05)
    wq, wref = quant_weights(w)
    md = synth.make_metadata(dims)
    dd = ddict(dims)
    ms = make_members(mgr, dims, wq, 2, 8)

    def refused(models, code, pattern, quantized=True):
        with pytest.raises(NfaiHipError, match=pattern) as e:
            LlamaBatch(models, quantized=quantized)
        assert e.value.code == code, e.value.args

    # admitted under the flag, still refused without it
    LlamaBatch(ms, quantized=True).Dispose()
    refused(ms, _lib.ERR_UNSUPPORTED, "member 0", quantized=False)
    # Q5_K and Q8_0 members: named tensor and ggml type
    w5 = {name: a if a.ndim == 1 else QuantTensor(np.frombuffer(synth.quantize_q5_k(a.astype(np.float32)), np.uint8).copy(), _lib.Q5_K, a.shape)
          for name, a in w.items()}
    q5 = LlamaModel(mgr, md, w5, 8, dims=dd)
    refused([q5], _lib.ERR_UNSUPPORTED, r"member 0: token_embd of block 0 has ggml type 13")
    w8 = {name: a if a.ndim == 1 else QuantTensor(np.frombuffer(synth.quantize_q8_0(a.astype(np.float32)), np.uint8).copy(), _lib.Q8_0, a.shape)
          for name, a in w.items()}
    q8 = LlamaModel(mgr, md, w8, 8, dims=dd)
    refused([q8], _lib.ERR_UNSUPPORTED, r"member 0: token_embd of block 0 has ggml type 8")
    # an fp16 model whose ffn_down alone is Q4_K (if finalize accepts such a model)
    extra = []
    wm = dict(w)
    for name, a in w.items():
        if name.endswith("ffn_down.weight"):
            wm[name] = QuantTensor(orc.quantize_q4k(a.astype(np.float32)), _lib.Q4_K, a.shape)
    try:
        mixed = LlamaModel(mgr, md, wm, 8, dims=dd)
    except NfaiHipError:
        mixed = None   # finalize does not take such a model: nothing to refuse
    if mixed is not None:
        refused([mixed], _lib.ERR_UNSUPPORTED, r"member 0 mixes fp16 and quantised matrices .*ffn_down of block 0 has ggml type 12")
        extra.append(mixed)
    # the fp16 batch's refusals under the flag
    stage = LlamaModel(mgr, md, wq, 8, dims=dd, layer_range=(0, 2))
    refused([stage], _lib.ERR_UNSUPPORTED, "pipeline stage")
    own = LlamaModel(mgr, md, wq, 8, dims=dd)
    refused([ms[0], own], _lib.ERR_UNSUPPORTED, "member 1")
    k16 = LlamaModel(mgr, md, wq, 8, dims=dd, share_from=ms[0], kv_f16=True)
    refused([ms[0], k16], _lib.ERR_UNSUPPORTED, "member 1")
    refused([ms[0], ms[1], ms[0]], _lib.ERR_INVALID, "member 2")
    # a member at capacity fails the step naming it; no position moves
    batch = LlamaBatch(ms, quantized=True)
    refs = [orc.OracleLlama(odesc(dims, 8), wref) for _ in range(2)]
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
    assert [m.Pos for m in ms] == [7, 8]
    with pytest.raises(KVCacheFull):
        batch.Greedy([1, 2], 1)
    assert [m.Pos for m in ms] == [7, 8]
    batch.Dispose()
    for m in [q5, q8, stage, own, k16] + extra + [ms[1], ms[0]]:
        m.Dispose()


def test_fp16_members_under_the_flag_behave_as_without_it(mgr):
    """Bit-equal logits to a batch from nfai_hip_llama_batch_create."""
    from nfai_amd.llama_model import LlamaBatch, LlamaModel
    dims, n = synth.TINY_D128, 3
    w = synth.make_weights(dims, seed=21, std=0.05)
    md = synth.make_metadata(dims)
    ms = [LlamaModel(mgr, md, w, CAP)]
    for i in range(1, n):
        ms.append(LlamaModel(mgr, md, w, CAP, share_from=ms[0]))
    toks = [seq_tokens(dims, s) for s in range(n)]
    got = {}
    for flag in (False, True):
        for s in range(n):
            ms[s].Reset()
            for t in toks[s][:2 + 3 * s]:
                ms[s].Step(int(t), want_logits=False)
        batch = LlamaBatch(ms, quantized=flag)
        out = []
        for i in range(6):
            lg, am = batch.Step([int(toks[s][2 + 3 * s + i]) for s in range(n)])
            out.append((lg.copy(), am.copy()))
        got[flag] = (out, batch.BytesPerToken())
        batch.Dispose()
    for (la, aa), (lb, ab) in zip(got[False][0], got[True][0]):
        np.testing.assert_array_equal(la, lb)
        np.testing.assert_array_equal(aa, ab)
    assert got[False][1] == got[True][1]
    dispose(None, ms)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [synth.TINY, synth.TINY_D128], ids=lambda d: d.name)
def test_byte_model(mgr, dims):
    """BytesPerToken() = every T16 plane once (144 B per 256 weights in Q4_K, 210 B in Q6_K; a tied token_embd is the head) + every norm
    gain once + an embedding row per member where token_embd is not the head + every member's KV rows at its position (p + 1 read,
    1 written per block)."""
    from nfai_amd.llama_model import LlamaBatch
    n = 3
    w = synth.make_weights(dims, seed=21, std=0.05)
    wq, _ = quant_weights(w)
    ms = make_members(mgr, dims, wq, n, CAP)
    toks = [seq_tokens(dims, s) for s in range(n)]
    for s in range(n):
        for t in toks[s][:1 + 4 * s]:
            ms[s].Step(int(t), want_logits=False)
    batch = LlamaBatch(ms, quantized=True)
    blk = {Q4_K: 144, Q6_K: 210}
    tied = "output.weight" not in w
    want = 0
    for name, a in w.items():
        if a.ndim == 1:
            want += a.size * 4
        elif name.startswith("token_embd") and not tied:
            want += n * (a.shape[1] // 256) * blk[mix_type(name, "q4_k_m")]
        else:
            want += (a.size // 256) * blk[mix_type(name, "q4_k_m")]
    kv_row = 2 * dims.Hkv * dims.D * 4
    for s in range(n):
        want += dims.L * (kv_row * (ms[s].Pos + 1) + kv_row)
    assert batch.BytesPerToken() == want
    batch.Step([int(toks[s][1 + 4 * s]) for s in range(n)], want_logits=False)
    assert batch.BytesPerToken() == want + n * dims.L * kv_row
    dispose(batch, ms)
