"""The batched decode step on Q5_K / Q8_0 members (nfai_hip_llama_batch_create_ex with NFAI_BATCH_QUANT | NFAI_BATCH_QUANT_ANY,
k_bgemv_kq on all four T16 types) on the GPU, against one CPU oracle per sequence on the DEQUANTISED weights.  The mirror of
tests/test_gpu_batch_quant.py, whose helpers, token sequences and weight seed it uses.

Tensor mixes: "q5_k_m" (synth.q5_k_m_type: Q5_K with Q6_K for the head and attn_v / ffn_down of the use_more_bits blocks),
"all_q5_k", "all_q8_0", "q8_0_v_q4k" (attn_v Q4_K, the rest Q8_0: two q|k|v launches), and a (q, k, v) tuple of types for the three
attention inputs (the rest Q5_K).

Tolerance: the project's 5e-4 * max(1, max|logit|) with an fp32 KV cache, 2e-2 with an fp16 one (tests/test_gpu_batch_quant.py,
tests/test_gpu_q5_k.py, tests/test_gpu_q8_0.py): the kernels keep the same 22-bit fixed-point activations.  In the fp32-cache runs
of test 1 the ArgMax also equals the oracle's wherever the oracle's two largest logits are more than twice the tolerance apart; the
rule depends on the oracle alone and leaves out at most ONE of a member's 24 steps (asserted).  Steps it leaves out per member
(members 0-7), from the oracle alone on these inputs:
    tiny-llama       q5_k_m 0 0 0 0 0 0 0 0   all_q5_k 0 0 1 0 1 1 0 0   all_q8_0 0 0 0 0 0 0 0 1   q8_0_v_q4k 0 0 0 0 0 0 1 0
    tiny-llama-d128  q5_k_m 0 1 0 0 1 0 0 0   all_q5_k 1 0 0 0 0 0 0 0   all_q8_0 0 0 1 0 0 0 1 1   q8_0_v_q4k 0 0 0 0 1 0 0 1"""
from dataclasses import replace

import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth
from test_gpu_batch_quant import CAP, check_step, ddict, dispose, logit_tol, make_members, odesc, seq_tokens

pytestmark = pytest.mark.gpu

Q8_0, Q4_K, Q5_K, Q6_K = 8, 12, 13, 14
MIXES = ["q5_k_m", "all_q5_k", "all_q8_0", "q8_0_v_q4k"]


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


def dequant_q5_k(raw, rows, cols):
    """ggml dequantize_row_q5_K (tests/test_gpu_q5_k.py::dequant_q5_k)."""
    b = np.frombuffer(np.ascontiguousarray(raw, np.uint8).tobytes(), np.uint8).reshape(rows * cols // 256, 176)
    d = b[:, 0:2].copy().view(np.float16).astype(np.float32)
    dmin = b[:, 2:4].copy().view(np.float16).astype(np.float32)
    s = b[:, 4:16]
    sc = np.concatenate([s[:, 0:4] & 63, (s[:, 8:12] & 0xF) | ((s[:, 0:4] >> 6) << 4)], axis=1).astype(np.float32)
    mn = np.concatenate([s[:, 4:8] & 63, (s[:, 8:12] >> 4) | ((s[:, 4:8] >> 6) << 4)], axis=1).astype(np.float32)
    n = np.arange(4, dtype=np.uint8)[None, :, None]
    qh, qs = b[:, None, 16:48], b[:, 48:176].reshape(-1, 4, 32)
    q = np.stack([(qs & 0xF) | (((qh >> (2 * n)) & 1) << 4), (qs >> 4) | (((qh >> (2 * n + 1)) & 1) << 4)], axis=2)
    q = q.reshape(-1, 8, 32).astype(np.float32)
    return ((d * sc)[:, :, None] * q - (dmin * mn)[:, :, None]).reshape(rows, cols)


def dequant_q8_0(raw, rows, cols):
    """ggml dequantize_row_q8_0 (tests/test_gpu_q8_0.py::dequant_q8_0)."""
    b = np.frombuffer(np.ascontiguousarray(raw, np.uint8).tobytes(), np.uint8).reshape(rows * cols // 32, 34)
    d = b[:, :2].copy().view(np.float16).astype(np.float32)[:, 0]
    q = b[:, 2:].copy().view(np.int8).astype(np.float32)
    return (d[:, None] * q).reshape(rows, cols)


def mix_type(name, mix, dims):
    if isinstance(mix, tuple):
        parts = name.split(".")
        return mix[("attn_q", "attn_k", "attn_v").index(parts[2])] if len(parts) > 2 and parts[2] in ("attn_q", "attn_k", "attn_v") else Q5_K
    if mix == "q5_k_m":
        return synth.q5_k_m_type(name, dims)
    if mix == "all_q5_k":
        return Q5_K
    if mix == "q8_0_v_q4k" and name.endswith("attn_v.weight"):
        return Q4_K
    return Q8_0


def quantize(a, qt):
    """fp32 [N][K] -> (raw block bytes, dequantised fp32 [N][K])."""
    a = np.ascontiguousarray(a, np.float32)
    if qt == Q4_K:
        b = orc.quantize_q4k(a)
        return b, orc.dequant_q4k(b, a.size).reshape(a.shape)
    if qt == Q6_K:
        b = orc.quantize_q6k(a)
        return b, orc.dequant_q6k(b, a.size).reshape(a.shape)
    if qt == Q5_K:
        b = np.frombuffer(synth.quantize_q5_k(a), np.uint8).copy()
        return b, dequant_q5_k(b, *a.shape)
    b = np.frombuffer(synth.quantize_q8_0(a), np.uint8).copy()
    return b, dequant_q8_0(b, *a.shape)


_WEIGHTS = {}


def quant_weights(dims, mix, seed=21, std=0.05):
    """({name: QuantTensor | gains}, {name: dequantised fp32 | gains}, the synth weights), quantised once per module."""
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
            raw, deq = quantize(a, qt)
            wq[name] = QuantTensor(raw, qt, a.shape)
            wref[name] = deq
        _WEIGHTS[key] = (wq, wref, w)
    return _WEIGHTS[key]


def any_batch(ms):
    from nfai_amd.llama_model import LlamaBatch
    return LlamaBatch(ms, quantized=True, any_quant=True)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_member(dims, mix, s):
    """Member s of test 1 through the oracle alone, computed once and shared by every n and KV type (a member's sequence depends on
    neither): the logits of its 24 batch steps, then its hidden state and last K / V rows."""
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


@pytest.mark.parametrize("n,kv_f16", [(1, False), (2, False), (3, False), (4, False), (5, False), (8, False), (2, True), (8, True)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("dims", [synth.TINY, synth.TINY_D128], ids=lambda d: d.name)
def test_staggered_batch_matches_the_oracle(mgr, dims, mix, n, kv_f16):
    """Member s takes its first 5 + 7 s tokens alone through _decode_step (positions 5 ... 54), then 24 batch steps."""
    wq, _, _ = quant_weights(dims, mix)
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
    assert max(excluded) <= 1, excluded   # the near-tie rule may leave out at most one of a member's 24 steps
    for s in range(n):
        last = 5 + 7 * s + 24
        assert ms[s].Pos == last
        atol = 1e-3 if not kv_f16 else 2e-2
        np.testing.assert_allclose(ms[s].Read(0, dims.E), refs[s][1], rtol=0, atol=atol)
        for l in range(dims.L):
            np.testing.assert_allclose(ms[s].ReadKV(l, False, last - 1), refs[s][2][l], rtol=0, atol=atol)
            np.testing.assert_allclose(ms[s].ReadKV(l, True, last - 1), refs[s][3][l], rtol=0, atol=atol)
    dispose(batch, ms)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", ["q5_k_m", "all_q8_0"])
@pytest.mark.parametrize("dims", [synth.TINY, synth.TINY_D128], ids=lambda d: d.name)
def test_a_column_does_not_depend_on_its_neighbours(mgr, dims, mix):
    """The same member state and token in column 0 of a batch of 2 and in column 7 of a batch of 8 whose other members sit at other
    depths: BIT-IDENTICAL logits; a permutation of the members changes no member's logits by a bit
    (tests/test_gpu_batch_quant.py::test_a_column_does_not_depend_on_its_neighbours on the new types)."""
    wq, _, _ = quant_weights(dims, mix)
    ms = make_members(mgr, dims, wq, 8, CAP)
    toks = [seq_tokens(dims, s) for s in range(8)]

    def bring(s, count):
        ms[s].Reset()
        for t in toks[s][:count]:
            ms[s].Step(int(t), want_logits=False)

    probe, depth, tok = 3, 17, int(toks[3][17])
    bring(probe, depth)
    bring(0, 9)
    b2 = any_batch([ms[probe], ms[0]])
    lg_a, am_a = b2.Step([tok, int(toks[0][9])])
    b2.Dispose()
    for s in range(8):
        bring(s, depth if s == probe else 4 + 5 * s)
    order = [s for s in range(8) if s != probe] + [probe]
    b8 = any_batch([ms[s] for s in order])
    lg_b, am_b = b8.Step([tok if s == probe else int(toks[s][4 + 5 * s]) for s in order])
    b8.Dispose()
    np.testing.assert_array_equal(lg_a[0], lg_b[7])
    assert am_a[0] == am_b[7]
    first = {s: lg_b[i].copy() for i, s in enumerate(order)}
    for s in range(8):
        bring(s, depth if s == probe else 4 + 5 * s)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    bp = any_batch([ms[s] for s in perm])
    lg_p, _ = bp.Step([tok if s == probe else int(toks[s][4 + 5 * s]) for s in perm])
    for i, s in enumerate(perm):
        np.testing.assert_array_equal(lg_p[i], first[s])
    dispose(bp, ms)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def test_three_types_in_one_qkv(mgr):
    """attn_q Q5_K, attn_k Q8_0, attn_v Q6_K: the q|k|v of every block runs as three launches, one per type."""
    dims, n = synth.TINY_D128, 3
    wq, wref, _ = quant_weights(dims, (Q5_K, Q8_0, Q6_K))
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


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
def edit_extremes(raw, qt, rng):
    """A share of the raw blocks of one tensor, edited in place: the codes, bits and scales at the ends of their ranges."""
    if qt == Q5_K:
        b = raw.reshape(-1, 176)
        pick = rng.permutation(b.shape[0])
        k = max(1, b.shape[0] // 16)
        b[pick[0 * k:1 * k], 16:176] = 0          # codes 0 (nibbles and fifth bits clear)
        b[pick[1 * k:2 * k], 16:176] = 0xFF       # codes 31
        b[pick[2 * k:3 * k], 16:48] = 0xFF        # every fifth bit set
        b[pick[3 * k:4 * k], 16:48] = 0           # every fifth bit clear
        b[pick[4 * k:5 * k], 4:16] = 0xFF         # 6-bit scales and mins at 63
        b[pick[5 * k:6 * k], 4:16] = 0            # ... and at 0
    else:
        b = raw.reshape(-1, 34)
        pick = rng.permutation(b.shape[0])
        k = max(1, b.shape[0] // 16)
        b[pick[0 * k:1 * k], 2:] = 0x80           # -128
        b[pick[1 * k:2 * k], 2:] = 0x7F           # 127
        b[pick[2 * k:3 * k], 2::2] = 0x80         # alternating with what was there
        b[pick[3 * k:4 * k], 0:2] = 0             # d = 0


@pytest.mark.parametrize("mix", ["all_q5_k", "all_q8_0"])
def test_extreme_codes(mgr, mix):
    """Codes 0 / 31 and -128 / 127, all fifth bits set / clear, scales and mins at 63 / 0, a d of zero, in a sixteenth of the blocks
    each of every matrix; the oracle computes on the dequantised EDITED bytes."""
    from nfai_amd.llama_model import QuantTensor
    dims, n = synth.TINY, 8
    qt = Q5_K if mix == "all_q5_k" else Q8_0
    w = synth.make_weights(dims, seed=21, std=0.05)
    rng = np.random.Generator(np.random.PCG64(404))
    wq, wref = {}, {}
    for name, a in w.items():
        if a.ndim == 1:
            wq[name] = wref[name] = a
            continue
        raw, _ = quantize(a, qt)
        edit_extremes(raw, qt, rng)
        wq[name] = QuantTensor(raw, qt, a.shape)
        wref[name] = (dequant_q5_k if qt == Q5_K else dequant_q8_0)(raw, *a.shape)
        assert np.isfinite(wref[name]).all()
    ms = make_members(mgr, dims, wq, n, CAP)
    refs = [orc.OracleLlama(odesc(dims, CAP), wref) for _ in range(n)]
    toks = [seq_tokens(dims, s) for s in range(n)]
    for s in range(n):
        for t in toks[s][:1 + 2 * s]:
            ms[s].Step(int(t), want_logits=False)
            refs[s].step(int(t))
    batch = any_batch(ms)
    for i in range(6):
        st = [int(toks[s][1 + 2 * s + i]) for s in range(n)]
        lg, am = batch.Step(st)
        check_step(lg, am, [refs[s].step(st[s]) for s in range(n)], 5e-4, f"step {i}")
    dispose(batch, ms)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
WIDE = replace(synth.LLAMA_32_3B, L=1, V=2048, F=4352, name="llama-3.2-3b-1blk-f4352")


@pytest.mark.parametrize("n", [8, 3])
@pytest.mark.parametrize("mix", ["q5_k_m", "all_q8_0", "all_q5_k"])
def test_tiled_k_two_slots_per_wave_and_the_ragged_last_tile(mgr, mix, n):
    """The smallest shape that reaches them: E = 3072 is 12 super-blocks (two slots per wave); F = 4352 is 17: Wdown runs as two K
    tiles of 9 on 5 waves, the last wave's second slot is empty and the second tile ends one super-block past K.  (In q5_k_m the one
    block's ffn_down is Q6_K; all_q5_k puts Q5_K on the tiled launch too.)"""
    wq, wref, _ = quant_weights(WIDE, mix, seed=31, std=0.02)
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


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", ["q5_k_m", "all_q8_0"])
@pytest.mark.parametrize("n", [2, 5])
def test_greedy_on_the_device(mgr, n, mix):
    dims = synth.TINY_D128
    wq, _, _ = quant_weights(dims, mix)
    ms = make_members(mgr, dims, wq, n, CAP)
    toks = [seq_tokens(dims, s) for s in range(n)]
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


def test_batch_and_single_steps_interleave(mgr):
    """Step, SetPos and Ingest (the MFMA prefill) on Q5_K_M members between batch steps
    (tests/test_gpu_batch_quant.py::test_batch_and_single_steps_interleave)."""
    dims, n = synth.TINY_D128, 3
    wq, wref, _ = quant_weights(dims, "q5_k_m")
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
    batch = any_batch(ms)
    batch_step(batch, "batch 0")
    lg, am = ms[1].Step(int(toks[1][cur[1]]))   # one member alone
    want = refs[1].step(int(toks[1][cur[1]]))
    cur[1] += 1
    assert np.abs(lg - want).max() <= logit_tol(want)
    batch_step(batch, "batch 1")
    batch_step(batch, "batch 2")
    back = cur[2] - 3                            # member 2 goes back by 3 and the batch re-feeds those tokens
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


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def test_admissions_and_refusals(mgr):
    from nfai_amd import _lib
    from nfai_amd._lib import NfaiHipError
    from nfai_amd.llama_model import LlamaBatch, LlamaModel, QuantTensor
    dims = synth.TINY_D128
    md, dd = synth.make_metadata(dims), ddict(dims)

    def refused(models, pattern, **kw):
        with pytest.raises(NfaiHipError, match=pattern) as e:
            LlamaBatch(models, **kw)
        assert e.value.code == _lib.ERR_UNSUPPORTED, e.value.args

    made = []
    for mix, ggml in (("all_q5_k", 13), ("all_q8_0", 8)):
        wq, _, _ = quant_weights(dims, mix)
        ms = make_members(mgr, dims, wq, 2, 8)
        made += reversed(ms)
        any_batch(ms).Dispose()                                                            # admitted with both flags
        refused(ms, rf"member 0: token_embd of block 0 has ggml type {ggml}\b", quantized=True)   # exactly as before with one
        refused(ms, rf"member 0: token_embd of block 0 has ggml type {ggml}; the batched kernels take fp16", quantized=False)
    any_batch(make_members_keep(mgr, dims, quant_weights(dims, "q5_k_m")[0], made)).Dispose()
    # Q4_K / Q6_K members are admitted under both flags as under one
    from test_gpu_batch_quant import quant_weights as q4km_weights
    w = synth.make_weights(dims, seed=21, std=0.05)
    any_batch(make_members_keep(mgr, dims, q4km_weights(w)[0], made)).Dispose()
    # still refused by name: fp16 beside quantised matrices
    wq8, _, _ = quant_weights(dims, "all_q8_0")
    wm = dict(w)
    for name in w:
        if name.endswith("ffn_down.weight"):
            wm[name] = wq8[name]
    mixed = LlamaModel(mgr, md, wm, 8, dims=dd)
    made.append(mixed)
    refused([mixed], r"member 0 mixes fp16 and quantised matrices .*ffn_down of block 0 has ggml type 8", quantized=True, any_quant=True)
    # ... ffn_gate and ffn_up of different types: no such model of the fused path exists, _finalize refuses it by name, so a batch
    # (which takes finalized models of the fused path only) never sees one
    wq5, _, _ = quant_weights(dims, "all_q5_k")
    wg = dict(wq8)
    for name in w:
        if name.endswith("ffn_gate.weight"):
            wg[name] = wq5[name]
    with pytest.raises(NfaiHipError, match="blk.0 ffn_gate and ffn_up have different tensor types") as e:
        LlamaModel(mgr, md, wg, 8, dims=dd)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    # ... and a pipeline stage
    stage = LlamaModel(mgr, md, wq8, 8, dims=dd, layer_range=(0, 2))
    made.append(stage)
    refused([stage], "pipeline stage", quantized=True, any_quant=True)
    for m in made:
        m.Dispose()


def make_members_keep(mgr, dims, wq, made):
    ms = make_members(mgr, dims, wq, 2, 8)
    made += reversed(ms)
    return ms


@pytest.mark.parametrize("mix,blk", [("all_q5_k", 176), ("all_q8_0", 8 * 34)], ids=["all_q5_k", "all_q8_0"])
@pytest.mark.parametrize("dims", [synth.TINY, synth.TINY_D128], ids=lambda d: d.name)
def test_byte_model(mgr, dims, mix, blk):
    """BytesPerToken() = every T16 plane once (176 B per 256 weights in Q5_K, 34 B per 32 in Q8_0: the per-weight figures of
    tests/test_gpu_q5_k.py / test_gpu_q8_0.py::test_model_*_graph_eager_unfused; a tied token_embd is the head and is counted once)
    + every norm gain once + an embedding row per member where token_embd is not the head + every member's KV rows at its position
    (tests/test_gpu_batch_quant.py::test_byte_model)."""
    n = 3
    wq, _, w = quant_weights(dims, mix)
    ms = make_members(mgr, dims, wq, n, CAP)
    toks = [seq_tokens(dims, s) for s in range(n)]
    for s in range(n):
        for t in toks[s][:1 + 4 * s]:
            ms[s].Step(int(t), want_logits=False)
    batch = any_batch(ms)
    tied = "output.weight" not in w
    assert tied == dims.tied
    want = 0
    for name, a in w.items():
        if a.ndim == 1:
            want += a.size * 4
        elif name.startswith("token_embd") and not tied:
            want += n * (a.shape[1] // 256) * blk
        else:
            want += (a.size // 256) * blk
    kv_row = 2 * dims.Hkv * dims.D * 4
    for s in range(n):
        want += dims.L * (kv_row * (ms[s].Pos + 1) + kv_row)
    assert batch.BytesPerToken() == want
    batch.Step([int(toks[s][1 + 4 * s]) for s in range(n)], want_logits=False)
    assert batch.BytesPerToken() == want + n * dims.L * kv_row
    dispose(batch, ms)
