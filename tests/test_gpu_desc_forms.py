"""Every model path on the GPU away from the one descriptor point the rest of the suite pins (rope_dims = D, full frequency table,
base 500000, eps 1e-5): the forms of tests/desc_forms.py (half, six, cut, ref32, none) on tiny-llama (D = 64) and tiny-llama-d128,
weights make_weights(seed 21, std 0.05), against the C oracle built with the same descriptor.  tests/test_desc_forms.py shows on the
CPU that the oracle is right under every form and how far each wrong model a kernel could compute instead moves what is compared here.

One oracle walk of desc_forms.tokens (134 positions) per (model, form, weights) is the reference of every path; a batch's members and
a window's columns sit at different positions of that one sequence.  Every case asserts
  (a) the logits within the bar the path has elsewhere in the suite: 5e-4 * max(1, max|logit|) for an fp32 KV cache, 2e-2 * the same
      with an fp16 KV cache and behind an MFMA prefill (tests/test_gpu_batch_decode.py::logit_tol, tests/test_gpu_q4_0.py,
      tests/test_gpu_scale_sweep.py), quantised models against the oracle on the dequantised weights at the same bars; the ArgMax
      is the first index of the maximum of the returned logits;
  (b) the K row of the last position and an early V row the path wrote, of every block, at 1e-3 (2e-2 on the 2e-2 paths), and on
      the single-decode paths q after RoPE of the last block (nfai_hip_llama_read, which = 1) at the same bar;
  (c) the switch does something: the K row of every block is more than one bar from the DEFAULT-descriptor oracle's, and so is
      some compared logit row.  A harness that silently built the default model fails here.

Paths: single decode (graph, eager, the 1:1 chain; fp32 and fp16 KV), the engine (tiny-llama-d128), quantised single decode (the
Q4_K_M mix, all Q5_K, all Q8_0, all Q4_0: the int8-MFMA kernels), batches of 5 at positions 0, 3, 17, 40, 41 for 8 steps (fp16;
Q4_K_M with NFAI_BATCH_QUANT; a mix of all five types with NFAI_BATCH_QUANT_ANY), the wide batch of 16 for 4 steps, windows (fp16
and Q4_K_M: 8 tokens from position 0 and from 37, and a verify of 7 drafts of which the first 3 are right), the MFMA prefill (37
tokens; 130 in chunks of 64, and of 128 on tiny-llama-d128; RoPE in the GEMM epilogue and NFAI_PREFILL_ROPE_FUSED=0; fp16 KV;
Q4_K_M), two pipeline stages on one device (stage_ingest, then stage_step: bit-identical to the whole model), and the refusal of a
batch whose members' descriptors differ.  The rope_dims = 0 form runs on the single-decode, batch and prefill paths.

kernels_gemv_kq.hip (the VALU K-quant GEMV) takes matrices whose row count is not a multiple of 16.  With D = 64 or 128 no model's
q | k | v has such a count, so its RoPE epilogue is reached through nfai_hip_gemv_qkv_rope only (test_valu_kquant_qkv_rope_op, a
head size of 40); a model reaches that file with a vocabulary of 520 rows: the lm_head with the output RMSNorm, i.e. eps
(kind "q4k_v520").

Measured on an MI355X (every case prints a FORM line): max|dlogit| is 0.003 - 0.016 bars on the 5e-4 paths and 0.03 - 0.12 bars on
the 2e-2 ones; the distance to the default model is the oracles' own: in the logits 1100 - 3500 bars on the 5e-4 paths and 28 - 82
on the 2e-2 ones, in the K rows 2200 - 6800 and 131 - 273 bars.  No path failed; nothing in the kernels had to change.  Against
scratch builds with one line mutated: rope_dims forced to D in the arguments of launch_gemv 92 of the 194 cases fail,
of launch_gemv_kqm 66, eps forced to 1e-5 in the batch launches 26; rope_dims forced to D in the batch launches and k_rope_table
rotating every pair fail none, and cannot: both take cos / sin from the frequency table, which is padded with zeros up to D / 2."""
import functools
from dataclasses import replace

import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth
from oracle import np_oracle as npo

import desc_forms as df

pytestmark = pytest.mark.gpu

TINY_V520 = replace(synth.TINY, V=520, name="tiny-llama-v520")
MODELS = [synth.TINY, synth.TINY_D128]
BY_NAME = {d.name: d for d in MODELS + [TINY_V520]}
CAP = df.N_WALK + 2
DECODE, LOOSE = (5e-4, 1e-3), (2e-2, 2e-2)   # (logit scale, K / V / q row atol)
Q4_0, Q8_0, Q4_K, Q5_K, Q6_K = 2, 8, 12, 13, 14


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


def cases(none=True, models=MODELS):
    return [pytest.param(d.name, f, id=f"{d.name}-{f}") for d in models for f in df.forms_for(d, none=none)]


# ---- weights and the oracle --------------------------------------------------------------------------------------------------------
def five_type(name, dims):
    """A per-tensor mix of all five block types: the head Q6_K; q / k / v in three different types (three q | k | v launches); gate and
    up of one type per block, as the batched kernels ask."""
    if name.startswith(("token_embd", "output.")):
        return Q6_K
    _, l, kind, _ = name.split(".")
    odd = int(l) % 2
    return {"attn_q": Q4_0, "attn_k": Q5_K, "attn_v": Q8_0, "attn_output": Q4_K, "ffn_gate": (Q5_K, Q4_0)[odd], "ffn_up": (Q5_K, Q4_0)[odd],
            "ffn_down": (Q6_K, Q8_0)[odd]}[kind]


@functools.lru_cache(maxsize=None)
def weights(name, kind):
    """(what the model loads, what the oracle computes on), quantised the way the quantised tests of each type do it."""
    from nfai_amd.llama_model import QuantTensor
    dims = BY_NAME[name]
    w = synth.make_weights(dims, seed=21, std=0.05)
    if kind == "f16":
        return w, w
    if kind == "q4_k_m":
        from test_gpu_batch_quant import quant_weights
        return quant_weights(w)
    if kind == "q4k_v520":
        from test_gpu_batch_quant import quant_weights
        return quant_weights(w, "all_q4_k")
    if kind in ("all_q5_k", "all_q8_0"):
        from test_gpu_batch_quant_any import quant_weights
        return quant_weights(dims, kind, seed=21, std=0.05)[:2]
    if kind == "all_q4_0":
        from test_gpu_q4_0 import quant_weights
        return quant_weights(dims, 21, "all_q4_0", std=0.05)
    assert kind == "five"
    from test_gpu_batch_quant_any import quantize
    from test_gpu_q4_0 import quantize as quantize_q4_0
    wq, wref = {}, {}
    for n, a in w.items():
        if a.ndim == 1:
            wq[n] = wref[n] = a
            continue
        qt = five_type(n, dims)
        raw, deq = quantize_q4_0(a.astype(np.float32)) if qt == Q4_0 else quantize(a.astype(np.float32), qt)
        wq[n], wref[n] = QuantTensor(raw, qt, a.shape), deq
    return wq, wref


class Walk:
    pass


@functools.lru_cache(maxsize=None)
def walk(name, form, kind):
    """The oracle under `form` ("default": the default descriptor) over the N_WALK tokens: logits, K and V caches."""
    dims = BY_NAME[name]
    ref = orc.OracleLlama(df.odesc(dims, form, df.N_WALK), weights(name, kind)[1])
    r = Walk()
    r.logits = [ref.step(t).copy() for t in df.tokens(dims, df.N_WALK)]
    r.K = [ref.kcache(l).copy() for l in range(dims.L)]
    r.V = [ref.vcache(l).copy() for l in range(dims.L)]
    ref.close()
    return r


@functools.lru_cache(maxsize=None)
def q_last(name, form, kind, n):
    """q after RoPE of the last block at position n - 1, by the oracle's operators on its own hidden state."""
    dims = BY_NAME[name]
    rd, nf, base, eps = df.resolve(form, dims)
    wref = weights(name, kind)[1]
    ref = orc.OracleLlama(df.odesc(dims, form, n), wref)
    toks = df.tokens(dims, n)
    for t in toks[:-1]:
        ref.step(t, want_logits=False)
    h = ref.layers(np.asarray(wref["token_embd.weight"][toks[-1]], np.float32), 0, dims.L - 1)
    ref.close()
    b = f"blk.{dims.L - 1}."
    q = orc.gemv(np.asarray(wref[b + "attn_q.weight"], np.float32), orc.rmsnorm(h, wref[b + "attn_norm.weight"], eps))
    return q if rd == 0 else orc.rope(q, orc.rope_freqs(rd, base, nf), rd, dims.H, dims.D, n - 1)


def build(mgr, name, form, kind, **kw):
    from nfai_amd.llama_model import LlamaModel
    md, args = df.model_args(BY_NAME[name], form)
    return LlamaModel(mgr, md, weights(name, kind)[0], CAP, **args, **kw)


class Check:
    """What every case asserts; `bars` = DECODE or LOOSE."""

    def __init__(self, name, form, kind, bars, where):
        self.dims, self.form, self.where = BY_NAME[name], form, where
        self.scale, self.atol = bars
        self.ref, self.dflt = walk(name, form, kind), walk(name, "default", kind)
        self.err = self.moved = self.margin = 0.0
        self.k_moved = {}

    def logits(self, pos, lg, am=None, want=None):
        own = want is not None   # a reference of the caller's (the verify branch): no default-descriptor counterpart
        want = want if own else self.ref.logits[pos]
        bar = self.scale * max(1.0, float(np.abs(want).max()))
        err = float(np.abs(lg - want).max()) / bar
        self.err = max(self.err, err)
        assert err <= 1.0, (self.where, self.form, "position", pos, "max|dlogit| / bar", err)
        if am is not None:
            assert int(am) == int(np.argmax(lg)), (self.where, self.form, pos, int(am), int(np.argmax(lg)))
        if not own:
            self.moved = max(self.moved, float(np.abs(lg - self.dflt.logits[pos]).max()) / bar)
            self.margin = max(self.margin, float(np.abs(want - self.dflt.logits[pos]).max()) / bar)

    def rows(self, m, k_pos, v_pos):
        for l in range(self.dims.L):
            k = m.ReadKV(l, False, k_pos)
            np.testing.assert_allclose(k, self.ref.K[l][k_pos], rtol=0, atol=self.atol, err_msg=f"{self.where} {self.form} K block {l} position {k_pos}")
            np.testing.assert_allclose(m.ReadKV(l, True, v_pos), self.ref.V[l][v_pos], rtol=0, atol=self.atol,
                                       err_msg=f"{self.where} {self.form} V block {l} position {v_pos}")
            self.k_moved[l] = max(self.k_moved.get(l, 0.0), float(np.abs(k - self.dflt.K[l][k_pos]).max()) / self.atol)

    def q(self, m, want):
        np.testing.assert_allclose(m.Read(1, self.dims.H * self.dims.D), want, rtol=0, atol=self.atol, err_msg=f"{self.where} {self.form} q after RoPE")

    def finish(self):
        print(f"FORM {self.where} {self.dims.name} {self.form}: max|dlogit| {self.err:.4f} bars; from the default model: logits {self.moved:.1f} bars "
              f"(oracles {self.margin:.1f}), K rows {min(self.k_moved.values()):.1f} bars (smallest block)")
        assert sorted(self.k_moved) == list(range(self.dims.L))
        assert min(self.k_moved.values()) > 1.0, (self.where, self.form, self.k_moved)
        assert self.moved > 1.0, (self.where, self.form, self.moved, self.margin)


def dispose(*objs):
    for o in objs:
        if o is not None:
            o.Dispose()


# ---- single decode -----------------------------------------------------------------------------------------------------------------
def run_single(mgr, name, form, kind, bars, where, n=None, **kw):
    dims = BY_NAME[name]
    toks = df.tokens(dims, n)
    chk = Check(name, form, kind, bars, where)
    m = build(mgr, name, form, kind, **kw)
    try:
        for i, t in enumerate(toks):
            lg, am = m.Step(t)
            chk.logits(i, lg, am)
        assert m.Pos == len(toks)
        chk.rows(m, len(toks) - 1, 1)
        chk.q(m, q_last(name, form, kind, len(toks)))
    finally:
        m.Dispose()
    chk.finish()


SINGLE = {"graph": {}, "eager": dict(graph=False), "unfused": dict(unfused=True), "graph-kv16": dict(kv_f16=True),
          "eager-kv16": dict(graph=False, kv_f16=True)}


@pytest.mark.parametrize("name,form", cases())
@pytest.mark.parametrize("variant", list(SINGLE))
def test_single_decode_fp16(mgr, variant, name, form):
    kw = SINGLE[variant]
    run_single(mgr, name, form, "f16", LOOSE if kw.get("kv_f16") else DECODE, f"single {variant}", **kw)


@pytest.mark.parametrize("name,form", cases(models=[synth.TINY_D128]))
@pytest.mark.parametrize("variant", ["graph", "eager"])
def test_engine(mgr, variant, name, form):
    run_single(mgr, name, form, "f16", DECODE, f"engine {variant}", engine=True, **SINGLE[variant])


@pytest.mark.parametrize("name,form", cases())
@pytest.mark.parametrize("kind", ["q4_k_m", "all_q5_k", "all_q8_0", "all_q4_0"])
def test_single_decode_quantised(mgr, kind, name, form):
    run_single(mgr, name, form, kind, DECODE, f"single {kind}")


@pytest.mark.parametrize("form", df.forms_for(TINY_V520))
def test_single_decode_with_the_valu_kquant_lm_head(mgr, form):
    """520 vocabulary rows: the tied Q4_K table stays in its raw layout, the lm_head with the output RMSNorm (eps) runs in
    kernels_gemv_kq.hip and the embedding row comes from the raw blocks."""
    run_single(mgr, TINY_V520.name, form, "q4k_v520", DECODE, "single q4k_v520", n=df.N_POS["tiny-llama"])


OP_FORMS = {"half": (20, 10, 500000.0, df.EPS_BIG), "six": (6, 3, 10000.0, df.EPS_BIG), "cut": (24, 5, 1000.0, 1e-5), "none": (0, 0, 500000.0, df.EPS_BIG)}


@pytest.mark.parametrize("form", list(OP_FORMS))
def test_valu_kquant_qkv_rope_op(mgr, form):
    """RMSNorm -> q | k | v -> RoPE -> cache rows of kernels_gemv_kq.hip (Q4_K rows in the raw layout: 120 / 40 / 40 rows, no multiple
    of 16) under the forms at a head size of 40, position 37, against the fp32 operators of the oracle on the dequantised rows at
    the bar of tests/test_gpu_q4_0.py::test_qkv_rope_q4_0_op; the result is more than that bar from the default arguments'."""
    from nfai_amd._lib import F32, call
    from nfai_amd.hip import ShaderProperty
    from test_gpu_kquant import quantize, tol
    H, Hkv, D, E, pos = 3, 1, 40, 512, 37
    rd, nf, base, eps = OP_FORMS[form]
    r = np.random.Generator(np.random.PCG64(40 + rd))
    (rq, dq), (rk, dk), (rv, dv) = (quantize((0.05 * r.standard_normal((n, E))).astype(np.float32), Q4_K) for n in (H * D, Hkv * D, Hkv * D))
    bq, bk, bv = (mgr.UploadWeight(Q4_K, raw, n, E) for raw, n in ((rq, H * D), (rk, Hkv * D), (rv, Hkv * D)))
    x = (0.05 * r.standard_normal(E)).astype(np.float32)
    g = (1 + 0.1 * r.standard_normal(E)).astype(np.float32)
    freqs = np.zeros(max(rd // 2, 1), np.float32)
    freqs[:rd // 2] = orc.rope_freqs(rd, base, nf) if rd else []
    px, pg, pf = ShaderProperty(mgr, E), ShaderProperty(mgr, E), ShaderProperty(mgr, freqs.size)
    pq, kc, vc = ShaderProperty(mgr, H * D), ShaderProperty(mgr, (pos + 1) * Hkv * D), ShaderProperty(mgr, (pos + 1) * Hkv * D)
    px.SetValue(x); pg.SetValue(g); pf.SetValue(freqs)
    call("nfai_hip_gemv_qkv_rope", mgr.handle, bq.handle, bk.handle, bv.handle, Q4_K, px.handle, pg.handle, eps, pf.handle, rd,
         pq.handle, kc.handle, vc.handle, H, Hkv, D, pos, F32, E)

    def expect(rd_, freqs_, eps_):
        xn = orc.rmsnorm(x, g, eps_)
        q, k, v = orc.gemv(dq, xn), orc.gemv(dk, xn), orc.gemv(dv, xn)
        return (npo.rope(q, freqs_, rd_, H, D, pos).astype(np.float32), npo.rope(k, freqs_, rd_, Hkv, D, pos).astype(np.float32), v, xn)

    wq_, wk_, wv_, xn = expect(rd, freqs, eps)
    dq_, dk_, _, _ = expect(D, orc.rope_freqs(D), 1e-5)
    got_q, got_k, got_v = pq.GetValue(), kc.GetValue()[pos * Hkv * D:], vc.GetValue()[pos * Hkv * D:]
    bar_q, bar_k = 2 * tol(dq, xn) + 1e-6, 2 * tol(dk, xn) + 1e-6
    print(f"FORM op {form}: q {float((np.abs(got_q - wq_) / bar_q).max()):.3f} k {float((np.abs(got_k - wk_) / bar_k).max()):.3f} bars; "
          f"from the default arguments: q {float((np.abs(got_q - dq_) / bar_q).max()):.0f} k {float((np.abs(got_k - dk_) / bar_k).max()):.0f} bars")
    assert (np.abs(got_q - wq_) <= bar_q).all() and (np.abs(got_k - wk_) <= bar_k).all() and (np.abs(got_v - wv_) <= tol(dv, xn)).all()
    assert (np.abs(got_q - dq_) > bar_q).any() and (np.abs(got_k - dk_) > bar_k).any()


# ---- batches -----------------------------------------------------------------------------------------------------------------------
STARTS5 = (0, 3, 17, 40, 41)
STARTS16 = tuple((11 * s) % 45 for s in range(16))   # 16 different positions from 0 to 44


def run_batch(mgr, name, form, kind, starts, steps, where, wide=False, any_quant=False):
    from nfai_amd.llama_model import LlamaBatch
    dims = BY_NAME[name]
    toks = df.tokens(dims, df.N_WALK)
    chk = Check(name, form, kind, DECODE, where)
    ms, batch = [build(mgr, name, form, kind)], None
    try:
        ms += [build(mgr, name, form, kind, share_from=ms[0]) for _ in starts[1:]]
        for m, p in zip(ms, starts):   # every member to its own position through the single path, token by token
            m.Ingest(toks[:p])
            assert m.Pos == p
        batch = LlamaBatch(ms, wide=True) if wide else LlamaBatch(ms, quantized=kind != "f16", any_quant=any_quant)
        for i in range(steps):
            lg, am = batch.Step([toks[p + i] for p in starts])
            for s, p in enumerate(starts):
                chk.logits(p + i, lg[s], am[s])
        for m, p in zip(ms, starts):
            assert m.Pos == p + steps
            chk.rows(m, p + steps - 1, p)   # the last and the first row the batch wrote for this member
    finally:
        dispose(batch, *ms[::-1])
    chk.finish()


@pytest.mark.parametrize("name,form", cases())
def test_batch_fp16(mgr, name, form):
    run_batch(mgr, name, form, "f16", STARTS5, 8, "batch5")


@pytest.mark.parametrize("name,form", cases())
@pytest.mark.parametrize("kind", ["q4_k_m", "five"])
def test_batch_quantised(mgr, kind, name, form):
    run_batch(mgr, name, form, kind, STARTS5, 8, f"batch5 {kind}", any_quant=kind == "five")


@pytest.mark.parametrize("name,form", cases())
def test_batch_wide(mgr, name, form):
    run_batch(mgr, name, form, "f16", STARTS16, 4, "wide16", wide=True)


# ---- windows -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def verify_branch(name, form, kind, p):
    """The oracle behind tokens[:p]: tokens[p], then its own greedy tokens g1, g2, g3, then a WRONG fourth draft, then three more
    tokens.  (the 8 inputs, the logits of the 8 columns, whether every one of the first four ArgMax is clear of a near-tie at 5e-4)."""
    dims = BY_NAME[name]
    toks = df.tokens(dims, df.N_WALK)
    ref = orc.OracleLlama(df.odesc(dims, form, p + 8), weights(name, kind)[1])
    for t in toks[:p]:
        ref.step(t, want_logits=False)
    inputs, logits, clear = [toks[p]], [], True
    for i in range(8):
        lg = ref.step(inputs[i]).copy()
        logits.append(lg)
        top2 = np.partition(lg, -2)[-2:]
        if i < 4:
            clear = clear and float(top2[1] - top2[0]) > 2 * DECODE[0] * max(1.0, float(np.abs(lg).max()))
        g = orc.argmax(lg)
        inputs.append(g if i < 3 else ((g + 1) % dims.V if i == 3 else toks[p + i + 1]))
    ref.close()
    return inputs[:8], logits, clear


@pytest.mark.parametrize("name,form", cases(none=False))
@pytest.mark.parametrize("kind", ["f16", "q4_k_m"])
def test_window(mgr, kind, name, form):
    from nfai_amd.llama_model import LlamaWindow
    dims = BY_NAME[name]
    toks = df.tokens(dims, df.N_WALK)
    chk = Check(name, form, kind, DECODE, f"window8 {kind}")
    m, win = build(mgr, name, form, kind), None
    try:
        win = LlamaWindow(m, 8, quantized=kind != "f16")
        for p in (0, 37):   # column i against the oracle at position p + i
            m.Reset()
            m.Ingest(toks[:p])
            lg, am = win.Step(toks[p:p + 8])
            assert m.Pos == p + 8
            for i in range(8):
                chk.logits(p + i, lg[i], am[i])
        chk.rows(m, 44, 37)
        # verify: the token at position 37 and 7 drafts, the first 3 of them the model's own choice
        m.Reset()
        m.Ingest(toks[:37])
        inputs, wants, clear = verify_branch(name, form, kind, 37)
        lg, out = win.Verify(inputs[0], inputs[1:], want_logits=True)
        for i in range(8):
            chk.logits(37 + i, lg[i], want=wants[i])
        kept = 0
        while kept < 7 and inputs[kept + 1] == int(np.argmax(lg[kept])):
            kept += 1
        assert [int(t) for t in out] == [int(np.argmax(lg[i])) for i in range(kept + 1)] and m.Pos == 37 + kept + 1
        if clear:
            assert kept == 3, (kept, out, inputs)
    finally:
        dispose(win, m)
    chk.finish()


# ---- the MFMA prefill --------------------------------------------------------------------------------------------------------------
PREFILL = {"fused": ("f16", {}, None), "rope-kernel": ("f16", {}, "0"), "kv16": ("f16", dict(kv_f16=True), None), "q4_k_m": ("q4_k_m", {}, None)}


@pytest.mark.parametrize("name,form", cases())
@pytest.mark.parametrize("variant", list(PREFILL))
def test_prefill(mgr, monkeypatch, variant, name, form):
    kind, kw, rope_fused = PREFILL[variant]
    if rope_fused is not None:
        monkeypatch.setenv("NFAI_PREFILL_ROPE_FUSED", rope_fused)   # read at every prefill call
    dims = BY_NAME[name]
    toks = df.tokens(dims, df.N_WALK)
    for n, chunk in [(37, 64), (130, 64)] + ([(130, 128)] if dims.D == 128 else []):
        chk = Check(name, form, kind, LOOSE, f"prefill {variant} {n}/{chunk}")
        m = build(mgr, name, form, kind, max_batch=chunk, **kw)
        try:
            chk.logits(n - 1, m.Prefill(toks[:n]))
            assert m.Pos == n
            chk.rows(m, n - 1, 1)
            if n > chunk:
                chk.rows(m, chunk, chunk + 1)   # the first rows of a chunk behind the first (pos0 > 0)
            for i in range(4):
                lg, am = m.Step(toks[n + i])
                chk.logits(n + i, lg, am)
            chk.rows(m, n + 3, n)
        finally:
            m.Dispose()
        chk.finish()


# ---- pipeline stages ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", cases(none=False))
def test_two_stages_bit_identical_to_the_whole_model(mgr, name, form):
    """Two stages on one device, built as tests/test_gpu_model.py::test_pipeline_stages_bit_identical_to_single builds them:
    stage_ingest of 37 tokens (rows handed on in device memory), then 4 stage steps."""
    from nfai_amd.hip import ShaderProperty
    dims = BY_NAME[name]
    toks = df.tokens(dims, df.N_WALK)
    n = 37
    chk = Check(name, form, "f16", DECODE, "stages")
    whole = build(mgr, name, form, "f16", graph=False)
    s0 = build(mgr, name, form, "f16", layer_range=(0, 1))
    s1 = build(mgr, name, form, "f16", layer_range=(1, dims.L))
    rows, h01 = ShaderProperty(mgr, n * dims.E), ShaderProperty(mgr, dims.E)
    try:
        for i in range(n):
            chk.logits(i, *whole.Step(toks[i]))
        s0.StageIngest(toks[:n], None, rows.buffer.device_ptr)
        s1.StageIngest(None, rows.buffer.device_ptr, None, n)
        assert s0.Pos == s1.Pos == n
        for i in range(n, n + 4):
            want, am = whole.Step(toks[i])
            chk.logits(i, want, am)
            s0.StageStep(toks[i], None, h01.buffer.device_ptr)
            lg, am2 = s1.StageStep(0, h01.buffer.device_ptr, None, want_logits=True)
            np.testing.assert_array_equal(lg, want)
            assert am == am2
        for l in range(dims.L):
            for p in (0, n - 1, n + 3):
                for is_v in (False, True):
                    np.testing.assert_array_equal((s0 if l == 0 else s1).ReadKV(l, is_v, p), whole.ReadKV(l, is_v, p))
        chk.rows(whole, n + 3, 1)
    finally:
        dispose(s1, s0, whole)
    chk.finish()


# ---- refusal -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [d.name for d in MODELS])
def test_a_batch_refuses_members_whose_descriptors_differ(mgr, name):
    """A slot that shares member 0's tensors but differs from it in exactly one of eps, rope_dims, rope_n_freqs, rope_base is answered
    NFAI_ERR_UNSUPPORTED by _batch_create, _batch_create_ex and _batch_create_wide with the message of admit_member
    (llama_batch.hip; it is the message for tensors that are not shared as well: the control is the `good` slot, which shares
    them with the same descriptor and is admitted).  No handle comes back, and the members go on as a batch of their own
    afterwards.  That nothing stays allocated is NOT observed here: the ABI shows no allocation count and the free memory of a
    shared device moves under other processes.  It rests on the code: admit_member runs in front of `new Batch`, the first
    allocation of batch_create_impl."""
    import ctypes as C
    from nfai_amd import _lib
    from nfai_amd.llama_model import LlamaBatch, LlamaModel
    dims = BY_NAME[name]
    md, args = df.model_args(dims, "cut")
    w = weights(name, "f16")[0]
    m0 = LlamaModel(mgr, md, w, CAP, **args)
    good = LlamaModel(mgr, md, w, CAP, share_from=m0, **args)
    rd, nf, base, eps = df.resolve("cut", dims)
    others = {"eps": dict(args, dims=dict(args["dims"], eps=2e-5)), "rope_dims": dict(args, dims=dict(args["dims"], rope_dims=rd + 2)),
              "rope_n_freqs": dict(args, rope_n_freqs=nf + 1), "rope_base": dict(args, rope_base=base * 2)}
    made = []
    try:
        for field, a in others.items():
            bad = LlamaModel(mgr, md, w, CAP, share_from=m0, **a)
            made.append(bad)
            hs = (_lib.H * 2)(m0.handle.value, bad.handle.value)
            for fn, extra in (("nfai_hip_llama_batch_create", ()), ("nfai_hip_llama_batch_create_ex", (_lib.BATCH_QUANT,)),
                              ("nfai_hip_llama_batch_create_wide", (0,))):
                h = _lib.H()
                with pytest.raises(_lib.NfaiHipError, match="member 1 does not read the same tensors as member 0") as e:
                    _lib.call(fn, hs, 2, *extra, C.byref(h))
                assert e.value.code == _lib.ERR_UNSUPPORTED and not h.value, (field, fn, e.value.args, h.value)
        toks = df.tokens(dims, 4)
        ref = walk(name, "cut", "f16")
        for kw in ({}, dict(wide=True)):
            m0.Reset(); good.Reset()
            batch = LlamaBatch([m0, good], **kw)
            for i, t in enumerate(toks):
                lg, _ = batch.Step([t, t])
                for s in range(2):
                    assert np.abs(lg[s] - ref.logits[i]).max() <= DECODE[0] * max(1.0, float(np.abs(ref.logits[i]).max()))
            batch.Dispose()
    finally:
        dispose(*made, good, m0)
