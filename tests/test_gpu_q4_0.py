"""Q4_0 weights on the GPU against the oracle.

The reference throws for Q4_0 (NFAI.GGUF/Parser.cs:111-114), so parity is UNPINNED by the reference: the oracle is ggml's block_q4_0
(fp16 d, qs[16]; weight j = d * ((qs[j] & 0xF) - 8), weight j + 16 = d * ((qs[j] >> 4) - 8), d signed), restated below in NumPy,
followed by the reference's fp32 GEMV / the whole-model oracle on the dequantised weights.  The mirror of tests/test_gpu_q8_0.py case
for case; tol() and stage_tol() are its bounds restated (same arithmetic class: exact int32 dot products, 22-bit fixed-point
activations, fp32 scales).  The quantisation error itself is never measured."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth

pytestmark = pytest.mark.gpu

Q4_0, Q4_K, Q6_K = 2, 12, 14
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dequant_q4_0(raw, rows, cols):
    """ggml dequantize_row_q4_0: block i of a row = bytes [18 i, 18 i + 18): d = fp16 at +0, qs at +2 .. +18; weight j = low nibble
    of qs[j], weight j + 16 = its high nibble, each d * (q - 8) in fp32."""
    b = np.frombuffer(np.ascontiguousarray(raw, np.uint8).tobytes(), np.uint8).reshape(rows * cols // 32, 18)
    d = b[:, :2].copy().view(np.float16).astype(np.float32)[:, 0]
    q = np.concatenate([b[:, 2:] & 0xF, b[:, 2:] >> 4], axis=1).astype(np.float32) - np.float32(8)
    return (d[:, None] * q).reshape(rows, cols)


def quantize(W, qt=Q4_0):
    """W [N][K] fp32 -> (raw block bytes, dequantised fp32 [N][K])."""
    W = np.ascontiguousarray(W, np.float32)
    N, K = W.shape
    if qt == Q4_K:
        b = orc.quantize_q4k(W)
        return b, orc.dequant_q4k(b, N * K).reshape(N, K)
    if qt == Q6_K:
        b = orc.quantize_q6k(W)
        return b, orc.dequant_q6k(b, N * K).reshape(N, K)
    b = np.frombuffer(synth.quantize_q4_0(W), np.uint8).copy()
    return b, dequant_q4_0(b, N, K)


def tol(Wd, x):
    s = np.abs(Wd.astype(np.float64)) @ np.abs(x.astype(np.float64))
    return 2e-6 * np.sqrt(Wd.shape[1] / 256.0) * s + 1e-6


def stage_tol(Wd, x):
    """Bound for the int8-MFMA GEMV with no absolute floor: x rounded to 24 bits relative to each 256-element super-block's largest
    |x| (2^-21 * max|x_b| * sum_{k in b} |w_k|, twice the rounding error) plus the fp32 accumulation term of tol()."""
    W, xa = np.abs(Wd.astype(np.float64)), np.abs(x.astype(np.float64))
    N, K = W.shape
    bmax = xa.reshape(K // 256, 256).max(axis=1)
    return 2.0 ** -21 * (W.reshape(N, K // 256, 256).sum(axis=2) @ bmax) + 2e-6 * np.sqrt(K / 256.0) * (W @ xa)


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


def gemv(mgr, raw, N, K, x):
    from nfai_amd.shaders import MatrixMultiplyShader
    op = MatrixMultiplyShader(mgr, 1, K, N, None)
    op.GetWeightProperty().set(raw, Q4_0, N, K)
    op.GetInputProperty().SetValue(x)
    op.Compute()
    return op.GetOutputs()


@pytest.mark.parametrize("N,K", [(16, 256), (96, 256), (2048, 2048), (1024, 3072), (512, 8192), (304, 14336), (64, 28672)])
def test_gemv_q4_0(mgr, N, K):
    """One tile and one super-block; ragged tile counts against the grid; both super-blocks-per-wave settings (K <= 16384 and above)."""
    r = rng(N + K)
    raw, Wd = quantize((0.02 * r.standard_normal((N, K))).astype(np.float32))
    x = r.standard_normal(K).astype(np.float32)
    err = np.abs(gemv(mgr, raw, N, K, x) - orc.gemv(Wd, x))
    assert (err <= tol(Wd, x)).all(), (err.max(), tol(Wd, x).min())


@pytest.mark.parametrize("xscale", [0.0, 1e-30, 1e-6, 3e4], ids=["zero", "tiny", "small", "large"])
def test_gemv_q4_0_activation_range(mgr, xscale):
    N, K = 256, 2048
    r = rng(77)
    raw, Wd = quantize((0.02 * r.standard_normal((N, K))).astype(np.float32))
    x = (xscale * r.standard_normal(K)).astype(np.float32)
    if xscale == 1e-6:
        x[256:512] *= 1e6  # one loud super-block beside quiet ones
    got = gemv(mgr, raw, N, K, x)
    assert np.isfinite(got).all()
    ref = orc.gemv(Wd, x)
    if xscale == 0.0:
        assert (got == 0).all()
    # no absolute floor: at 1e-30 every output is ~1e-29, and at 1e-6 the quiet super-blocks must keep their own 24 bits
    bound = np.minimum(stage_tol(Wd, x), tol(Wd, x))
    err = np.abs(got - ref)
    assert (err <= bound).all(), (float((err / np.maximum(bound, 1e-300)).max()), float(err.max()), float(bound.min()))


def _f16_bytes(v):
    return np.asarray(v, np.float16).view(np.uint8).reshape(-1, 2)


def _extreme(kind, N, K, r):
    """Raw Q4_0 blocks [N * K / 32][18] of one extreme pattern, built from a quantised random matrix."""
    b = np.frombuffer(synth.quantize_q4_0((0.02 * r.standard_normal((N, K))).astype(np.float32)), np.uint8).copy().reshape(-1, 18)
    nb = b.shape[0]
    if kind == "codes_0":
        b[:, 2:] = 0x00
    elif kind == "codes_15":
        b[:, 2:] = 0xFF
    elif kind == "alternating":        # low nibble 0 / high nibble 15 in even blocks, the other way round in odd ones
        b[0::2, 2:] = 0xF0
        b[1::2, 2:] = 0x0F
    elif kind == "d_max":              # +-65504, sign alternating by block
        b[:, :2] = _f16_bytes(np.where(np.arange(nb) % 2 == 0, 65504.0, -65504.0))
    elif kind == "d_subnormal":        # the smallest fp16 subnormal, 2^-24
        b[:, :2] = _f16_bytes(np.full(nb, 2.0 ** -24))
    elif kind == "d_neg_zero":         # every third block of a row: d = -0.0 (what ggml stores for an all-zero block)
        b[0::3, :2] = _f16_bytes(np.full(len(b[0::3]), -0.0))
        assert (b[0::3, 1] == 0x80).all()
    elif kind == "d_sign_by_block":    # |d| kept, sign alternating block by block along every row
        d = np.abs(b[:, :2].copy().view(np.float16)[:, 0].astype(np.float32))
        b[:, :2] = _f16_bytes(np.where(np.arange(nb) % 2 == 0, d, -d))
    elif kind == "d_distinct":         # every (row of a tile, 32-block of a super-block) its own d: a permuted d plane shows
        row, blk = np.arange(nb) // (K // 32), np.arange(nb) % (K // 32)
        d = 2.0 ** -10 * (1 + row % 16 + 16 * (blk % 8)) * np.where((row + blk) % 2 == 0, 1.0, -1.0)   # 128 magnitudes, exact in fp16
        b[:, :2] = _f16_bytes(d)
        assert len(set(np.abs(d[(row < 16) & (blk < 8)]).tolist())) == 128
    else:
        raise KeyError(kind)
    return b.ravel()


@pytest.mark.parametrize("kind", ["codes_0", "codes_15", "alternating", "d_max", "d_subnormal", "d_neg_zero", "d_sign_by_block", "d_distinct"])
def test_gemv_q4_0_extreme_blocks(mgr, kind):
    N, K = 64, 1024
    r = rng(5)
    raw = _extreme(kind, N, K, r)
    Wd = dequant_q4_0(raw, N, K)
    assert np.isfinite(Wd).all()
    if kind == "codes_0":
        assert (Wd.reshape(-1, 32) == Wd.reshape(-1, 32)[:, :1]).all() and np.abs(Wd).max() > 0   # every weight of a block is -8 d
    if kind == "alternating":
        w = Wd.reshape(-1, 32)
        assert (np.sign(w[0, :16]) == -np.sign(w[0, 16:])).all()
        assert (np.abs(w[0::2, :16] / 8) == np.abs(w[0::2, 16:] / 7)).all() and (np.abs(w[1::2, :16] / 7) == np.abs(w[1::2, 16:] / 8)).all()
    x = r.standard_normal(K).astype(np.float32)
    got = gemv(mgr, raw, N, K, x)
    err = np.abs(got - orc.gemv(Wd, x))
    assert (err <= tol(Wd, x)).all(), (kind, float(err.max()), float(tol(Wd, x).min()))


@pytest.mark.parametrize("N,K", [(3072, 8192), (256, 28672)])
def test_gemv_fused_norm_and_residual_q4_0(mgr, N, K):
    from nfai_amd._lib import call
    from nfai_amd.hip import ShaderProperty
    r = rng(9 + K)
    raw, Wd = quantize((0.02 * r.standard_normal((N, K))).astype(np.float32))
    w = mgr.UploadWeight(Q4_0, raw, N, K)
    x = r.standard_normal(K).astype(np.float32)
    g = (1 + 0.1 * r.standard_normal(K)).astype(np.float32)
    res = r.standard_normal(N).astype(np.float32)
    px, pg, pr, py = ShaderProperty(mgr, K), ShaderProperty(mgr, K), ShaderProperty(mgr, N), ShaderProperty(mgr, N)
    px.SetValue(x); pg.SetValue(g); pr.SetValue(res)
    call("nfai_hip_gemv_fused", mgr.handle, w.handle, Q4_0, px.handle, pg.handle, 1e-5, pr.handle, py.handle, N, K)
    xn = orc.rmsnorm(x, g, 1e-5)
    assert (np.abs(py.GetValue() - orc.add(res, orc.gemv(Wd, xn))) <= tol(Wd, xn) + 1e-5).all()


def test_embed_q4_0(mgr):
    from nfai_amd._lib import call
    from nfai_amd.hip import ShaderProperty
    V, E = 304, 768
    raw, Wd = quantize((0.05 * rng(3).standard_normal((V, E))).astype(np.float32))
    tab = mgr.UploadWeight(Q4_0, raw, V, E)
    tok, y = ShaderProperty(mgr, 1, np.uint32), ShaderProperty(mgr, E)
    for t in (0, 1, 303, 123):
        tok.SetValue(np.array([t], np.uint32))
        call("nfai_hip_embed", mgr.handle, tab.handle, Q4_0, tok.handle, y.handle, E)
        np.testing.assert_array_equal(y.GetValue(), Wd[t])  # d * (q - 8) is exact in fp32


@pytest.mark.parametrize("V,E", [(128256, 256), (48, 256), (4000, 3072)])
def test_lmhead_argmax_q4_0(mgr, V, E):
    """Three equal maximal rows (identical block bytes): the first index wins."""
    from nfai_amd._lib import call
    from nfai_amd.hip import ShaderProperty
    r = rng(V + E)
    rows = min(V, 2048)
    W = np.tile((0.02 * r.standard_normal((rows, E))).astype(np.float32), ((V + rows - 1) // rows, 1))[:V].copy()
    W *= (1 + 0.01 * r.standard_normal((V, 1))).astype(np.float32)
    x = r.standard_normal(E).astype(np.float32)
    g = (1 + 0.1 * r.standard_normal(E)).astype(np.float32)
    xn = orc.rmsnorm(x, g, 1e-5)
    dup = (V - 1, 35, V // 2 + 1)
    for j in dup:
        W[j] = np.sign(xn) * 0.06
    raw, Wd = quantize(W)
    rb = raw.reshape(V, -1)
    assert (rb[dup[0]] == rb[dup[1]]).all() and (rb[dup[0]] == rb[dup[2]]).all()
    tab = mgr.UploadWeight(Q4_0, raw, V, E)
    px, pg, pl, pi = ShaderProperty(mgr, E), ShaderProperty(mgr, E), ShaderProperty(mgr, V), ShaderProperty(mgr, 1, np.uint32)
    px.SetValue(x); pg.SetValue(g)
    call("nfai_hip_lmhead_argmax", mgr.handle, tab.handle, Q4_0, px.handle, pg.handle, 1e-5, pl.handle, pi.handle, V, E)
    lg = pl.GetValue()
    want = orc.gemv(Wd, xn)
    assert (np.abs(lg - want) <= tol(Wd, xn)).all()
    assert int(pi.GetValue()[0]) == orc.argmax(want) == min(dup)


def test_gemm_kq_refuses_q4_0(mgr):
    from nfai_amd import _lib
    from nfai_amd.hip import ShaderProperty
    M, N, K = 64, 64, 256
    raw, _ = quantize((0.02 * rng(1).standard_normal((N, K))).astype(np.float32))
    w = mgr.UploadWeight(Q4_0, raw, N, K)
    pa, pc = ShaderProperty(mgr, M * K, np.float16), ShaderProperty(mgr, M * N)
    with pytest.raises(_lib.NfaiHipError, match="Q4_0") as e:
        _lib.call("nfai_hip_gemm_kq", mgr.handle, pa.handle, w.handle, Q4_0, 0, pc.handle, M, N, K)
    assert e.value.code == _lib.ERR_UNSUPPORTED


@pytest.mark.parametrize("E,F", [(3072, 8192), (256, 512)])
def test_gateup_silu_and_down_residual_q4_0(mgr, E, F):
    from nfai_amd._lib import call
    from nfai_amd.hip import ShaderProperty
    r = rng(E + F)
    (rg, dg), (ru, du), (rd, dd) = (quantize((0.02 * r.standard_normal(s)).astype(np.float32)) for s in ((F, E), (F, E), (E, F)))
    x = r.standard_normal(E).astype(np.float32)
    g = (1 + 0.1 * r.standard_normal(E)).astype(np.float32)
    pg_, pu, pd = mgr.UploadWeight(Q4_0, rg, F, E), mgr.UploadWeight(Q4_0, ru, F, E), mgr.UploadWeight(Q4_0, rd, E, F)
    px, pg, pa, py = ShaderProperty(mgr, E), ShaderProperty(mgr, E), ShaderProperty(mgr, F), ShaderProperty(mgr, E)
    px.SetValue(x); pg.SetValue(g)
    call("nfai_hip_gemv_gateup_silu", mgr.handle, pg_.handle, pu.handle, Q4_0, px.handle, pg.handle, 1e-5, pa.handle, F, E)
    xn = orc.rmsnorm(x, g, 1e-5)
    np.testing.assert_allclose(pa.GetValue(), orc.mul(orc.gemv(du, xn), orc.silu(orc.gemv(dg, xn))), rtol=1e-4, atol=2e-5)
    call("nfai_hip_gemv_fused", mgr.handle, pd.handle, Q4_0, pa.handle, 0, 0.0, px.handle, py.handle, E, F)
    assert (np.abs(py.GetValue() - orc.add(x, orc.gemv(dd, pa.GetValue()))) <= tol(dd, pa.GetValue()) + 1e-5).all()


@pytest.mark.parametrize("E", [3072, 17408])
def test_qkv_rope_q4_0_op(mgr, E):
    from nfai_amd._lib import call, F32
    from nfai_amd.hip import ShaderProperty
    H, Hkv, D, pos = 24, 8, 128, 5
    r = rng(31 + E)
    (rq, dq), (rk, dk), (rv, dv) = (quantize((0.02 * r.standard_normal((n, E))).astype(np.float32)) for n in (H * D, Hkv * D, Hkv * D))
    bq, bk, bv = mgr.UploadWeight(Q4_0, rq, H * D, E), mgr.UploadWeight(Q4_0, rk, Hkv * D, E), mgr.UploadWeight(Q4_0, rv, Hkv * D, E)
    x = r.standard_normal(E).astype(np.float32)
    g = (1 + 0.1 * r.standard_normal(E)).astype(np.float32)
    freqs = orc.rope_freqs(D)
    px, pg, pf = ShaderProperty(mgr, E), ShaderProperty(mgr, E), ShaderProperty(mgr, D // 2)
    pq, kc, vc = ShaderProperty(mgr, H * D), ShaderProperty(mgr, (pos + 1) * Hkv * D), ShaderProperty(mgr, (pos + 1) * Hkv * D)
    px.SetValue(x); pg.SetValue(g); pf.SetValue(freqs)
    call("nfai_hip_gemv_qkv_rope", mgr.handle, bq.handle, bk.handle, bv.handle, Q4_0, px.handle, pg.handle, 1e-5, pf.handle, D,
         pq.handle, kc.handle, vc.handle, H, Hkv, D, pos, F32, E)
    xn = orc.rmsnorm(x, g, 1e-5)
    q, k, v = orc.gemv(dq, xn), orc.gemv(dk, xn), orc.gemv(dv, xn)
    qr, kr = orc.rope(q, freqs, D, H, D, pos), orc.rope(k, freqs, D, Hkv, D, pos)
    assert (np.abs(pq.GetValue() - qr) <= 2 * tol(dq, xn) + 1e-6).all()
    krow = kc.GetValue()[pos * Hkv * D:]
    vrow = vc.GetValue()[pos * Hkv * D:]
    assert (np.abs(krow - kr) <= 2 * tol(dk, xn) + 1e-6).all()
    assert (np.abs(vrow - v) <= tol(dv, xn)).all()


# ---- whole models -------------------------------------------------------------------------------------------------------------

def mix_type(name, mix, dims):
    """all_q4_0 / q4_0: synth.q4_0_type; qk_q4_0_v_q6k: attn_v in Q6_K, the rest Q4_0 (the q|k|v launch splits at the change);
    a (q, k, v) tuple: those types for the three attention inputs, the rest Q4_0."""
    if isinstance(mix, tuple):
        parts = name.split(".")
        return mix[("attn_q", "attn_k", "attn_v").index(parts[2])] if len(parts) > 2 and parts[2] in ("attn_q", "attn_k", "attn_v") else Q4_0
    if mix == "qk_q4_0_v_q6k":
        return Q6_K if name.endswith("attn_v.weight") else Q4_0
    return synth.q4_0_type(name, dims, mix)


_WEIGHTS = {}


def quant_weights(dims, seed, mix="all_q4_0", std=0.05):
    """synth weights -> ({name: QuantTensor | gains}, {name: dequantised fp32 | gains}), quantised once per module."""
    from nfai_amd.llama_model import QuantTensor
    key = (dims.name, seed, mix, std)
    if key not in _WEIGHTS:
        w = synth.make_weights(dims, seed=seed, std=std)
        wq, wref = {}, {}
        for name, a in w.items():
            if a.ndim == 1:
                wq[name] = wref[name] = a
                continue
            qt = mix_type(name, mix, dims)
            raw, deq = quantize(a.astype(np.float32), qt)
            wq[name] = QuantTensor(raw, qt, a.shape)
            wref[name] = deq
        _WEIGHTS[key] = (wq, wref)
    return _WEIGHTS[key]


def ddict(dims):
    return dict(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, eps=1e-5, rope_dims=dims.D, rope_base=500000.0)


def odesc(dims, C):
    return orc.LlamaDesc(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, C=C)


@pytest.mark.parametrize("dims", [synth.TINY, synth.TINY_D128], ids=lambda d: d.name)
@pytest.mark.parametrize("mix", ["all_q4_0", "q4_0", "qk_q4_0_v_q6k"])
def test_model_q4_0_graph_eager_unfused(mgr, dims, mix):
    """Graph, eager and the unfused 1:1 chain against OracleLlama: greedy tokens identical, logits within 5e-4 * max(1, |logit|)
    (the bar of test_model_q8_0_graph_eager_unfused).  q4_0: the head in Q6_K; qk_q4_0_v_q6k: the q|k|v launch splits."""
    from nfai_amd.llama_model import LlamaModel
    wq, wref = quant_weights(dims, 61, mix)
    md = synth.make_metadata(dims)
    models = [LlamaModel(mgr, md, wq, 40, dims=ddict(dims)), LlamaModel(mgr, md, wq, 40, dims=ddict(dims), graph=False),
              LlamaModel(mgr, md, wq, 40, dims=ddict(dims), unfused=True)]
    ref = orc.OracleLlama(odesc(dims, 40), wref)
    tok = 7
    for i in range(24):
        want = ref.step(tok)
        scale = max(1.0, float(np.abs(want).max()))
        for m in models:
            lg, am = m.Step(tok)
            assert np.abs(lg - want).max() <= 5e-4 * scale, (i, np.abs(lg - want).max())
            assert am == orc.argmax(want)
        tok = orc.argmax(want)
    total, _ = models[0].BytesPerToken(0)
    prof = models[0].ProfileStep(tok)
    for m in models:
        m.Dispose()
    assert prof["qkv"][1] == (2 if mix == "qk_q4_0_v_q6k" else 1) * dims.L, prof
    if mix == "all_q4_0":
        E, F, V, KD, HD = dims.E, dims.F, dims.V, dims.Hkv * dims.D, dims.H * dims.D
        blk = (HD * E + 2 * KD * E + E * HD + 3 * E * F) * 18 // 32
        kv = 2 * KD * 4 * 1 + 2 * KD * 4
        head = V * E * 18 // 32
        assert total == dims.L * (blk + kv) + E * 18 // 32 + head


def test_model_q4_0_fp16_kv(mgr):
    """The same with an fp16 KV cache, at the bar the fp16-cache runs of the batched tests state (2e-2 * max(1, |logit|))."""
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY_D128
    wq, wref = quant_weights(dims, 61, "all_q4_0")
    m = LlamaModel(mgr, synth.make_metadata(dims), wq, 40, dims=ddict(dims), kv_f16=True)
    ref = orc.OracleLlama(odesc(dims, 40), wref)
    tok = 7
    for i in range(24):
        want = ref.step(tok)
        lg, _ = m.Step(tok)
        assert np.abs(lg - want).max() <= 2e-2 * max(1.0, float(np.abs(want).max())), i
        tok = orc.argmax(want)
    m.Dispose()


def _ingest_case(mgr, n, chunk):
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY_D128
    wq, wref = quant_weights(dims, 67)
    m = LlamaModel(mgr, synth.make_metadata(dims), wq, 160, dims=ddict(dims), max_batch=chunk)
    mt = LlamaModel(mgr, synth.make_metadata(dims), wq, 160, dims=ddict(dims))   # no workspace: token by token
    ref = orc.OracleLlama(odesc(dims, 160), wref)
    toks = synth.make_tokens(dims, n, seed=21)
    want = None
    for t in toks:
        want = ref.step(int(t))
    got = m.Prefill(toks)
    mt.Prefill(toks)
    assert m.Pos == n
    tol5 = 2e-2 * max(1.0, float(np.abs(want).max()))
    assert np.abs(got - want).max() <= tol5, np.abs(got - want).max()
    assert int(np.argmax(got)) == orc.argmax(want)
    kv_mfma, kv_tok = m.ReadKV(dims.L - 1, False, n - 1), mt.ReadKV(dims.L - 1, False, n - 1)
    np.testing.assert_allclose(kv_mfma, ref.kcache(dims.L - 1)[n - 1], rtol=0, atol=2e-2)
    assert not np.array_equal(kv_mfma, kv_tok)   # the MFMA path ran: fp16 operands, not the M = 1 path's bits
    tok = orc.argmax(want)
    for _ in range(6):
        lg, _ = m.Step(tok)
        wl = ref.step(tok)
        assert np.abs(lg - wl).max() <= tol5
        tok = orc.argmax(wl)
    m.Dispose()
    mt.Dispose()


@pytest.mark.parametrize("n,chunk", [(70, 64), (40, 128)], ids=["chunked", "one-chunk"])
def test_prefill_mfma_q4_0(mgr, n, chunk):
    _ingest_case(mgr, n, chunk)


def test_prefill_q4_0_kept_copies_match_the_per_block_scratch(mgr, monkeypatch):
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY_D128
    wq, _ = quant_weights(dims, 68)
    toks = synth.make_tokens(dims, 100, seed=22)
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("NFAI_PREFILL_WIDE_ALL", mode)
        m = LlamaModel(mgr, synth.make_metadata(dims), wq, 128, dims=ddict(dims), max_batch=64)
        a = m.Prefill(toks)
        kv = m.ReadKV(dims.L - 1, True, 99)
        m.Reset()
        assert np.array_equal(a, m.Prefill(toks))
        outs[mode] = (a, kv)
        m.Dispose()
    for x, y in zip(outs["1"], outs["0"]):
        assert np.array_equal(x, y)


def test_prefill_q4_0_under_fused_flag_in_child_process():
    """NFAI_PREFILL_FUSED=1 sends K-quant matrices to the dequant-in-LDS GEMM; Q4_0 matrices are still widened.  Read once per
    process: the ingest tests run again in a child with the variable set."""
    env = dict(os.environ, NFAI_PREFILL_FUSED="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_q4_0.py"), "-m", "gpu", "-x", "-q",
                        "-k", "test_prefill_mfma_q4_0", "-p", "no:cacheprovider"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("ranges", [[(0, 2), (2, 3)], [(0, 1), (1, 2), (2, 3)]], ids=["2-stage", "3-stage"])
def test_pipeline_stages_q4_0(mgr, ranges):
    """Stages of a Q4_0 model (stage_ingest for the prompt, stage_step for the tokens; a second slot made with share_tensors)
    against the single-stage model: the ingested prompt and the steps within the fp16 tolerance, the ArgMax equal."""
    import torch
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY_D128
    wq, _ = quant_weights(dims, 71)
    md = synth.make_metadata(dims)
    whole = LlamaModel(mgr, md, wq, 64, dims=ddict(dims), max_batch=32)
    stages = [LlamaModel(mgr, md, wq, 64, dims=ddict(dims), layer_range=rg, max_batch=32) for rg in ranges]
    slots = [LlamaModel(mgr, md, wq, 64, dims=ddict(dims), layer_range=rg, max_batch=32, share_from=s) for rg, s in zip(ranges, stages)]
    toks = synth.make_tokens(dims, 20, seed=5)
    rows = torch.zeros((len(toks), dims.E), dtype=torch.float32, device="cuda")
    for chain in (stages, slots):
        for i, st in enumerate(chain):
            first, last = i == 0, i == len(chain) - 1
            st.StageIngest(toks[:-1] if first else None, None if first else rows.data_ptr(), None if last else rows.data_ptr(),
                           None if first else len(toks) - 1)
        torch.cuda.synchronize()
    whole.Ingest(toks[:-1])
    tok = int(toks[-1])
    h = torch.zeros(dims.E, dtype=torch.float32, device="cuda")
    for step in range(6):
        want, wam = whole.Step(tok)
        for chain in (stages, slots):
            for i, st in enumerate(chain):
                first, last = i == 0, i == len(chain) - 1
                lg, am = st.StageStep(tok if first else 0, None if first else h.data_ptr(), None if last else h.data_ptr(),
                                      want_logits=last)
            assert np.abs(lg - want).max() <= 2e-2 * max(1.0, float(np.abs(want).max()))
            assert am == wam, step
        tok = wam
    for m in [whole] + stages + slots:
        m.Dispose()


def test_q4_0_gguf_file_to_generation(mgr, tmp_path):
    """A Q4_0 GGUF file (synth.q4_0_type: every matrix Q4_0, the tied embedding Q6_K) -> Parser().Parse -> the provider's model ->
    greedy generation through RunAsync, against the oracle's greedy tokens on the dequantised weights read back from the same file."""
    from nfai_amd import gguf
    from nfai_amd.llama_model import LlamaModelFactory, ModelOptions
    from test_gpu_window_decode import _IdTokenizer
    dims = synth.TINY
    wq, _ = quant_weights(dims, 81, "q4_0")
    path = str(tmp_path / "q4_0.gguf")
    gguf.write_model(path, synth.make_metadata(dims), wq)
    _, t = gguf.Parser().Read(path)
    assert all(t[k].ggml_type == synth.q4_0_type(k, dims) for k in wq if not isinstance(wq[k], np.ndarray))
    assert t["blk.0.attn_q.weight"].ggml_type == Q4_0 and t["token_embd.weight"].ggml_type == Q6_K

    def deq(v):
        if not hasattr(v, "ggml_type"):
            return v
        return dequant_q4_0(v.data, *v.shape) if v.ggml_type == Q4_0 else orc.dequant_q6k(v.data, v.shape[0] * v.shape[1]).reshape(v.shape)

    fac = LlamaModelFactory(0)
    m = gguf.Parser([fac]).Parse(ModelOptions(GGUFPath=path, KVCacheSize=64))
    ref = orc.OracleLlama(odesc(dims, 64), {k: deq(v) for k, v in t.items()})
    tok, want_toks = 3, []
    for _ in range(12):
        lg, am = m.Step(tok)
        want = ref.step(tok)
        assert np.abs(lg - want).max() <= 5e-4 * max(1.0, float(np.abs(want).max()))
        assert am == orc.argmax(want)
        tok = am
        want_toks.append(int(am))
    m.Reset()
    m.tokenizer = _IdTokenizer()
    m.promptPrefill = False
    got = [int(s) for s in "".join(m.RunAsync("3", greedy=True, max_tokens=12)).split()]
    assert got == want_toks[:len(got)] and len(got) >= 1
    m.Dispose()
    fac.Dispose()


def test_decode_q4_0_is_bit_reproducible(mgr):
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY_D128
    wq, _ = quant_weights(dims, 91)
    a = LlamaModel(mgr, synth.make_metadata(dims), wq, 160, dims=ddict(dims))
    b = LlamaModel(mgr, synth.make_metadata(dims), wq, 160, dims=ddict(dims))
    toks = synth.make_tokens(dims, 150, seed=4)
    first = [a.Step(int(t))[0] for t in toks]
    a.Reset()
    for i, t in enumerate(toks):
        la, _ = a.Step(int(t))
        lb, _ = b.Step(int(t))
        assert np.array_equal(la, first[i]) and np.array_equal(lb, first[i]), i
    a.Dispose()
    b.Dispose()
