"""Q5_K weights on the GPU against the oracle.

The reference has no Q5_K path (NFAI.GGUF/Parser.cs:111-114 throws "Unsupported data type"), so parity is UNPINNED by the
reference: the oracle is ggml's block_q5_K (fp16 d, fp16 dmin, scales[12], qh[32], qs[128]; weight = d * sc * q - dmin * m with
q = nibble | fifth bit << 4), restated below in NumPy (tests/test_q5_k.py pins the restatement), followed by the reference's fp32
GEMV / the whole-model oracle on the dequantised weights.  Q6_K matrices of the Q5_K_M mix go through the oracle's Q6_K dequantiser.
Tolerances are the ones the K-quant and model tests state (tests/test_gpu_kquant.py, tests/test_gpu_model.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth

pytestmark = pytest.mark.gpu

Q5_K, Q6_K = 13, 14
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dequant_q5_k(raw, rows, cols):
    """ggml dequantize_row_q5_K, vectorised: for pair n (sub-blocks 2n, 2n+1) and l = 0..31, q = (qs[32n + l] & 0xF | bit 2n of
    qh[l] << 4) and (qs[32n + l] >> 4 | bit 2n+1 of qh[l] << 4); (sc, m) = get_scale_min_k4; y = d * sc * q - dmin * m."""
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


def quantize(W, qt=Q5_K):
    """W [N][K] fp32 -> (raw block bytes, dequantised fp32 [N][K])."""
    N, K = W.shape
    if qt == Q6_K:
        b = orc.quantize_q6k(W)
        return b, orc.dequant_q6k(b, N * K).reshape(N, K)
    b = np.frombuffer(synth.quantize_q5_k(W), np.uint8).copy()
    return b, dequant_q5_k(b, N, K)


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
    op.GetWeightProperty().set(raw, Q5_K, N, K)
    op.GetInputProperty().SetValue(x)
    op.Compute()
    return op.GetOutputs()


@pytest.mark.parametrize("N,K", [(2048, 2048), (1024, 3072), (512, 8192), (96, 256), (304, 14336), (4096, 14336), (64, 28672)])
def test_gemv_q5_k(mgr, N, K):
    r = rng(N + K)
    raw, Wd = quantize((0.02 * r.standard_normal((N, K))).astype(np.float32))
    x = r.standard_normal(K).astype(np.float32)
    err = np.abs(gemv(mgr, raw, N, K, x) - orc.gemv(Wd, x))
    assert (err <= tol(Wd, x)).all(), (err.max(), tol(Wd, x).min())


@pytest.mark.parametrize("xscale", [0.0, 1e-30, 1e-6, 3e4], ids=["zero", "tiny", "small", "large"])
def test_gemv_q5_k_activation_range(mgr, xscale):
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


@pytest.mark.parametrize("case", ["all_zero", "all_31", "every_qh_bit", "max_scales_mins", "one_qh_bit_per_row"])
def test_gemv_q5_k_extreme_codes(mgr, case):
    """Codes 0 and 31 everywhere, every fifth bit set, the largest 6-bit scales and mins, and a single qh bit per row (each row a
    different (l, bit): a fifth bit landing on the wrong weight changes exactly that row's output)."""
    N, K = 64, 1024
    r = rng(5)
    b = np.frombuffer(synth.quantize_q5_k((0.02 * r.standard_normal((N, K))).astype(np.float32)), np.uint8).copy().reshape(-1, 176)
    if case == "all_zero":
        b[:, 16:176] = 0
    elif case == "all_31":
        b[:, 16:176] = 0xFF
    elif case == "every_qh_bit":
        b[:, 16:48] = 0xFF
    elif case == "max_scales_mins":
        b[:, 4:16] = 0xFF
    else:
        b[:, 16:48] = 0
        for row in range(N):
            l, bit = (row * 7) % 32, row % 8
            b[row * (K // 256) + row % (K // 256), 16 + l] = 1 << bit
    raw = b.ravel()
    Wd = dequant_q5_k(raw, N, K)
    x = r.standard_normal(K).astype(np.float32)
    assert (np.abs(gemv(mgr, raw, N, K, x) - orc.gemv(Wd, x)) <= tol(Wd, x)).all()


@pytest.mark.parametrize("N,K", [(3072, 8192), (3072, 14336), (256, 28672)])
def test_gemv_fused_norm_and_residual_q5_k(mgr, N, K):
    """K = 14336 and 28672: four and eight super-blocks per wave with the RMSNorm gains."""
    from nfai_amd._lib import call
    from nfai_amd.hip import ShaderProperty
    r = rng(9 + K)
    raw, Wd = quantize((0.02 * r.standard_normal((N, K))).astype(np.float32))
    w = mgr.UploadWeight(Q5_K, raw, N, K)
    x = r.standard_normal(K).astype(np.float32)
    g = (1 + 0.1 * r.standard_normal(K)).astype(np.float32)
    res = r.standard_normal(N).astype(np.float32)
    px, pg, pr, py = ShaderProperty(mgr, K), ShaderProperty(mgr, K), ShaderProperty(mgr, N), ShaderProperty(mgr, N)
    px.SetValue(x); pg.SetValue(g); pr.SetValue(res)
    call("nfai_hip_gemv_fused", mgr.handle, w.handle, Q5_K, px.handle, pg.handle, 1e-5, pr.handle, py.handle, N, K)
    xn = orc.rmsnorm(x, g, 1e-5)
    assert (np.abs(py.GetValue() - orc.add(res, orc.gemv(Wd, xn))) <= tol(Wd, xn) + 1e-5).all()


def test_embed_q5_k(mgr):
    from nfai_amd._lib import call
    from nfai_amd.hip import ShaderProperty
    V, E = 304, 768
    raw, Wd = quantize((0.05 * rng(3).standard_normal((V, E))).astype(np.float32))
    tab = mgr.UploadWeight(Q5_K, raw, V, E)
    tok, y = ShaderProperty(mgr, 1, np.uint32), ShaderProperty(mgr, E)
    for t in (0, 1, 303, 123):
        tok.SetValue(np.array([t], np.uint32))
        call("nfai_hip_embed", mgr.handle, tab.handle, Q5_K, tok.handle, y.handle, E)
        np.testing.assert_array_equal(y.GetValue(), Wd[t])  # d * sc * q - dmin * m in the restatement's order


@pytest.mark.parametrize("V,E", [(128256, 256), (48, 256), (4000, 3072)])
def test_lmhead_argmax_q5_k(mgr, V, E):
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
    tab = mgr.UploadWeight(Q5_K, raw, V, E)
    px, pg, pl, pi = ShaderProperty(mgr, E), ShaderProperty(mgr, E), ShaderProperty(mgr, V), ShaderProperty(mgr, 1, np.uint32)
    px.SetValue(x); pg.SetValue(g)
    call("nfai_hip_lmhead_argmax", mgr.handle, tab.handle, Q5_K, px.handle, pg.handle, 1e-5, pl.handle, pi.handle, V, E)
    lg = pl.GetValue()
    want = orc.gemv(Wd, xn)
    assert (np.abs(lg - want) <= tol(Wd, xn)).all()
    assert int(pi.GetValue()[0]) == orc.argmax(want) == min(dup)


def test_gemm_kq_refuses_q5_k(mgr):
    from nfai_amd import _lib
    from nfai_amd.hip import ShaderProperty
    M, N, K = 64, 64, 256
    raw, _ = quantize((0.02 * rng(1).standard_normal((N, K))).astype(np.float32))
    w = mgr.UploadWeight(Q5_K, raw, N, K)
    pa, pc = ShaderProperty(mgr, M * K, np.float16), ShaderProperty(mgr, M * N)
    with pytest.raises(_lib.NfaiHipError) as e:
        _lib.call("nfai_hip_gemm_kq", mgr.handle, pa.handle, w.handle, Q5_K, 0, pc.handle, M, N, K)
    assert e.value.code == _lib.ERR_UNSUPPORTED and "Q5_K" in str(e.value)


@pytest.mark.parametrize("E,F", [(3072, 8192), (4096, 14336), (256, 512)])
def test_gateup_silu_and_down_residual_q5_k(mgr, E, F):
    from nfai_amd._lib import call
    from nfai_amd.hip import ShaderProperty
    r = rng(E + F)
    (rg, dg), (ru, du), (rd, dd) = (quantize((0.02 * r.standard_normal(s)).astype(np.float32)) for s in ((F, E), (F, E), (E, F)))
    x = r.standard_normal(E).astype(np.float32)
    g = (1 + 0.1 * r.standard_normal(E)).astype(np.float32)
    pg_, pu, pd = mgr.UploadWeight(Q5_K, rg, F, E), mgr.UploadWeight(Q5_K, ru, F, E), mgr.UploadWeight(Q5_K, rd, E, F)
    px, pg, pa, py = ShaderProperty(mgr, E), ShaderProperty(mgr, E), ShaderProperty(mgr, F), ShaderProperty(mgr, E)
    px.SetValue(x); pg.SetValue(g)
    call("nfai_hip_gemv_gateup_silu", mgr.handle, pg_.handle, pu.handle, Q5_K, px.handle, pg.handle, 1e-5, pa.handle, F, E)
    xn = orc.rmsnorm(x, g, 1e-5)
    np.testing.assert_allclose(pa.GetValue(), orc.mul(orc.gemv(du, xn), orc.silu(orc.gemv(dg, xn))), rtol=1e-4, atol=2e-5)
    call("nfai_hip_gemv_fused", mgr.handle, pd.handle, Q5_K, pa.handle, 0, 0.0, px.handle, py.handle, E, F)
    assert (np.abs(py.GetValue() - orc.add(x, orc.gemv(dd, pa.GetValue()))) <= tol(dd, pa.GetValue()) + 1e-5).all()


@pytest.mark.parametrize("E", [3072, 4096, 14336])
def test_qkv_rope_q5_k_op(mgr, E):
    from nfai_amd._lib import call, F32
    from nfai_amd.hip import ShaderProperty
    H, Hkv, D, pos = 24, 8, 128, 5
    r = rng(31 + E)
    (rq, dq), (rk, dk), (rv, dv) = (quantize((0.02 * r.standard_normal((n, E))).astype(np.float32)) for n in (H * D, Hkv * D, Hkv * D))
    bq, bk, bv = mgr.UploadWeight(Q5_K, rq, H * D, E), mgr.UploadWeight(Q5_K, rk, Hkv * D, E), mgr.UploadWeight(Q5_K, rv, Hkv * D, E)
    x = r.standard_normal(E).astype(np.float32)
    g = (1 + 0.1 * r.standard_normal(E)).astype(np.float32)
    freqs = orc.rope_freqs(D)
    px, pg, pf = ShaderProperty(mgr, E), ShaderProperty(mgr, E), ShaderProperty(mgr, D // 2)
    pq, kc, vc = ShaderProperty(mgr, H * D), ShaderProperty(mgr, (pos + 1) * Hkv * D), ShaderProperty(mgr, (pos + 1) * Hkv * D)
    px.SetValue(x); pg.SetValue(g); pf.SetValue(freqs)
    call("nfai_hip_gemv_qkv_rope", mgr.handle, bq.handle, bk.handle, bv.handle, Q5_K, px.handle, pg.handle, 1e-5, pf.handle, D,
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

def quant_weights(dims, seed, mix="all_q5_k"):
    """synth weights -> ({name: QuantTensor | gains}, {name: dequantised fp32 | gains}).  mix: "all_q5_k" (every matrix, the
    embedding included), "q5_k_m" (synth.q5_k_m_type), or a (q, k, v) tuple of types for attn_q / attn_k / attn_v of every block
    (the rest Q5_K)."""
    from nfai_amd.llama_model import QuantTensor
    w = synth.make_weights(dims, seed=seed, std=0.05)
    wq, wref = {}, {}
    for name, a in w.items():
        if a.ndim == 1:
            wq[name] = wref[name] = a
            continue
        if mix == "q5_k_m":
            qt = synth.q5_k_m_type(name, dims)
        elif isinstance(mix, tuple) and name.endswith(("attn_q.weight", "attn_k.weight", "attn_v.weight")):
            qt = mix[("attn_q", "attn_k", "attn_v").index(name.split(".")[2])]
        else:
            qt = Q5_K
        raw, deq = quantize(a.astype(np.float32), qt)
        wq[name] = QuantTensor(raw, qt, a.shape)
        wref[name] = deq
    return wq, wref


def ddict(dims):
    return dict(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, eps=1e-5, rope_dims=dims.D, rope_base=500000.0)


def odesc(dims, C):
    return orc.LlamaDesc(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, C=C)


def run_against_oracle(mgr, dims, wq, wref, steps, **variants):
    from nfai_amd.llama_model import LlamaModel
    md = synth.make_metadata(dims)
    models = [LlamaModel(mgr, md, wq, 40, dims=ddict(dims), **kw) for kw in variants.values()]
    ref = orc.OracleLlama(odesc(dims, 40), wref)
    tok = 7
    for i in range(steps):
        want = ref.step(tok)
        scale = max(1.0, float(np.abs(want).max()))
        for m in models:
            lg, am = m.Step(tok)
            assert np.abs(lg - want).max() <= 5e-4 * scale, (i, np.abs(lg - want).max())
            assert am == orc.argmax(want)
        tok = orc.argmax(want)
    return models


@pytest.mark.parametrize("dims", [synth.TINY, synth.TINY_D128], ids=lambda d: d.name)
@pytest.mark.parametrize("mix", ["all_q5_k", "q5_k_m"])
def test_model_q5_k_graph_eager_unfused(mgr, dims, mix):
    """Graph, eager and the unfused 1:1 chain against OracleLlama: greedy tokens identical, logits within 5e-4 * max(1, |logit|).
    all_q5_k: a Q5_K token_embd (through the q|k|v launch's BEGIN prologue in graph / eager, k_embed_t16 unfused) and, on TINY, a
    tied Q5_K lm_head.  q5_k_m: llama.cpp's mix; one block of each dims keeps attn_v in Q6_K (the mixed q|k|v launch)."""
    wq, wref = quant_weights(dims, 61, mix)
    models = run_against_oracle(mgr, dims, wq, wref, 24, graph={}, eager={"graph": False}, unfused={"unfused": True})
    total, _ = models[0].BytesPerToken(0)
    for m in models:
        m.Dispose()
    if mix == "all_q5_k":
        E, F, V, KD, HD = dims.E, dims.F, dims.V, dims.Hkv * dims.D, dims.H * dims.D
        blk = (HD * E + 2 * KD * E + E * HD + 3 * E * F) * 176 // 256
        kv = 2 * KD * 4 * 1 + 2 * KD * 4
        assert total == dims.L * (blk + kv) + E * 176 // 256 + V * E * 176 // 256


@pytest.mark.parametrize("qkv", [(a, b, c) for a in (Q5_K, Q6_K) for b in (Q5_K, Q6_K) for c in (Q5_K, Q6_K)],
                         ids=lambda t: "".join("5" if x == Q5_K else "6" for x in t))
def test_qkv_rope_q5_k_q6_k_combinations(mgr, qkv):
    """Every Q5_K / Q6_K assignment of (q, k, v): one mixed q|k|v launch (or a plain one when all agree), graph and eager."""
    dims = synth.TINY_D128
    wq, wref = quant_weights(dims, 63, qkv)
    for m in run_against_oracle(mgr, dims, wq, wref, 10, graph={}, eager={"graph": False}):
        m.Dispose()


def _ingest_case(mgr, n, chunk, mix="q5_k_m"):
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY_D128
    wq, wref = quant_weights(dims, 67, mix)
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


@pytest.mark.parametrize("n,chunk,mix", [(70, 64, "q5_k_m"), (40, 128, "q5_k_m"), (150, 32, "all_q5_k")],
                         ids=["chunked", "one-chunk", "five-chunks-all-q5_k"])
def test_prefill_mfma_q5_k(mgr, n, chunk, mix):
    _ingest_case(mgr, n, chunk, mix)


def test_prefill_q5_k_under_fused_flag_in_child_process():
    """NFAI_PREFILL_FUSED=1 sends Q4_K / Q6_K matrices to the dequant-in-LDS GEMM; Q5_K matrices are still widened.  Read once per
    process: the ingest tests run again in a child with the variable set."""
    env = dict(os.environ, NFAI_PREFILL_FUSED="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_q5_k.py"), "-m", "gpu", "-x", "-q",
                        "-k", "test_prefill_mfma_q5_k", "-p", "no:cacheprovider"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "3 passed" in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("ranges", [[(0, 2), (2, 3)], [(0, 1), (1, 2), (2, 3)]], ids=["2-stage", "3-stage"])
def test_pipeline_stages_q5_k(mgr, ranges):
    """Stages of a Q5_K_M model (stage_ingest for the prompt, stage_step for the tokens; a second slot made with share_tensors)
    against the single-stage model: stage steps bit-identical, the ingested prompt within the fp16 tolerance."""
    import torch
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY_D128
    wq, _ = quant_weights(dims, 71, "q5_k_m")
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


def test_q5_k_gguf_file_to_generation(mgr, tmp_path):
    """A Q5_K_M GGUF file (TINY: tied Q6_K embedding, Q5_K / Q6_K blocks) -> Parser().Parse -> the provider's model -> greedy
    generation, against the oracle on the dequantised weights read back from the same file."""
    from nfai_amd import gguf
    from nfai_amd.llama_model import LlamaModelFactory, ModelOptions
    dims = synth.TINY
    wq, wref = quant_weights(dims, 81, "q5_k_m")
    path = str(tmp_path / "q5_k_m.gguf")
    gguf.write_model(path, synth.make_metadata(dims), wq)
    _, t = gguf.Parser().Read(path)
    assert {t[k].ggml_type for k in wq if not isinstance(wq[k], np.ndarray)} == {Q5_K, Q6_K}
    fac = LlamaModelFactory(0)
    m = gguf.Parser([fac]).Parse(ModelOptions(GGUFPath=path, KVCacheSize=64))
    def deq(v):
        if not hasattr(v, "ggml_type"):
            return v
        if v.ggml_type == Q5_K:
            return dequant_q5_k(v.data, *v.shape)
        return orc.dequant_q6k(np.ascontiguousarray(v.data), v.shape[0] * v.shape[1]).reshape(v.shape)
    ref = orc.OracleLlama(odesc(dims, 64), {k: deq(v) for k, v in t.items()})
    tok = 3
    for _ in range(12):
        lg, am = m.Step(tok)
        want = ref.step(tok)
        assert np.abs(lg - want).max() <= 5e-4 * max(1.0, float(np.abs(want).max()))
        assert am == orc.argmax(want)
        tok = am
    m.Dispose()
    fac.Dispose()


def test_decode_q5_k_is_bit_reproducible(mgr):
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY_D128
    wq, _ = quant_weights(dims, 91, "q5_k_m")
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


def test_full_depth_llama_3_2_1b_q5_k_m_against_the_oracle():
    """The whole Llama-3.2-1B in Q5_K_M (16 blocks, V = 128256, tied Q6_K embedding, attn_v / ffn_down in Q6_K on the use_more_bits
    blocks; weights from tools/q5_k_bench.py's generator in HBM): a 512-token prompt through the MFMA prefill, then 8 greedy tokens, against OracleLlama fed the same tokens one by one on
    the dequantised weights.  Bar: 2e-2 * max(1, |logit|) with identical greedy tokens (the fp16 prefill tolerance)."""
    import torch
    from nfai_amd import _lib
    from nfai_amd.hip import HipBufferManager
    from nfai_amd.llama_model import LlamaModel
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import q5_k_bench as QB
    dims = synth.LLAMA_32_1B
    T, G = 512, 8
    C = T + G + 1
    torch.cuda.set_device(0)
    weights = QB.gen_q5_k_m_weights_hbm(torch, dims)
    mg = HipBufferManager(0)
    m = LlamaModel(mg, synth.make_metadata(dims), {k: (t.data_ptr(), ty, r, c) for k, (t, ty, r, c) in weights.items()}, C, max_batch=T,
                   dims=ddict(dims))
    prompt = synth.make_tokens(dims, T, seed=99)
    prompt[0] = 128000 % dims.V
    got = [m.Prefill(prompt)]
    toks = [int(np.argmax(got[0]))]
    for _ in range(G):
        lg, am = m.Step(toks[-1])
        got.append(lg)
        toks.append(am)
    m.Dispose()
    mg.Dispose()
    assert {ty for (_, ty, _, _) in weights.values()} == {0, Q5_K, Q6_K}
    host = {k: (dequant_q5_k(t.cpu().numpy(), r, c) if ty == Q5_K else QB.dequant(t, ty, r, c)) for k, (t, ty, r, c) in weights.items()}
    del weights
    ref = orc.OracleLlama(odesc(dims, C), host)
    for t in prompt[:-1]:
        ref.step(int(t), want_logits=False)
    wants = [ref.step(int(prompt[-1]))] + [None] * G
    for i in range(G):
        wants[i + 1] = ref.step(toks[i])
    worst = 0.0
    for i in range(G + 1):
        err, scale = float(np.abs(got[i] - wants[i]).max()), max(1.0, float(np.abs(wants[i]).max()))
        worst = max(worst, err / scale)
        assert err <= 2e-2 * scale, (i, err, scale)
        assert orc.argmax(wants[i]) == toks[i], i
    print(f"full-depth 1B Q5_K_M: worst max|dlogit| / max(1, max|logit|) = {worst:.3g}")
