"""Q3_K weights on the GPU against the oracle.

The reference throws for every quantised type (NFAI.GGUF/Parser.cs:111-114), so parity is UNPINNED by the reference: the oracle is
ggml's block_q3_K (hmask[32], qs[64], scales[12], fp16 d; weight = d * (sc - 32) * (q - 4), q = two low bits | high bit << 2)
as restated from memory in synth.dequantize_q3_k (tests/test_q3_k.py pins it against a scalar transcription; check it against a real
file when one is at hand), followed by the reference's fp32 GEMV / the whole-model oracle on the dequantised weights.  Q4_K, Q5_K and
Q6_K matrices of the Q3_K_M mix go through their own dequantisers.  tol() / stage_tol() and the model bars are those of
tests/test_gpu_q5_k.py: the arithmetic class is the same (exact int32 dots, 22-bit fixed-point activations, fp32 scales)."""
import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth

pytestmark = pytest.mark.gpu

Q3_K, Q4_K, Q5_K, Q6_K = 11, 12, 13, 14


def dequant(raw, qt, N, K):
    if qt == Q3_K:
        return synth.dequantize_q3_k(np.ascontiguousarray(raw, np.uint8).tobytes(), N, K)
    if qt == Q4_K:
        return orc.dequant_q4k(raw, N * K).reshape(N, K)
    if qt == Q6_K:
        return orc.dequant_q6k(raw, N * K).reshape(N, K)
    from test_gpu_q5_k import dequant_q5_k
    return dequant_q5_k(raw, N, K)


def quantize(W, qt=Q3_K):
    """W [N][K] fp32 -> (raw block bytes, dequantised fp32 [N][K])."""
    N, K = W.shape
    if qt == Q4_K:
        b = orc.quantize_q4k(W)
    elif qt == Q6_K:
        b = orc.quantize_q6k(W)
    elif qt == Q5_K:
        b = np.frombuffer(synth.quantize_q5_k(W), np.uint8).copy()
    else:
        b = np.frombuffer(synth.quantize_q3_k(W), np.uint8).copy()
    return b, dequant(b, qt, N, K)


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
    op.GetWeightProperty().set(raw, Q3_K, N, K)
    op.GetInputProperty().SetValue(x)
    op.Compute()
    return op.GetOutputs()


# (16, 256): one tile, one super-block; (304, 14336): a ragged tile count against the grid, four super-blocks per wave;
# (64, 28672): eight super-blocks per wave (K > 16384)
@pytest.mark.parametrize("N,K", [(16, 256), (96, 256), (304, 14336), (512, 8192), (64, 28672)])
def test_gemv_q3_k(mgr, N, K):
    r = rng(N + K)
    raw, Wd = quantize((0.02 * r.standard_normal((N, K))).astype(np.float32))
    x = r.standard_normal(K).astype(np.float32)
    err = np.abs(gemv(mgr, raw, N, K, x) - orc.gemv(Wd, x))
    assert (err <= tol(Wd, x)).all(), (err.max(), tol(Wd, x).min())


@pytest.mark.parametrize("xscale", [0.0, 1e-30, 1e-6, 3e4], ids=["zero", "tiny", "small", "large"])
def test_gemv_q3_k_activation_range(mgr, xscale):
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


# ---- extreme blocks at (32, 512): two tiles and two super-blocks, so a plane addressed by the wrong tile or block shows ---------------
def pack_scales(sc):
    """[nb][16] 6-bit scales -> [nb][12] scale bytes."""
    sc = np.asarray(sc, np.uint8)
    out = np.zeros((sc.shape[0], 12), np.uint8)
    out[:, 0:8] = (sc[:, 0:8] & 0xF) | ((sc[:, 8:16] & 0xF) << 4)
    for i in range(16):
        out[:, 8 + i % 4] |= (sc[:, i] >> 4) << (2 * (i // 4))
    return out


def _f16_bytes(v):
    return np.asarray(v, np.float16).view(np.uint8).reshape(-1, 2)


def set_code(b, blk, k, code):
    """Write 3-bit code of element k (0..255) of block blk."""
    n, j, lh, l = k >> 7, (k >> 5) & 3, (k >> 4) & 1, k & 15
    qi, hi = 32 + 32 * n + 16 * lh + l, 16 * lh + l
    b[blk, qi] = (int(b[blk, qi]) & (0xFF ^ (3 << (2 * j)))) | ((code & 3) << (2 * j))
    b[blk, hi] = (int(b[blk, hi]) & (0xFF ^ (1 << (4 * n + j)))) | ((code >> 2) << (4 * n + j))


EXTREME = ["codes_0", "codes_7", "hmask_only", "qs_only", "scales_0", "scales_63", "scales_32", "d_max", "d_subnormal", "d_neg_zero",
           "scales_distinct", "d_distinct", "one_high_bit", "one_high_bit_clear", "one_low_code"]


def _extreme(kind, N, K, r):
    b = np.frombuffer(synth.quantize_q3_k((0.02 * r.standard_normal((N, K))).astype(np.float32)), np.uint8).copy().reshape(-1, 110)
    nb, NB = b.shape[0], K // 256
    row, blk = np.arange(nb) // NB, np.arange(nb) % NB
    if kind == "codes_0":
        b[:, 0:96] = 0x00
    elif kind == "codes_7":
        b[:, 0:96] = 0xFF
    elif kind == "hmask_only":         # every code 4: q - 4 = 0 everywhere
        b[:, 0:32], b[:, 32:96] = 0xFF, 0x00
    elif kind == "qs_only":            # every code 3
        b[:, 0:32], b[:, 32:96] = 0x00, 0xFF
    elif kind in ("scales_0", "scales_63", "scales_32"):
        b[:, 96:108] = pack_scales(np.full((nb, 16), int(kind.split("_")[1])))
    elif kind == "d_max":              # +-65504, sign alternating by block; scales 31 / 33 keep |w| <= 65504 * 4 finite in fp32
        b[:, 108:110] = _f16_bytes(np.where(np.arange(nb) % 2 == 0, 65504.0, -65504.0))
    elif kind == "d_subnormal":
        b[:, 108:110] = _f16_bytes(np.full(nb, 2.0 ** -24))
    elif kind == "d_neg_zero":
        b[:, 108:110] = _f16_bytes(np.full(nb, -0.0))
        assert (b[:, 109] == 0x80).all()
    elif kind == "scales_distinct":    # a distinct scale per (row of a tile, group of a block): 16 x 16 values cycling through 0..63
        g = np.arange(16)[None, :]
        b[:, 96:108] = pack_scales((7 * (row % 16)[:, None] + 4 * g + 3 * blk[:, None] + (row // 16)[:, None]) % 64)
    elif kind == "d_distinct":         # a distinct d per (row, block), exact in fp16
        d = 2.0 ** -12 * (1 + row + N * blk) * np.where((row + blk) % 2 == 0, 1.0, -1.0)
        assert len(set(np.abs(d).tolist())) == nb and (d.astype(np.float16).astype(np.float64) == d).all()
        b[:, 108:110] = _f16_bytes(d)
    elif kind == "one_high_bit":       # exactly one hmask bit per block, at a place that depends on (row, block), qs = 0: that weight
        b[:, 0:32], b[:, 32:96] = 0x00, 0x00   # is code 4 - 4 = 0, every other one code 0 - 4: the zero moves if the hmask plane is permuted
        for i in range(nb):
            set_code(b, i, (37 * int(row[i]) + 101 * int(blk[i]) + 5) % 256, 4)
    elif kind == "one_high_bit_clear":  # the inverse: every weight at code 4 - 4 = 0 but one per block with its high bit cleared (-4):
        b[:, 0:32], b[:, 32:96] = 0xFF, 0x00    # the block's ONLY non-zero contribution moves if the hmask plane is permuted
        for i in range(nb):
            set_code(b, i, (37 * int(row[i]) + 101 * int(blk[i]) + 5) % 256, 0)
    elif kind == "one_low_code":       # every element at code 4 (zero weight) but one per block at code 4 + c, c = 1..3
        b[:, 0:32], b[:, 32:96] = 0xFF, 0x00
        for i in range(nb):
            set_code(b, i, (53 * int(row[i]) + 89 * int(blk[i]) + 11) % 256, 4 + 1 + (int(row[i]) + int(blk[i])) % 3)
    else:
        raise KeyError(kind)
    return b.ravel()


@pytest.fixture(scope="module")
def extreme_x():
    return rng(55).standard_normal(512).astype(np.float32)


@pytest.mark.parametrize("kind", EXTREME)
def test_gemv_q3_k_extreme_blocks(mgr, kind, extreme_x):
    N, K = 32, 512
    raw = _extreme(kind, N, K, rng(5))
    Wd = synth.dequantize_q3_k(raw.tobytes(), N, K)
    assert np.isfinite(Wd).all()
    nz = (Wd.reshape(-1, 256) != 0).sum(axis=1)
    if kind in ("one_high_bit_clear", "one_low_code"):
        assert (nz == 1).all()     # (the quantiser leaves no group at scale 32 on this matrix)
    if kind == "one_high_bit":
        assert (nz == 255).all()
    if kind in ("hmask_only", "scales_32", "d_neg_zero"):
        assert not Wd.any()
    if kind == "codes_7":
        assert (np.abs(Wd) > 0).any()
    x = extreme_x
    got = gemv(mgr, raw, N, K, x)
    err = np.abs(got - orc.gemv(Wd, x))
    assert (err <= tol(Wd, x)).all(), (kind, float(err.max()), float(tol(Wd, x).min()))


# ---- fused ops -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(256, 8192), (256, 28672)])
def test_gemv_fused_norm_and_residual_q3_k(mgr, N, K):
    """K = 8192 and 28672: two and eight super-blocks per wave with the RMSNorm gains."""
    from nfai_amd._lib import call
    from nfai_amd.hip import ShaderProperty
    r = rng(9 + K)
    raw, Wd = quantize((0.02 * r.standard_normal((N, K))).astype(np.float32))
    w = mgr.UploadWeight(Q3_K, raw, N, K)
    x = r.standard_normal(K).astype(np.float32)
    g = (1 + 0.1 * r.standard_normal(K)).astype(np.float32)
    res = r.standard_normal(N).astype(np.float32)
    px, pg, pr, py = ShaderProperty(mgr, K), ShaderProperty(mgr, K), ShaderProperty(mgr, N), ShaderProperty(mgr, N)
    px.SetValue(x); pg.SetValue(g); pr.SetValue(res)
    call("nfai_hip_gemv_fused", mgr.handle, w.handle, Q3_K, px.handle, pg.handle, 1e-5, pr.handle, py.handle, N, K)
    xn = orc.rmsnorm(x, g, 1e-5)
    assert (np.abs(py.GetValue() - orc.add(res, orc.gemv(Wd, xn))) <= tol(Wd, xn) + 1e-5).all()


@pytest.mark.parametrize("E,F", [(256, 512), (256, 14336)])
def test_gateup_silu_and_down_residual_q3_k(mgr, E, F):
    from nfai_amd._lib import call
    from nfai_amd.hip import ShaderProperty
    r = rng(E + F)
    (rg, dg), (ru, du), (rd, dd) = (quantize((0.02 * r.standard_normal(s)).astype(np.float32)) for s in ((F, E), (F, E), (E, F)))
    x = r.standard_normal(E).astype(np.float32)
    g = (1 + 0.1 * r.standard_normal(E)).astype(np.float32)
    pg_, pu, pd = mgr.UploadWeight(Q3_K, rg, F, E), mgr.UploadWeight(Q3_K, ru, F, E), mgr.UploadWeight(Q3_K, rd, E, F)
    px, pg, pa, py = ShaderProperty(mgr, E), ShaderProperty(mgr, E), ShaderProperty(mgr, F), ShaderProperty(mgr, E)
    px.SetValue(x); pg.SetValue(g)
    call("nfai_hip_gemv_gateup_silu", mgr.handle, pg_.handle, pu.handle, Q3_K, px.handle, pg.handle, 1e-5, pa.handle, F, E)
    xn = orc.rmsnorm(x, g, 1e-5)
    np.testing.assert_allclose(pa.GetValue(), orc.mul(orc.gemv(du, xn), orc.silu(orc.gemv(dg, xn))), rtol=1e-4, atol=2e-5)
    call("nfai_hip_gemv_fused", mgr.handle, pd.handle, Q3_K, pa.handle, 0, 0.0, px.handle, py.handle, E, F)
    assert (np.abs(py.GetValue() - orc.add(x, orc.gemv(dd, pa.GetValue()))) <= tol(dd, pa.GetValue()) + 1e-5).all()


@pytest.mark.parametrize("kv16", [False, True], ids=["kv32", "kv16"])
@pytest.mark.parametrize("E", [256, 3072])
def test_qkv_rope_q3_k_op(mgr, E, kv16):
    """q|k|v all Q3_K through the 1:1 entry point: q, the K row and the V row."""
    from nfai_amd._lib import call, F16, F32
    from nfai_amd.hip import ShaderProperty
    H, Hkv, D, pos = 4, 2, 64, 5
    r = rng(31 + E)
    (rq, dq), (rk, dk), (rv, dv) = (quantize((0.02 * r.standard_normal((n, E))).astype(np.float32)) for n in (H * D, Hkv * D, Hkv * D))
    bq, bk, bv = mgr.UploadWeight(Q3_K, rq, H * D, E), mgr.UploadWeight(Q3_K, rk, Hkv * D, E), mgr.UploadWeight(Q3_K, rv, Hkv * D, E)
    x = r.standard_normal(E).astype(np.float32)
    g = (1 + 0.1 * r.standard_normal(E)).astype(np.float32)
    freqs = orc.rope_freqs(D)
    kvt = np.float16 if kv16 else np.float32
    px, pg, pf = ShaderProperty(mgr, E), ShaderProperty(mgr, E), ShaderProperty(mgr, D // 2)
    pq, kc, vc = ShaderProperty(mgr, H * D), ShaderProperty(mgr, (pos + 1) * Hkv * D, kvt), ShaderProperty(mgr, (pos + 1) * Hkv * D, kvt)
    px.SetValue(x); pg.SetValue(g); pf.SetValue(freqs)
    call("nfai_hip_gemv_qkv_rope", mgr.handle, bq.handle, bk.handle, bv.handle, Q3_K, px.handle, pg.handle, 1e-5, pf.handle, D,
         pq.handle, kc.handle, vc.handle, H, Hkv, D, pos, F16 if kv16 else F32, E)
    xn = orc.rmsnorm(x, g, 1e-5)
    q, k, v = orc.gemv(dq, xn), orc.gemv(dk, xn), orc.gemv(dv, xn)
    qr, kr = orc.rope(q, freqs, D, H, D, pos), orc.rope(k, freqs, D, Hkv, D, pos)
    assert (np.abs(pq.GetValue() - qr) <= 2 * tol(dq, xn) + 1e-6).all()
    krow = kc.GetValue()[pos * Hkv * D:].astype(np.float32)
    vrow = vc.GetValue()[pos * Hkv * D:].astype(np.float32)
    h16 = 2.0 ** -11 if kv16 else 0.0    # an fp16 cache rounds the stored value: half an ulp of it
    assert (np.abs(krow - kr) <= 2 * tol(dk, xn) + 1e-6 + h16 * np.abs(kr)).all()
    assert (np.abs(vrow - v) <= tol(dv, xn) + h16 * np.abs(v)).all()


# ---- table and head ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,E", [(48, 256), (64, 512)])
def test_embed_q3_k_every_row(mgr, V, E):
    from nfai_amd._lib import call
    from nfai_amd.hip import ShaderProperty
    raw, Wd = quantize((0.05 * rng(3 + V).standard_normal((V, E))).astype(np.float32))
    tab = mgr.UploadWeight(Q3_K, raw, V, E)
    tok, y = ShaderProperty(mgr, 1, np.uint32), ShaderProperty(mgr, E)
    for t in range(V):
        tok.SetValue(np.array([t], np.uint32))
        call("nfai_hip_embed", mgr.handle, tab.handle, Q3_K, tok.handle, y.handle, E)
        np.testing.assert_array_equal(y.GetValue(), Wd[t])  # (d * (sc - 32)) * (q - 4) in the restatement's order


@pytest.mark.parametrize("V,E", [(48, 256), (4000, 3072)])
def test_lmhead_argmax_q3_k(mgr, V, E):
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
    tab = mgr.UploadWeight(Q3_K, raw, V, E)
    px, pg, pl, pi = ShaderProperty(mgr, E), ShaderProperty(mgr, E), ShaderProperty(mgr, V), ShaderProperty(mgr, 1, np.uint32)
    px.SetValue(x); pg.SetValue(g)
    call("nfai_hip_lmhead_argmax", mgr.handle, tab.handle, Q3_K, px.handle, pg.handle, 1e-5, pl.handle, pi.handle, V, E)
    lg = pl.GetValue()
    want = orc.gemv(Wd, xn)
    assert (np.abs(lg - want) <= tol(Wd, xn)).all()
    assert int(pi.GetValue()[0]) == orc.argmax(want) == min(dup)


def test_gemm_kq_refuses_q3_k(mgr):
    from nfai_amd import _lib
    from nfai_amd.hip import ShaderProperty
    M, N, K = 64, 64, 256
    raw, _ = quantize((0.02 * rng(1).standard_normal((N, K))).astype(np.float32))
    w = mgr.UploadWeight(Q3_K, raw, N, K)
    pa, pc = ShaderProperty(mgr, M * K, np.float16), ShaderProperty(mgr, M * N)
    with pytest.raises(_lib.NfaiHipError, match="Q3_K") as e:
        _lib.call("nfai_hip_gemm_kq", mgr.handle, pa.handle, w.handle, Q3_K, 0, pc.handle, M, N, K)
    assert e.value.code == _lib.ERR_UNSUPPORTED


# ---- whole models ------------------------------------------------------------------------------------------------------------------
def mix_type(name, mix, dims):
    """all_q3_k / q3_k_m / q3_k_s: synth.q3_k_type; a (q, k, v) tuple: those types for the three attention inputs, the rest Q3_K."""
    if isinstance(mix, tuple):
        parts = name.split(".")
        return mix[("attn_q", "attn_k", "attn_v").index(parts[2])] if len(parts) > 2 and parts[2] in ("attn_q", "attn_k", "attn_v") else Q3_K
    return synth.q3_k_type(name, dims, mix)


_WEIGHTS = {}


def quant_weights(dims, seed, mix="all_q3_k", std=0.05):
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


def run_against_oracle(mgr, dims, wq, wref, steps, bar=5e-4, **variants):
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
            assert np.abs(lg - want).max() <= bar * scale, (i, np.abs(lg - want).max())
            assert am == orc.argmax(want)
        tok = orc.argmax(want)
    return models, ref


@pytest.mark.parametrize("dims", [synth.TINY, synth.TINY_D128], ids=lambda d: d.name)
@pytest.mark.parametrize("mix", ["all_q3_k", "q3_k_m", "q3_k_s"])
def test_model_q3_k_graph_eager_unfused(mgr, dims, mix):
    """Graph, eager and the unfused 1:1 chain against OracleLlama, 8 decode steps: greedy tokens identical, logits within
    5e-4 * max(1, |logit|) (the bar of test_model_q5_k_graph_eager_unfused).  all_q3_k: a Q3_K token_embd (through the q|k|v launch's
    BEGIN prologue in graph / eager, k_embed_t16 unfused) and a Q3_K lm_head + ArgMax.  q3_k_m: q and k in Q3_K share a launch, the
    Q5_K (blocks 0, 1) or Q4_K v gets its own: two q|k|v launches per block."""
    wq, wref = quant_weights(dims, 61, mix)
    models, _ = run_against_oracle(mgr, dims, wq, wref, 8, graph={}, eager={"graph": False}, unfused={"unfused": True})
    total, _ = models[0].BytesPerToken(0)
    prof = models[0].ProfileStep(7)
    for m in models:
        m.Dispose()
    assert prof["qkv"][1] == (2 if mix == "q3_k_m" else 1) * dims.L, prof
    if mix == "all_q3_k":
        E, F, V, KD, HD = dims.E, dims.F, dims.V, dims.Hkv * dims.D, dims.H * dims.D
        blk = (HD * E + 2 * KD * E + E * HD + 3 * E * F) * 110 // 256
        kv = 2 * KD * 4 * 1 + 2 * KD * 4
        head = V * E * 110 // 256
        assert total == dims.L * (blk + kv) + E * 110 // 256 + head


QKV_MIXES = [(Q3_K, Q3_K, Q3_K), (Q3_K, Q3_K, Q4_K), (Q3_K, Q3_K, Q5_K), (Q6_K, Q3_K, Q6_K)]
QKV_E256 = synth.LlamaDims("qkv-e256", 256, 1, 4, 2, 64, 512, 512, True)
QKV_E3072 = synth.LlamaDims("qkv-e3072", 3072, 1, 4, 2, 64, 512, 512, True)


@pytest.mark.parametrize("kv16", [False, True], ids=["kv32", "kv16"])
@pytest.mark.parametrize("qkv", QKV_MIXES, ids=lambda t: "".join(str(x % 10) for x in t))
@pytest.mark.parametrize("dims", [QKV_E256, QKV_E3072], ids=lambda d: d.name)
def test_qkv_rope_q3_k_type_combinations(mgr, dims, qkv, kv16):
    """q|k|v of one block with (q, k, v) in the types a Q3_K_M file has (and Q6_K around a Q3_K k: three launches), fp32 and fp16 KV:
    the K and V cache rows of four positions against the oracle's under the bounds of the q|k|v operator test (2 tol() for the rotated
    K row, tol() for the V row, on the block's normed input), and q through the logits (the model does not expose q; the all-Q3_K q
    is checked directly in test_qkv_rope_q3_k_op).  Launch count: Q3_K segments share a launch only with each other."""
    from nfai_amd.llama_model import LlamaModel
    wq, wref = quant_weights(dims, 63, qkv)
    m = LlamaModel(mgr, synth.make_metadata(dims), wq, 16, dims=ddict(dims), kv_f16=kv16)
    ref = orc.OracleLlama(odesc(dims, 16), wref)
    tok, fed = 7, []
    bar = 2e-2 if kv16 else 5e-4          # the fp16-cache bar of the batched tests / the model bar
    for i in range(4):
        want = ref.step(tok)
        lg, am = m.Step(tok)
        assert np.abs(lg - want).max() <= bar * max(1.0, float(np.abs(want).max())), i
        fed.append(tok)
        tok = orc.argmax(want)
    h16 = 2.0 ** -11 if kv16 else 0.0     # an fp16 cache rounds the stored value: half an ulp of it
    for pos in range(4):
        xn = orc.rmsnorm(np.asarray(wref["token_embd.weight"][fed[pos]], np.float32), wref["blk.0.attn_norm.weight"], 1e-5)
        wk, wv = ref.kcache(0)[pos], ref.vcache(0)[pos]
        assert (np.abs(m.ReadKV(0, False, pos) - wk) <= 2 * tol(wref["blk.0.attn_k.weight"], xn) + 1e-6 + h16 * np.abs(wk)).all(), pos
        assert (np.abs(m.ReadKV(0, True, pos) - wv) <= tol(wref["blk.0.attn_v.weight"], xn) + h16 * np.abs(wv)).all(), pos
    prof = m.ProfileStep(tok)
    m.Dispose()
    assert prof["qkv"][1] == {(Q3_K, Q3_K, Q3_K): 1, (Q6_K, Q3_K, Q6_K): 3}.get(qkv, 2), prof


def test_model_q3_k_down_projection_above_8192(mgr):
    """THIN_F14336, one block: Wdown at K = 14336 (four super-blocks per wave) inside the model."""
    dims = synth.THIN_F14336
    wq, wref = quant_weights(dims, 65, "q3_k_s")   # (q3_k_m keeps ffn_down in Q4_K)
    assert wq["blk.0.ffn_down.weight"].ggml_type == Q3_K
    models, _ = run_against_oracle(mgr, dims, wq, wref, 6, graph={})
    for m in models:
        m.Dispose()


def test_decode_q3_k_is_bit_reproducible(mgr):
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY_D128
    wq, _ = quant_weights(dims, 61, "q3_k_m")
    a = LlamaModel(mgr, synth.make_metadata(dims), wq, 48, dims=ddict(dims))
    b = LlamaModel(mgr, synth.make_metadata(dims), wq, 48, dims=ddict(dims))
    toks = synth.make_tokens(dims, 40, seed=4)
    first = [a.Step(int(t))[0] for t in toks]
    a.Reset()
    for i, t in enumerate(toks):
        la, _ = a.Step(int(t))
        lb, _ = b.Step(int(t))
        assert np.array_equal(la, first[i]) and np.array_equal(lb, first[i]), i
    a.Dispose()
    b.Dispose()


@pytest.mark.parametrize("n,chunk", [(70, 64), (40, 128)], ids=["chunked", "one-chunk"])
def test_prefill_mfma_q3_k(mgr, n, chunk):
    """The MFMA prefill widens Q3_K to fp16: the bar of tests/test_gpu_q5_k.py's prefill (2e-2 * max(1, |logit|))."""
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY_D128
    wq, wref = quant_weights(dims, 61, "q3_k_m")
    m = LlamaModel(mgr, synth.make_metadata(dims), wq, 96, dims=ddict(dims), max_batch=chunk)
    mt = LlamaModel(mgr, synth.make_metadata(dims), wq, 96, dims=ddict(dims))   # no workspace: token by token
    ref = orc.OracleLlama(odesc(dims, 96), wref)
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
    # Ingest (no logits) leaves the rows under the same bar
    mi = LlamaModel(mgr, synth.make_metadata(dims), wq, 96, dims=ddict(dims), max_batch=chunk)
    mi.Ingest(toks)
    assert mi.Pos == n
    np.testing.assert_allclose(mi.ReadKV(dims.L - 1, False, n - 1), ref.kcache(dims.L - 1)[n - 1], rtol=0, atol=2e-2)
    tok = orc.argmax(want)
    for _ in range(4):
        lg, _ = m.Step(tok)
        wl = ref.step(tok)
        assert np.abs(lg - wl).max() <= tol5
        tok = orc.argmax(wl)
    for x in (m, mt, mi):
        x.Dispose()


def test_score_q3_k_against_the_per_step_logits(mgr):
    """nfai_hip_llama_score on 40 tokens: the log-probability of every next token and of the maximum against log-softmax of a twin's
    token-by-token logits.  Score runs the MFMA path on fp16-widened weights: a logit moves by at most the prefill bar
    b = 2e-2 * max(1, max|logit|), a log-probability (a difference of a logit and a log-sum-exp, each within b) by at most 2 b."""
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY_D128
    wq, _ = quant_weights(dims, 61, "q3_k_m")
    m = LlamaModel(mgr, synth.make_metadata(dims), wq, 48, dims=ddict(dims), max_batch=64)
    twin = LlamaModel(mgr, synth.make_metadata(dims), wq, 48, dims=ddict(dims))
    toks = synth.make_tokens(dims, 40, seed=33)
    lp, am, lpm = m.Score(toks)
    lg = np.stack([twin.Step(int(t))[0] for t in toks]).astype(np.float64)
    ls = lg - (lg.max(axis=1, keepdims=True) + np.log(np.exp(lg - lg.max(axis=1, keepdims=True)).sum(axis=1, keepdims=True)))
    bars = 2e-2 * np.maximum(1.0, np.abs(lg).max(axis=1))
    rows = np.arange(39)
    assert (np.abs(lp[:39] - ls[rows, toks[1:]]) <= 2 * bars[:39]).all()
    assert lp[39] == 0.0
    assert (np.abs(lpm - ls.max(axis=1)) <= 2 * bars).all()
    assert (lg.max(axis=1) - lg[np.arange(40), am] <= 2 * bars).all()
    assert m.Pos == 40
    m.Dispose()
    twin.Dispose()


@pytest.mark.parametrize("ranges", [[(0, 2), (2, 3)], [(0, 1), (1, 2), (2, 3)]], ids=["2-stage", "3-stage"])
def test_pipeline_stages_q3_k(mgr, ranges):
    """Stages of a Q3_K_M model (stage_step token by token) against the single model: bit-equal logits and tokens."""
    import torch
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY_D128
    wq, _ = quant_weights(dims, 61, "q3_k_m")
    md = synth.make_metadata(dims)
    whole = LlamaModel(mgr, md, wq, 32, dims=ddict(dims))
    stages = [LlamaModel(mgr, md, wq, 32, dims=ddict(dims), layer_range=rg) for rg in ranges]
    h = torch.zeros(dims.E, dtype=torch.float32, device="cuda")
    tok = 7
    for step in range(8):
        want, wam = whole.Step(tok)
        for i, st in enumerate(stages):
            first, last = i == 0, i == len(stages) - 1
            lg, am = st.StageStep(tok if first else 0, None if first else h.data_ptr(), None if last else h.data_ptr(), want_logits=last)
        assert np.array_equal(lg, want), step
        assert am == wam, step
        tok = wam
    for m in [whole] + stages:
        m.Dispose()


def test_q3_k_gguf_file_to_generation(mgr, tmp_path):
    """A Q3_K_M GGUF file (TINY: tied Q6_K embedding; Q3_K, Q4_K and Q5_K blocks) -> Parser().Parse -> the provider's model -> 8 greedy
    tokens, against the oracle on the dequantised weights read back from the same file."""
    from nfai_amd import gguf
    from nfai_amd.llama_model import LlamaModelFactory, ModelOptions
    dims = synth.TINY
    wq, _ = quant_weights(dims, 81, "q3_k_m")
    path = str(tmp_path / "q3_k_m.gguf")
    gguf.write_model(path, synth.make_metadata(dims), wq)
    _, t = gguf.Parser().Read(path)
    assert {t[k].ggml_type for k in wq if not isinstance(wq[k], np.ndarray)} == {Q3_K, Q4_K, Q5_K, Q6_K}
    fac = LlamaModelFactory(0)
    m = gguf.Parser([fac]).Parse(ModelOptions(GGUFPath=path, KVCacheSize=64))
    ref = orc.OracleLlama(odesc(dims, 64), {k: (dequant(np.ascontiguousarray(v.data), v.ggml_type, *v.shape) if hasattr(v, "ggml_type") else v)
                                            for k, v in t.items()})
    tok, got, wanted = 3, [], []
    for _ in range(8):
        lg, am = m.Step(tok)
        want = ref.step(tok)
        assert np.abs(lg - want).max() <= 5e-4 * max(1.0, float(np.abs(want).max()))
        got.append(am)
        wanted.append(orc.argmax(want))
        tok = am
    assert got == wanted
    m.Dispose()
    fac.Dispose()
