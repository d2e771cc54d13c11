"""IQ4_XS weights on the GPU against the oracle.

The reference throws for every quantised type (NFAI.GGUF/Parser.cs:111-114), so parity is UNPINNED by the reference: the oracle is
ggml's block_iq4_xs (fp16 d, uint16 scales_h, scales_l[4], qs[128]; weight = d * (ls - 32) * KV[q], q a nibble that indexes a
16-entry table) as restated from memory in synth.dequantize_iq4_xs (tests/test_iq4_xs.py pins it against a scalar transcription; check
it against a real file when one is at hand), followed by the reference's fp32 GEMV / the whole-model oracle on the dequantised
weights.  Q5_K and Q6_K matrices of the IQ4_XS mix go through their own dequantisers.  tol() / stage_tol() and the model bars are
those of tests/test_gpu_q3_k.py: the arithmetic class is the same (exact int32 dots, 22-bit fixed-point activations, fp32 scales)."""
import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth
from test_gpu_q3_k import ddict, odesc, rng, stage_tol, tol
from test_gpu_q3_k import dequant as dequant_other, quantize as quantize_other

pytestmark = pytest.mark.gpu

Q4_0, Q3_K, Q4_K, Q5_K, Q6_K, IQ4_XS = 2, 11, 12, 13, 14, 23


def dequant(raw, qt, N, K):
    if qt == IQ4_XS:
        return synth.dequantize_iq4_xs(np.ascontiguousarray(raw, np.uint8).tobytes(), N, K)
    if qt == Q4_0:
        return synth.dequantize_q4_0(np.ascontiguousarray(raw, np.uint8).tobytes(), N, K)
    return dequant_other(raw, qt, N, K)


def quantize(W, qt=IQ4_XS):
    """W [N][K] fp32 -> (raw block bytes, dequantised fp32 [N][K])."""
    N, K = W.shape
    if qt == IQ4_XS:
        b = np.frombuffer(synth.quantize_iq4_xs(W), np.uint8).copy()
    elif qt == Q4_0:
        b = np.frombuffer(synth.quantize_q4_0(W), np.uint8).copy()
    else:
        return quantize_other(W, qt)
    return b, dequant(b, qt, N, K)


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


def gemv(mgr, raw, N, K, x):
    from nfai_amd.shaders import MatrixMultiplyShader
    op = MatrixMultiplyShader(mgr, 1, K, N, None)
    op.GetWeightProperty().set(raw, IQ4_XS, N, K)
    op.GetInputProperty().SetValue(x)
    op.Compute()
    return op.GetOutputs()


# (16, 256): one tile, one super-block; (304, 14336): a ragged tile count against the grid, four super-blocks per wave;
# (64, 28672): eight super-blocks per wave (K > 16384)
@pytest.mark.parametrize("N,K", [(16, 256), (96, 256), (304, 14336), (512, 8192), (64, 28672)])
def test_gemv_iq4_xs(mgr, N, K):
    r = rng(N + K)
    raw, Wd = quantize((0.02 * r.standard_normal((N, K))).astype(np.float32))
    x = r.standard_normal(K).astype(np.float32)
    err = np.abs(gemv(mgr, raw, N, K, x) - orc.gemv(Wd, x))
    assert (err <= tol(Wd, x)).all(), (err.max(), tol(Wd, x).min())


@pytest.mark.parametrize("xscale", [0.0, 1e-30, 1e-6, 3e4], ids=["zero", "tiny", "small", "large"])
def test_gemv_iq4_xs_activation_range(mgr, xscale):
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
def pack_ls(b, ls):
    """Write [nb][8] 6-bit scales into the scales_h / scales_l bytes of blocks b [nb][136]."""
    ls = np.asarray(ls, np.uint16)
    b[:, 2:8] = 0
    sh = np.zeros(b.shape[0], np.uint16)
    for ib in range(8):
        sh |= (ls[:, ib] >> 4) << (2 * ib)
        b[:, 4 + ib // 2] |= ((ls[:, ib] & 0xF) << (4 * (ib % 2))).astype(np.uint8)
    b[:, 2:4] = sh.view(np.uint8).reshape(-1, 2)


def _f16_bytes(v):
    return np.asarray(v, np.float16).view(np.uint8).reshape(-1, 2)


EXTREME = ["codes_0", "codes_15", "codes_8", "codes_rotated", "low_nibbles_only", "high_nibbles_only", "ls_0", "ls_63", "ls_32",
           "scales_h_only", "scales_l_only", "ls_distinct", "d_distinct", "d_negative", "d_neg_zero", "d_subnormal", "d_max"]


def _extreme(kind, N, K, r):
    b = np.frombuffer(synth.quantize_iq4_xs((0.02 * r.standard_normal((N, K))).astype(np.float32)), np.uint8).copy().reshape(-1, 136)
    nb, NB = b.shape[0], K // 256
    row, blk = np.arange(nb) // NB, np.arange(nb) % NB
    if kind == "codes_0":
        b[:, 8:136] = 0x00
    elif kind == "codes_15":
        b[:, 8:136] = 0xFF
    elif kind == "codes_8":
        b[:, 8:136] = 0x88
    elif kind == "codes_rotated":      # sub-block ib of block i holds code (j + ib + 3 i) % 16 at weight j: every table entry meets
        i = np.arange(nb)[:, None, None]   # every byte lane of the lookup, as a low and as a high nibble
        codes = ((np.arange(32)[None, None, :] + np.arange(8)[None, :, None] + 3 * i) % 16).astype(np.uint8)
        b[:, 8:136] = (codes[:, :, :16] | (codes[:, :, 16:] << 4)).reshape(nb, 128)
    elif kind == "low_nibbles_only":   # every high nibble code 0 (-127)
        b[:, 8:136] &= 0x0F
    elif kind == "high_nibbles_only":  # every low nibble code 0
        b[:, 8:136] &= 0xF0
    elif kind in ("ls_0", "ls_63", "ls_32"):
        pack_ls(b, np.full((nb, 8), int(kind.split("_")[1])))
    elif kind == "scales_h_only":
        b[:, 4:8] = 0
    elif kind == "scales_l_only":
        b[:, 2:4] = 0
    elif kind == "ls_distinct":        # eight distinct ls per block, another eight per (row of a tile, block, tile)
        ib = np.arange(8)[None, :]
        ls = (8 * ib + 5 * (row % 16)[:, None] + 3 * blk[:, None] + (row // 16)[:, None]) % 64
        assert all(len(set(x)) == 8 for x in ls.tolist())
        pack_ls(b, ls)
    elif kind == "d_distinct":         # a distinct d per (row, block), exact in fp16
        d = 2.0 ** -14 * (1 + row + N * blk) * np.where((row + blk) % 2 == 0, 1.0, -1.0)
        assert len(set(np.abs(d).tolist())) == nb and (d.astype(np.float16).astype(np.float64) == d).all()
        b[:, 0:2] = _f16_bytes(d)
    elif kind == "d_negative":
        b[:, 1] |= 0x80
    elif kind == "d_neg_zero":
        b[:, 0:2] = _f16_bytes(np.full(nb, -0.0))
        assert (b[:, 1] == 0x80).all() and (b[:, 0] == 0).all()
    elif kind == "d_subnormal":
        b[:, 0:2] = _f16_bytes(np.full(nb, 2.0 ** -24))
    elif kind == "d_max":              # the largest power of two the fp16 widening allows: 16 * 32 * 127 = 65024 < 65504; sign alternating
        b[:, 0:2] = _f16_bytes(np.where(np.arange(nb) % 2 == 0, 16.0, -16.0))
        pack_ls(b, np.where((np.arange(8)[None, :] + np.arange(nb)[:, None]) % 2 == 0, 0, 63))
    else:
        raise KeyError(kind)
    return b.ravel()


@pytest.fixture(scope="module")
def extreme_x():
    return rng(55).standard_normal(512).astype(np.float32)


@pytest.mark.parametrize("kind", EXTREME)
def test_gemv_iq4_xs_extreme_blocks(mgr, kind, extreme_x):
    N, K = 32, 512
    raw = _extreme(kind, N, K, rng(5))
    Wd = synth.dequantize_iq4_xs(raw.tobytes(), N, K)
    assert np.isfinite(Wd).all()
    if kind in ("ls_32", "d_neg_zero"):
        assert not Wd.any()
    else:
        assert (Wd != 0).mean() > 0.5
    if kind == "d_max":
        assert np.abs(Wd).max() == 16.0 * 32 * 127
    if kind == "d_negative":
        pos = raw.copy().reshape(-1, 136)
        pos[:, 1] ^= 0x80
        assert (pos[:, 1] < 0x80).all() and np.array_equal(Wd, -synth.dequantize_iq4_xs(pos.tobytes(), N, K))
    x = extreme_x
    got = gemv(mgr, raw, N, K, x)
    if kind == "ls_32":
        assert (got == 0).all()        # a zero scale: exactly nothing, whatever the codes
    err = np.abs(got - orc.gemv(Wd, x))
    assert (err <= tol(Wd, x)).all(), (kind, float(err.max()), float(tol(Wd, x).min()))


# ---- fused ops -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(256, 8192), (256, 28672)])
def test_gemv_fused_norm_and_residual_iq4_xs(mgr, N, K):
    """K = 8192 and 28672: two and eight super-blocks per wave with the RMSNorm gains; against the unfused chain's arithmetic."""
    from nfai_amd._lib import call
    from nfai_amd.hip import ShaderProperty
    r = rng(9 + K)
    raw, Wd = quantize((0.02 * r.standard_normal((N, K))).astype(np.float32))
    w = mgr.UploadWeight(IQ4_XS, raw, N, K)
    x = r.standard_normal(K).astype(np.float32)
    g = (1 + 0.1 * r.standard_normal(K)).astype(np.float32)
    res = r.standard_normal(N).astype(np.float32)
    px, pg, pr, py = ShaderProperty(mgr, K), ShaderProperty(mgr, K), ShaderProperty(mgr, N), ShaderProperty(mgr, N)
    px.SetValue(x); pg.SetValue(g); pr.SetValue(res)
    call("nfai_hip_gemv_fused", mgr.handle, w.handle, IQ4_XS, px.handle, pg.handle, 1e-5, pr.handle, py.handle, N, K)
    xn = orc.rmsnorm(x, g, 1e-5)
    assert (np.abs(py.GetValue() - orc.add(res, orc.gemv(Wd, xn))) <= tol(Wd, xn) + 1e-5).all()
    # the unfused chain on the device: plain GEMV of the normed vector, then the residual
    chain = orc.add(res, gemv(mgr, raw, N, K, xn))
    assert (np.abs(py.GetValue() - chain) <= 2 * tol(Wd, xn) + 1e-5).all()


@pytest.mark.parametrize("E,F", [(256, 512), (256, 14336)])
def test_gateup_silu_and_down_residual_iq4_xs(mgr, E, F):
    from nfai_amd._lib import call
    from nfai_amd.hip import ShaderProperty
    r = rng(E + F)
    (rg, dg), (ru, du), (rd, dd) = (quantize((0.02 * r.standard_normal(s)).astype(np.float32)) for s in ((F, E), (F, E), (E, F)))
    x = r.standard_normal(E).astype(np.float32)
    g = (1 + 0.1 * r.standard_normal(E)).astype(np.float32)
    pg_, pu, pd = mgr.UploadWeight(IQ4_XS, rg, F, E), mgr.UploadWeight(IQ4_XS, ru, F, E), mgr.UploadWeight(IQ4_XS, rd, E, F)
    px, pg, pa, py = ShaderProperty(mgr, E), ShaderProperty(mgr, E), ShaderProperty(mgr, F), ShaderProperty(mgr, E)
    px.SetValue(x); pg.SetValue(g)
    call("nfai_hip_gemv_gateup_silu", mgr.handle, pg_.handle, pu.handle, IQ4_XS, px.handle, pg.handle, 1e-5, pa.handle, F, E)
    xn = orc.rmsnorm(x, g, 1e-5)
    np.testing.assert_allclose(pa.GetValue(), orc.mul(orc.gemv(du, xn), orc.silu(orc.gemv(dg, xn))), rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(pa.GetValue(), orc.mul(gemv(mgr, ru, F, E, xn), orc.silu(gemv(mgr, rg, F, E, xn))), rtol=1e-4, atol=2e-5)
    call("nfai_hip_gemv_fused", mgr.handle, pd.handle, IQ4_XS, pa.handle, 0, 0.0, px.handle, py.handle, E, F)
    assert (np.abs(py.GetValue() - orc.add(x, orc.gemv(dd, pa.GetValue()))) <= tol(dd, pa.GetValue()) + 1e-5).all()


@pytest.mark.parametrize("kv16", [False, True], ids=["kv32", "kv16"])
@pytest.mark.parametrize("E", [256, 3072])
def test_qkv_rope_iq4_xs_op(mgr, E, kv16):
    """q|k|v all IQ4_XS through the 1:1 entry point: q, the K row and the V row."""
    from nfai_amd._lib import call, F16, F32
    from nfai_amd.hip import ShaderProperty
    H, Hkv, D, pos = 4, 2, 64, 5
    r = rng(31 + E)
    (rq, dq), (rk, dk), (rv, dv) = (quantize((0.02 * r.standard_normal((n, E))).astype(np.float32)) for n in (H * D, Hkv * D, Hkv * D))
    bq, bk, bv = mgr.UploadWeight(IQ4_XS, rq, H * D, E), mgr.UploadWeight(IQ4_XS, rk, Hkv * D, E), mgr.UploadWeight(IQ4_XS, rv, Hkv * D, E)
    x = r.standard_normal(E).astype(np.float32)
    g = (1 + 0.1 * r.standard_normal(E)).astype(np.float32)
    freqs = orc.rope_freqs(D)
    kvt = np.float16 if kv16 else np.float32
    px, pg, pf = ShaderProperty(mgr, E), ShaderProperty(mgr, E), ShaderProperty(mgr, D // 2)
    pq, kc, vc = ShaderProperty(mgr, H * D), ShaderProperty(mgr, (pos + 1) * Hkv * D, kvt), ShaderProperty(mgr, (pos + 1) * Hkv * D, kvt)
    px.SetValue(x); pg.SetValue(g); pf.SetValue(freqs)
    call("nfai_hip_gemv_qkv_rope", mgr.handle, bq.handle, bk.handle, bv.handle, IQ4_XS, px.handle, pg.handle, 1e-5, pf.handle, D,
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
    # the unfused chain on the device: three plain GEMVs of the normed vector, then RoPE; both sides are within tol() of the exact
    # product, so within 2 tol() of each other (twice that for the rotated pairs, as above)
    q1, k1, v1 = gemv(mgr, rq, H * D, E, xn), gemv(mgr, rk, Hkv * D, E, xn), gemv(mgr, rv, Hkv * D, E, xn)
    assert (np.abs(pq.GetValue() - orc.rope(q1, freqs, D, H, D, pos)) <= 4 * tol(dq, xn) + 1e-6).all()
    assert (np.abs(krow - orc.rope(k1, freqs, D, Hkv, D, pos)) <= 4 * tol(dk, xn) + 1e-6 + h16 * np.abs(kr)).all()
    assert (np.abs(vrow - v1) <= 2 * tol(dv, xn) + h16 * np.abs(v)).all()


# ---- table and head ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,E", [(48, 256), (64, 512)])
def test_embed_iq4_xs_every_row(mgr, V, E):
    from nfai_amd._lib import call
    from nfai_amd.hip import ShaderProperty
    raw, Wd = quantize((0.05 * rng(3 + V).standard_normal((V, E))).astype(np.float32))
    tab = mgr.UploadWeight(IQ4_XS, raw, V, E)
    tok, y = ShaderProperty(mgr, 1, np.uint32), ShaderProperty(mgr, E)
    for t in range(V):
        tok.SetValue(np.array([t], np.uint32))
        call("nfai_hip_embed", mgr.handle, tab.handle, IQ4_XS, tok.handle, y.handle, E)
        np.testing.assert_array_equal(y.GetValue(), Wd[t])  # (d * (ls - 32)) * KV[q] in the restatement's order


def test_embed_iq4_xs_rotated_codes_and_distinct_scales(mgr):
    """The table lookup of t16_row_load4 with every code at every byte place, under eight distinct scales per block."""
    from nfai_amd._lib import call
    from nfai_amd.hip import ShaderProperty
    V, E = 32, 512
    b = _extreme("codes_rotated", V, E, rng(5)).reshape(-1, 136)
    row, blk = np.arange(b.shape[0]) // 2, np.arange(b.shape[0]) % 2
    pack_ls(b, (8 * np.arange(8)[None, :] + 5 * (row % 16)[:, None] + 3 * blk[:, None] + (row // 16)[:, None]) % 64)
    raw = b.ravel()
    Wd = synth.dequantize_iq4_xs(raw.tobytes(), V, E)
    tab = mgr.UploadWeight(IQ4_XS, raw, V, E)
    tok, y = ShaderProperty(mgr, 1, np.uint32), ShaderProperty(mgr, E)
    for t in range(V):
        tok.SetValue(np.array([t], np.uint32))
        call("nfai_hip_embed", mgr.handle, tab.handle, IQ4_XS, tok.handle, y.handle, E)
        np.testing.assert_array_equal(y.GetValue(), Wd[t])


@pytest.mark.parametrize("V,E", [(48, 256), (4000, 3072)])
def test_lmhead_argmax_iq4_xs(mgr, V, E):
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
    tab = mgr.UploadWeight(IQ4_XS, raw, V, E)
    px, pg, pl, pi = ShaderProperty(mgr, E), ShaderProperty(mgr, E), ShaderProperty(mgr, V), ShaderProperty(mgr, 1, np.uint32)
    px.SetValue(x); pg.SetValue(g)
    call("nfai_hip_lmhead_argmax", mgr.handle, tab.handle, IQ4_XS, px.handle, pg.handle, 1e-5, pl.handle, pi.handle, V, E)
    lg = pl.GetValue()
    want = orc.gemv(Wd, xn)
    assert (np.abs(lg - want) <= tol(Wd, xn)).all()
    assert int(pi.GetValue()[0]) == orc.argmax(want) == min(dup)
    # the unfused chain on the device: the plain GEMV of the normed vector, then ArgMax (both sides within tol() of the exact product)
    chain = gemv(mgr, raw, V, E, xn)
    assert (np.abs(lg - chain) <= 2 * tol(Wd, xn)).all()
    assert int(pi.GetValue()[0]) == orc.argmax(chain)


def test_gemm_kq_refuses_iq4_xs(mgr):
    from nfai_amd import _lib
    from nfai_amd.hip import ShaderProperty
    M, N, K = 64, 64, 256
    raw, _ = quantize((0.02 * rng(1).standard_normal((N, K))).astype(np.float32))
    w = mgr.UploadWeight(IQ4_XS, raw, N, K)
    pa, pc = ShaderProperty(mgr, M * K, np.float16), ShaderProperty(mgr, M * N)
    with pytest.raises(_lib.NfaiHipError, match="IQ4_XS") as e:
        _lib.call("nfai_hip_gemm_kq", mgr.handle, pa.handle, w.handle, IQ4_XS, 0, pc.handle, M, N, K)
    assert e.value.code == _lib.ERR_UNSUPPORTED


def test_upload_refuses_iq4_xs_outside_the_shape_rule(mgr):
    from nfai_amd import _lib
    with pytest.raises(_lib.NfaiHipError, match="IQ4_XS needs rows % 16 == 0") as e:
        mgr.UploadWeight(IQ4_XS, np.zeros(8 * 136, np.uint8), 8, 256)
    assert e.value.code == _lib.ERR_UNSUPPORTED


# ---- whole models ------------------------------------------------------------------------------------------------------------------
# H / Hkv = 4 and eight blocks: the iq4_xs mix keeps attn_v in Q5_K (two q|k|v launches per block) and ffn_down of block 0 in Q5_K
GQA4 = synth.LlamaDims("iq4-gqa4", 256, 8, 4, 1, 64, 512, 512, True)


def mix_type(name, mix, dims):
    """iq4_xs / all_iq4_xs: synth.iq4_xs_type; a (q, k, v) tuple: those types for the three attention inputs, the rest IQ4_XS."""
    if isinstance(mix, tuple):
        parts = name.split(".")
        return mix[("attn_q", "attn_k", "attn_v").index(parts[2])] if len(parts) > 2 and parts[2] in ("attn_q", "attn_k", "attn_v") else IQ4_XS
    return synth.iq4_xs_type(name, dims, mix)


_WEIGHTS = {}


def quant_weights(dims, seed, mix="all_iq4_xs", std=0.05, type_of=None):
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
            qt = type_of(name) if type_of else mix_type(name, mix, dims)
            raw, deq = quantize(a.astype(np.float32), qt)
            wq[name] = QuantTensor(raw, qt, a.shape)
            wref[name] = deq
        _WEIGHTS[key] = (wq, wref)
    return _WEIGHTS[key]


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


@pytest.mark.parametrize("dims,mix", [(synth.TINY, "all_iq4_xs"), (synth.TINY_D128, "all_iq4_xs"), (synth.TINY_D128, "iq4_xs"), (GQA4, "iq4_xs")],
                         ids=lambda v: getattr(v, "name", v))
def test_model_iq4_xs_graph_eager_unfused(mgr, dims, mix):
    """Graph (the default), NFAI_LLAMA_NO_GRAPH and the unfused 1:1 chain against OracleLlama, 8 decode steps: greedy tokens identical,
    logits within 5e-4 * max(1, |logit|) (the bar of test_model_q3_k_graph_eager_unfused).  all_iq4_xs: an IQ4_XS token_embd (through
    the q|k|v launch's BEGIN prologue in graph / eager, k_embed_t16 unfused) and an IQ4_XS lm_head + ArgMax.  GQA4 in the iq4_xs mix:
    q and k in IQ4_XS share a launch, the Q5_K v gets its own; ffn_down of block 0 is Q5_K, the tied table Q6_K."""
    wq, wref = quant_weights(dims, 61, mix)
    models, _ = run_against_oracle(mgr, dims, wq, wref, 8, graph={}, eager={"graph": False}, unfused={"unfused": True})
    total, _ = models[0].BytesPerToken(0)
    prof = models[0].ProfileStep(7)
    for m in models:
        m.Dispose()
    types = {k: v.ggml_type for k, v in wq.items() if hasattr(v, "ggml_type")}
    if dims is GQA4:
        assert types["blk.0.attn_v.weight"] == Q5_K and types["blk.0.ffn_down.weight"] == Q5_K and types["blk.1.ffn_down.weight"] == IQ4_XS
        assert types["token_embd.weight"] == Q6_K
    assert prof["qkv"][1] == (2 if dims is GQA4 else 1) * dims.L, prof
    if mix == "all_iq4_xs":
        assert set(types.values()) == {IQ4_XS}
        E, F, V, KD, HD = dims.E, dims.F, dims.V, dims.Hkv * dims.D, dims.H * dims.D
        blk = (HD * E + 2 * KD * E + E * HD + 3 * E * F) * 136 // 256
        kv = 2 * KD * 4 * 1 + 2 * KD * 4
        head = V * E * 136 // 256
        assert total == dims.L * (blk + kv) + E * 136 // 256 + head


def test_decode_greedy_iq4_xs_equals_stepped(mgr):
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY_D128
    for mix in ("iq4_xs", "all_iq4_xs"):
        wq, _ = quant_weights(dims, 61, mix)
        a = LlamaModel(mgr, synth.make_metadata(dims), wq, 48, dims=ddict(dims))
        b = LlamaModel(mgr, synth.make_metadata(dims), wq, 48, dims=ddict(dims))
        got = [int(t) for t in a.Greedy(7, 24)]
        tok, want = 7, []
        for _ in range(24):
            tok = b.Step(tok, want_logits=False)[1]
            want.append(tok)
        assert got == want, mix
        assert a.Pos == b.Pos == 24
        a.Dispose()
        b.Dispose()


def test_model_iq4_xs_fp16_kv(mgr):
    """fp16 KV cache: the bar of the batched tests' fp16-cache runs (2e-2 * max(1, |logit|)), ArgMax wherever the oracle's margin exceeds it."""
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY_D128
    wq, wref = quant_weights(dims, 61, "iq4_xs")
    m = LlamaModel(mgr, synth.make_metadata(dims), wq, 40, dims=ddict(dims), kv_f16=True)
    ref = orc.OracleLlama(odesc(dims, 40), wref)
    tok = 7
    for i in range(8):
        want = ref.step(tok)
        lg, am = m.Step(tok)
        bar = 2e-2 * max(1.0, float(np.abs(want).max()))
        assert np.abs(lg - want).max() <= bar, i
        top = np.sort(want)[-2:]
        if top[1] - top[0] > 2 * bar:
            assert am == orc.argmax(want)
        tok = orc.argmax(want)
    m.Dispose()


QKV_MIXES = [(IQ4_XS, IQ4_XS, IQ4_XS), (IQ4_XS, IQ4_XS, Q5_K), (Q6_K, IQ4_XS, Q6_K), (IQ4_XS, Q4_0, Q4_K)]
QKV_E256 = synth.LlamaDims("qkv-e256", 256, 1, 4, 2, 64, 512, 512, True)
QKV_E3072 = synth.LlamaDims("qkv-e3072", 3072, 1, 4, 2, 64, 512, 512, True)


@pytest.mark.parametrize("qkv", QKV_MIXES, ids=lambda t: "-".join(str(x) for x in t))
@pytest.mark.parametrize("dims", [QKV_E256, QKV_E3072], ids=lambda d: d.name)
def test_qkv_rope_iq4_xs_type_combinations(mgr, dims, qkv):
    """q|k|v of one block with (q, k, v) in the types an IQ4_XS file has (and Q6_K around an IQ4_XS k, and IQ4_XS beside Q4_0 and
    Q4_K, which stage alike: three launches each): the K and V cache rows of four positions against the oracle's under the bounds of
    the q|k|v operator test, q through the logits.  Launch count: IQ4_XS segments share a launch only with each other."""
    from nfai_amd.llama_model import LlamaModel
    wq, wref = quant_weights(dims, 63, qkv)
    m = LlamaModel(mgr, synth.make_metadata(dims), wq, 16, dims=ddict(dims))
    ref = orc.OracleLlama(odesc(dims, 16), wref)
    tok, fed = 7, []
    for i in range(4):
        want = ref.step(tok)
        lg, am = m.Step(tok)
        assert np.abs(lg - want).max() <= 5e-4 * max(1.0, float(np.abs(want).max())), i
        fed.append(tok)
        tok = orc.argmax(want)
    for pos in range(4):
        xn = orc.rmsnorm(np.asarray(wref["token_embd.weight"][fed[pos]], np.float32), wref["blk.0.attn_norm.weight"], 1e-5)
        wk, wv = ref.kcache(0)[pos], ref.vcache(0)[pos]
        assert (np.abs(m.ReadKV(0, False, pos) - wk) <= 2 * tol(wref["blk.0.attn_k.weight"], xn) + 1e-6).all(), pos
        assert (np.abs(m.ReadKV(0, True, pos) - wv) <= tol(wref["blk.0.attn_v.weight"], xn)).all(), pos
    prof = m.ProfileStep(tok)
    m.Dispose()
    assert prof["qkv"][1] == {QKV_MIXES[0]: 1, QKV_MIXES[1]: 2}.get(qkv, 3), prof


def test_model_iq4_xs_down_projection_above_8192(mgr):
    """THIN_F14336, one block: Wdown at K = 14336 (four super-blocks per wave) inside the model."""
    dims = synth.THIN_F14336
    wq, wref = quant_weights(dims, 65, "iq4_xs")
    assert wq["blk.0.ffn_down.weight"].ggml_type == IQ4_XS
    models, _ = run_against_oracle(mgr, dims, wq, wref, 6, graph={})
    for m in models:
        m.Dispose()


def test_decode_iq4_xs_is_bit_reproducible(mgr):
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY_D128
    wq, _ = quant_weights(dims, 61, "iq4_xs")
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


@pytest.mark.parametrize("mix", ["iq4_xs", "all_iq4_xs"])
@pytest.mark.parametrize("n,chunk", [(70, 64), (40, 128)], ids=["chunked", "one-chunk"])
def test_prefill_mfma_iq4_xs(mgr, n, chunk, mix):
    """The MFMA prefill widens IQ4_XS to fp16: the bar of tests/test_gpu_q3_k.py's prefill (2e-2 * max(1, |logit|)) and the fp16 bar of
    nfai_hip.h for the cache rows (2e-2 absolute on these weights)."""
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY_D128
    wq, wref = quant_weights(dims, 61, mix)
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


def test_fp16_widening_of_iq4_xs_element_by_element(mgr):
    """k_dequant_t16<IQ4_XS> seen through the prefill: with an fp16 embedding table whose row t is the unit vector e_t and a gain of
    ones, the normed row of token t is c e_t (c = the fp16 rounding of 1 / sqrt(1 / E + eps), the same for every token), so the V row
    that the MFMA prefill writes for position t in block 0 is c * W16[:, t] with W16 the fp16-widened attn_v: the product of two fp16
    values is exact in fp32 and every other term of the dot is an exact zero.  512 tokens give every column of the matrix; c is read
    off the first non-zero element and must be the one fp16 value for all positions; every element is then compared EXACTLY with
    dequantize_iq4_xs rounded to fp16.  The matrix holds rotated codes under distinct scales and signs of d, and d = 16 (the widening
    condition's edge: 16 * 32 * 127 = 65024) in its first rows."""
    from nfai_amd.llama_model import LlamaModel, QuantTensor
    dims = synth.TINY_D128
    E, KD = dims.E, dims.Hkv * dims.D
    wq, _ = quant_weights(dims, 61, "iq4_xs")
    wq = dict(wq)
    wq["token_embd.weight"] = np.eye(dims.V, E, dtype=np.float16)
    wq["blk.0.attn_norm.weight"] = np.ones(E, np.float32)
    b = _extreme("codes_rotated", KD, E, rng(8)).reshape(-1, 136)
    nb = b.shape[0]
    row, blk = np.arange(nb) // (E // 256), np.arange(nb) % (E // 256)
    pack_ls(b, (8 * np.arange(8)[None, :] + 5 * (row % 16)[:, None] + 3 * blk[:, None] + (row // 16)[:, None]) % 64)
    b[::3, 1] ^= 0x80                                   # every third block: d negated
    b[:2 * (E // 256), 0:2] = _f16_bytes(np.full(2 * (E // 256), 16.0))
    raw = b.ravel()
    wq["blk.0.attn_v.weight"] = QuantTensor(raw, IQ4_XS, (KD, E))
    Wd = synth.dequantize_iq4_xs(raw.tobytes(), KD, E)
    assert np.abs(Wd).max() <= 65024 and np.abs(Wd[:2]).max() >= 16 * 31 * 113
    W16 = Wd.astype(np.float16)
    assert np.isfinite(W16).all() and (W16 != 0).any(axis=0).all()
    m = LlamaModel(mgr, synth.make_metadata(dims), wq, E, dims=ddict(dims), max_batch=128)
    m.Ingest(np.arange(E, dtype=np.uint32))
    cs = set()
    for t in range(E):
        v = m.ReadKV(0, True, t)
        col = W16[:, t].astype(np.float32)
        i0 = int(np.flatnonzero(col)[0])
        c = np.float32(v[i0]) / col[i0]
        cs.add(float(c))
        np.testing.assert_array_equal(v, c * col, err_msg=f"column {t}")
    m.Dispose()
    assert len(cs) == 1, cs
    c = cs.pop()
    assert np.float32(np.float16(c)) == c and abs(c - 1 / np.sqrt(1 / E + 1e-5)) <= 2.0 ** -10 * c   # (an fp16 value next to the quotient)


def test_score_iq4_xs_against_the_per_step_logits(mgr):
    """nfai_hip_llama_score on 40 tokens (all_iq4_xs: the IQ4_XS head widened slab by slab): the log-probability of every next token
    and of the maximum against log-softmax of a twin's token-by-token logits, bars as tests/test_gpu_q3_k.py's."""
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY_D128
    wq, _ = quant_weights(dims, 61, "all_iq4_xs")
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


def test_pipeline_two_stage_split_iq4_xs(mgr):
    """Two stages of the GQA4 model in the iq4_xs mix (blocks 0-2 and 3-7, each numbering its blocks within the file: only the file's
    block 0 keeps ffn_down in Q5_K) against the single model: bit-equal logits and tokens."""
    import torch
    from nfai_amd.llama_model import LlamaModel
    dims = GQA4
    wq, _ = quant_weights(dims, 61, "iq4_xs")
    assert [wq[f"blk.{l}.ffn_down.weight"].ggml_type for l in (0, 1, 3)] == [Q5_K, IQ4_XS, IQ4_XS]
    assert synth.iq4_xs_type("blk.0.ffn_down.weight", dims, "iq4_xs", layer_offset=3, n_layers_file=dims.L) == IQ4_XS
    md = synth.make_metadata(dims)
    whole = LlamaModel(mgr, md, wq, 32, dims=ddict(dims))
    stages = [LlamaModel(mgr, md, wq, 32, dims=ddict(dims), layer_range=rg) for rg in [(0, 3), (3, 8)]]
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


def test_iq4_xs_gguf_file_to_generation(mgr, tmp_path):
    """An IQ4_XS GGUF file (GQA4: tied Q6_K embedding; IQ4_XS and Q5_K blocks) -> Parser().Parse -> the provider's model -> 8 greedy
    tokens, against the oracle on the dequantised weights read back from the same file."""
    from nfai_amd import gguf
    from nfai_amd.llama_model import LlamaModelFactory, ModelOptions
    dims = GQA4
    wq, _ = quant_weights(dims, 61, "iq4_xs")
    path = str(tmp_path / "iq4_xs.gguf")
    gguf.write_model(path, synth.make_metadata(dims), wq)
    _, t = gguf.Parser().Read(path)
    assert {t[k].ggml_type for k in wq if not isinstance(wq[k], np.ndarray)} == {IQ4_XS, Q5_K, Q6_K}
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
