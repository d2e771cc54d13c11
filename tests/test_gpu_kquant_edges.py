"""K-quant and Q8_0 kernels at the edges: every activation scale the fixed-point staging must survive, adversarial Q4_K / Q6_K blocks
through every kernel that reads them, and the prefill's fp16 widening element by element.

Oracle: the blocks dequantised by the oracle (oracle/nfai_oracle.c for Q4_K / Q6_K, the NumPy restatements of tests/test_gpu_q5_k.py
and tests/test_gpu_q8_0.py for Q5_K / Q8_0), then the operation in fp64.  Bound of an int8-MFMA GEMV output, with no absolute floor:
x rounded to 24 bits relative to its super-block's largest |x| (2^-21 * sum_b max|x_b| * sum_{k in b} |w_k|, twice the rounding
error) plus the fp32 accumulation term the K-quant tests state (2e-6 * sqrt(K / 256) * sum |w| |x|)."""
import ctypes as C

import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth

pytestmark = pytest.mark.gpu

F32, Q8_0, Q4_K, Q5_K, Q6_K = 0, 8, 12, 13, 14


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


# ---- the oracle's dequantisation -------------------------------------------------------------------------------------------------

def dequant_q5_k(raw, rows, cols):
    """ggml dequantize_row_q5_K (the restatement tests/test_q5_k.py pins): y = d * sc * q - dmin * m, q = nibble | fifth bit << 4."""
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
    b = np.frombuffer(np.ascontiguousarray(raw, np.uint8).tobytes(), np.uint8).reshape(rows * cols // 32, 34)
    d = b[:, :2].copy().view(np.float16).astype(np.float32)[:, 0]
    return (d[:, None] * b[:, 2:].copy().view(np.int8).astype(np.float32)).reshape(rows, cols)


def dequant(raw, qt, rows, cols):
    if qt == Q4_K:
        return orc.dequant_q4k(raw, rows * cols).reshape(rows, cols)
    if qt == Q6_K:
        return orc.dequant_q6k(raw, rows * cols).reshape(rows, cols)
    if qt == Q5_K:
        return dequant_q5_k(raw, rows, cols)
    return dequant_q8_0(raw, rows, cols)


def quantize(W, qt):
    """W [N][K] fp32 -> (raw block bytes, dequantised fp32 [N][K])."""
    N, K = W.shape
    if qt == Q4_K:
        b = orc.quantize_q4k(W)
    elif qt == Q6_K:
        b = orc.quantize_q6k(W)
    elif qt == Q5_K:
        b = np.frombuffer(synth.quantize_q5_k(W), np.uint8).copy()
    else:
        b = np.frombuffer(synth.quantize_q8_0(W), np.uint8).copy()
    return b, dequant(b, qt, N, K)


def stage_tol(Wd, x):
    W, xa = np.abs(np.asarray(Wd, np.float64)), np.abs(np.asarray(x, np.float64))
    N, K = W.shape
    bmax = xa.reshape(K // 256, 256).max(axis=1)
    return 2.0 ** -21 * (W.reshape(N, K // 256, 256).sum(axis=2) @ bmax) + 2e-6 * np.sqrt(K / 256.0) * (W @ xa)


def check(got, want, bound, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    bad = err > bound
    assert not bad.any(), (what, int(bad.sum()), float((err / np.maximum(bound, 1e-300)).max()), float(err.max()))


def rmsnorm64(x, g, eps):
    x64 = np.asarray(x, np.float64)
    return x64 / np.sqrt(np.mean(x64 * x64) + eps) * np.asarray(g, np.float64)


# ---- 3a: activation scales ------------------------------------------------------------------------------------------------------

K_SW = 2048          # eight super-blocks: one per decade of the "decades" case
SCALES = ["1e-37", "1e-30", "1e-20", "1", "1e20", "1e34", "decades", "denormal"]


def staged(case, r, K=K_SW):
    """The values the launch stages, as (x, per-element magnitude).  decades: super-block b at 10^e_b, e from -35 to 30; denormal:
    one super-block of fp32 subnormals (|x| < 2^-126), the others zero so that its contribution is the whole output."""
    z = r.standard_normal(K)
    if case == "decades":
        mag = np.repeat(10.0 ** np.linspace(-35, 30, K // 256), 256)
    elif case == "denormal":
        mag = np.zeros(K)
        mag[512:768] = 1e-40
    else:
        mag = np.full(K, float(case))
    return z, mag


def floor_for(case, K, rms=1.0):
    """The denormal case's products are fp32 subnormals themselves: each (super-block, lane group) partial is rounded once to that
    grid (2^-150) before the launch divides by the RMSNorm's rms, and nothing else is left of the bound."""
    return (K // 256) * 4 * 2.0 ** -150 / rms if case == "denormal" else 0.0


def rms64(x, eps):
    x64 = np.asarray(x, np.float64)
    return float(np.sqrt(np.mean(x64 * x64) + eps))


def silu64(a):
    e = np.exp(-np.abs(a))
    return np.where(a >= 0, a / (1 + e), a * e / (1 + e))


def upload(mgr, qt, raw, N, K):
    return mgr.UploadWeight(qt, raw, N, K)


def prop(mgr, a, dtype=np.float32):
    from nfai_amd.hip import ShaderProperty
    a = np.ascontiguousarray(a, dtype)
    p = ShaderProperty(mgr, a.size, dtype)
    p.SetValue(a.ravel())
    return p


def weights(qt, N, K, seed):
    r = rng(seed)
    return quantize((0.02 * r.standard_normal((N, K))).astype(np.float32), qt)


def normed_inputs(case, r, K=K_SW):
    """RMSNorm launches stage x * g.  The norm's fp32 sum of squares (as in the reference) overflows for |x| above ~1e18, so the
    magnitude rides on x up to 1 and on the gains above it: x * g still sweeps every scale of `staged`."""
    z, mag = staged(case, r, K)
    xm, gm = np.minimum(mag, 1.0), np.maximum(mag, 1.0)
    if case == "denormal":
        xm, gm = mag, np.ones(K)
    x = (xm * z).astype(np.float32)
    g = (gm * (1 + 0.1 * r.standard_normal(K))).astype(np.float32)
    return x, g


@pytest.mark.parametrize("qt", [Q4_K, Q5_K, Q6_K, Q8_0], ids=["q4_k", "q5_k", "q6_k", "q8_0"])
def test_scale_sweep_plain_gemv(mgr, qt):
    from nfai_amd._lib import call
    N, K = 64, K_SW
    raw, Wd = weights(qt, N, K, 10 + qt)
    w = upload(mgr, qt, raw, N, K)
    py = prop(mgr, np.zeros(N))
    for case in SCALES:
        z, mag = staged(case, rng(qt))
        x = (mag * z).astype(np.float32)
        if case == "denormal":
            assert (np.abs(x[512:768]) < 2.0 ** -126).all() and (x[512:768] != 0).all()
        px = prop(mgr, x)
        call("nfai_hip_gemv", mgr.handle, w.handle, qt, px.handle, py.handle, 0, N, K)
        want = Wd.astype(np.float64) @ x.astype(np.float64)
        check(py.GetValue(), want, stage_tol(Wd, x) + floor_for(case, K), (case, "plain"))


@pytest.mark.parametrize("qt", [Q4_K, Q5_K, Q6_K, Q8_0], ids=["q4_k", "q5_k", "q6_k", "q8_0"])
def test_scale_sweep_fused_norm_residual(mgr, qt):
    """nfai_hip_gemv_fused with the RMSNorm gains and a residual: y = res + W (x / rms * g)."""
    from nfai_amd._lib import call
    N, K = 64, K_SW
    raw, Wd = weights(qt, N, K, 20 + qt)
    w = upload(mgr, qt, raw, N, K)
    py = prop(mgr, np.zeros(N))
    for case in SCALES:
        r = rng(100 + qt)
        x, g = normed_inputs(case, r)
        xn = rmsnorm64(x, g, 1e-5)
        mv = Wd.astype(np.float64) @ xn
        res = (np.abs(mv).max() * r.standard_normal(N)).astype(np.float32)
        px, pg, pr = prop(mgr, x), prop(mgr, g), prop(mgr, res)
        call("nfai_hip_gemv_fused", mgr.handle, w.handle, qt, px.handle, pg.handle, 1e-5, pr.handle, py.handle, N, K)
        want = res.astype(np.float64) + mv
        # + the rounding of the residual add (2^-24 |y|, taken twice)
        fl = floor_for(case, K, rms64(x, 1e-5))
        check(py.GetValue(), want, stage_tol(Wd, xn) + 2.0 ** -23 * np.abs(want) + fl, (case, "fused"))


@pytest.mark.parametrize("qt", [Q4_K, Q5_K, Q6_K, Q8_0], ids=["q4_k", "q5_k", "q6_k", "q8_0"])
def test_scale_sweep_gateup_silu(mgr, qt):
    """act = silu(Wg xn) * (Wu xn): quadratic in the staged scale, so the sweep keeps act a normal fp32 number.  With eps = 0 the
    norm divides by rms(x) alone, which decouples the staged magnitude of x * g from the outputs' magnitude (that of g)."""
    from nfai_amd._lib import call
    F, E = 64, K_SW
    rg_, Wg = weights(qt, F, E, 30 + qt)
    ru_, Wu = weights(qt, F, E, 40 + qt)
    bg, bu = upload(mgr, qt, rg_, F, E), upload(mgr, qt, ru_, F, E)
    pa = prop(mgr, np.zeros(F))
    # staged scale of x * g = (scale of x) * (scale of g): name -> (scale of x, scale of g, eps)
    cases = {"1e-36": (1e-18, 1e-18, 0.0), "1e-30": (1e-12, 1e-18, 0.0), "1e-20": (1e-10, 1e-10, 0.0), "1": (1.0, 1.0, 1e-5),
             "1e34": (1e17, 1e17, 0.0)}
    for case, (sx, sg, eps) in cases.items():
        r = rng(200 + qt)
        x = (sx * r.standard_normal(E)).astype(np.float32)
        g = (sg * (1 + 0.1 * r.standard_normal(E))).astype(np.float32)
        xn = rmsnorm64(x, g, eps)
        px, pg = prop(mgr, x), prop(mgr, g)
        call("nfai_hip_gemv_gateup_silu", mgr.handle, bg.handle, bu.handle, qt, px.handle, pg.handle, eps, pa.handle, F, E)
        a, b = Wg.astype(np.float64) @ xn, Wu.astype(np.float64) @ xn
        ta, tb = stage_tol(Wg, xn), stage_tol(Wu, xn)
        sa = silu64(a)
        want = sa * b
        # d silu / da <= 1.1; the kernel's silu (expf, division) and product: a few fp32 roundings of |act|
        bound = 1.1 * ta * (np.abs(b) + tb) + np.abs(sa) * tb + 1e-6 * np.abs(want)
        check(pa.GetValue(), want, bound, (case, "gateup"))


@pytest.mark.parametrize("qt", [Q4_K, Q5_K, Q6_K, Q8_0], ids=["q4_k", "q5_k", "q6_k", "q8_0"])
def test_scale_sweep_qkv_rope(mgr, qt):
    """nfai_hip_gemv_qkv_rope (RMSNorm, q | k | v, RoPE at pos, q out, k / v into an fp32 cache): q and k are rotated pairs, so their
    bound is twice that of the products; v is stored as computed."""
    from nfai_amd._lib import call
    H, Hkv, D, pos, E = 2, 1, 64, 3, K_SW
    (rq, dq), (rk, dk), (rv, dv) = (weights(qt, n, E, 50 + qt + s) for s, n in enumerate((H * D, Hkv * D, Hkv * D)))
    bq, bk, bv = upload(mgr, qt, rq, H * D, E), upload(mgr, qt, rk, Hkv * D, E), upload(mgr, qt, rv, Hkv * D, E)
    freqs = orc.rope_freqs(D)
    pf = prop(mgr, freqs)
    pq, kc, vc = prop(mgr, np.zeros(H * D)), prop(mgr, np.zeros((pos + 1) * Hkv * D)), prop(mgr, np.zeros((pos + 1) * Hkv * D))
    for case in SCALES:
        x, g = normed_inputs(case, rng(300 + qt))
        xn = rmsnorm64(x, g, 1e-5)
        px, pg = prop(mgr, x), prop(mgr, g)
        call("nfai_hip_gemv_qkv_rope", mgr.handle, bq.handle, bk.handle, bv.handle, qt, px.handle, pg.handle, 1e-5, pf.handle, D,
             pq.handle, kc.handle, vc.handle, H, Hkv, D, pos, F32, E)
        q, k, v = (W.astype(np.float64) @ xn for W in (dq, dk, dv))
        qr = orc.np_oracle.rope(q, freqs.astype(np.float64), D, H, D, pos)
        kr = orc.np_oracle.rope(k, freqs.astype(np.float64), D, Hkv, D, pos)
        fl = floor_for(case, E, rms64(x, 1e-5))
        # the rotation: |q| of the pair times the fp32 angle's error (pos * 2^-24, cos / sin to a few ulp)
        check(pq.GetValue(), qr, 2 * stage_tol(dq, xn) + 1e-6 * np.abs(q).max() * (1 + pos) + 2 * fl, (case, "q"))
        check(kc.GetValue()[pos * Hkv * D:], kr, 2 * stage_tol(dk, xn) + 1e-6 * np.abs(k).max() * (1 + pos) + 2 * fl, (case, "k"))
        check(vc.GetValue()[pos * Hkv * D:], v, stage_tol(dv, xn) + fl, (case, "v"))


@pytest.mark.parametrize("qt", [Q4_K, Q5_K, Q6_K, Q8_0], ids=["q4_k", "q5_k", "q6_k", "q8_0"])
def test_scale_sweep_lmhead_argmax(mgr, qt):
    """RMSNorm + lm_head + ArgMax: logits within the bound, the index the oracle's first maximum.  Row 37 is a clear winner
    (sign(xn) * 0.06: its logit exceeds every other by far more than the bounds)."""
    from nfai_amd._lib import call
    V, E = 256, K_SW
    r = rng(60 + qt)
    W = (0.02 * r.standard_normal((V, E))).astype(np.float32)
    pl, pi = prop(mgr, np.zeros(V)), prop(mgr, np.zeros(1), np.uint32)
    for case in SCALES:
        x, g = normed_inputs(case, rng(400 + qt))
        xn = rmsnorm64(x, g, 1e-5)
        W[37] = np.where(xn >= 0, 0.06, -0.06)
        raw, Wd = quantize(W, qt)
        w = upload(mgr, qt, raw, V, E)
        px, pg = prop(mgr, x), prop(mgr, g)
        call("nfai_hip_lmhead_argmax", mgr.handle, w.handle, qt, px.handle, pg.handle, 1e-5, pl.handle, pi.handle, V, E)
        want = Wd.astype(np.float64) @ xn
        bound = stage_tol(Wd, xn) + floor_for(case, E, rms64(x, 1e-5))
        check(pl.GetValue(), want, bound, (case, "lm_head"))
        top = int(np.argmax(want))
        assert top == 37 and np.sort(want)[-2] + 2 * bound.max() < want[top], case
        assert int(pi.GetValue()[0]) == top, case
        w.free()


# ---- 3b: adversarial Q4_K / Q6_K blocks ---------------------------------------------------------------------------------------

def f16_bits(v):
    return np.asarray(v, np.float16).view(np.uint16)


def pack_q4k(d, dmin, scales, codes):
    """ggml block_q4_K from its fields: d, dmin (fp16 bit patterns [nb]), scales [nb][12] bytes, codes [nb][256] in 0..15
    (weight 64j + l <- low nibble of qs[32j + l], 64j + 32 + l <- its high nibble)."""
    nb = codes.shape[0]
    c = codes.reshape(nb, 4, 2, 32).astype(np.uint8)
    qs = (c[:, :, 0, :] | (c[:, :, 1, :] << 4)).reshape(nb, 128)
    out = np.empty((nb, 144), np.uint8)
    out[:, 0:2] = np.asarray(d, np.uint16).reshape(nb, 1).view(np.uint8)
    out[:, 2:4] = np.asarray(dmin, np.uint16).reshape(nb, 1).view(np.uint8)
    out[:, 4:16] = scales
    out[:, 16:] = qs
    return out.ravel()


def pack_q6k(d, scales, codes):
    """ggml block_q6_K from its fields: codes [nb][256] in 0..63 (q = code - 32), scales [nb][16] int8, d fp16 bits [nb].
    Half n, l = 0..31: weights 128n + l + 32i take ql[64n + l + 32 (i & 1)] (low nibble for i < 2, high for i >= 2) and bits 2i of
    qh[32n + l]."""
    nb = codes.shape[0]
    c = codes.reshape(nb, 2, 4, 32).astype(np.uint8)
    lo, hi = c & 0xF, c >> 4
    ql = np.concatenate([lo[:, :, 0] | (lo[:, :, 2] << 4), lo[:, :, 1] | (lo[:, :, 3] << 4)], axis=2).reshape(nb, 128)
    qh = (hi[:, :, 0] | (hi[:, :, 1] << 2) | (hi[:, :, 2] << 4) | (hi[:, :, 3] << 6)).reshape(nb, 64)
    out = np.empty((nb, 210), np.uint8)
    out[:, :128] = ql
    out[:, 128:192] = qh
    out[:, 192:208] = np.asarray(scales, np.int8).view(np.uint8)
    out[:, 208:210] = np.asarray(d, np.uint16).reshape(nb, 1).view(np.uint8)
    return out.ravel()


Q4K_CASES = ["codes_0", "codes_15", "scales_ff", "d_0", "d_dmin_0", "negative_d_dmin", "subnormal_d_dmin", "random_bytes", "one_hot"]
Q6K_CASES = ["codes_0", "codes_63", "scales_min", "scales_max", "negative_d", "subnormal_d", "random_bytes", "one_hot"]


def adversarial(qt, case, N, K, seed=0):
    """Raw blocks of the named case for an N x K matrix.  Fields not named by the case come from the oracle's quantiser (moderate
    d, every scale used); one_hot: exactly one non-zero weight per row, each row at its own (super-block, sub-block, position)."""
    r = rng(seed + 7 * N + K + qt)
    nb, NB = N * K // 256, K // 256
    raw = (orc.quantize_q4k if qt == Q4_K else orc.quantize_q6k)((0.02 * r.standard_normal((N, K))).astype(np.float32))
    if qt == Q4_K:
        b = raw.reshape(nb, 144).copy()
        d, dmin, sc = b[:, 0:2].copy().view(np.uint16)[:, 0], b[:, 2:4].copy().view(np.uint16)[:, 0], b[:, 4:16].copy()
        q = np.stack([b[:, 16:].reshape(nb, 4, 32) & 0xF, b[:, 16:].reshape(nb, 4, 32) >> 4], axis=2).reshape(nb, 256)
        if case == "codes_0":
            q[:] = 0
        elif case == "codes_15":
            q[:] = 15
        elif case == "scales_ff":
            sc[:] = 0xFF
        elif case == "d_0":
            d[:] = 0
        elif case == "d_dmin_0":
            d[:] = 0
            dmin[:] = 0
        elif case == "negative_d_dmin":
            d |= 0x8000
            dmin |= 0x8000
        elif case == "subnormal_d_dmin":
            d[:] = r.integers(1, 0x400, nb)
            dmin[:] = r.integers(1, 0x400, nb) | 0x8000 * r.integers(0, 2, nb)
        elif case == "random_bytes":
            sc = r.integers(0, 256, (nb, 12), dtype=np.uint8)
            q = r.integers(0, 16, (nb, 256))
            d = f16_bits(r.uniform(1e-3, 1e-2, nb) * r.choice([-1, 1], nb))
            dmin = f16_bits(r.uniform(1e-3, 1e-2, nb) * r.choice([-1, 1], nb))
        elif case == "one_hot":
            q[:] = 0
            dmin[:] = 0
            sc = r.integers(0, 256, (nb, 12), dtype=np.uint8)
            sc[:, 0:4] |= 1  # sub-blocks 0-3: 6-bit scale >= 1
            sc[:, 8:12] |= 0x11  # sub-blocks 4-7: low four bits of the scale >= 1 (and of the min)
            for row in range(N):
                sb, l = row % 8, (row * 7 + row // 8) % 32
                q[row * NB + (row // 8) % NB, 32 * sb + l] = 9
        return pack_q4k(d, dmin, sc, q)
    b = raw.reshape(nb, 210).copy()
    d, sc = b[:, 208:210].copy().view(np.uint16)[:, 0], b[:, 192:208].copy().view(np.int8)
    ql, qh = b[:, :128].reshape(nb, 2, 2, 32), b[:, 128:192].reshape(nb, 2, 32)
    lo = np.stack([ql[:, :, 0] & 0xF, ql[:, :, 1] & 0xF, ql[:, :, 0] >> 4, ql[:, :, 1] >> 4], axis=2)
    hi = np.stack([(qh >> (2 * i)) & 3 for i in range(4)], axis=2)
    q = (lo | (hi << 4)).reshape(nb, 256).astype(np.int64)
    if case == "codes_0":
        q[:] = 0
    elif case == "codes_63":
        q[:] = 63
    elif case == "scales_min":
        sc[:] = -128
    elif case == "scales_max":
        sc[:] = 127
    elif case == "negative_d":
        d |= 0x8000
    elif case == "subnormal_d":
        d[:] = r.integers(1, 0x400, nb) | 0x8000 * r.integers(0, 2, nb)
    elif case == "random_bytes":
        q = r.integers(0, 64, (nb, 256))
        sc = r.integers(-128, 128, (nb, 16)).astype(np.int8)
        d = f16_bits(r.uniform(1e-4, 1e-3, nb) * r.choice([-1, 1], nb))
    elif case == "one_hot":
        q[:] = 32
        sc = r.integers(1, 128, (nb, 16)).astype(np.int8) * r.choice([-1, 1], (nb, 16)).astype(np.int8)
        for row in range(N):
            g16, l = row % 16, (row * 5 + row // 16) % 16
            q[row * NB + (row // 16) % NB, 16 * g16 + l] = 32 + 9 + row % 20
    return pack_q6k(d, sc, q)


def case_ids(qt):
    return [(qt, c) for c in (Q4K_CASES if qt == Q4_K else Q6K_CASES)]


ADV = case_ids(Q4_K) + case_ids(Q6_K)
ADV_IDS = [f"{'q4_k' if qt == Q4_K else 'q6_k'}-{c}" for qt, c in ADV]


def accumulated_magnitude(raw, qt, N, K):
    """|terms| the raw-layout VALU GEMV (k_gemv_kq) sums in fp32: it forms d * sc * sum q x - dmin * m * sum x (Q4_K) and
    d * sc * (sum code x - 32 sum x) (Q6_K, q = code - 32), so its rounding is relative to |d sc q| + |dmin m| and to
    |d sc| (code + 32) <= |w| + 64 |d sc|, not to |w|: one non-zero Q6_K weight among codes of 32 is the difference of two sums."""
    nb = N * K // 256
    if qt == Q4_K:
        b = np.asarray(raw, np.uint8).reshape(nb, 144).copy()
        bd, bm = b.copy(), b.copy()
        bd[:, 2:4] = 0  # dmin = 0: d * sc * q
        bm[:, 0:2] = 0  # d = 0: -dmin * m
        return np.abs(dequant(bd.ravel(), qt, N, K)) + np.abs(dequant(bm.ravel(), qt, N, K))
    b = np.asarray(raw, np.uint8).reshape(nb, 210).copy()
    b[:, :128], b[:, 128:192] = 0x11, 0xAA  # every code 33: q = 1, the weight is d * sc
    return np.abs(dequant(raw, qt, N, K)) + 64 * np.abs(dequant(b.ravel(), qt, N, K))


def one_hot_rows_distinct(Wd):
    nz = [tuple(np.flatnonzero(row)) for row in Wd]
    assert all(len(p) == 1 for p in nz) and len(set(nz)) == len(nz), "one_hot: one weight per row, each at its own position"


@pytest.mark.parametrize("qt,case", ADV, ids=ADV_IDS)
def test_adversarial_blocks_decode(mgr, qt, case):
    """One case through the T16 int8-MFMA GEMV (N = 64), the raw-layout VALU GEMV (N = 40), the fused RMSNorm + residual launch,
    gate|up + SiLU, q|k|v + RoPE, lm_head + ArgMax and the embedding lookup (T16 at V = 64, raw at V = 40)."""
    from nfai_amd._lib import call
    K = 1024
    r = rng(qt * 100 + len(case))
    x = r.standard_normal(K).astype(np.float32)
    g = (1 + 0.1 * r.standard_normal(K)).astype(np.float32)
    xn = rmsnorm64(x, g, 1e-5)
    px, pg = prop(mgr, x), prop(mgr, g)
    for N in (64, 40):
        raw = adversarial(qt, case, N, K)
        Wd = dequant(raw, qt, N, K)
        assert np.isfinite(Wd).all()
        if case == "one_hot":
            one_hot_rows_distinct(Wd)
        w = upload(mgr, qt, raw, N, K)
        py = prop(mgr, np.zeros(N))
        call("nfai_hip_gemv", mgr.handle, w.handle, qt, px.handle, py.handle, 0, N, K)
        # N = 40: the VALU fallback stages nothing; its fp32 sums are bounded by the accumulation term on what it accumulates
        mag = Wd if N % 16 == 0 else accumulated_magnitude(raw, qt, N, K)
        check(py.GetValue(), Wd.astype(np.float64) @ x, stage_tol(mag, x), (case, "gemv", N))
        # embedding rows: the dequantised weights exactly (d * sc * q - dmin * m in fp32, as the oracle)
        tok, ye = prop(mgr, np.zeros(1), np.uint32), prop(mgr, np.zeros(K))
        for t in (0, 1, N // 2 + 3, N - 1):
            tok.SetValue(np.array([t], np.uint32))
            call("nfai_hip_embed", mgr.handle, w.handle, qt, tok.handle, ye.handle, K)
            assert np.array_equal(ye.GetValue(), Wd[t]), (case, "embed", N, t)
        if N == 64:
            res = r.standard_normal(N).astype(np.float32)
            pr = prop(mgr, res)
            call("nfai_hip_gemv_fused", mgr.handle, w.handle, qt, px.handle, pg.handle, 1e-5, pr.handle, py.handle, N, K)
            want = res + Wd.astype(np.float64) @ xn
            check(py.GetValue(), want, stage_tol(Wd, xn) + 2.0 ** -23 * np.abs(want), (case, "fused"))
            # lm_head + ArgMax: ties (every row equal, e.g. all-zero blocks) must give the first index
            pl, pi = prop(mgr, np.zeros(N)), prop(mgr, np.zeros(1), np.uint32)
            call("nfai_hip_lmhead_argmax", mgr.handle, w.handle, qt, px.handle, pg.handle, 1e-5, pl.handle, pi.handle, N, K)
            want = Wd.astype(np.float64) @ xn
            bound = stage_tol(Wd, xn)
            lg = pl.GetValue()
            check(lg, want, bound, (case, "lm_head"))
            idx = int(pi.GetValue()[0])
            assert idx == int(np.argmax(lg)), (case, idx)
            top = int(np.argmax(want))
            if (want == want[top]).sum() > 1 or np.sort(want)[-2] + 2 * bound.max() < want[top]:
                assert idx == top, (case, idx, top)
        w.free()
    # gate|up with both matrices of this case (second one from another seed), then q|k|v + RoPE at one type per launch
    F = 64
    rg_, ru_ = adversarial(qt, case, F, K, 1), adversarial(qt, case, F, K, 2)
    dg, du = dequant(rg_, qt, F, K), dequant(ru_, qt, F, K)
    bg, bu, pa = upload(mgr, qt, rg_, F, K), upload(mgr, qt, ru_, F, K), prop(mgr, np.zeros(F))
    call("nfai_hip_gemv_gateup_silu", mgr.handle, bg.handle, bu.handle, qt, px.handle, pg.handle, 1e-5, pa.handle, F, K)
    a, b = dg.astype(np.float64) @ xn, du.astype(np.float64) @ xn
    ta, tb = stage_tol(dg, xn), stage_tol(du, xn)
    sa = silu64(a)
    check(pa.GetValue(), sa * b, 1.1 * ta * (np.abs(b) + tb) + np.abs(sa) * tb + 1e-6 * np.abs(sa * b), (case, "gateup"))
    H, Hkv, D, pos = 2, 1, 64, 2
    rq, rk, rv = adversarial(qt, case, H * D, K, 3), adversarial(qt, case, Hkv * D, K, 4), adversarial(qt, case, Hkv * D, K, 5)
    dq, dk, dv = dequant(rq, qt, H * D, K), dequant(rk, qt, Hkv * D, K), dequant(rv, qt, Hkv * D, K)
    bq, bk, bv = upload(mgr, qt, rq, H * D, K), upload(mgr, qt, rk, Hkv * D, K), upload(mgr, qt, rv, Hkv * D, K)
    freqs = orc.rope_freqs(D)
    pf = prop(mgr, freqs)
    pq, kc, vc = prop(mgr, np.zeros(H * D)), prop(mgr, np.zeros((pos + 1) * Hkv * D)), prop(mgr, np.zeros((pos + 1) * Hkv * D))
    call("nfai_hip_gemv_qkv_rope", mgr.handle, bq.handle, bk.handle, bv.handle, qt, px.handle, pg.handle, 1e-5, pf.handle, D,
         pq.handle, kc.handle, vc.handle, H, Hkv, D, pos, F32, K)
    q, k, v = (W.astype(np.float64) @ xn for W in (dq, dk, dv))
    qr = orc.np_oracle.rope(q, freqs.astype(np.float64), D, H, D, pos)
    kr = orc.np_oracle.rope(k, freqs.astype(np.float64), D, Hkv, D, pos)
    check(pq.GetValue(), qr, 2 * stage_tol(dq, xn) + 1e-6 * np.abs(q).max() * (1 + pos), (case, "q"))
    check(kc.GetValue()[pos * Hkv * D:], kr, 2 * stage_tol(dk, xn) + 1e-6 * np.abs(k).max() * (1 + pos), (case, "k"))
    check(vc.GetValue()[pos * Hkv * D:], v, stage_tol(dv, xn), (case, "v"))
    for t in (bg, bu, bq, bk, bv):
        t.free()


@pytest.mark.parametrize("qt,case", ADV, ids=ADV_IDS)
def test_adversarial_blocks_gemm_kq(mgr, qt, case):
    """The dequant-in-LDS prefill GEMM (k_gemm_kq) on the case's blocks against fp64 on the oracle's weights rounded to fp16 (the
    kernel forms each weight in fp32 and rounds it to fp16 on the way into LDS): identical operands, fp32 summation-order noise."""
    from nfai_amd._lib import call
    M, N, K = 32, 64, 1024
    raw = adversarial(qt, case, N, K)
    W16 = dequant(raw, qt, N, K).astype(np.float16).astype(np.float64)
    A = rng(qt + 3).standard_normal((M, K)).astype(np.float16)
    w = upload(mgr, qt, raw, N, K)
    pa, pc = prop(mgr, A, np.float16), prop(mgr, np.zeros(M * N))
    call("nfai_hip_gemm_kq", mgr.handle, pa.handle, w.handle, qt, 0, pc.handle, M, N, K)
    want = A.astype(np.float64) @ W16.T
    bound = 2e-6 * np.sqrt(K / 256.0) * (np.abs(A.astype(np.float64)) @ np.abs(W16).T)
    check(pc.GetValue().reshape(M, N), want, bound, (case, "gemm_kq"))
    w.free()


def test_adversarial_blocks_mixed_qkv_in_the_model(mgr):
    """q, k in adversarial Q4_K and v in adversarial Q6_K blocks: the model's mixed q|k|v launch (one launch, two fragment layouts)
    against OracleLlama on the dequantised weights, graph and unfused."""
    from nfai_amd.llama_model import LlamaModel, QuantTensor
    dims = synth.TINY_D128
    w = synth.make_weights(dims, seed=71, std=0.05)
    wq, wref = {}, {}
    for i, (name, a) in enumerate(w.items()):
        if a.ndim == 1:
            wq[name] = wref[name] = a
            continue
        qt = Q6_K if name.endswith(("attn_v.weight", "ffn_down.weight")) or name.startswith(("token_embd", "output.")) else Q4_K
        N, K = a.shape
        if name.endswith(("attn_q.weight", "attn_k.weight")):
            raw = adversarial(Q4_K, Q4K_CASES[i % len(Q4K_CASES)] if "attn_q" in name else "scales_ff", N, K, i)
        elif name.endswith("attn_v.weight"):
            raw = adversarial(Q6_K, Q6K_CASES[i % len(Q6K_CASES)], N, K, i)
        else:
            raw = quantize(a.astype(np.float32), qt)[0]
        wq[name] = QuantTensor(raw, qt, a.shape)
        wref[name] = dequant(raw, qt, N, K)
    dd = dict(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, eps=1e-5, rope_dims=dims.D, rope_base=500000.0)
    m = LlamaModel(mgr, synth.make_metadata(dims), wq, 24, dims=dd)
    mu = LlamaModel(mgr, synth.make_metadata(dims), wq, 24, dims=dd, unfused=True)
    ref = orc.OracleLlama(orc.LlamaDesc(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, C=24), wref)
    for i, t in enumerate(synth.make_tokens(dims, 12, seed=5)):
        lg, am = m.Step(int(t))
        lu, _ = mu.Step(int(t))
        want = ref.step(int(t))
        scale = max(1.0, float(np.abs(want).max()))
        assert np.abs(lg - want).max() <= 5e-4 * scale, (i, np.abs(lg - want).max())
        assert np.abs(lu - want).max() <= 5e-4 * scale, i
        assert am == orc.argmax(want)
    m.Dispose()
    mu.Dispose()


# ---- 3c: the prefill's fp16 widening, element by element ------------------------------------------------------------------------

LAYER_MATS = ["attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down"]  # the shadow's order per layer


def read_shadow(mgr, m):
    from nfai_amd import _lib
    from nfai_amd.hip import DeviceBuffer
    lib = _lib.load()
    lib.nfai_hip_debug_prefill_shadow.argtypes = [_lib.H, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.nfai_hip_debug_prefill_shadow.restype = C.c_int32
    p, n = C.c_void_p(), C.c_uint64()
    assert lib.nfai_hip_debug_prefill_shadow(m.handle, C.byref(p), C.byref(n)) == 0
    assert p.value and n.value
    buf = DeviceBuffer(mgr, n.value, wrap_ptr=p.value)
    host = np.empty(n.value, np.uint8)
    _lib.call("nfai_hip_buf_download", mgr.handle, buf.handle, 0, host.ctypes.data_as(C.c_void_p), n.value)
    buf.free()
    return host


def mix_type(mix, name, dims):
    if mix == "q8_0":
        return Q8_0
    if mix == "q5_k_m":
        return synth.q5_k_m_type(name, dims)
    return Q6_K if name.endswith(("attn_v.weight", "ffn_down.weight")) or name.startswith(("token_embd", "output.")) else Q4_K


BIG = synth.LlamaDims("one-3b-block", 3072, 1, 24, 8, 128, 8192, 256, True)


@pytest.mark.parametrize("mix,dims", [("q4_k_m", synth.TINY_D128), ("q5_k_m", synth.TINY_D128), ("q8_0", synth.TINY_D128),
                                      ("q4_k_m", BIG)], ids=["q4_k_m", "q5_k_m", "q8_0", "q4_k_m-3b-widths"])
def test_prefill_widening_matches_the_oracle_bit_for_bit(mgr, monkeypatch, mix, dims):
    """One Prefill keeps every block's fp16 copy (NFAI_PREFILL_WIDE_ALL=1); every element of every copy must equal
    float16(oracle dequant) exactly: both sides form d * sc, then * q, then - dmin * m in fp32 (-ffp-contract=off) and round once.
    On the TINY models block 0's attn_q / ffn_gate (Q4_K, Q5_K) and attn_v / ffn_down (Q6_K) hold the adversarial cases, one per
    16-row tile, so a field read from a neighbouring row or sub-block shows up."""
    from nfai_amd.llama_model import LlamaModel, QuantTensor
    monkeypatch.setenv("NFAI_PREFILL_WIDE_ALL", "1")
    w = synth.make_weights(dims, seed=73, std=0.05)
    wq, deq = {}, {}
    for name, a in w.items():
        if a.ndim == 1:
            wq[name] = a
            continue
        qt = mix_type(mix, name, dims)
        N, K = a.shape
        raw = quantize(a.astype(np.float32), qt)[0] if dims is BIG or not name.startswith("blk.0.") else None
        if raw is None:
            cases = Q4K_CASES if qt == Q4_K else Q6K_CASES if qt == Q6_K else []
            if cases and name.endswith(("attn_q.weight", "ffn_gate.weight", "attn_v.weight", "ffn_down.weight")):
                per_tile = [adversarial(qt, cases[t % len(cases)], 16, K, t) for t in range(N // 16)]
                raw = np.concatenate(per_tile)
            else:
                raw = quantize(a.astype(np.float32), qt)[0]
        wq[name] = QuantTensor(raw, qt, a.shape)
        if name.startswith("blk."):
            deq[name] = dequant(raw, qt, N, K)
    dd = dict(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, eps=1e-5, rope_dims=dims.D, rope_base=500000.0)
    m = LlamaModel(mgr, synth.make_metadata(dims), wq, 32, dims=dd, max_batch=16)
    lg = m.Prefill(synth.make_tokens(dims, 16, seed=3))
    assert np.isfinite(lg).all()
    host = read_shadow(mgr, m)
    m.Dispose()
    slot = host.size // dims.L
    assert slot * dims.L == host.size
    for li in range(dims.L):
        off = li * slot
        for mat in LAYER_MATS:
            Wd = deq[f"blk.{li}.{mat}.weight"]
            n = Wd.size * 2
            got = host[off:off + n].view(np.float16).reshape(Wd.shape)
            want = Wd.astype(np.float16)
            same = (got.view(np.uint16) == want.view(np.uint16))
            assert same.all(), (mix, li, mat, int((~same).sum()), np.argwhere(~same)[:4].tolist())
            off += (n + 255) // 256 * 256
