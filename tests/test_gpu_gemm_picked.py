"""The prefill GEMM in the configurations gemm_pick chooses by itself (variant = 0), at op level, every element against float64.

test_gpu_ops.py asks for tile configurations by number; several of the picker's own choices have no number (the 64-row tiles of
prompts of <= 64 rows, the K-split launch shapes with batch > 1) and the others were reached at 512 / 200 / 128 rows only.  Here
each case names the configuration it is meant to reach and proves through nfai_hip_debug_gemm_last — the launch's own template
parameters, recorded by gemm_launch / gemm_launch_glds — that it did; nothing in this file restates the picker.  The shapes are the
smallest that reach each branch on the 256 CUs of an MI355X, with K kept tiny (the picker looks at M and N): K = 64 is ONE K tile,
fewer than any LDS ring has stages (the prologue and the refills repeat tile KT - 1), K = 128 one tile of the BK = 128 forms,
192 and 320 no multiple of 128, and 2048 / 3072 a real depth at one shape per configuration family.

  reference   A.astype(f64) @ W.astype(f64).T (+ R; up * silu(gate)) on the same fp16 operands
  tolerance   fp32 epilogue: 2e-6 * sqrt(K) * mean|A| mean|W| K + 1e-5; fp16 / SiLU epilogue: 1e-3 * max|want| + 1e-4
              (test_gpu_ops.py: test_gemm_f16_variants, test_gemm_f16_fp16_epilogue, test_gemm_f16_silu_up_epilogue)
  every row and column of every batch is compared; C starts as a sentinel pattern, so an element nobody stored fails too
  GUARD rows of sentinel behind the last row of C must come back bit-unchanged (a store of a row past M lands there)

The op-level entries set ldc = N, so C has no column outside the product: there is no N-side guard to assert here.  The
register-staged fallback for a segment end off the 128 grid is reached with N % 128 == 64 (the entry's one segment ends at N); a
q | k | v boundary inside a tile needs three weight tensors, which only the model passes (tests/test_gpu_prefill_rows.py).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 4                     # sentinel rows behind C
SENT32, SENT16 = np.float32(-12345.678), np.float16(-1234.0)

# (BM, BN, WM, WN, BK, stages, weight-ring stages, KS, pipelined, LDS-staged): the first ten words of a descriptor
M64 = (64, 64, 4, 1, 64, 4, 4, 1, 0, 1)          # prompts of <= 64 rows
W256 = (256, 128, 4, 2, 64, 3, 3, 1, 1, 1)       # wide N, even number of 128-row blocks; the four K quarters of Wdown
W128 = (128, 128, 2, 2, 64, 2, 2, 1, 0, 1)       # wide N, odd number of 128-row blocks
N48_BK128 = (128, 48, 4, 1, 128, 3, 3, 2, 0, 1)  # narrow N, two wave groups: BK = 128 where K % 128 == 0, else four stages of 64
N48_BK64 = (128, 48, 4, 1, 64, 4, 4, 2, 0, 1)
N80_BK128 = (128, 80, 4, 1, 128, 3, 3, 2, 1, 1)
N80_BK64 = (128, 80, 4, 1, 64, 4, 4, 2, 0, 1)
N96 = (128, 96, 4, 1, 64, 4, 4, 2, 0, 1)
N64_BK128 = (128, 64, 4, 1, 128, 3, 3, 2, 0, 1)
N64_BK64 = (128, 64, 4, 1, 64, 4, 4, 2, 0, 1)
N64_3 = (128, 64, 4, 1, 64, 3, 3, 1, 0, 1)       # SiLU below the wide thresholds; batch > 1 at 65 .. 128 rows (the short K split)
REG = (128, 64, 4, 1, 64, 3, 3, 1, 0, 0)         # register-staged: a segment end that is no multiple of 128
NAMES = {M64: "64x64", W256: "256x128-pipe", W128: "128x128", N48_BK128: "128x48-bk128", N48_BK64: "128x48-bk64", N80_BK128: "128x80-bk128",
         N80_BK64: "128x80-bk64", N96: "128x96", N64_BK128: "128x64-bk128", N64_BK64: "128x64-bk64", N64_3: "128x64-glds3", REG: "128x64-reg"}
EPI = {"f32": 0, "f32r": 0, "f16": 1, "silu": 2}
KS4 = [64, 128, 192, 320]


def _cases():
    out = []

    def add(cfg, epi, M, N, K, batch=1, b_div=1):
        out.append(pytest.param(cfg, epi, M, N, K, batch, b_div, id=f"{NAMES[cfg]}-{epi}-M{M}-N{N}-K{K}" + (f"-b{batch}" if batch > 1 else "")))

    # 64-row tiles: every row count around the 16-row wave slices, every epilogue (SiLU: N = 2 F = 192), every K
    for i, M in enumerate([1, 15, 16, 17, 33, 63, 64]):
        for j, epi in enumerate(["f32", "f32r", "f16", "silu"]):
            add(M64, epi, M, 192 if epi == "silu" else 256, KS4[(i + j) % 4])
    add(M64, "f32r", 33, 256, 3072)
    # ... with batch > 1: the launch shape of the short K split (K / ks >= 512 there)
    for M, b, epi, K in [(1, 2, "f32", 64), (17, 3, "f32r", 128), (64, 4, "f32", 192), (16, 2, "f16", 320), (63, 4, "f16", 64), (33, 3, "f32", 2048)]:
        add(M64, epi, M, 256, K, b)
    # 256 x 128: an even number of 128-row blocks and ceil(M / 256) * N / 128 >= 192
    for i, (M, N) in enumerate([(129, 24576), (255, 24576), (256, 24576), (385, 12288), (500, 12288), (512, 12288)]):
        for j, epi in enumerate(["f32r" if i % 2 == 0 else "f32", "f16", "silu"]):
            add(W256, epi, M, N, KS4[(i + j) % 4])
    # ... with batch > 1 (the four K quarters of Wdown at >= 256 rows; 2048 = K / 4 of F = 8192)
    for i, (M, b) in enumerate([(256, 4), (500, 4), (512, 2)]):
        for j, epi in enumerate(["f32", "f16"]):
            add(W256, epi, M, 256, KS4[(2 * i + j) % 4], b)
    add(W256, "f32", 256, 256, 2048, 4)
    # 128 x 128: an odd number of 128-row blocks and ceil(M / 128) * N / 128 >= 384
    for i, (M, N) in enumerate([(65, 49152), (127, 49152), (128, 49152), (384, 16384)]):
        for j, epi in enumerate(["f32r", "f16", "silu"]):
            add(W128, epi, M, N, KS4[(i + j) % 4])
    # narrow N, tile width 48 (N = 384: one round at either width, fewer operand bytes) and 64 (N = 256)
    for N, bk128, bk64 in [(384, N48_BK128, N48_BK64), (256, N64_BK128, N64_BK64)]:
        for i, M in enumerate([65, 127, 128, 129, 200]):
            add(bk128, ["f32r", "f16"][i % 2], M, N, 128)
            add(bk64, ["f16", "f32", "f32r"][i % 3], M, N, [64, 192, 320][i % 3])
    add(N48_BK128, "f32r", 200, 384, 3072)
    # width 80: 64-wide tiles need a second round of workgroups, 80-wide ones fit one (tm * N / 64 > 256 >= tm * N / 80)
    for i, (M, N) in enumerate([(512, 5120), (200, 10240), (128, 20480), (65, 20480)]):
        add(N80_BK128, ["f32r", "f16"][i % 2], M, N, 128)
        add(N80_BK64, ["f16", "f32", "f32r"][i % 3], M, N, [64, 192, 320][i % 3])
    # width 96 (one form)
    for i, (M, N, K) in enumerate([(512, 6144, 64), (512, 6144, 128), (129, 12288, 192), (200, 12288, 128), (127, 24576, 320), (385, 6144, 64)]):
        add(N96, ["f32r", "f16", "f32"][i % 3], M, N, K)
    # 128 x 64, three stages: SiLU with a small F; batch > 1 at 65 .. 128 rows
    for i, M in enumerate([65, 127, 128, 129, 200]):
        add(N64_3, "silu", M, 192, KS4[i % 4])
    add(N64_3, "silu", 200, 1024, 3072)
    for M, b, epi, N, K in [(100, 2, "f32", 128, 64), (100, 2, "f16", 256, 192), (128, 3, "f32r", 128, 128), (65, 4, "f32", 128, 320)]:
        add(N64_3, epi, M, N, K, b)
    # register-staged fallback: N % 128 == 64 (non-SiLU), at every row count, the 64-row ones included
    for M, epi, K, b in [(1, "f32r", 64, 1), (64, "f16", 128, 1), (65, "f32", 192, 1), (200, "f32r", 320, 1), (129, "f16", 64, 1), (100, "f32", 128, 2)]:
        add(REG, epi, M, 192, K, b)
    # a weight matrix shared by the batches of a group (b_div), as the attention GEMMs pass kv heads
    add(N64_3, "f32", 100, 128, 64, 4, 2)
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


def gemm_last():
    """The descriptors (16 words each) of the prefill GEMM launches since the last call, oldest first."""
    from nfai_amd import _lib
    lib = _lib.load()
    lib.nfai_hip_debug_gemm_last.argtypes = [C.POINTER(C.c_uint32), C.c_uint32]
    lib.nfai_hip_debug_gemm_last.restype = C.c_uint32
    buf = (C.c_uint32 * (16 * 256))()
    n = lib.nfai_hip_debug_gemm_last(buf, 256)
    return [tuple(buf[16 * i:16 * i + 16]) for i in range(n)]


def _silu64(x):
    return x / (1.0 + np.exp(-x))


def test_cases_cover_the_table():
    """Every configuration of the default picker with every epilogue it takes there, each K class, each row count of its tile height."""
    seen = {}
    for p in CASES:
        cfg, epi, M, N, K, batch, _ = p.values
        seen.setdefault(cfg, []).append((epi, M, K, batch))
    assert set(seen) == set(NAMES)
    assert len(CASES) <= 160
    rows = {M64: {1, 15, 16, 17, 33, 63, 64}, W256: {129, 255, 256, 385, 500, 512}, N48_BK128: {65, 127, 128, 129, 200},
            N48_BK64: {65, 127, 128, 129, 200}, N64_BK128: {65, 127, 128, 129, 200}, N64_BK64: {65, 127, 128, 129, 200}, N64_3: {65, 127, 128, 129, 200}}
    for cfg, want in rows.items():
        assert want <= {M for _, M, _, _ in seen[cfg]}, NAMES[cfg]
    for cfg in (M64, W256, W128):
        assert {"f32r", "f16", "silu"} <= {e for e, _, _, _ in seen[cfg]}, NAMES[cfg]
        assert {64, 128, 192, 320} <= {K for _, _, K, _ in seen[cfg]}, NAMES[cfg]
    for cfg in (M64, W256, N64_3, REG):
        assert any(b > 1 for _, _, _, b in seen[cfg]), NAMES[cfg]


@pytest.mark.parametrize("cfg,epi,M,N,K,batch,b_div", CASES)
def test_gemm_f16_picked(mgr, cfg, epi, M, N, K, batch, b_div):
    from nfai_amd._lib import call
    from nfai_amd.hip import ShaderProperty
    r = np.random.Generator(np.random.PCG64(1000 * M + N + K + 7 * batch))
    silu = epi == "silu"
    nw = N // 2 if silu else N                                                    # output columns
    A = r.standard_normal((batch, M, K), dtype=np.float32).astype(np.float16)
    W = (0.05 * r.standard_normal((batch // b_div, N, K), dtype=np.float32)).astype(np.float16)   # SiLU: rows [0, F) gate, [F, 2F) up
    R = r.standard_normal((batch, M, N), dtype=np.float32) if epi == "f32r" else None
    cdt, sent = (np.float32, SENT32) if EPI[epi] == 0 else (np.float16, SENT16)
    pa = ShaderProperty(mgr, A.size, np.float16)
    pa.SetValue(A.ravel())
    pc = ShaderProperty(mgr, (batch * M + GUARD) * nw, cdt)
    pc.SetValue(np.full((batch * M + GUARD) * nw, sent, cdt))
    pr = None
    if R is not None:
        pr = ShaderProperty(mgr, R.size, np.float32)
        pr.SetValue(R.ravel())
    if silu:
        pw, pw1 = ShaderProperty(mgr, nw * K, np.float16), ShaderProperty(mgr, nw * K, np.float16)
        pw.SetValue(W[0, :nw].ravel())
        pw1.SetValue(W[0, nw:].ravel())
    else:
        pw, pw1 = ShaderProperty(mgr, W.size, np.float16), None
        pw.SetValue(W.ravel())
    gemm_last()
    if batch == 1 and epi in ("f32", "f32r"):
        call("nfai_hip_gemm_f16", mgr.handle, pa.handle, pw.handle, pr.handle if pr else 0, pc.handle, M, N, K, 0)
    else:
        call("nfai_hip_gemm_f16_ex", mgr.handle, pa.handle, pw.handle, pw1.handle if pw1 else 0, pr.handle if pr else 0, pc.handle, M, N, K, 0,
             EPI[epi], batch, b_div, 0, 0)
    out = pc.GetValue().reshape(batch * M + GUARD, nw)
    ran = gemm_last()
    assert len(ran) == 1, ran
    assert ran[0] == cfg + (EPI[epi], batch, 1, M, N, K), (NAMES.get(ran[0][:10], ran[0][:10]), ran[0])

    uint = np.uint32 if cdt == np.float32 else np.uint16
    assert np.all(out[batch * M:].view(uint) == np.array(sent).view(uint)), "a row past M was stored"
    got = out[:batch * M].reshape(batch, M, nw).astype(np.float64)
    A64, W64 = A.astype(np.float64), W.astype(np.float64)
    want = np.empty((batch, M, nw))
    for b in range(batch):
        w = W64[b // b_div]
        if silu:
            want[b] = (A64[b] @ w[nw:].T) * _silu64(A64[b] @ w[:nw].T)
        else:
            want[b] = A64[b] @ w.T + (R[b].astype(np.float64) if R is not None else 0.0)
    if EPI[epi] == 0:
        tol = 2e-6 * np.sqrt(K) * float(np.abs(A64).mean() * np.abs(W64).mean() * K) + 1e-5
    else:
        tol = 1e-3 * float(np.abs(want).max()) + 1e-4
    err = np.abs(got - want)
    b, row, col = np.unravel_index(int(err.argmax()), err.shape)
    print(f"{NAMES[cfg]} {epi} M={M} N={N} K={K} batch={batch}: max|d| = {err.max():.3e} (bar {tol:.3e}) at batch {b} row {row} col {col}")
    assert err.max() <= tol, (float(err.max()), tol, int(b), int(row), int(col))
