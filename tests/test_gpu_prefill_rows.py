"""Every K / V row the MFMA prefill writes, at prompt lengths on the tile edges, against the oracle's token-by-token fp32 path.

The model-level prefill tests compare the last row's logits and a handful of K / V rows; a wrong row in the middle of a chunk
reaches them only through attention, diluted.  Here two thin TWO-block models run the prefill, so that block 1's K / V row t
witnesses block 0's q, attention, Wo, gate|up and Wdown of row t — and every row is compared:

  thin-f8192    E 256, H 4 / Hkv 2, D 64, F 8192: Wdown takes the short K split (8 slabs + k_sum_slabs) up to 128 rows and the four
                K quarters on 256 x 128 tiles (+ the combine fused into block 1's norm, the plain tail behind block 1) from 256
                rows with an even number of 128-row blocks; gate|up takes 256 x 128 tiles at 512 rows and 128 x 128 at 384;
                q|k|v takes <64, 64, RoPE> up to 64 rows and <128, 64, BK 128, two wave groups, RoPE> above
  thin-h9-d128  H 9 / Hkv 3, D 128: (H + 2 Hkv) D = 1920 columns, a multiple of 80 and of 48: <64, 80, RoPE> and <128, 48, RoPE>

One oracle run over 512 tokens per model serves every prefix (attention is causal).  Per cache type one model is reused over the
prompt lengths in DESCENDING order: after Reset() the rows [n, 512) still hold the previous, longer prompt's values and must be
bit-identical after the call — a store past the chunk's end shows.  Bars: the project's K / V atol 2e-2 and logits 2e-2 *
max(1, max|logit|) with equal argmax; tests/test_prefill_rows_bar.py measures on the CPU that the prefill's legitimate fp16
rounding stays under half of that and one dropped 64-deep K tile or one misplaced RoPE position exceeds five times it.
Which configurations ran is taken from nfai_hip_debug_gemm_last, never re-derived here.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth

pytestmark = pytest.mark.gpu

T = 512
KV_ATOL, LOGIT_BAR = 2e-2, 2e-2
LENGTHS = [512, 500, 385, 384, 257, 256, 255, 129, 128, 127, 65, 64, 63, 17, 16, 2, 1]   # descending: see above
F32, ROPE, SILU = 0, 3, 2
# (BM, BN, WM, WN, BK, stages, weight-ring stages, KS, pipelined, LDS-staged) + (epilogue, batch, K): what must have run per model
M64, M64_80 = (64, 64, 4, 1, 64, 4, 4, 1, 0, 1), (64, 80, 4, 1, 64, 4, 4, 1, 0, 1)
N64_BK128, N48_BK128 = (128, 64, 4, 1, 128, 3, 3, 2, 0, 1), (128, 48, 4, 1, 128, 3, 3, 2, 0, 1)
N64_3, W256, W128 = (128, 64, 4, 1, 64, 3, 3, 1, 0, 1), (256, 128, 4, 2, 64, 3, 3, 1, 1, 1), (128, 128, 2, 2, 64, 2, 2, 1, 0, 1)
FORMS = {
    "thin-f8192": {"q|k|v <= 64 rows": M64 + (ROPE, 1, 256), "q|k|v > 64 rows": N64_BK128 + (ROPE, 1, 256),
                   "Wdown short K split <= 64 rows": M64 + (F32, 8, 1024), "Wdown short K split 65 .. 128 rows": N64_3 + (F32, 8, 1024),
                   "Wdown K quarters": W256 + (F32, 4, 2048), "gate|up 256 x 128": W256 + (SILU, 1, 256), "gate|up 128 x 128": W128 + (SILU, 1, 256)},
    "thin-h9-d128": {"q|k|v <= 64 rows": M64_80 + (ROPE, 1, 256), "q|k|v > 64 rows": N48_BK128 + (ROPE, 1, 256)},
}
MODELS = [synth.THIN_F8192, synth.THIN_H9]


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


def kv_rows(m, layer, is_v, pos, n):
    """[n][Hkv*D] fp32 rows of one block's K or V cache in one synchronising call (fp16 caches widened)."""
    from nfai_amd import _lib
    from nfai_amd._lib import call
    lib = _lib.load()
    lib.nfai_hip_debug_read_kv_rows.argtypes = [_lib.H, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
    lib.nfai_hip_debug_read_kv_rows.restype = C.c_int32
    out = np.empty((n, m.dims["Hkv"] * m.dims["D"]), np.float32)
    call("nfai_hip_debug_read_kv_rows", m.handle, layer, int(is_v), pos, n, out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """weights, tokens and the oracle's K / V rows [block][512][Hkv*D] and logits [512][V]: computed once, never written again."""
    d = next(x for x in MODELS if x.name == name)
    w = synth.make_weights(d, seed=61, std=0.05)
    toks = synth.make_tokens(d, T, seed=13)
    ref = orc.OracleLlama(orc.LlamaDesc(E=d.E, L=d.L, H=d.H, Hkv=d.Hkv, D=d.D, F=d.F, V=d.V, C=T), w)
    logits = np.stack([ref.step(int(t)) for t in toks])
    K = [ref.kcache(l).copy() for l in range(d.L)]
    V = [ref.vcache(l).copy() for l in range(d.L)]
    ref.close()
    for a in K + V + [logits]:
        a.setflags(write=False)
    return w, toks, K, V, logits


def check_rows(m, d, n, K, V, tag):
    """Every K / V row [0, n) of both blocks within KV_ATOL of the oracle's; returns the largest |d|."""
    worst = 0.0
    for l in range(d.L):
        for is_v, want in ((False, K[l]), (True, V[l])):
            err = np.abs(kv_rows(m, l, is_v, 0, n).astype(np.float64) - want[:n]).max(axis=1)
            worst = max(worst, float(err.max()))
            assert err.max() <= KV_ATOL, (tag, f"block {l} {'V' if is_v else 'K'} row {int(err.argmax())} of {n}", float(err.max()),
                                          f"{int((err > KV_ATOL).sum())} rows over the bar")
    return worst


def check_logits(got, want, tag):
    err, tol = float(np.abs(got - want).max()), LOGIT_BAR * max(1.0, float(np.abs(want).max()))
    assert err <= tol, (tag, err, tol)
    assert int(np.argmax(got)) == orc.argmax(want), tag
    return err / tol


def tail_rows(m, d, n):
    return [kv_rows(m, l, v, n, T - n).view(np.uint32).copy() for l in range(d.L) for v in (False, True)] if n < T else []


@pytest.mark.parametrize("kv16", [False, True], ids=["kv-f32", "kv-f16"])
@pytest.mark.parametrize("dims", MODELS, ids=lambda d: d.name)
def test_prefill_every_row_at_tile_edges(mgr, dims, kv16):
    from nfai_amd.llama_model import LlamaModel
    w, toks, K, V, logits = reference(dims.name)
    m = LlamaModel(mgr, synth.make_metadata(dims), w, T, max_batch=T, kv_f16=kv16)
    seen, worst, worst_lg = set(), 0.0, 0.0
    for n in LENGTHS:
        m.Reset()
        before = tail_rows(m, dims, n)
        gemm_last()
        got = m.Prefill(toks[:n])
        ran = gemm_last()
        assert ran and all(r[13] == n for r in ran), (n, ran)   # one chunk: every GEMM has M = n rows
        seen |= {r[:12] + (r[15],) for r in ran}
        assert m.Pos == n
        worst = max(worst, check_rows(m, dims, n, K, V, f"{n} rows"))
        worst_lg = max(worst_lg, check_logits(got, logits[n - 1], f"{n} rows"))
        for a, b in zip(before, tail_rows(m, dims, n)):
            assert np.array_equal(a, b), f"{n} rows: a K / V row at or past position {n} changed"
    m.Dispose()
    print(f"{dims.name} {'fp16' if kv16 else 'fp32'} cache: K / V max|d| = {worst:.2e} (bar {KV_ATOL:.0e}), logits at {worst_lg:.2f} of their bar")
    missing = {k: v for k, v in FORMS[dims.name].items() if v not in seen}
    assert not missing, (missing, sorted(seen))


@pytest.mark.parametrize("kv16", [False, True], ids=["kv-f32", "kv-f16"])
@pytest.mark.parametrize("dims", MODELS, ids=lambda d: d.name)
def test_prefill_every_row_chunked(mgr, dims, kv16):
    """300 tokens in chunks of 128, 128 and 44: pos0 > 0, and an Spad (320) the last chunk does not fill."""
    from nfai_amd.llama_model import LlamaModel
    w, toks, K, V, logits = reference(dims.name)
    n = 300
    m = LlamaModel(mgr, synth.make_metadata(dims), w, T, max_batch=128, kv_f16=kv16)
    before = tail_rows(m, dims, n)
    gemm_last()
    got = m.Prefill(toks[:n])
    assert sorted({r[13] for r in gemm_last()}) == [44, 128]
    assert m.Pos == n
    worst = check_rows(m, dims, n, K, V, "128 + 128 + 44 rows")
    worst_lg = check_logits(got, logits[n - 1], "128 + 128 + 44 rows")
    print(f"{dims.name} {'fp16' if kv16 else 'fp32'} cache, chunks of 128: K / V max|d| = {worst:.2e} (bar {KV_ATOL:.0e}), logits at {worst_lg:.2f} of their bar")
    for a, b in zip(before, tail_rows(m, dims, n)):
        assert np.array_equal(a, b), f"a K / V row at or past position {n} changed"
    m.Dispose()
