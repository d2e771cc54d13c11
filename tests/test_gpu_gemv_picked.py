"""The fp16 / fp32 decode GEMV in every form its pickers launch on the 256 CUs of an MI355X, through the public op entries, every
output element against float64.

launch_gemv is two kernels (k_gemv, k_gemv_sk) behind two shape pickers; tests/gemv_cases.py names, for each of the 246 classes
(kernel, w_type, mode, norm, UPW | CH, U | RW, guard) they reach below 128 MB of weights, the smallest shapes that reach it and
still exercise its edges (a partial last unit group, waves without a group, a partial last workgroup of the split-K form, every wave
count, ragged K), and tests/test_gemv_picked.py proves on the CPU that the table is exactly what the planner returns.  Here every
case drains nfai_hip_debug_gemv_last, makes ONE call and asserts exactly one descriptor whose class, threads per workgroup and grid
are the ones the case names: nothing in this file restates the picker.

  entries     PLAIN: nfai_hip_gemv; PLAIN with RMSNorm and / or the fused ArgMax: nfai_hip_lmhead_argmax; RESIDUAL:
              nfai_hip_gemv_fused (gamma or none); gate|up: nfai_hip_gemv_gateup_silu; q|k|v: nfai_hip_gemv_qkv_rope (both take
              gamma or none, so every class is reachable from the ABI)
  XCD shares  pinned uniform on the context (nfai_hip_debug_xcd_shares), so no launch deals rows by share: xd = 0
  values      W = 0.02 N(0, 1) in the weight type, x = N(0, 1), gamma = 1 + 0.1 N(0, 1), residual = N(0, 1)
  reference   float64 NumPy on the same fp16 / fp32 operands; RMSNorm, rotation, SiLU * up and the residual in float64
  bars        gemv_tol of tests/test_gpu_ops.py (4e-7 sqrt(K / 64) sum |w| |x| + 1e-7 per output, on the normed x), propagated in
              float64: residual + one fp32 ulp of the result; gate|up |silu(g)| tol_up + 1.1 |up| tol_gate + one ulp; q|k|v
              tol_0 + tol_1 for both rows of a rotated pair + 2e-6 pos / 8 for the device's cos / sin (test_gemv_qkv_rope_kvwrite),
              fp16 cache rows + 2e-3; fused ArgMax equal to the float64 argmax, whose top two lie more than twice the bar apart
              (asserted from the reference alone).  A dropped K slice, wave or row is ~ sum |w| |x| / sqrt(waves), six orders
              above these bars.
  sentinels   8 elements behind every output come back bit-unchanged; the q|k|v caches start as a sentinel and only row pos of
              KV_CAP changes; every compared element is finite

test_model_launches_are_tested_forms ties the first launch of a token (begin = 1, not reachable at op level) to its tested sibling:
in eager decode of the tiny models every recorded class is in the table, and the begin descriptors are the planner's q|k|v
descriptor of that shape with only the begin word differing.
"""
import ctypes as C

import numpy as np
import pytest

import gemv_cases as gc

pytestmark = pytest.mark.gpu

SENT = np.float32(-12345.678)
KV_SENT = 7.0


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd import _lib
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    lib = _lib.load()
    lib.nfai_hip_debug_xcd_shares.argtypes = [_lib.H, C.POINTER(C.c_uint16)]
    lib.nfai_hip_debug_xcd_shares.restype = C.c_int32
    assert lib.nfai_hip_debug_xcd_shares(m.handle, (C.c_uint16 * 8)(*([40] * 8))) == 0     # uniform: the plain dealing
    m.plain_w = {}      # (w_type, K) -> the uploaded rows of gemv_cases.weights, shared by the PLAIN / RESIDUAL cases of that key
    yield m
    for b in m.plain_w.values():
        b.free()
    m.Dispose()


def gemv_last():
    """The descriptors (16 words each) of the fp16 / fp32 launch_gemv calls since the last call, oldest first."""
    from nfai_amd import _lib
    lib = _lib.load()
    lib.nfai_hip_debug_gemv_last.argtypes = [C.POINTER(C.c_uint32), C.c_uint32]
    lib.nfai_hip_debug_gemv_last.restype = C.c_uint32
    buf = (C.c_uint32 * (16 * 256))()
    n = lib.nfai_hip_debug_gemv_last(buf, 256)
    return [tuple(buf[16 * i:16 * i + 16]) for i in range(n)]


def test_device_has_256_cus(mgr):
    assert mgr.info.compute_units == gc.N_CU, "the case table is built for 256 CUs"


def _plain_weights(mgr, c):
    key = (c.wt, c.K)
    if key not in mgr.plain_w:
        for b in mgr.plain_w.values():          # one table at a time on the device
            b.free()
        mgr.plain_w.clear()
        W = gc.weights(c.wt, c.K)
        mgr.plain_w[key] = mgr.UploadWeight(c.wt, W, W.shape[0], c.K)
    return mgr.plain_w[key]


def _check(name, got, want, bar):
    assert np.isfinite(got).all(), (name, np.flatnonzero(~np.isfinite(got))[:8])
    err = np.abs(got.astype(np.float64) - want)
    i = int(np.argmax(err / bar))
    print(f"  {name}: max err/bar = {err[i] / bar[i]:.3f} (err {err[i]:.3e}, bar {bar[i]:.3e}) at {i}")
    assert (err <= bar).all(), (name, i, float(err[i]), float(bar[i]), int((err > bar).sum()))


@pytest.mark.parametrize("c", gc.CASES, ids=gc.case_id)
def test_gemv_picked(mgr, c):
    from nfai_amd import _lib
    from nfai_amd._lib import call
    from nfai_amd.hip import ShaderProperty
    W, x, g, res = gc.inputs(c)
    want, bar = gc.reference(c, W, x, g, res)
    mine = []

    def prop(n, dt=np.float32, value=None):
        p = ShaderProperty(mgr, n, dt)
        mine.append(p)
        if value is not None:
            p.SetValue(value)
        return p

    try:
        px, pg = prop(c.K, value=x), (prop(c.K, value=g) if c.norm else None)
        gh = pg.handle if pg else 0
        if c.mode in (gc.PLAIN, gc.RESIDUAL):
            pw = _plain_weights(mgr, c)
            py = prop(c.NU + gc.GUARD, value=np.full(c.NU + gc.GUARD, SENT))
            if c.mode == gc.RESIDUAL:
                pr = prop(c.NU, value=res)
                launch = lambda: call("nfai_hip_gemv_fused", mgr.handle, pw.handle, c.wt, px.handle, gh, gc.EPS, pr.handle, py.handle, c.NU, c.K)
            elif c.norm or c.argmax:
                pi = prop(1, np.uint32, value=np.array([0xFFFFFFFF], np.uint32))
                launch = lambda: call("nfai_hip_lmhead_argmax", mgr.handle, pw.handle, c.wt, px.handle, gh, gc.EPS, py.handle, pi.handle, c.NU, c.K)
            else:
                launch = lambda: call("nfai_hip_gemv", mgr.handle, pw.handle, c.wt, px.handle, py.handle, 0, c.NU, c.K)
        elif c.mode == gc.GATEUP:
            wg, wu = mgr.UploadWeight(c.wt, W[:c.NU], c.NU, c.K), mgr.UploadWeight(c.wt, W[c.NU:], c.NU, c.K)
            mine += [wg, wu]
            py = prop(c.NU + gc.GUARD, value=np.full(c.NU + gc.GUARD, SENT))
            launch = lambda: call("nfai_hip_gemv_gateup_silu", mgr.handle, wg.handle, wu.handle, c.wt, px.handle, gh, gc.EPS, py.handle, c.NU, c.K)
        else:
            H, Hkv, D, kv16, pos = gc.qkv_shape(c)
            nq, nk = H * D, Hkv * D
            ws = [mgr.UploadWeight(c.wt, w, w.shape[0], c.K) for w in (W[:nq], W[nq:nq + nk], W[nq + nk:])]
            mine += ws
            dt = np.float16 if kv16 else np.float32
            pf = prop(D // 2, value=gc.rope_freqs(D))
            py = prop(nq + gc.GUARD, value=np.full(nq + gc.GUARD, SENT))
            pk, pv = (prop(gc.KV_CAP * nk, dt, value=np.full(gc.KV_CAP * nk, KV_SENT, dt)) for _ in range(2))
            launch = lambda: call("nfai_hip_gemv_qkv_rope", mgr.handle, ws[0].handle, ws[1].handle, ws[2].handle, c.wt, px.handle, gh, gc.EPS,
                                  pf.handle, D, py.handle, pk.handle, pv.handle, H, Hkv, D, pos, _lib.F16 if kv16 else _lib.F32, c.K)

        gemv_last()
        launch()
        out = py.GetValue()
        ran = gemv_last()
        assert len(ran) == 1, ran
        d = ran[0]
        assert gc.desc_cls(d) == gc.cls(c), d
        assert (d[9], d[10], d[12], d[13], d[14]) == (c.threads, c.grid, c.NU, c.K, c.argmax), d
        assert (d[4], d[5], d[15]) == (0, 0, 0), d                                    # no begin, no dealing by share, no prefetch-only launch

        n_y = out.size - gc.GUARD
        assert np.all(out[n_y:].view(np.uint32) == SENT.view(np.uint32)), "an element past the last output was stored"
        print()
        if c.mode != gc.QKV:
            _check("y", out[:n_y], want, bar)
            if c.mode == gc.PLAIN and (c.norm or c.argmax):
                idx, gap, b = gc.argmax_gap(want, bar)
                assert gap > 2 * b, ("the reference's top two are too close for this seed", gap, b)
                assert int(pi.GetValue()[0]) == idx, (int(pi.GetValue()[0]), idx)
        else:
            _check("q", out[:nq], want[:nq], bar[:nq])
            extra = 2e-3 if kv16 else 0.0
            for name, p, sl in (("k", pk, slice(nq, nq + nk)), ("v", pv, slice(nq + nk, nq + 2 * nk))):
                rows = p.GetValue().reshape(gc.KV_CAP, nk)
                _check(f"{name} row {pos}", rows[pos].astype(np.float32), want[sl], bar[sl] + extra)
                assert (np.delete(rows, pos, 0) == KV_SENT).all(), f"{name}: a cache row other than {pos} was written"
    finally:
        for p in mine:
            (p.buffer if hasattr(p, "buffer") else p).free()


@pytest.mark.parametrize("name", ["TINY", "TINY_D128"])
def test_model_launches_are_tested_forms(mgr, name):
    """Two eager decode steps of an fp16 tiny model: every class the model's launches take is a class of the table, and the first
    launch of each token (begin = 1) is the planner's q|k|v descriptor of that shape with only the begin word differing."""
    from nfai_amd import synth
    from nfai_amd.llama_model import LlamaModel
    dims = getattr(synth, name)
    m = LlamaModel(mgr, synth.make_metadata(dims), synth.make_weights(dims, seed=31, std=0.05), 16, graph=False)
    try:
        gemv_last()
        for t in synth.make_tokens(dims, 2, seed=5):
            m.Step(int(t))
        ran = gemv_last()
    finally:
        m.Dispose()
    named = {gc.cls(c) for c in gc.CASES}
    first = [d for d in ran if d[4] == 1]
    rest = [d for d in ran if d[4] == 0]
    assert len(first) == 2 and len(rest) >= 2 * dims.L, (len(first), len(rest))     # one begin launch per token; the other blocks' launches and the lm_head
    for d in rest:
        assert gc.desc_cls(d) in named, d
    plan = gc.load_plan()
    for d in first:
        sib = plan(gc.F16, gc.QKV, dims.H * dims.D, dims.Hkv * dims.D, dims.Hkv * dims.D, dims.E, gc.N_CU, 1, 0)
        assert sib is not None and gc.desc_cls(sib) in named, sib
        assert d[:4] + (0,) + d[5:] == sib and d[4] == 1, (d, sib)
