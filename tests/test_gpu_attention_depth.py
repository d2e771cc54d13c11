"""Decode and prompt attention at every head grouping the model accepts and at KV depths up to the 32768-position maximum,
against float64 references with bars sharp enough that one dropped key, slice or tile shows.

A  The model's own decode attention: after a step, the post-RoPE q of the last block (nfai_hip_llama_read 1), every K / V row
   it attended (fp16 caches widened) and its output (read 2) are read back, and softmax(q.k / sqrt(D)) . V is recomputed in
   float64.  Capacity C <= 2048 selects the two-pass body (fused with Wo in k_attn_wo for the kAttnWoShapes head shapes at
   E = H*D), C > 2048 the one-pass body; both hand over {value, tag} granules.  Bar: 3e-5 * max(1, max|V|) (the op-level bar).
B  Op-level needles: one dominant key in the first slice, the last slice or at the final position, and a rising maximum across
   slices, for the ticket form of nfai_hip_attn_decode (two-pass at C = 2048, one-pass at C = 32768); dominant keys and
   trap keys just past each query's causal limit for nfai_hip_attn_prefill at depth.
C  A second chat turn: ingest, greedy steps, ingest again at an unaligned position across 2048, greedy steps, against the oracle.
D  The contract: groupings the fused decode cannot launch are refused at creation; G = 8 decodes up to C = 32768.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth

pytestmark = pytest.mark.gpu

ATTN_BAR = 3e-5          # |d| <= ATTN_BAR * max(1, max|V|): fp32 accumulation over up to 32768 keys
PREFILL_BAR = 2e-2       # logits after an fp16 MFMA prefill: 2e-2 * max(1, max|logit|) (test_gpu_model.py)
MIN_CHUNK, MAX_SPLIT = 32, 32   # kernels_attn.hip: ATTN_MIN_CHUNK, ATTN_NSPLIT_MAX


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def odesc(d, C):
    return orc.LlamaDesc(E=d.E, L=d.L, H=d.H, Hkv=d.Hkv, D=d.D, F=d.F, V=d.V, C=C)


def attn_split(S):
    """attn_split of kernels_attn.hip: (active slices, positions per slice) for S cached positions."""
    ns = min(-(-S // MIN_CHUNK), MAX_SPLIT)
    ch = -(-S // ns)
    return -(-S // ch), ch


def decode_positions(C, D):
    """The sequence lengths S checked at capacity C: one key, one and two slices, 32 full slices of 32 and one more key, the only
    S whose last slice holds one row (993), the S in the upper half of C with the shortest last slice, exactly full slices, a
    slice of several one-pass iterations (STEP = 32 keys at D = 128, 64 at D = 64) and S = C (the last row)."""
    step = (256 // (D // 4)) * 4

    def last(S):
        ns, ch = attn_split(S)
        return S - (ns - 1) * ch

    short = min(range(C // 2, C + 1), key=lambda S: (last(S), -S))
    full = (C - 1) // MAX_SPLIT * MAX_SPLIT   # >= 1024: 32 slices of S / 32 keys
    assert attn_split(full) == (MAX_SPLIT, full // MAX_SPLIT)
    multi = min(C - 1, MAX_SPLIT * step * 3 + 7)
    assert attn_split(993)[0] > 1 and last(993) == 1
    return sorted({S for S in (1, 32, 33, 993, 1024, 1025, short, full, multi, C) if 1 <= S <= C})


def kv_rows(m, layer, is_v, pos, n):
    """[n][Hkv*D] fp32 rows of one block's K or V cache in one synchronising call (test hook nfai_hip_debug_read_kv_rows)."""
    from nfai_amd import _lib
    from nfai_amd._lib import call
    lib = _lib.load()
    lib.nfai_hip_debug_read_kv_rows.argtypes = [_lib.H, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
    lib.nfai_hip_debug_read_kv_rows.restype = C.c_int32
    out = np.empty((n, m.dims["Hkv"] * m.dims["D"]), np.float32)
    call("nfai_hip_debug_read_kv_rows", m.handle, layer, int(is_v), pos, n, out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


class KVMirror:
    """Host copy [Hkv][C][D] of the last block's K and V cache, kept equal to the device by reading back every row a call writes."""

    def __init__(self, m):
        d = m.dims
        self.m, self.layer, self.Hkv, self.D = m, d["L"] - 1, d["Hkv"], d["D"]
        self.K = np.zeros((self.Hkv, m.C, self.D), np.float32)
        self.V = np.zeros((self.Hkv, m.C, self.D), np.float32)

    def pull(self, pos, n):
        for is_v, dst in ((False, self.K), (True, self.V)):
            rows = kv_rows(self.m, self.layer, is_v, pos, n).reshape(n, self.Hkv, self.D)
            dst[:, pos:pos + n] = rows.transpose(1, 0, 2)

    def check(self, S, tag):
        """The last block's attention output of the step just taken (S keys) against float64; returns err / bar."""
        m, H, D = self.m, self.m.dims["H"], self.D
        G = H // self.Hkv
        q = m.Read(1, H * D).astype(np.float64).reshape(self.Hkv, G, D)
        got = m.Read(2, H * D).astype(np.float64).reshape(self.Hkv, G, D)
        want = np.empty_like(got)
        vmax = 0.0
        for h in range(self.Hkv):
            k64, v64 = self.K[h, :S].astype(np.float64), self.V[h, :S].astype(np.float64)
            sc = q[h] @ k64.T / np.sqrt(D)
            p = np.exp(sc - sc.max(axis=1, keepdims=True))
            want[h] = (p / p.sum(axis=1, keepdims=True)) @ v64
            vmax = max(vmax, float(np.abs(v64).max()))
        err, bar = float(np.abs(got - want).max()), ATTN_BAR * max(1.0, vmax)
        assert err <= bar, (tag, S, err, bar)
        return err / bar


# name, H, Hkv, D, E: E = H*D for the head shapes of kAttnWoShapes (k_attn_wo runs at C <= 2048), thin otherwise
HEADS = [("1b", 32, 8, 64, 2048), ("3b", 24, 8, 128, 3072), ("8b", 32, 8, 128, 4096), ("70b", 64, 8, 128, 512),
         ("g8-d64", 32, 4, 64, 512), ("g2", 16, 8, 128, 512), ("g1", 8, 8, 128, 512)]
CAPS = [2048, 2049, 8192, 32768]
# every head shape meets both KV types and both launch modes, and so does every capacity
CASES = [pytest.param(hs, cap, (i + j) % 2 == 1, (i + j // 2) % 2 == 0, id=f"{hs[0]}-C{cap}-{'f16' if (i + j) % 2 else 'f32'}-"
                      f"{'graph' if (i + j // 2) % 2 == 0 else 'eager'}")
         for i, hs in enumerate(HEADS) for j, cap in enumerate(CAPS)]


@functools.lru_cache(maxsize=None)
def _weights(name):
    _, H, Hkv, D, E = next(h for h in HEADS if h[0] == name)
    dims = synth.LlamaDims(f"attn-depth-{name}", E, 2, H, Hkv, D, 512, 1024, True)
    return dims, synth.make_weights(dims, seed=61, std=0.05 * np.sqrt(512.0 / E))


@pytest.mark.parametrize("heads,cap,kv16,graph", CASES)
def test_decode_attention_against_fp64(mgr, heads, cap, kv16, graph):
    """The cache is filled by Ingest (max_batch = 512) up to the deepest S checked; each check sets the position to S - 1 and
    steps, after a step at a distant position so that a form which stopped writing the output cannot pass on a stale one."""
    from nfai_amd.llama_model import LlamaModel
    dims, w = _weights(heads[0])
    pos = decode_positions(cap, dims.D)
    m = LlamaModel(mgr, synth.make_metadata(dims), w, cap, kv_f16=kv16, graph=graph, max_batch=512)
    try:
        toks = synth.make_tokens(dims, cap, seed=cap + dims.H)
        fill = max(pos) - 1
        if fill:
            m.Ingest(toks[:fill])
        mir = KVMirror(m)
        if fill:
            mir.pull(0, fill)
        worst = 0.0
        for S in pos:
            away = S // 2 if S > 2 else S + 40
            m.SetPos(away - 1)
            m.Step(int(toks[away]), want_logits=False)
            mir.pull(away - 1, 1)
            m.SetPos(S - 1)
            m.Step(int(toks[S - 1]), want_logits=False)
            mir.pull(S - 1, 1)
            worst = max(worst, mir.check(S, heads[0]))
        print(f"decode attention {heads[0]} C={cap} kv16={kv16} graph={graph}: worst err / bar = {worst:.3g} over S = {pos}")
    finally:
        m.Dispose()


# ---- B: op-level needles ---------------------------------------------------------------------------------------------------
def _ref_decode(q, K, V, H, Hkv, D, S):
    """float64 softmax(q.k / sqrt(D)) . V over K, V [C][Hkv*D] rows 0..S-1: [H*D]."""
    G = H // Hkv
    out = np.empty((H, D))
    for h in range(H):
        kv = h // G
        k64 = K[:S, kv * D:(kv + 1) * D].astype(np.float64)
        v64 = V[:S, kv * D:(kv + 1) * D].astype(np.float64)
        sc = k64 @ q[h * D:(h + 1) * D].astype(np.float64) / np.sqrt(D)
        p = np.exp(sc - sc.max())
        out[h] = (p / p.sum()) @ v64
    return out.ravel()


def _needle_dir(q, kv, G, D):
    """A key direction with a large positive score for all G query heads of kv head `kv`, scaled to score 1."""
    qs = q.reshape(-1, D)[kv * G:(kv + 1) * G].astype(np.float64)
    k = (qs / np.linalg.norm(qs, axis=1, keepdims=True)).sum(axis=0)
    return k / (qs @ k / np.sqrt(D)).min()


@pytest.mark.parametrize("H,Hkv,D", [(32, 8, 128), (16, 2, 128), (32, 8, 64)], ids=["8b", "g8", "1b"])
@pytest.mark.parametrize("C,S,kv16", [(2048, 2048, False), (2048, 1987, True), (32768, 32768, True), (32768, 31777, False)],
                         ids=["2pass-full-f32", "2pass-ragged-f16", "1pass-full-f16", "1pass-ragged-f32"])
@pytest.mark.parametrize("where", ["first-slice", "last-slice", "final", "rising"])
def test_attn_decode_needles(mgr, H, Hkv, D, C, S, where, kv16):
    """nfai_hip_attn_decode (ticket hand-off; C > 2048: one-pass body).  One key of kv head 0 scores 40 above the rest for all of its
    query heads: those heads' outputs must be its V row; a rising maximum (one key per slice, +1 per slice) makes every merge
    rescale.  Every head against float64 at the op-level bar."""
    from nfai_amd import _lib
    from nfai_amd._lib import call
    from nfai_amd.hip import ShaderProperty
    G = H // Hkv
    r = rng(C + S + H + D + len(where))
    q = r.standard_normal(H * D).astype(np.float32)
    K = (0.3 * r.standard_normal((C, Hkv * D))).astype(np.float32)
    V = r.standard_normal((C, Hkv * D)).astype(np.float32)
    ns, ch = attn_split(S)
    k1 = _needle_dir(q, 0, G, D)
    if where == "rising":
        needles = [(s * ch + (7 * s) % min(ch, S - s * ch), 10.0 + s) for s in range(ns)]
    else:
        t = {"first-slice": min(5, ch - 1), "last-slice": (ns - 1) * ch + (S - (ns - 1) * ch) // 2, "final": S - 1}[where]
        needles = [(t, 40.0)]
    for t, score in needles:
        K[t, :D] = score * k1
    dt = np.float16 if kv16 else np.float32
    K, V = K.astype(dt), V.astype(dt)
    pq, po = ShaderProperty(mgr, H * D), ShaderProperty(mgr, H * D)
    pk, pv = ShaderProperty(mgr, C * Hkv * D, dt), ShaderProperty(mgr, C * Hkv * D, dt)
    pq.SetValue(q); pk.SetValue(K); pv.SetValue(V)
    call("nfai_hip_attn_decode", mgr.handle, pq.handle, pk.handle, pv.handle, po.handle, H, Hkv, D, S, C, _lib.F16 if kv16 else _lib.F32)
    got = po.GetValue().astype(np.float64)
    want = _ref_decode(q, K, V, H, Hkv, D, S)
    bar = ATTN_BAR * max(1.0, float(np.abs(V[:S].astype(np.float32)).max()))
    err = float(np.abs(got - want).max())
    assert err <= bar, (err, bar)
    print(f"decode needles err / bar = {err / bar:.3g}")
    if where != "rising":
        t = needles[0][0]
        onehot = np.tile(V[t, :D].astype(np.float64), G)
        assert np.abs(want[:G * D] - onehot).max() <= 1e-3 * bar    # the data: the needle takes all the weight
        assert np.abs(got[:G * D] - onehot).max() <= bar, np.abs(got[:G * D] - onehot).max()


def attn_prefill_ref(Q, K, V, Hkv, pos0, S, shift=0):
    """float64 causal attention of a prompt chunk: query t (position pos0 + t) sees keys 0..pos0 + t (+ shift: a mask off by
    `shift`, to show that the data would expose it), softmax of q.k / sqrt(D), weighted sum of V.  Q [T][H][D], K / V [Hkv][>=S][D]."""
    T, H, D = Q.shape
    G = H // Hkv
    want = np.zeros((T, H, D))
    q64, k64, v64 = Q.astype(np.float64), K[:, :S].astype(np.float64), V[:, :S].astype(np.float64)
    mask = np.arange(S)[None, :] <= (pos0 + shift + np.arange(T))[:, None]
    for h in range(H):
        sc = q64[:, h] @ k64[h // G].T / np.sqrt(D)          # [T][S]
        sc = np.where(mask, sc, -np.inf)
        p = np.exp(sc - sc.max(axis=1, keepdims=True))
        p /= p.sum(axis=1, keepdims=True)
        want[:, h] = p @ v64[h // G]
    return want


def run_attn_prefill(mgr, Q, K, V, pos0, Spad):
    from nfai_amd._lib import call
    from nfai_amd.hip import ShaderProperty
    T, H, D = Q.shape
    Hkv = K.shape[0]
    Vt = np.ascontiguousarray(V.transpose(0, 2, 1))
    pq, pk = ShaderProperty(mgr, Q.size, np.float16), ShaderProperty(mgr, K.size, np.float16)
    pv, po = ShaderProperty(mgr, Vt.size, np.float16), ShaderProperty(mgr, Q.size, np.float16)
    pq.SetValue(Q.ravel()); pk.SetValue(K.ravel()); pv.SetValue(Vt.ravel())
    call("nfai_hip_attn_prefill", mgr.handle, pq.handle, pk.handle, pv.handle, po.handle, T, H, Hkv, D, Spad, pos0)
    return po.GetValue().reshape(T, H, D).astype(np.float64)


def _prefill_cases():
    out = []
    for T in (1, 63, 64, 65, 512):
        for pos0 in (2047, 2085, 8191 - T, 32768 - T):
            for where in ("tile0", "straddle", "diagonal"):
                heads = [(16, 2, 128)] + ([(32, 8, 64), (24, 8, 128)] if T in (65, 512) and pos0 < 8192 and where == "diagonal" else [])
                out += [pytest.param(H, Hkv, D, T, pos0, where, id=f"{H}-{Hkv}-{D}-T{T}-p{pos0}-{where}") for H, Hkv, D in heads]
    return out


@pytest.mark.parametrize("H,Hkv,D,T,pos0,where", _prefill_cases())
def test_attn_prefill_needles_and_traps(mgr, H, Hkv, D, T, pos0, where):
    """k_attn_prefill at depth (pos0 up to 32768 - T, unaligned, across 2048) with planted keys.  tile0 / straddle: every query
    shares a direction and one key scores ~40 above the rest, in key tile 0 or in the tile that holds pos0.  diagonal: each
    query's own key scores ~40 and the key just past its causal limit is a trap of the same size that must get zero weight, so
    a mask off by one either way is an O(1) error.  Bar of test_attn_prefill_one_launch (fp16 probabilities and output)."""
    r = rng(7000 + T + pos0 + len(where) + H)
    S = pos0 + T
    Spad = (S + 63) // 64 * 64
    G = H // Hkv
    K = np.zeros((Hkv, Spad, D), np.float32)
    V = np.zeros((Hkv, Spad, D), np.float32)
    K[:, :S] = 0.3 * r.standard_normal((Hkv, S, D))
    V[:, :S] = r.standard_normal((Hkv, S, D))
    if where == "diagonal":
        Q = r.standard_normal((T, H, D))
        for kv in range(Hkv):
            for t in range(T):
                k = _needle_dir(Q[t].ravel(), kv, G, D)
                K[kv, pos0 + t] += 40.0 * k                  # query t's own key
                if t + 1 < T:
                    K[kv, pos0 + t + 1] += 40.0 * k          # ... and the trap just past its limit
    else:
        U = r.standard_normal((Hkv, D))
        Q = 0.5 * r.standard_normal((T, H, D)) + np.repeat(U, G, axis=0)[None]
        t = 3 if where == "tile0" else (pos0 // 64) * 64 + (pos0 % 64) // 2
        for kv in range(Hkv):
            qs = Q[:, kv * G:(kv + 1) * G].reshape(-1, D)
            u = U[kv] / np.linalg.norm(U[kv])
            K[kv, t] = 40.0 * u / (qs @ u / np.sqrt(D)).min()
    Q, K, V = Q.astype(np.float16), K.astype(np.float16), V.astype(np.float16)
    got = run_attn_prefill(mgr, Q, K, V, pos0, Spad)
    want = attn_prefill_ref(Q, K, V, Hkv, pos0, S)
    tol = 2e-3 * float(np.abs(V[:, :S].astype(np.float64)).max()) + 2e-3 * np.abs(want).max()
    err = float(np.abs(got - want).max())
    assert err <= tol, (err, tol)
    print(f"prefill needles err / bar = {err / tol:.3g}")
    if where == "diagonal" and T > 1:  # the data: a mask one key too short or too long would be an O(1) error
        for shift in (-1, 1):  # head 0 (kv head 0); the last query has no trap
            sub = slice(0, T - 1) if shift > 0 else slice(0, T)
            off = attn_prefill_ref(Q[sub, :1], K[:1], V[:1], 1, pos0, S, shift)
            assert np.abs(off - want[sub, :1]).max() > 20 * tol, shift


# ---- C: a second chat turn against the oracle -------------------------------------------------------------------------------
TURN_DIMS = synth.LlamaDims("attn-depth-8b-thin", 512, 2, 32, 8, 128, 512, 1024, True)
TURN_C, TURN_ROWS = 2700, (511, 512, 1499, 1500, 1506, 1512, 1513, 2024, 2025, 2047, 2048, 2512, 2513)


@functools.lru_cache(maxsize=None)
def _second_turn_oracle():
    """The oracle's side of test_second_turn_ingest_after_decode, computed once for both KV types: a 1500-token first turn, 13
    greedy steps (the oracle's own argmax fed back), a 1000-token second turn, 8 greedy steps.  Returns the token fed at every
    step, the logits of every step, and the K / V rows TURN_ROWS of both blocks."""
    w = synth.make_weights(TURN_DIMS, seed=67, std=0.05)
    ref = orc.OracleLlama(odesc(TURN_DIMS, TURN_C), w)
    turn1, turn2 = synth.make_tokens(TURN_DIMS, 1501, seed=71), synth.make_tokens(TURN_DIMS, 1001, seed=73)
    steps = []
    for prompt, n in ((turn1, 13), (turn2, 8)):
        for t in prompt[:-1]:
            ref.step(int(t), want_logits=False)
        tok = int(prompt[-1])
        for _ in range(n):
            lg = ref.step(tok)
            steps.append((tok, lg))
            tok = orc.argmax(lg)
    rows = {(l, v, p): (ref.vcache(l) if v else ref.kcache(l))[p].copy() for l in range(TURN_DIMS.L) for v in (False, True) for p in TURN_ROWS}
    return w, turn1, turn2, steps, rows


@pytest.mark.parametrize("kv16", [False, True], ids=["kv-f32", "kv-f16"])
def test_second_turn_ingest_after_decode(mgr, kv16):
    """Thin model with 8B heads (E = 512, 32/8 heads of 128, F = 512, V = 1024, L = 2) at C = 2700 (one-pass decode): ingest 1500
    tokens, 13 greedy steps, ingest 1000 more at pos0 = 1513 (chunks 1513-2024 and 2025-2512: across 2048, over rows the decode
    wrote), 8 greedy steps — against OracleLlama fed the same tokens (the oracle's greedy choices).  Logits within the prefill
    bar, greedy tokens equal wherever the oracle's top-2 margin exceeds it, K / V rows at the chunk edges and the decode-written
    rows within 2e-2; the last block's attention against float64 (part A) after every step."""
    from nfai_amd.llama_model import LlamaModel
    w, turn1, turn2, steps, rows = _second_turn_oracle()
    m = LlamaModel(mgr, synth.make_metadata(TURN_DIMS), w, TURN_C, kv_f16=kv16, max_batch=512)
    worst_logit, worst_att = 0.0, 0.0
    try:
        mir = KVMirror(m)
        it = iter(steps)
        for prompt, n in ((turn1, 13), (turn2, 8)):
            p0 = m.Pos
            m.Ingest(prompt[:-1])
            mir.pull(p0, len(prompt) - 1)
            for _ in range(n):
                tok, want = next(it)
                S = m.Pos + 1
                lg, am = m.Step(tok)
                mir.pull(S - 1, 1)
                worst_att = max(worst_att, mir.check(S, "turn"))
                scale = max(1.0, float(np.abs(want).max()))
                err = float(np.abs(lg - want).max())
                worst_logit = max(worst_logit, err / (PREFILL_BAR * scale))
                assert err <= PREFILL_BAR * scale, (S, err, scale)
                top2 = np.sort(want)[-2:]
                if top2[1] - top2[0] > PREFILL_BAR * scale:
                    assert am == orc.argmax(want), (S, am, orc.argmax(want))
            assert m.Pos == (1513 if n == 13 else 2521)
        for (layer, is_v, p), row in rows.items():
            np.testing.assert_allclose(m.ReadKV(layer, is_v, p), row, rtol=0, atol=2e-2, err_msg=f"layer {layer} {'V' if is_v else 'K'} row {p}")
        print(f"second turn (kv16={kv16}): worst logit err / bar = {worst_logit:.3g}, worst attention err / bar = {worst_att:.3g}")
    finally:
        m.Dispose()


# ---- D: the contract ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [5, 6, 7])
def test_create_refuses_groupings_without_a_decode_kernel(mgr, G):
    """k_attn_decode exists for G = H/Hkv in {1, 2, 3, 4, 8}: any other grouping must be refused at creation.  Only the creation
    is attempted: a model the library should have refused is never stepped."""
    from nfai_amd import _lib
    from nfai_amd._lib import NfaiHipError
    from nfai_amd.llama_model import LlamaModel
    dims = synth.LlamaDims(f"g{G}", 256, 2, 2 * G, 2, 64, 512, 512, True)
    w = synth.make_weights(dims, seed=G)
    for kv16 in (False, True):
        try:
            m = LlamaModel(mgr, synth.make_metadata(dims), w, 64, kv_f16=kv16)
        except NfaiHipError as e:
            assert e.code == _lib.ERR_UNSUPPORTED, e
            assert "H/Hkv" in str(e), e
            continue
        m.Dispose()
        pytest.fail(f"llama_create accepted H/Hkv = {G} (kv16={kv16}), which the fused decode cannot launch")


def test_unfused_chain_takes_any_grouping(mgr):
    """NFAI_LLAMA_UNFUSED (the 1:1 kernels) is not refused at G = 6 and matches the oracle at the end-to-end bar."""
    from nfai_amd.llama_model import LlamaModel
    dims = synth.LlamaDims("g6", 256, 2, 12, 2, 64, 512, 512, True)
    w = synth.make_weights(dims, seed=6, std=0.05)
    m = LlamaModel(mgr, synth.make_metadata(dims), w, 48, unfused=True)
    ref = orc.OracleLlama(odesc(dims, 48), w)
    try:
        for i, t in enumerate(synth.make_tokens(dims, 40, seed=9)):
            lg, am = m.Step(int(t))
            want = ref.step(int(t))
            assert np.abs(lg - want).max() <= 5e-4 * max(1.0, float(np.abs(want).max())), (i, np.abs(lg - want).max())
            assert am == orc.argmax(want)
    finally:
        m.Dispose()


@pytest.mark.parametrize("heads", ["70b", "g8-d64"])
def test_g8_decodes_at_the_maximum_capacity(mgr, heads):
    """G = 8 at C = 32768 needs more than 64 KB of LDS per workgroup (66560 bytes at D = 128, 67072 at D = 64): the launch must
    allow it rather than refuse the step.  A short history: the depth itself is test_decode_attention_against_fp64's."""
    from nfai_amd._lib import NfaiHipError
    from nfai_amd.llama_model import LlamaModel
    dims, w = _weights(heads)
    m = LlamaModel(mgr, synth.make_metadata(dims), w, 32768)
    try:
        mir = KVMirror(m)
        for i, t in enumerate(synth.make_tokens(dims, 40, seed=3)):
            try:
                m.Step(int(t), want_logits=False)
            except NfaiHipError as e:
                pytest.fail(f"decode step {i} of a G = 8 model at C = 32768 failed: {e}")
            mir.pull(i, 1)
            mir.check(i + 1, heads)
    finally:
        m.Dispose()
