"""Every hand-off between the ways a sequence is advanced, on the GPU (tests/handoffs.py describes the kinds, the cases, the contract
table and the wrong models; tests/test_handoffs.py shows on the CPU that the bars here would see each wrong model).

Configurations: fp16 weights on tiny-llama with an fp32 KV cache; the Q4_K / Q6_K mix of tests/test_gpu_window_decode.py on
tiny-llama-d128 with an fp16 cache; tiny-llama with engine=True (the single-model kinds: _batch_create and _window_create refuse an
engine model, which test_refusals_that_leave_kinds_out pins).  Capacity 160, max_batch = 64; a case with I0 in it runs on models
created with max_batch = 0.  The subject, its twin, ten fillers, a batch of each family and a window of 8 per side live for the whole
module and are reused with Reset(): graphs captured by earlier cases stay alive, and a case run alone passes too.

Bars (the project's own): logits 5e-4 * max(1, max|logit|) and K / V rows 1e-3 with an fp32 cache; 2e-2 and 2e-2 with an fp16 cache and
for anything that reads rows the MFMA prefill wrote; the hidden state takes the rows' bar, as in tests/test_gpu_batch_wide.py.

The tight check: a twin (same weights, own cache) takes the lead-in and A the same way and B's tokens through Step.  After A the two
caches are BIT-IDENTICAL (asserted: every path is deterministic, the prefill included).  Then the subject's B and the tail are held
against the twin's at the decode bar of the cache (5e-4 / 1e-3 or 2e-2 / 2e-2), not at the prefill bar, so a B that reads prefill
rows wrongly cannot hide behind the prefill's precision.  Where B itself is the MFMA prefill, B's own rows ARE prefill rows (fp16
operands, stated at 2e-2 in include/nfai_hip.h) and the twin's are Step's: B and the tail behind it take the prefill bar there too.
S, K, G, E, R, Q, I0 and Z compute Step's bits (R and Q run the token's launches one by one instead of as a graph, with the same
arguments; Q's replay writes only K / V rows above the position and the activation vectors): when A and B both come from that list, the
tail's logits and every row equal the twin's bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import handoffs as ho
import oracle as orc
from nfai_amd import synth

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


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


def all_rows(m, L, pos, n):
    return [kv_rows(m, l, v, pos, n) for l in range(L) for v in (False, True)] if n else []


def make_model(mgr, cfg, max_batch=ho.MAX_BATCH, donor=None, cap=ho.CAP, alt=None):
    from nfai_amd.llama_model import LlamaModel
    kw = dict(kv_f16=cfg.kv_f16, max_batch=max_batch)
    if cfg.engine:
        kw["engine"] = True
    if cfg.quant:
        kw["dims"] = ho.ddict(cfg.dims)
    if donor is not None:
        kw["share_from"] = donor
    return LlamaModel(mgr, synth.make_metadata(cfg.dims), ho.weights(cfg, alt)[0], cap, **kw)


class Side:
    """One sequence and what advances it: the model, a window of 8, a narrow and a wide batch in which it is member c of n."""

    def __init__(self, mgr, cfg, max_batch, donor, fillers):
        from nfai_amd.llama_model import LlamaBatch, LlamaWindow
        self.cfg, self.d, self.max_batch = cfg, cfg.dims, max_batch
        self.m = make_model(mgr, cfg, max_batch, donor)
        self.fillers = fillers
        self.win = self.narrow = self.wide = None
        self.classes = None
        if "W" in cfg.kinds:
            self.win = LlamaWindow(self.m, ho.WINDOW, quantized=cfg.quant)
        if "B" in cfg.kinds:
            f = fillers[:ho.NARROW_N - 1]
            self.narrow = LlamaBatch(f[:ho.NARROW_C] + [self.m] + f[ho.NARROW_C:], quantized=cfg.quant)
        if "BW" in cfg.kinds:
            f = fillers[:ho.WIDE_N - 1]
            self.wide = LlamaBatch(f[:ho.WIDE_C] + [self.m] + f[ho.WIDE_C:], wide=True)

    def dispose(self):
        for x in (self.win, self.narrow, self.wide, self.m):
            if x is not None:
                x.Dispose()

    def launching(self):
        """The kernel classes a token of this model launches (from one profiled step at position 0)."""
        if self.classes is None:
            self.m.Reset()
            self.classes = [k for k, (_, n) in self.m.ProfileStep(1).items() if n]
            self.m.Reset()
        return self.classes

    def reset(self):
        self.launching()                      # (before the case: it runs a token)
        self.m.Reset()
        for i, f in enumerate(self.fillers):
            f.SetPos(1 + (5 * i) % 17)        # the other members sit at other depths, over rows the fixture ingested

    def _members(self, batch, c, t):
        toks = [(int(t) + 7 * (i + 1)) % self.d.V for i in range(batch.n)]
        toks[c] = int(t)
        return toks

    def run(self, seg, as_steps=False):
        """Run a segment; {"logits": {pos: vector}, "am": {pos: returned ArgMax}, "emitted": tokens | None}."""
        m, V = self.m, self.d.V
        kind = "S" if as_steps and seg.kind != "Z" else seg.kind
        lg, am, emitted = {}, {}, None
        p, fed, n = seg.start, seg.fed, len(seg.fed)
        last = p + n - 1
        if kind == "Z":
            m.SetPos(p)
            kind = "S"
        if kind == "S":
            for i, t in enumerate(fed):
                lg[p + i], am[p + i] = m.Step(t)
        elif kind == "K":
            for i, t in enumerate(fed):
                ids, probs = m.StepTopK(t)
                lg[p + i], am[p + i] = m.Read(4, V), int(ids[0])
                assert np.all(np.diff(probs) <= 0) and abs(float(probs.sum())) <= 1.0 + 1e-5
        elif kind == "G":
            emitted = [int(t) for t in m.Greedy(fed[0], n)]
            lg[last] = m.Read(4, V)
        elif kind == "E":
            m.Enqueue(n)
            emitted = [int(t) for t in m.FetchTokens(n)]
            lg[last] = m.Read(4, V)
        elif kind == "P":
            lg[last] = m.Prefill(fed)
        elif kind in ("I", "I0"):
            m.Ingest(fed)
            if self.max_batch == 0:           # token by token: the last token's logits are the model's
                lg[last] = m.Read(4, V)
        elif kind == "W":
            got, a = self.win.Step(fed)
            for i in range(n):
                lg[p + i], am[p + i] = got[i], int(a[i])
        elif kind == "V":
            got, out = self.win.Verify(fed[0], seg.drafts, want_logits=True)
            emitted = [int(t) for t in out]
            for i in range(min(len(out), n)):
                lg[p + i], am[p + i] = got[i], emitted[i]
        elif kind in ("B", "BW"):
            batch, c = (self.narrow, ho.NARROW_C) if kind == "B" else (self.wide, ho.WIDE_C)
            for i, t in enumerate(fed):
                got, a = batch.Step(self._members(batch, c, t))
                lg[p + i], am[p + i] = got[c], int(a[c])
        elif kind == "BK":
            for i, t in enumerate(fed):
                ids, _ = self.narrow.StepTopK(self._members(self.narrow, ho.NARROW_C, t))
                lg[p + i], am[p + i] = m.Read(4, V), int(ids[ho.NARROW_C][0])
        elif kind == "BG":
            out = self.narrow.Greedy(self._members(self.narrow, ho.NARROW_C, fed[0]), n)
            emitted = [int(t) for t in out[:, ho.NARROW_C]]
            lg[last] = m.Read(4, V)
        elif kind == "R":
            for i, t in enumerate(fed):
                m.ProfileStep(t)
                lg[p + i] = m.Read(4, V)
        elif kind == "Q":
            cls = self.launching()
            for i, t in enumerate(fed):
                us = m.ProfileKernel(t, cls[(seg.cls0 + i) % len(cls)], 2)
                assert us > 0
                lg[p + i] = m.Read(4, V)
        else:
            raise AssertionError(kind)
        return dict(logits=lg, am=am, emitted=emitted)


class Rig:
    """The models of one configuration: subject and twin with max_batch = 64, the same two with max_batch = 0, ten fillers."""

    def __init__(self, mgr, cfg):
        self.cfg = cfg
        self.donor = make_model(mgr, cfg)                   # holds the weights; every other model shares them
        self.fillers = []
        if "B" in cfg.kinds:
            toks = synth.make_tokens(cfg.dims, 24, seed=3)
            for i in range(ho.WIDE_N - 1):
                f = make_model(mgr, cfg, 0, self.donor)
                f.Ingest((toks + i) % cfg.dims.V)
                self.fillers.append(f)
        self.sides = {}
        for mb in (ho.MAX_BATCH, 0):
            pair = []
            for _ in range(2):
                pair.append(Side(mgr, cfg, mb, self.donor, self.fillers))
            self.sides[mb] = pair

    def dispose(self):
        for pair in self.sides.values():
            for s in pair:
                s.dispose()
        for f in self.fillers:
            f.Dispose()
        self.donor.Dispose()


@pytest.fixture(scope="module")
def rigs(mgr):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Rig(mgr, ho.CONFIGS[name])
        return made[name]

    yield get
    for r in made.values():
        r.dispose()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_segment(side, seg, obs, ref, scale, atol, where):
    """The subject against the oracle after one segment: position, every returned logit vector and ArgMax, emitted tokens, every
    K / V row the segment wrote, and what CONTRACT promises of Read(0) and the ring."""
    m, d = side.m, side.d
    n = len(seg.fed)
    assert m.Pos == seg.start + n, (where, m.Pos, seg.start + n)
    worst = 0.0
    for p, lg in obs["logits"].items():
        want = ref.logits[p]
        tol = scale * max(1.0, float(np.abs(want).max()))
        err = float(np.abs(lg - want).max())
        worst = max(worst, err / tol)
        assert err <= tol, (where, p, err, tol)
        if p in obs["am"]:
            assert obs["am"][p] == int(np.argmax(lg)), (where, p, obs["am"][p], int(np.argmax(lg)))   # the first maximum of its own logits
    if seg.kind in ho.GREEDY:
        assert obs["emitted"] == seg.emitted, (where, obs["emitted"], seg.emitted)
        if seg.start + n - 1 in obs["logits"]:
            assert obs["emitted"][-1] == int(np.argmax(obs["logits"][seg.start + n - 1]))
    rows = all_rows(m, d.L, seg.start, n)
    for l in range(d.L):
        np.testing.assert_allclose(rows[2 * l], ref.K[l][seg.start:seg.start + n], rtol=0, atol=atol, err_msg=f"{where} K block {l}")
        np.testing.assert_allclose(rows[2 * l + 1], ref.V[l][seg.start:seg.start + n], rtol=0, atol=atol, err_msg=f"{where} V block {l}")
    tok, ring, hidden = ho.CONTRACT[seg.kind]
    mfma = seg.kind in ho.MFMA and side.max_batch > 0
    if hidden and n:
        np.testing.assert_allclose(m.Read(0, d.E), ref.hidden[seg.start + n - 1], rtol=0, atol=atol, err_msg=f"{where} hidden state")
    if (ring or (seg.kind in ho.MFMA and not mfma)) and n:
        got = [int(t) for t in m.FetchTokens(n)]
        if seg.kind in ho.GREEDY:
            assert got == seg.emitted, (where, got, seg.emitted)
        for i in range(n):
            if seg.start + i in obs["am"]:
                assert got[i] == obs["am"][seg.start + i], (where, i, got, obs["am"])
        if seg.start + n - 1 in obs["logits"]:
            assert got[-1] == int(np.argmax(obs["logits"][seg.start + n - 1])), (where, got)
    return worst


# ---- pair cases ---------------------------------------------------------------------------------------------------------------------------
PAIRS = [pytest.param(c.name, i, a, b, id=f"{c.name}-{a}-{b}") for c in ho.CONFIGS.values() for i, a, b in ho.pairs(c)]


@pytest.mark.parametrize("name,index,A,B", PAIRS)
def test_pair(rigs, name, index, A, B):
    """Lead-in, A, B, one Step: the subject against the oracle after every segment, and against its twin (module docstring)."""
    cfg = ho.CONFIGS[name]
    d = cfg.dims
    ref = ho.case(cfg, index, A, B)
    on = ho.mfma_on((A, B))
    subject, twin = rigs(name).sides[ho.MAX_BATCH if on else 0]
    subject.reset()
    twin.reset()
    lead, segA, segB, tail = ref.segs
    obs = {}
    for s in (lead, segA):
        scale, atol = (ho.PREFILL_SCALE, ho.PREFILL_ATOL) if s.prefill_rows else (cfg.scale, cfg.atol)
        obs[id(s)] = subject.run(s)
        check_segment(subject, s, obs[id(s)], ref, scale, atol, f"{name} {A}->{B} {s.kind}@{s.start}")
        twin.run(s)
    p = lead.n + segA.n
    assert subject.m.Pos == twin.m.Pos == p
    for a, b in zip(all_rows(subject.m, d.L, 0, p), all_rows(twin.m, d.L, 0, p)):
        np.testing.assert_array_equal(bits(a), bits(b), err_msg=f"{name} {A}->{B}: the rows after A differ between subject and twin")
    exact = A in ho.EXACT + (() if on else ho.MFMA) and B in ho.EXACT + (() if on else ho.MFMA)
    b_is_prefill = on and B in ho.MFMA
    t_scale, t_atol = (ho.PREFILL_SCALE, ho.PREFILL_ATOL) if b_is_prefill else (cfg.scale, cfg.atol)
    worst_twin = 0.0
    for s in (segB, tail):
        scale, atol = (ho.PREFILL_SCALE, ho.PREFILL_ATOL) if s.prefill_rows else (cfg.scale, cfg.atol)
        where = f"{name} {A}->{B} {s.kind}@{s.start}"
        got = subject.run(s)
        check_segment(subject, s, got, ref, scale, atol, where)
        tw = twin.run(s, as_steps=True)
        assert twin.m.Pos == subject.m.Pos
        for q, lg in got["logits"].items():
            want = tw["logits"][q]
            tol = t_scale * max(1.0, float(np.abs(want).max()))
            err = float(np.abs(lg - want).max())
            worst_twin = max(worst_twin, err / tol)
            assert err <= tol, (where, "against the twin", q, err, tol)
            if exact and s is tail:
                np.testing.assert_array_equal(bits(lg), bits(want), err_msg=f"{where}: tail logits against the twin")
        n = len(s.fed)
        for a, b in zip(all_rows(subject.m, d.L, s.start, n), all_rows(twin.m, d.L, s.start, n)):
            np.testing.assert_allclose(a, b, rtol=0, atol=t_atol, err_msg=f"{where}: rows against the twin")
    if exact:
        end = subject.m.Pos
        for a, b in zip(all_rows(subject.m, d.L, 0, end), all_rows(twin.m, d.L, 0, end)):
            np.testing.assert_array_equal(bits(a), bits(b), err_msg=f"{name} {A}->{B}: rows against the twin, bit for bit")
    print(f"{name} {A}->{B}: against the twin {worst_twin:.3f} bars")


# ---- the refusals that leave kinds out of a configuration ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in ho.CONFIGS.values() if c.refused])
def test_refusals_that_leave_kinds_out(rigs, name):
    from nfai_amd import _lib
    from nfai_amd._lib import NfaiHipError
    from nfai_amd.llama_model import LlamaBatch, LlamaWindow
    cfg = ho.CONFIGS[name]
    rig = rigs(name)
    m = rig.sides[ho.MAX_BATCH][0].m
    for kind, (code, pattern) in cfg.refused.items():
        with pytest.raises(NfaiHipError, match=pattern) as e:
            if kind in ("W", "V"):
                LlamaWindow(m, ho.WINDOW, quantized=cfg.quant)
            elif kind == "BW":
                LlamaBatch([m], wide=True)
            else:
                LlamaBatch([m], quantized=cfg.quant)
        assert e.value.code == getattr(_lib, code), (kind, e.value.args)


# ---- one conversation in production order -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ho.CONFIGS))
def test_conversation(rigs, name):
    """Ingest(40); six Verify windows mixing accepted and rejected drafts; Ingest(70) at that position, across a chunk boundary, with
    rejected rows above it; StepTopK x 3; four steps in a batch; Greedy(5); ProfileStep x 2; ProfileKernel once per launching class;
    Step x 2; the window disposed, then Read(0).  (The engine configuration runs it without the windows and the batch.)"""
    from nfai_amd.llama_model import LlamaWindow
    cfg = ho.CONFIGS[name]
    subject = rigs(name).sides[ho.MAX_BATCH][0]
    ncls = len(subject.launching())
    segs = [(k, ncls if k == "Q" else c) for k, c in ho.CONVERSATION if k in cfg.kinds]
    ref = ho.case(cfg, 1000, "conversation", "", segments=segs)
    assert len(ref.toks) + 2 <= ho.CAP
    subject.reset()
    shared, subject.win = subject.win, (LlamaWindow(subject.m, ho.WINDOW, quantized=cfg.quant) if "V" in cfg.kinds else None)
    try:
        if "V" in cfg.kinds:
            vs = [s for s in ref.segs if s.kind == "V"]
            assert any(s.a == 0 for s in vs) and any(0 < s.a < s.k for s in vs) and any(s.k == 7 for s in vs)
        for s in ref.segs:
            obs = subject.run(s)
            check_segment(subject, s, obs, ref, ho.PREFILL_SCALE, ho.PREFILL_ATOL, f"{name} conversation {s.kind}@{s.start}")
    finally:
        if subject.win is not None:
            subject.win.Dispose()
        subject.win = shared
    np.testing.assert_allclose(subject.m.Read(0, cfg.dims.E), ref.hidden[-1], rtol=0, atol=ho.PREFILL_ATOL)


# ---- a tensor replaced after finalize ----------------------------------------------------------------------------------------------------
REPLACED = ["blk.{last}.ffn_down.weight", "blk.0.attn_norm.weight", "token_embd.weight"]
KINDS_ONCE = [("S", 2), ("K", 2), ("G", 2), ("E", 2), ("P", 5), ("I", 5), ("R", 2), ("Q", 2), ("Z", 2), ("W", 3), ("S", 1)]


@pytest.mark.parametrize("tensor", REPLACED)
@pytest.mark.parametrize("name", list(ho.CONFIGS))
def test_replaced_tensor_reaches_every_graph(mgr, name, tensor):
    """A model nobody shares runs every single-model kind and a window once, so that the step, top-k and greedy graphs, the engine
    plans and the window's graphs exist.  Then ONE tensor is replaced (same type, other values) with SetTensor + finalize: every kind
    matches the oracle on the new weights and is more than a bar away from the old weights' logits for the same tokens; the old window
    is refused by name and moves nothing; a new window works."""
    from nfai_amd._lib import NfaiHipError, call
    from nfai_amd.llama_model import LlamaWindow
    cfg = ho.CONFIGS[name]
    d = cfg.dims
    tensor = tensor.format(last=d.L - 1)
    alt = (tensor, 909)
    segs = [(k, c) for k, c in KINDS_ONCE if k in cfg.kinds]
    side = Side.__new__(Side)
    side.cfg, side.d, side.fillers, side.narrow, side.wide, side.classes, side.max_batch = cfg, d, [], None, None, None, ho.MAX_BATCH
    side.m = make_model(mgr, cfg)
    side.win = LlamaWindow(side.m, ho.WINDOW, quantized=cfg.quant) if "W" in cfg.kinds else None
    new_win = None
    try:
        side.launching()
        old = ho.case(cfg, 2000, "replace-old", tensor, segments=segs)
        for s in old.segs:
            check_segment(side, s, side.run(s), old, ho.PREFILL_SCALE, ho.PREFILL_ATOL, f"{name} before {s.kind}@{s.start}")
        wdev, wref = ho.weights(cfg, alt)
        side.m.SetTensor(tensor, wdev[tensor])
        call("nfai_hip_llama_finalize", side.m.handle)
        side.m.Reset()
        if side.win is not None:
            with pytest.raises(NfaiHipError, match="tensors changed after the window was created"):
                side.win.Step([1, 2])
            assert side.m.Pos == 0
            new_win, stale = LlamaWindow(side.m, ho.WINDOW, quantized=cfg.quant), side.win
            side.win = new_win
            stale.Dispose()
        key = ("new", cfg.name, tensor)
        if key not in ho._CASES:
            for t in range(ho.RESTARTS):
                r = ho.walk(cfg, segs, cfg.tseed + 2100 + 1009 * t, wref=wref, min_bars=ho.GAP_BARS)
                if r is not None:
                    break
            assert r is not None
            ho._CASES[key] = r
        new = ho._CASES[key]
        before = orc.OracleLlama(ho.odesc(cfg), ho.weights(cfg)[1])        # the old weights on the tokens the new walk feeds
        old_logits = [before.step(t).copy() for t in new.toks]
        before.close()
        moved = {}
        for s in new.segs:
            obs = side.run(s)
            check_segment(side, s, obs, new, ho.PREFILL_SCALE, ho.PREFILL_ATOL, f"{name} after {s.kind}@{s.start}")
            for p, lg in obs["logits"].items():
                bar = ho.PREFILL_SCALE * max(1.0, float(np.abs(old_logits[p]).max()))
                moved[s.kind] = max(moved.get(s.kind, 0.0), float(np.abs(lg - old_logits[p]).max()) / bar)
        print(f"{name} {tensor}: distance from the old weights' logits, in bars: " + ", ".join(f"{k} {v:.1f}" for k, v in moved.items()))
        assert set(moved) == {k for k, _ in segs if k != "I"} and min(moved.values()) > 1.0, moved
    finally:
        if side.win is not None:
            side.win.Dispose()
        side.m.Dispose()


# ---- ProfileKernel at the end of the cache ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ho.CONFIGS))
def test_profile_kernel_at_the_end_of_the_cache(mgr, name):
    """The replayed launches of ProfileKernel read the position word after the token advanced it: a replayed q|k|v stores K / V at
    position + 1, a replayed attention reads up to it.  In the head-major cache [Hkv][C][D], position C of head h is row 0 of head
    h + 1 (past the allocation for the last head).  At Pos = C - 1 every class is either refused before anything runs (Pos, the logits
    and every row keep their bits) or succeeds; if it succeeds, row 0 of every head and block keeps its bits, the rows up to C - 1 match
    the oracle, and so does the Step after a SetPos.  At Pos = C - 2 the call fits and must succeed."""
    from nfai_amd._lib import KVCacheFull
    cfg = ho.CONFIGS[name]
    d = cfg.dims
    assert d.Hkv >= 2
    cap = 24
    m = make_model(mgr, cfg, max_batch=0, cap=cap)
    ref = orc.OracleLlama(ho.odesc(cfg, cap), ho.weights(cfg)[1])
    toks = [int(t) for t in synth.make_tokens(d, cap, seed=515)]
    try:
        classes = [k for k, (_, n) in m.ProfileStep(toks[0]).items() if n]
        m.Reset()
        want = None
        for t in toks[:cap - 2]:
            m.Step(t, want_logits=False)
            ref.step(t, want_logits=False)
        # Pos = C - 2: the token runs at C - 2, the replay touches row C - 1, the last one
        row0 = all_rows(m, d.L, 0, 1)
        us = m.ProfileKernel(toks[cap - 2], "qkv", 2)
        want = ref.step(toks[cap - 2])
        assert us > 0 and m.Pos == cap - 1
        lg = m.Read(4, d.V)
        assert float(np.abs(lg - want).max()) <= cfg.scale * max(1.0, float(np.abs(want).max()))
        for a, b in zip(all_rows(m, d.L, 0, 1), row0):
            np.testing.assert_array_equal(bits(a), bits(b))
        rows = all_rows(m, d.L, 0, cap)
        for cls in classes:
            try:
                m.ProfileKernel(toks[cap - 1], cls, 2)
            except KVCacheFull:
                assert m.Pos == cap - 1
                np.testing.assert_array_equal(bits(m.Read(4, d.V)), bits(lg))
                for a, b in zip(all_rows(m, d.L, 0, cap), rows):
                    np.testing.assert_array_equal(bits(a), bits(b), err_msg=f"{name} {cls}: a refused call moved a row")
                continue
            assert m.Pos == cap
            for a, b in zip(all_rows(m, d.L, 0, 1), row0):
                np.testing.assert_array_equal(bits(a), bits(b), err_msg=f"{name} {cls}: row 0 changed (an overrun lands there)")
            m.SetPos(cap - 1)
        for l in range(d.L):
            np.testing.assert_allclose(kv_rows(m, l, False, 0, cap - 1), ref.kcache(l)[:cap - 1], rtol=0, atol=cfg.atol)
            np.testing.assert_allclose(kv_rows(m, l, True, 0, cap - 1), ref.vcache(l)[:cap - 1], rtol=0, atol=cfg.atol)
        m.SetPos(cap - 2)
        got, am = m.Step(toks[cap - 2])
        assert float(np.abs(got - want).max()) <= cfg.scale * max(1.0, float(np.abs(want).max())) and am == int(np.argmax(got))
        got, am = m.Step(toks[cap - 1])
        want = ref.step(toks[cap - 1])
        assert float(np.abs(got - want).max()) <= cfg.scale * max(1.0, float(np.abs(want).max())) and m.Pos == cap
    finally:
        ref.close()
        m.Dispose()
