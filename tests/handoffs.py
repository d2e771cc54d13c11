"""Hand-offs between the ways a sequence is advanced, shared by tests/test_handoffs.py (CPU) and tests/test_gpu_handoffs.py.

A sequence is one model's KV cache, position word, token word, token ring and "last hidden state" pointer.  A dozen entry points
advance it and each keeps that state in its own way; a case here runs one kind of segment (A) and then another (B) on the same
sequence and checks everything B could have inherited wrongly.

Kinds (a segment is a kind and a count):
  S   Step                      K   StepTopK                 G   Greedy(first, n)
  E   Enqueue(n) without SetToken: it continues from the token word on the device
  P   Prefill on the MFMA path (max_batch = 64)             I   Ingest on the MFMA path
  I0  Ingest on a model created with max_batch = 0 (token by token).  A case with I0 in it runs on that model, so a P or I beside it is
      the token-by-token form too and computes Step's bits: mfma_on() says which cases run the MFMA prefill
  W   LlamaWindow.Step(t)       V   Verify with k drafts: the first a are the model's own choice, draft a is wrong
  B   LlamaBatch.Step           BG  LlamaBatch.Greedy        BK  LlamaBatch.StepTopK      BW  Step on a wide batch (11 members)
  R   ProfileStep               Q   ProfileKernel (each use takes the next of the classes that launch)
  Z   SetPos(p - r), then the same r tokens fed again by Step

A case: a lead-in of 3 + (index % 5) Steps, A, B, one Step.  ONE oracle walk (oracle.OracleLlama) gives the logits, the hidden state and
the K / V rows of every position; greedy kinds are fed the oracle's own greedy continuation.  The given tokens of each segment come
from a seed of their own: the first one, counted up, at which every token a greedy kind must emit (and the token word an E continues
from) leads the runner-up by at least GAP_BARS bars of that case; the search goes back a segment where one has no tokens of its own
to redraw (E, Z).  No case waives a token.  Weight seed and std are per configuration; RESEED lists the cases that start from a later
seed because a wrong model's margin failed with the first one.

CONTRACT says what each kind leaves behind (include/nfai_hip.h states it per entry point):
  tok     the token word is the ArgMax of the last token the kind ran (Ingest on the MFMA path forms no logits: the word stays)
  ring    the ring took every token of the segment, so FetchTokens returns them (the MFMA prefill writes no ring entries)
  hidden  Read(0) is the hidden state of the last token (ProfileKernel's replay overwrites the activation vectors)

WRONG are the state bugs a hand-off can have, as models on oracle.np_oracle.NpLlama (fp64; pos, K, V are plain attributes).  With p
the position A leaves:
  pos_minus    B's first token runs at p - 1 (row p is never written), the next one at p + 1
  pos_plus     B's first token runs at p + 1 (row p is never written), the next one at p + 2
  skip_last    the attention of B's tokens skips row p - 1, the last row A wrote
  draft_row    row p - 1 holds the row of another token (a rejected draft's) instead of the one A fed
  prev_argmax  B's first token is A's last ArgMax (the token word) instead of the given token
  count_rejected  (A = V only) the position counts the rejected columns: B starts at p + k - a over the drafts' rows
A wrong model that is the model itself is left out: prev_argmax where B continues from the token word anyway, and pos_minus where B is a
rewind whose first token equals the one in front of it (row p - 1 is rewritten with what it held, and row p still holds its own).
"""
from dataclasses import dataclass, field

import numpy as np

from nfai_amd import synth

CAP = 160
MAX_BATCH = 64
LONG = 70            # P / I once per configuration: a chunk boundary (64) inside the segment
GAP_BARS = 4.0
WRONG_BARS = 5.0
WINDOW = 8
NARROW_N, NARROW_C = 4, 2     # the subject is member c of n
WIDE_N, WIDE_C = 11, 9

KINDS = ("S", "K", "G", "E", "P", "I", "I0", "W", "V", "B", "BG", "BK", "BW", "R", "Q", "Z")
SINGLE = ("S", "K", "G", "E", "P", "I", "I0", "R", "Q", "Z")
# computes the bits Step computes (the same kernels with the same arguments: R and Q run the token launch by launch instead of as a
# graph; Q's replay touches only rows above the position and the activation vectors)
EXACT = ("S", "K", "G", "E", "R", "Q", "I0", "Z")
GREEDY = ("G", "E", "BG", "V")
MFMA = ("P", "I")

CONTRACT = {
    #        tok    ring   hidden
    "S":   (True,  True,  True),
    "K":   (True,  True,  True),
    "G":   (True,  True,  True),
    "E":   (True,  True,  True),
    "P":   (True,  False, True),
    "I":   (False, False, True),
    "I0":  (True,  True,  True),
    "W":   (True,  True,  True),
    "V":   (True,  True,  True),
    "B":   (True,  True,  True),
    "BG":  (True,  True,  True),
    "BK":  (True,  True,  True),
    "BW":  (True,  True,  True),
    "R":   (True,  True,  True),
    "Q":   (True,  True,  False),
    "Z":   (True,  True,  True),
}


@dataclass(frozen=True)
class Config:
    name: str
    dims: synth.LlamaDims
    quant: bool
    kv_f16: bool
    engine: bool
    kinds: tuple
    refused: dict          # kind -> (status name, pattern of nfai_hip_last_error): the library's refusal that forbids it here
    wseed: int
    std: float
    tseed: int

    @property
    def scale(self):       # logits bar / max(1, max|logit|) of the decode path
        return 2e-2 if self.kv_f16 else 5e-4

    @property
    def atol(self):        # K / V rows and the hidden state
        return 2e-2 if self.kv_f16 else 1e-3


_ENGINE_REFUSAL = ("ERR_UNSUPPORTED", "runs the engine path")
CONFIGS = {c.name: c for c in (
    Config("f16", synth.TINY, False, False, False, KINDS, {}, 21, 0.05, 5000),
    Config("q4km", synth.TINY_D128, True, True, False, tuple(k for k in KINDS if k != "BW"),
           {"BW": ("ERR_UNSUPPORTED", "the batched kernels take fp16 matrices")}, 21, 0.05, 6000),
    Config("engine", synth.TINY, False, False, True, SINGLE,
           {k: _ENGINE_REFUSAL for k in ("W", "V", "B", "BG", "BK", "BW")}, 21, 0.05, 7000),
)}
PREFILL_SCALE, PREFILL_ATOL = 2e-2, 2e-2


def pairs(cfg):
    """[(index, A, B)]: every ordered pair of the kinds the configuration admits."""
    ks = cfg.kinds
    return [(i * len(ks) + j, a, b) for i, a in enumerate(ks) for j, b in enumerate(ks)]


def coverage():
    """(pairs run on at least one configuration, pairs excluded: {(A, B): refusal}).  A pair is excluded only where EVERY
    configuration refuses one of its kinds; the refusal listed is the first configuration's."""
    run, out = set(), {}
    for cfg in CONFIGS.values():
        run |= {(a, b) for _, a, b in pairs(cfg)}
    for a in KINDS:
        for b in KINDS:
            if (a, b) not in run:
                cfg = next(iter(CONFIGS.values()))
                k = a if a in cfg.refused else b
                out[(a, b)] = cfg.refused[k]
    return run, out


# ---- weights ------------------------------------------------------------------------------------------------------------------------------
_W = {}


def weights(cfg, alt=None):
    """(what the model loads, what the oracle computes on).  alt = (tensor name, seed): that tensor redrawn (the replacement cases)."""
    key = (cfg.name, alt)
    if key not in _W:
        w = dict(synth.make_weights(cfg.dims, seed=cfg.wseed, std=cfg.std))
        if alt is not None:
            name, seed = alt
            rng = np.random.Generator(np.random.PCG64(seed))
            a = w[name]
            w[name] = ((1.0 + 0.1 * rng.standard_normal(a.shape, dtype=np.float32)).astype(np.float32) if a.ndim == 1 else
                       (cfg.std * rng.standard_normal(a.shape, dtype=np.float32)).astype(np.float16))
        if cfg.quant:
            from test_gpu_window_decode import quant_weights
            _W[key] = quant_weights(w)
        else:
            _W[key] = (w, w)
    return _W[key]


def odesc(cfg, cap=CAP):
    import oracle as orc
    d = cfg.dims
    return orc.LlamaDesc(E=d.E, L=d.L, H=d.H, Hkv=d.Hkv, D=d.D, F=d.F, V=d.V, C=cap)


def ddict(d):
    return dict(E=d.E, L=d.L, H=d.H, Hkv=d.Hkv, D=d.D, F=d.F, V=d.V, eps=1e-5, rope_dims=d.D, rope_base=500000.0)


# ---- segments -----------------------------------------------------------------------------------------------------------------------------
@dataclass
class Seg:
    kind: str
    n: int                      # positions the segment advances (Z: 0)
    start: int = 0              # the position it starts at
    fed: list = field(default_factory=list)       # the tokens at positions start .. start + n - 1 (Z: the r tokens fed again)
    k: int = 0                  # V: drafts
    a: int = 0                  # V: accepted drafts
    drafts: list = field(default_factory=list)    # V: all k drafts
    r: int = 0                  # Z: tokens fed again
    cls0: int = 0               # Q: the first use takes class cls0 (mod the classes that launch)
    emitted: list = field(default_factory=list)   # the tokens a greedy kind emits
    tok_after: int = -1         # the token word after the segment
    prefill_rows: bool = False  # the segment, or one before it, ran the MFMA prefill: its rows are read from here on


def count(kind, index, role, long=False, loose=False):
    """Tokens of a segment: 2 .. 9; P / I 5 .. 20 (LONG where asked); W 2 .. 8 columns; V 1 .. 7 drafts.  loose (the case applies
    the fp16-KV / prefill bar): a greedy kind runs 2 to 5 tokens and a Verify accepts at most 3 drafts.  GAP_BARS of that bar are 8 % of the largest logit, which a token
    of these models clears with probability 0.45: nine of them running would take thousands of seeds."""
    if kind in MFMA:
        return LONG if long else 5 + (index * 7 + role * 3) % 16
    if kind == "W":
        return 2 + (index + role) % 7
    if kind == "V":
        return 1 + (index + 3 * role) % 7        # k drafts
    if loose and kind in GREEDY:
        return 2 + (index + role) % 4
    return 2 + (index * 3 + role * 5) % 8


def mfma_on(kinds):
    """Whether P and I run the MFMA prefill in a case of these kinds: not on the max_batch = 0 model that I0 needs."""
    return "I0" not in kinds


def plan(cfg, index, A, B):
    """[(kind, count)] of a pair case.  P and I take LONG tokens as A where B is the other of the two."""
    long = A in MFMA and B in MFMA and A != B
    loose = cfg.kv_f16 or (mfma_on((A, B)) and (A in MFMA or B in MFMA))
    return [("S", 3 + index % 5), (A, count(A, index, 0, long, loose)), (B, count(B, index, 1, False, loose)), ("S", 1)]


@dataclass
class Ref:
    """One oracle walk: per position the token fed, its logits, ArgMax, hidden state; the K / V rows of every block."""
    toks: list
    logits: list
    am: list
    hidden: list
    K: list
    V: list
    gap: list                   # (largest - second largest logit) / max(1, max|logit|) per position
    segs: list
    must: list                  # positions whose ArgMax the GPU must reproduce (greedy emissions, token words an E reads)


def walk(cfg, segments, tseed, wref=None, min_bars=None, tries=300):
    """Walk [(kind, count)] on the oracle.  The given tokens of segment i come from synth.make_tokens(seed = tseed + 7919 i + 104729 t),
    the greedy ones are the oracle's own ArgMax.  min_bars: t is the first try at which every must-position of the segment (and the
    token word a following E reads) leads by that many bars; the oracle is rewound to the segment's start between tries (its reset
    and advance move the position without touching the cache).  None where a segment finds no such try."""
    import oracle as orc
    d = cfg.dims
    ref = orc.OracleLlama(odesc(cfg), wref if wref is not None else weights(cfg)[1])
    toks, logits, am, hidden, gap = [], [], [], [], []
    must, segs = set(), []
    on = mfma_on([k for k, _ in segments])
    loose = cfg.kv_f16 or (on and any(k in MFMA for k, _ in segments))
    state = dict(tokword=-1, tokword_pos=-1, pre=False)

    class Short(Exception):
        pass

    def need(pos):
        must.add(pos)
        if min_bars is not None and gap[pos] / (PREFILL_SCALE if state["pre"] else cfg.scale) < min_bars:
            raise Short

    def feed(t):
        lg = np.array(ref.step(int(t)), np.float32)
        toks.append(int(t))
        logits.append(lg)
        am.append(int(np.argmax(lg)))
        hidden.append(np.array(ref.hidden(), np.float32))
        top = np.partition(lg, -2)[-2:]
        gap.append(float(top[1] - top[0]) / max(1.0, float(np.abs(lg).max())))
        return am[-1]

    def segment(idx, kind, cnt, given):
        p = len(toks)
        s = Seg(kind, 0, p)
        if kind in MFMA and on:
            state["pre"] = True
        if kind == "Z":
            s.r = min(cnt, p - 1)            # a row stays in front of the rewind
            s.fed = toks[p - s.r:]
            s.start = p - s.r
            if s.r:
                state["tokword"], state["tokword_pos"] = am[p - 1], p - 1
        elif kind in ("G", "BG"):
            t = next(given)
            for _ in range(cnt):
                s.fed.append(t)
                t = feed(t)
                s.emitted.append(t)
                need(len(toks) - 1)
        elif kind == "E":
            assert state["tokword"] >= 0, "E needs a token word"
            need(state["tokword_pos"])
            t = state["tokword"]
            for _ in range(cnt):
                s.fed.append(t)
                t = feed(t)
                s.emitted.append(t)
                need(len(toks) - 1)
        elif kind == "V":
            s.k, s.a = cnt, (idx + cnt + p) % (min(cnt, 3) + 1 if loose else cnt + 1)
            t = next(given)
            for i in range(s.a + 1):
                s.fed.append(t)
                t = feed(t)
                s.emitted.append(t)
                need(len(toks) - 1)
                if i < s.a:
                    s.drafts.append(t)
            if s.a < s.k:
                s.drafts.append((s.emitted[-1] + 1) % d.V)               # draft a is wrong
                s.drafts += [next(given) for _ in range(s.k - s.a - 1)]
        else:
            for _ in range(cnt):
                t = next(given)
                s.fed.append(t)
                feed(t)
        s.n = len(toks) - p
        if kind == "Q":
            s.cls0 = idx + p
        if kind != "Z" and s.n and CONTRACT[kind][0]:
            state["tokword"], state["tokword_pos"] = am[-1], len(toks) - 1
        # the token word an E behind this segment reads (an Ingest or a rewind between them leaves it where it is)
        later = [k for k, _ in segments[idx + 1:idx + 3]]
        if later[:1] == ["E"] or (len(later) == 2 and later[0] in ("I", "Z") and later[1] == "E"):
            if state["tokword_pos"] >= 0:
                need(state["tokword_pos"])
        s.tok_after = state["tokword"]
        s.prefill_rows = state["pre"]
        return s

    # depth-first over the segments' tries: a segment without tokens of its own (E, Z) has one try, and its failure sends the search
    # back to the segment before it
    n = len(segments)
    t, starts, saved, total = [0] * n, [0] * n, [None] * n, 0
    idx = 0
    while idx < n:
        kind, cnt = segments[idx]
        if t[idx] == 0:
            starts[idx], saved[idx] = len(toks), dict(state)
        if t[idx] >= (1 if kind in ("E", "Z") or min_bars is None else tries) or total > 20 * tries:
            t[idx] = 0
            idx -= 1
            if idx < 0 or total > 20 * tries:
                ref.close()
                return None
            t[idx] += 1
            continue
        p = starts[idx]
        for lst in (toks, logits, am, hidden, gap):
            del lst[p:]
        del segs[idx:]
        must.difference_update({q for q in must if q >= p})
        state.clear()
        state.update(saved[idx])
        ref.reset()
        for _ in range(p):
            ref.advance()
        given = iter(int(x) for x in synth.make_tokens(d, max(cnt, 8) + 16, seed=tseed + 7919 * idx + 104729 * t[idx]))
        total += 1
        try:
            segs.append(segment(idx, kind, cnt, given))
            idx += 1
            if idx < n:
                t[idx] = 0
        except Short:
            t[idx] += 1
    K = [np.array(ref.kcache(l)[:len(toks)], np.float32) for l in range(d.L)]
    V = [np.array(ref.vcache(l)[:len(toks)], np.float32) for l in range(d.L)]
    ref.close()
    return Ref(toks, logits, am, hidden, K, V, gap, segs, sorted(must))


def case_bars(cfg, ref):
    """The smallest lead, in bars of the segment that must reproduce it, of every ArgMax the GPU must reproduce.  The token word an E
    continues from is held to the bar of the E segment (the later, looser one)."""
    out = float("inf")
    for p in ref.must:
        seg = next(s for s in ref.segs if s.kind != "Z" and s.start <= p < s.start + s.n)
        later = [s for s in ref.segs if s.kind == "E" and s.start == p + 1] or [seg]
        loosest = max(PREFILL_SCALE if s.prefill_rows else cfg.scale for s in [seg] + later)
        out = min(out, ref.gap[p] / loosest)
    return out


RESTARTS = 8
# Cases whose first token seed left a wrong model of tests/test_handoffs.py under WRONG_BARS (mostly greedy runs that settle on one
# repeated token, where a shifted or skipped row changes little): they start from a later seed, found by reseed_search() below.
_RESEED = {   # configuration: "A>B:restart" ...
    "f16": (
        "S>I0:1 S>V:1 S>B:1 S>BK:1 S>Q:1 K>S:1 K>G:1 K>E:1 K>P:1 K>I0:1 K>BK:1 K>Q:1 G>G:2 G>E:5 G>I:2 G>I0:2 G>BG:1 G>BK:1 "
        "G>R:2 G>Q:1 G>Z:1 E>K:1 E>E:1 E>P:3 E>I:2 E>B:1 E>BG:6 E>BK:1 P>G:2 P>I:1 P>BG:2 P>R:1 P>Q:1 I>P:3 I>I0:1 I0>S:3 "
        "I0>E:4 I0>P:1 I0>B:1 I0>BG:1 I0>R:2 W>S:1 W>E:1 W>P:2 W>V:1 W>BK:1 W>R:1 V>E:2 V>P:1 V>BG:2 V>Q:3 B>K:3 B>G:1 B>I0:1 "
        "B>BG:2 B>BK:1 B>Q:1 BG>G:2 BG>I:1 BG>V:1 BG>BG:2 BG>Q:1 BG>Z:2 BK>K:1 BK>G:2 BK>E:1 BK>BG:1 R>P:1 R>V:3 R>BG:4 R>Q:1 "
        "Q>P:1 Q>V:1 Q>BG:1 Z>S:1 Z>E:1 Z>P:1 Z>I:1 Z>V:2 Z>BG:1 Z>R:3 "
    ),
    "q4km": (
        "Q>W:1 "
    ),
}
RESEED = {(c, *ab.split(">")): int(t) for c, txt in _RESEED.items() for ab, t in (x.split(":") for x in txt.split())}
_CASES = {}


def case(cfg, index, A, B, segments=None):
    """The Ref of a pair case (or of `segments`, keyed by A): every must-token leads by GAP_BARS bars.  Deterministic, so the CPU and
    the GPU tests build the same case; cached."""
    key = (cfg.name, index, A, B, None if segments is None else tuple(segments))
    if key not in _CASES:
        segs = plan(cfg, index, A, B) if segments is None else list(segments)
        t0 = RESEED.get((cfg.name, A, B), 0) if segments is None else 0
        for t in range(t0, t0 + RESTARTS):
            ref = walk(cfg, segs, cfg.tseed + 13 * index + 1009 * t, min_bars=GAP_BARS)
            if ref is not None:
                break
        else:
            raise AssertionError(f"{cfg.name} {A}->{B}: no token seeds give every greedy token {GAP_BARS} bars")
        assert case_bars(cfg, ref) >= GAP_BARS
        _CASES[key] = ref
    return _CASES[key]


# ---- the production-order conversation --------------------------------------------------------------------------------------------------
CONVERSATION = [("I", 40), ("V", 7), ("V", 5), ("V", 7), ("V", 3), ("V", 6), ("V", 7), ("I", LONG), ("K", 3), ("B", 4), ("G", 5), ("R", 2),
                ("Q", 0), ("S", 2)]      # Q's count is set by the caller: once per launching class


# ---- wrong models -----------------------------------------------------------------------------------------------------------------------
WRONG = ("pos_minus", "pos_plus", "skip_last", "draft_row", "prev_argmax", "count_rejected")


class NpHandoff:
    """oracle.np_oracle.NpLlama with the attention of later tokens optionally skipping one row."""

    def __init__(self, cfg, wref):
        from oracle import np_oracle as npo
        self.npo = npo
        self.m = npo.NpLlama(odesc(cfg), wref)
        self.skip = None

    def clone(self):
        import copy
        c = copy.copy(self)
        c.m = copy.copy(self.m)
        c.m.K = [k.copy() for k in self.m.K]
        c.m.V = [v.copy() for v in self.m.V]
        return c

    def step(self, tok):
        m, npo = self.m, self.npo
        if self.skip is None:
            return m.step(tok)
        d, w, p = m.d, m.w, m.pos
        keep = [i for i in range(p + 1) if i != self.skip]
        x = w["token_embd.weight"][tok].copy()
        for l in range(d.L):
            b = f"blk.{l}."
            xn = npo.rmsnorm(x, w[b + "attn_norm.weight"], d.eps)
            q = npo.rope(w[b + "attn_q.weight"] @ xn, m.freqs, m.rd, d.H, d.D, p)
            m.K[l][p] = npo.rope(w[b + "attn_k.weight"] @ xn, m.freqs, m.rd, d.Hkv, d.D, p)
            m.V[l][p] = w[b + "attn_v.weight"] @ xn
            att = npo.attention(q, m.K[l][keep], m.V[l][keep], d.H, d.Hkv, d.D, len(keep))
            h = x + w[b + "attn_output.weight"] @ att
            hn = npo.rmsnorm(h, w[b + "ffn_norm.weight"], d.eps)
            x = h + w[b + "ffn_down.weight"] @ ((w[b + "ffn_up.weight"] @ hn) * npo.silu(w[b + "ffn_gate.weight"] @ hn))
        m.pos += 1
        return w.get("output.weight", w["token_embd.weight"]) @ npo.rmsnorm(x, w["output_norm.weight"], d.eps)


def wrong_runs(cfg, ref, wref):
    """{wrong model: (logits of B's last token, the K rows [L][KD] B's first token wrote)} and the same under "exact", on NpLlama,
    for a pair case's Ref (segments lead-in, A, B, tail).  B's tokens are the ones the case feeds; where B is Z they are fed again
    at the rewound position."""
    d = cfg.dims
    segA, segB = ref.segs[1], ref.segs[2]
    base = NpHandoff(cfg, wref)
    p = ref.segs[0].n + segA.n        # the position A leaves
    for t in ref.toks[:p]:
        base.step(t)
    toksB = list(segB.fed)
    p0 = segB.start                   # where B's first token belongs (Z: p - r)
    word = ref.segs[1].tok_after

    def run(name):
        m = base.clone()
        m.m.pos = p0
        first = p0
        toks = list(toksB)
        if name == "pos_minus":
            first = p0 - 1
        elif name == "pos_plus":
            first = p0 + 1
        elif name == "skip_last":
            m.skip = p0 - 1
        elif name == "draft_row":
            m.m.pos = p0 - 1
            m.step((ref.toks[p0 - 1] + 1) % d.V)
        elif name == "prev_argmax":
            toks[0] = word
        elif name == "count_rejected":
            for t in segA.drafts[segA.a:]:
                m.step(t)
            first = m.m.pos
        m.m.pos = first
        lg = m.step(toks[0])
        krow = [m.m.K[l][first].copy() for l in range(d.L)]
        if name in ("pos_minus", "pos_plus"):
            m.m.pos = first + (2 if name == "pos_minus" else 1)
        for t in toks[1:]:
            lg = m.step(t)
        return np.asarray(lg), krow

    out = {"exact": run("exact")}
    for name in WRONG:
        if name == "count_rejected" and not (segA.kind == "V" and segA.a < segA.k):
            continue
        if name == "prev_argmax" and (word < 0 or word == toksB[0]):
            continue                  # the model itself
        if p0 < 1:
            continue
        if name == "pos_minus" and segB.kind == "Z" and len(toksB) > 1 and ref.toks[p0 - 1] == toksB[0]:
            continue                  # a rewind over a repeated token: row p - 1 is rewritten with what it held, the model itself
        out[name] = run(name)
    return out


def pair_bar(A, B):
    """(logits scale, row atol): the loosest bar any GPU case applies to the pair."""
    cfgs = [c for c in CONFIGS.values() if A in c.kinds and B in c.kinds]
    if mfma_on((A, B)) and (A in MFMA or B in MFMA):
        return PREFILL_SCALE, PREFILL_ATOL
    return max(c.scale for c in cfgs), max(c.atol for c in cfgs)


def wrong_margins(cfg, ref, A, B):
    """{wrong model: (logits margin, K row margin)} of a pair case, in bars of pair_bar(A, B)."""
    scale, atol = pair_bar(A, B)
    runs = wrong_runs(cfg, ref, weights(cfg)[1])
    lg0, k0 = runs.pop("exact")
    return {w: (float(np.abs(lg - lg0).max()) / (scale * max(1.0, float(np.abs(lg0).max()))),
                max(float(np.abs(k[l] - k0[l]).max()) for l in range(cfg.dims.L)) / atol) for w, (lg, k) in runs.items()}


def reseed_search(names=("f16", "q4km"), want=WRONG_BARS + 0.25, limit=60):
    """How RESEED was made: for every pair case, the first restart seed at which every wrong model clears `want` bars."""
    out = {}
    for name in names:
        cfg = CONFIGS[name]
        for i, a, b in pairs(cfg):
            for t in range(limit):
                RESEED[(name, a, b)] = t
                _CASES.pop((name, i, a, b, None), None)
                try:
                    ref = case(cfg, i, a, b)
                except AssertionError:
                    continue
                if min(min(v) for v in wrong_margins(cfg, ref, a, b).values()) >= want:
                    break
            else:
                raise AssertionError((name, a, b))
            if t:
                out[(name, a, b)] = t
            else:
                del RESEED[(name, a, b)]
    return out
