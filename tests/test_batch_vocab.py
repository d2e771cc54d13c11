"""CPU side of tests/test_gpu_batch_vocab.py: how the lm_head launches of the batched decode (k_bgemv, k_bgemv_kq, GEMV_PLAIN) deal
the rows of the vocabulary, the vocabularies derived from the CU count at which their multi-pass code runs, and the construction of
EQUAL maxima (rows of output.weight replaced by copies of a column's winning row) placed by that dealing.  Everything here uses the
CPU oracle alone and runs without a GPU; the GPU module imports it.

Dealing (kernels_gemv_batch.hip::plan_bgemv and k_bgemv; kernels_gemv_batch_kqm.hip::plan_bkq and k_bgemv_kq):
  fp16    a unit is a group of 4 rows; 8 waves per workgroup; grid = min(n_cu, ceil(groups / 8)); group g belongs to wave
          g % (8 grid) (workgroup = wave // 8) and is that wave's pass g // (8 grid).  A row's lane follows from its place in the group.
  K-quant a unit is a tile of 16 rows; grid = min(V / 16, n_cu); unit u belongs to workgroup u % grid and is its pass u // grid; row r
          of the tile is finished by lane r.
  Both leave one (value, index) partial per column and workgroup, merged by the last workgroup: lane l reads the partials of the
  workgroups l, l + 64, ... in that order, then the lanes meet.

A tie is resolved (a) in a lane's carry from one pass to the next, (b) between the lanes of a wave, (c) between the waves of a
workgroup (fp16), (d) in a lane's walk over the partials and (e) between those lanes.  TIE_KINDS places one copy per column so that
every one of them decides a column.

Margin: after the copies the oracle's maximum must exceed every logit outside the tie set by more than twice the tolerance
5e-4 * max(1, max|logit|) the GPU logits are held to, so that no rounding on the GPU can lift another row above the tie.  Seeds
(TIE_SEEDS) were chosen here with the oracle alone; the tests below assert the condition for each of them at several CU counts."""
from dataclasses import replace

import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth

V_REAL = 128256          # the vocabulary of every Llama 3 model
CAP = 48
SCALE = 5e-4             # fp32 KV cache: tests/test_gpu_batch_decode.py::logit_tol
Q6K_BLOCK = 210          # bytes per 256 weights
CU_COUNTS = (256, 304, 128)   # MI355X, and two others so that nothing below is true at 256 only
TIE_KINDS = ("same-unit", "later-pass", "earlier-pass", "other-wave", "across-order", "same-merge-lane", "row-0", "row-last")


def odesc(d, C):
    return orc.LlamaDesc(E=d.E, L=d.L, H=d.H, Hkv=d.Hkv, D=d.D, F=d.F, V=d.V, C=C)


def logit_tol(want, scale=SCALE):
    return scale * max(1.0, float(np.abs(want).max()))


# ---- the dealing ----------------------------------------------------------------------------------------------------------------------
class Deal:
    """Row -> (pass, workgroup, sub, off).  fp16: U = 4 rows per unit, S = 8 units (waves) per workgroup and pass; K-quant: U = 16, S = 1."""

    def __init__(self, V, n_cu, quant):
        self.V, self.n_cu, self.quant = int(V), int(n_cu), bool(quant)
        if quant:
            assert V % 16 == 0
            self.U, self.S = 16, 1
            self.units = V // 16
            self.grid = min(self.units, n_cu)
        else:
            self.U, self.S = 4, 8
            self.units = -(-V // 4)
            self.grid = min(n_cu, -(-self.units // 8))
        self.per_pass = self.grid * self.S   # units of one pass of the whole grid

    def place(self, row):
        u = row // self.U
        w = u % self.per_pass
        return u // self.per_pass, w // self.S, w % self.S, row % self.U

    def row(self, pas, wg, sub, off):
        if pas < 0 or not (0 <= wg < self.grid) or not (0 <= sub < self.S) or not (0 <= off < self.U):
            return -1
        r = ((pas * self.grid + wg) * self.S + sub) * self.U + off
        return r if r < self.V else -1

    def passes(self):
        """Units per wave (fp16) / per workgroup (K-quant): (fewest, most, how many have the most)."""
        lo, extra = divmod(self.units, self.per_pass)
        return (lo, lo, self.per_pass) if extra == 0 else (lo, lo + 1, extra)

    def nonvacuous(self):
        """The condition under which a wave / workgroup of the lm_head launch has more than one unit."""
        return self.V > (16 if self.quant else 32) * self.n_cu


def ragged_vocabs(n_cu):
    """The small vocabularies of the GPU module, from the CU count."""
    wide = 32 * n_cu + 2064
    return {"f16+4": 32 * n_cu + 4, "f16+5": 32 * n_cu + 5, "mix+16": 16 * n_cu + 16, "f16-wide": wide, "mix-wide": -(-wide // 16) * 16}


# ---- models and weights ---------------------------------------------------------------------------------------------------------------
def vocab_dims(base, V, tied=None, L=None):
    tied = base.tied if tied is None else tied
    L = base.L if L is None else L
    return replace(base, V=int(V), tied=tied, L=L, name=f"{base.name}-v{V}-{'tied' if tied else 'untied'}-{L}blk")


_WEIGHTS = {}


def weights(dims, quant, seed=21, std=0.05):
    """(what the model loads, what the oracle computes on), cached per (dims, quant, seed) and never modified."""
    key = (dims, bool(quant), seed, std)
    if key not in _WEIGHTS:
        w = synth.make_weights(dims, seed=seed, std=std)
        if quant:
            from test_gpu_batch_quant import quant_weights
            _WEIGHTS[key] = quant_weights(w)
        else:
            _WEIGHTS[key] = (w, w)
    return _WEIGHTS[key]


def with_copied_rows(dims, quant, wdev, wref, copies):
    """New weight dicts in which row `dst` of output.weight is row `src` for every (dst, src): the fp16 row, or the raw Q6_K bytes of
    the row (and its dequantised values for the oracle).  Every other tensor is shared with the originals."""
    from nfai_amd.llama_model import QuantTensor
    dst = np.array([d for d, _ in copies], np.int64)
    src = np.array([s for _, s in copies], np.int64)
    wdev2, wref2 = dict(wdev), dict(wref)
    if quant:
        t = wdev["output.weight"]
        assert t.ggml_type == 14 and dims.E % 256 == 0
        raw = np.array(t.data, np.uint8).reshape(dims.V, dims.E // 256 * Q6K_BLOCK)
        raw[dst] = raw[src]
        wdev2["output.weight"] = QuantTensor(raw.reshape(-1), t.ggml_type, t.shape)
        ref = np.array(wref["output.weight"], np.float32)
        ref[dst] = ref[src]
        wref2["output.weight"] = ref
    else:
        a = np.array(wdev["output.weight"])
        a[dst] = a[src]
        wdev2["output.weight"] = wref2["output.weight"] = a
    return wdev2, wref2


# ---- tie sets ----------------------------------------------------------------------------------------------------------------------------
def tie_row(deal, r, kind, taken, flip=False):
    """The row that receives a copy of row r's weights for placement `kind`: (row, what was placed).  Candidates in order of
    preference (`flip`: the other way round); one is unusable when it falls outside the vocabulary or on a row in `taken`."""
    p, g, s, o = deal.place(r)
    U, G = deal.U, deal.grid
    if kind == "same-unit":          # decided between the lanes of one wave
        cand = [((p, g, s, (o + 1) % U), "same unit, next lane")]
    elif kind == "later-pass":       # the lane's carry: the copy comes later and must not replace r
        cand = [((p + 1, g, s, o), "same lane, next pass"), ((p + 2, g, s, o), "same lane, two passes on")]
    elif kind == "earlier-pass":     # the lane's carry: the copy came first and r must not replace it
        cand = [((p - 1, g, s, o), "same lane, previous pass"), ((p - 2, g, s, o), "same lane, two passes back")]
    elif kind == "other-wave":       # fp16: the LDS merge over the waves of a workgroup; K-quant has none: the same workgroup, other lane and pass
        if deal.S > 1:
            cand = [((p, g, (s + 3) % deal.S, o), "same workgroup and pass, wave + 3 (mod 8)")]
        else:
            cand = [((p + 2, g, 0, (o + 5) % U), "same workgroup, two passes on, other lane"), ((p - 2, g, 0, (o + 5) % U), "same workgroup, two passes back, other lane")]
    elif kind == "across-order":     # the LOWER row in the workgroup with the HIGHER block index
        cand = [((p + 1, g - 1, s, o), "previous workgroup, next pass"), ((p - 1, g + 1, s, o), "next workgroup, previous pass")]
    elif kind == "same-merge-lane":  # two partials read by one lane of the final merge (64 workgroups apart), the lower row first
        cand = [((p, g + 64, s, o), "workgroup + 64, same pass"), ((p, g - 64, s, o), "workgroup - 64, same pass")]
    elif kind == "row-0":
        return (0, "row 0") if r != 0 and 0 not in taken else (-1, "none")
    elif kind == "row-last":
        return (deal.V - 1, "row V - 1") if r != deal.V - 1 and deal.V - 1 not in taken else (-1, "none")
    else:
        raise ValueError(kind)
    if flip:
        cand.reverse()
    # one pass only (a small vocabulary): any other unit of the launch
    cand += [((p, (g + 1) % G, s, o), "fallback: next workgroup"), ((p, g, (s + 1) % deal.S, (o + 1) % U), "fallback: next wave")]
    for pos, what in cand:
        x = deal.row(*pos)
        if x >= 0 and x != r and x not in taken:
            return x, what
    return -1, "none"


def tie_sets(deal, winners, kinds=TIE_KINDS):
    """One copy per column: [(copy row, what)]; no copy falls on a winner or on another copy."""
    taken = set(int(r) for r in winners)
    out = []
    # "across-order" takes the workgroup on the side that "same-merge-lane" does not: one copy below its winner's block index, one above
    flip = False
    if "same-merge-lane" in kinds:
        p, g, s, o = deal.place(int(winners[kinds.index("same-merge-lane")]))
        flip = deal.row(p, g + 64, s, o) < 0
    for r, kind in zip(winners, kinds):
        x, what = tie_row(deal, int(r), kind, taken, flip and kind == "across-order")
        assert x >= 0, (kind, r, deal.place(int(r)))
        taken.add(x)
        out.append((x, what))
    return out


def check_tied_columns(logits, winners, sets, where):
    """After the copies, per column: the tie set holds the maximum, bit-equal; everything else is more than twice the tolerance below.
    Returns the expected tokens (the lowest index of each tie set)."""
    rows = [r for r in winners] + [x for x, _ in sets]
    assert len(set(rows)) == len(rows), (where, rows)           # disjoint, and no copy on a winner
    expect = []
    for b, lg in enumerate(logits):
        tie = [int(winners[b]), int(sets[b][0])]
        tol = logit_tol(lg)
        mx = float(lg.max())
        assert float(lg[tie[0]]) == mx and float(lg[tie[1]]) == mx, (where, b, lg[tie], mx)
        rest = np.array(lg)
        rest[tie] = -np.inf
        gap = mx - float(rest.max())
        assert gap > 2 * tol, (where, b, gap, tol)
        expect.append(min(tie))
    return expect


# ---- section 2: eight columns of one batch step -----------------------------------------------------------------------------------------
# weights seed, token seed per weight kind: chosen with the oracle alone (see the module docstring)
TIE_SEEDS = {False: (21, 400), True: (21, 400)}


def tie_dims(V=V_REAL):
    return vocab_dims(synth.TINY, V, tied=False, L=1)


def batch_columns(dims, seed, n=8):
    """Member s is fed s + 1 tokens alone, then its token of the batch step: (what it is fed alone, the token of the step)."""
    toks = [synth.make_tokens(dims, s + 2, seed=seed + s) for s in range(n)]
    return [[int(t) for t in tk[:-1]] for tk in toks], [int(tk[-1]) for tk in toks]


def oracle_columns(dims, wref, alone, step):
    out = []
    for a, t in zip(alone, step):
        ref = orc.OracleLlama(odesc(dims, CAP), wref)
        for tok in a:
            ref.step(tok, want_logits=False)
        out.append(ref.step(t))
        ref.close()
    return out


_BATCH_BASE = {}


def batch_ties(quant, n_cu):
    """(dims, weights with the copies, the oracle's weights with them, alone, step, winners, sets, expected tokens, the oracle's logits)."""
    dims = tie_dims()
    wseed, tseed = TIE_SEEDS[quant]
    wdev, wref = weights(dims, quant, wseed)
    alone, step = batch_columns(dims, tseed)
    if quant not in _BATCH_BASE:
        _BATCH_BASE[quant] = [orc.argmax(lg) for lg in oracle_columns(dims, wref, alone, step)]   # (does not depend on n_cu)
    winners = _BATCH_BASE[quant]
    assert len(set(winners)) == 8, winners
    deal = Deal(dims.V, n_cu, quant)
    sets = tie_sets(deal, winners)
    wdev2, wref2 = with_copied_rows(dims, quant, wdev, wref, [(x, r) for (x, _), r in zip(sets, winners)])
    logits = oracle_columns(dims, wref2, alone, step)
    expect = check_tied_columns(logits, winners, sets, f"batch ties quant={quant} n_cu={n_cu}")
    return dims, wdev2, wref2, alone, step, winners, sets, expect, logits


# ---- section 3: a greedy chain of eight window columns ----------------------------------------------------------------------------------
CHAIN_KINDS = ("same-unit", "later-pass", "earlier-pass", "other-wave", "later-pass", "same-merge-lane", "row-0", "row-last")
CHAIN_SEEDS = {(False, V_REAL): (21, 504), (True, V_REAL): (21, 504), (False, 512): (21, 500)}
CHAIN_PROMPT = 4   # tokens fed one by one before t0


def chain_ties(quant, V, n_cu):
    """t0 -> a_0 -> ... -> a_7 where a_i is the lowest index of column i's tie set: (dims, weights, the oracle's weights, prompt, t0,
    winners, sets, a).  The hidden states do not depend on the head (untied), so the chain is walked once on the original weights
    and checked as a whole on the final ones."""
    dims = tie_dims(V)
    wseed, tseed = CHAIN_SEEDS[(quant, V)]
    wdev, wref = weights(dims, quant, wseed)
    toks = [int(t) for t in synth.make_tokens(dims, CHAIN_PROMPT + 1, seed=tseed)]
    prompt, t0 = toks[:-1], toks[-1]
    deal = Deal(dims.V, n_cu, quant)
    ref = orc.OracleLlama(odesc(dims, CAP), wref)
    for t in prompt:
        ref.step(t, want_logits=False)
    winners, sets, a, taken, tok = [], [], [], set(), t0
    for i in range(8):
        r = orc.argmax(ref.step(tok))
        assert r not in taken, (i, r)
        x, what = tie_row(deal, r, CHAIN_KINDS[i], taken | {r})
        assert x >= 0, (i, r)
        taken |= {r, x}
        winners.append(r)
        sets.append((x, what))
        tok = min(r, x)
        a.append(tok)
    ref.close()
    wdev2, wref2 = with_copied_rows(dims, quant, wdev, wref, [(x, r) for (x, _), r in zip(sets, winners)])
    # on the final weights: every column's tie set is its maximum by the margin (a copy only adds a non-maximal logit elsewhere)
    ref = orc.OracleLlama(odesc(dims, CAP), wref2)
    for t in prompt:
        ref.step(t, want_logits=False)
    logits = [ref.step(t) for t in [t0] + a[:7]]
    ref.close()
    assert check_tied_columns(logits, winners, sets, f"chain quant={quant} V={V} n_cu={n_cu}") == a
    return dims, wdev2, wref2, prompt, t0, winners, sets, a


def chain_wrong(winners, sets, i):
    """The higher member of column i's tie set: the same logit, the wrong index."""
    return max(int(winners[i]), int(sets[i][0]))


# ---- the tests -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cu", CU_COUNTS)
def test_vocabularies_from_the_cu_count(n_cu):
    """The ragged vocabularies make exactly the deals they are chosen for, and V = 128256 the ones the issue of every model states."""
    v = ragged_vocabs(n_cu)
    d = Deal(v["f16+4"], n_cu, False)
    assert d.nonvacuous() and d.grid == n_cu and d.passes() == (1, 2, 1)          # one wave has two groups, every other wave one
    d = Deal(v["f16+5"], n_cu, False)
    assert d.nonvacuous() and d.passes() == (1, 2, 2) and d.V - 4 * (d.units - 1) == 1   # and the last group has one live row
    assert d.place(d.V - 1) == (1, 0, 1, 0)
    d = Deal(v["mix+16"], n_cu, True)
    assert d.nonvacuous() and d.grid == n_cu and d.passes() == (1, 2, 1)          # one workgroup has two units
    d = Deal(v["f16-wide"], n_cu, False)
    assert d.nonvacuous() and d.passes() == (1, 2, 516)
    d = Deal(v["mix-wide"], n_cu, True)
    assert d.nonvacuous() and v["mix-wide"] % 16 == 0 and v["mix-wide"] >= v["f16-wide"] and d.passes()[1] >= 2
    d = Deal(V_REAL, n_cu, False)
    assert d.nonvacuous() and d.grid == n_cu
    if n_cu == 256:
        assert d.passes() == (15, 16, 1344)                                        # each wave walks 15 or 16 groups
        assert Deal(V_REAL, n_cu, True).passes() == (31, 32, 80)                   # each workgroup has 31 or 32 units
    # at the largest vocabulary of the existing tests neither launch has a second pass on 256 CUs
    assert not Deal(4096, 256, False).nonvacuous() and Deal(4096, 256, False).passes() == (1, 1, 1024)
    assert not Deal(4096, 256, True).nonvacuous() and Deal(4096, 256, True).passes() == (1, 1, 256)


@pytest.mark.parametrize("quant", [False, True], ids=["f16", "mix"])
def test_the_dealing_is_a_bijection(quant):
    for V, n_cu in ((V_REAL, 256), (32 * 256 + (16 if quant else 5), 256), (512, 256)):
        d = Deal(V, n_cu, quant)
        rows = np.arange(V)
        back = [d.row(*d.place(int(r))) for r in rows[:: max(1, V // 997)]]
        assert back == [int(r) for r in rows[:: max(1, V // 997)]]
        assert d.place(V - 1)[0] == d.passes()[1] - 1 or d.passes()[0] == d.passes()[1]
        assert d.row(d.passes()[1], 0, 0, 0) == -1


@pytest.mark.parametrize("n_cu", CU_COUNTS)
@pytest.mark.parametrize("quant", [False, True], ids=["f16", "mix"])
def test_batch_tie_sets(quant, n_cu):
    """Section 2's construction: disjoint sets, the margin, and every placement the one its kind names (no fallback at V = 128256)."""
    dims, _, _, alone, step, winners, sets, expect, _ = batch_ties(quant, n_cu)
    deal = Deal(dims.V, n_cu, quant)
    assert deal.nonvacuous() and deal.grid > 64
    print(f"quant={quant} n_cu={n_cu} winners {winners} copies {sets} expected {expect}")
    assert not any(what.startswith("fallback") or what == "none" for _, what in sets), sets
    own = sum(1 for b in range(8) if expect[b] == winners[b])
    assert own >= 2 and 8 - own >= 2, (expect, winners)          # the winner itself is the lowest index / a copy is
    for b, kind in enumerate(TIE_KINDS):
        r, x = winners[b], sets[b][0]
        (p, g, s, o), (px, gx, sx, ox) = deal.place(r), deal.place(x)
        if kind == "same-unit":
            assert (p, g, s) == (px, gx, sx) and o != ox
        elif kind in ("later-pass", "earlier-pass"):
            assert (g, s, o) == (gx, sx, ox) and (px > p) == (kind == "later-pass") and px != p
            assert (expect[b] == r) == (kind == "later-pass")
        elif kind == "other-wave":
            assert g == gx and ((p == px and s != sx) if not quant else (p != px and o != ox))
        elif kind == "across-order":
            assert g != gx and (min(r, x) == r) == (g > gx)       # the lower row sits in the workgroup with the higher index
        elif kind == "same-merge-lane":
            assert g != gx and g % 64 == gx % 64 and p == px and (min(r, x) == r) == (g < gx)
        elif kind == "row-0":
            assert x == 0 and expect[b] == 0
        else:
            assert x == dims.V - 1 and expect[b] == r
    lower = [deal.place(sets[b][0])[1] < deal.place(winners[b])[1] for b in (4, 5)]
    assert True in lower and False in lower, lower               # a copy in a workgroup with a lower block index, and with a higher one


@pytest.mark.parametrize("quant,V", [(False, 512), (False, V_REAL), (True, V_REAL)], ids=["f16-512", "f16-128256", "mix-128256"])
def test_window_chain_tie_sets(quant, V):
    """Section 3's construction at the CU counts above: the chain is greedy under the lowest-index rule, every column's tie set is its
    maximum by the margin on the final weights, and the drafts that are spoiled (1, 4, 6) have a higher member to be spoiled with."""
    for n_cu in CU_COUNTS:
        dims, _, _, prompt, t0, winners, sets, a = chain_ties(quant, V, n_cu)
        print(f"quant={quant} V={V} n_cu={n_cu}: t0 {t0} chain {a} winners {winners} copies {sets}")
        for i in (1, 4, 6):
            assert chain_wrong(winners, sets, i) > a[i]
        assert len(set(a)) >= 4                                    # (a chain of different tokens)
        if V == V_REAL and n_cu == 256:   # (the placements matter in section 2; here they only have to exist)
            assert not any(what.startswith("fallback") for _, what in sets), sets
