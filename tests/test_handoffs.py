"""tests/handoffs.py on the CPU: the oracle walk does not depend on how a sequence is cut into segments, every wrong hand-off the
helper models would be seen by the GPU cases' bars, every greedy token of every case leads by the required gap, and every ordered
pair of kinds is run somewhere or excluded by a refusal of the library.

Measured (printed by the tests; DESIGN.md lists them): smallest wrong-model margin over both models and all pairs, logits and K rows;
smallest greedy lead."""
import numpy as np
import pytest

import handoffs as ho
import oracle as orc

MODELS = ("f16", "q4km")   # the engine configuration runs the f16 model's weights: the same arithmetic


def test_the_walk_does_not_depend_on_the_cut():
    """The tokens a case feeds, fed to a fresh oracle one by one, give bit-identical logits, hidden states and K / V rows: the walk's
    own bookkeeping (greedy feedback, the token word an E continues from, Verify's accepted drafts, the rewind) adds nothing.  A
    rewind feeds again exactly the tokens of the positions it goes back over."""
    for name in ("f16", "q4km"):
        cfg = ho.CONFIGS[name]
        picked = [(i, a, b) for i, a, b in ho.pairs(cfg) if (a, b) in (("G", "E"), ("V", "Z"), ("Z", "V"), ("I", "E"), ("BG", "W"), ("E", "G"))]
        assert len(picked) == 6
        for i, a, b in picked:
            ref = ho.case(cfg, i, a, b)
            one = orc.OracleLlama(ho.odesc(cfg), ho.weights(cfg)[1])
            for p, t in enumerate(ref.toks):
                np.testing.assert_array_equal(one.step(t), ref.logits[p])
                np.testing.assert_array_equal(one.hidden(), ref.hidden[p])
            for l in range(cfg.dims.L):
                np.testing.assert_array_equal(one.kcache(l)[:len(ref.toks)], ref.K[l])
                np.testing.assert_array_equal(one.vcache(l)[:len(ref.toks)], ref.V[l])
            one.close()
            pos = 0
            for s in ref.segs:
                assert s.start == (pos - s.r if s.kind == "Z" else pos) and s.fed == ref.toks[s.start:s.start + len(s.fed)], (name, a, b, s)
                pos += s.n
                if s.kind in ho.GREEDY:
                    assert s.emitted == [ref.am[q] for q in range(s.start, s.start + s.n)]
                if s.kind == "V":
                    assert s.n == s.a + 1 and len(s.drafts) == s.k and s.drafts[:s.a] == s.emitted[:s.a]
                    assert s.a == s.k or s.drafts[s.a] != s.emitted[s.a]
            assert pos == len(ref.toks)


@pytest.mark.parametrize("name", MODELS)
def test_every_wrong_handoff_moves_the_logits_and_the_first_k_row(name):
    """Each wrong model of tests/handoffs.py, on the fp64 NumPy oracle, against the same oracle run right: the logits of B's last token
    move by at least WRONG_BARS logits bars and the K row B's first token writes (the block where it moves most) by as many row bars;
    the bars are the loosest any GPU case applies to the pair."""
    cfg = ho.CONFIGS[name]
    wref = ho.weights(cfg)[1]
    worst = {}
    for i, a, b in ho.pairs(cfg):
        ref = ho.case(cfg, i, a, b)
        scale, atol = ho.pair_bar(a, b)
        runs = ho.wrong_runs(cfg, ref, wref)
        lg0, k0 = runs.pop("exact")
        # the fp64 model run right is the case's oracle to far less than a bar
        segB = ref.segs[2]
        last = segB.start + len(segB.fed) - 1
        assert float(np.abs(lg0 - ref.logits[last]).max()) < 0.05 * cfg.scale * max(1.0, float(np.abs(lg0).max()))
        for w, (lg, k) in runs.items():
            ml = float(np.abs(lg - lg0).max()) / (scale * max(1.0, float(np.abs(lg0).max())))
            mk = max(float(np.abs(k[l] - k0[l]).max()) for l in range(cfg.dims.L)) / atol
            for key, v in ((w + " logits", ml), (w + " K row", mk)):
                if v < worst.get(key, (np.inf,))[0]:
                    worst[key] = (v, f"{a}->{b}")
    for key in sorted(worst):
        print(f"{name}: {key}: smallest margin {worst[key][0]:.1f} bars at {worst[key][1]}")
    low = min(worst.values())
    print(f"{name}: smallest wrong-model margin {low[0]:.2f} bars ({low[1]})")
    assert set(k.rsplit(" ", 2 if k.endswith("K row") else 1)[0] for k in worst) == set(ho.WRONG)
    assert low[0] >= ho.WRONG_BARS, worst


@pytest.mark.parametrize("name", list(ho.CONFIGS))
def test_every_greedy_token_leads_by_the_gap(name):
    """No case waives a token: every token a greedy kind emits, and every token word an E continues from, leads the runner-up by at
    least GAP_BARS bars of the segment that must reproduce it.  Also the shapes the cases promise: W and V use all 8 columns at least
    once, P and I cross a chunk boundary once, every count is in its range."""
    cfg = ho.CONFIGS[name]
    low, n_must = np.inf, 0
    w8 = v8 = long_p = long_i = False
    for i, a, b in ho.pairs(cfg):
        ref = ho.case(cfg, i, a, b)
        low = min(low, ho.case_bars(cfg, ref))
        n_must += len(ref.must)
        assert [s.kind for s in ref.segs] == ["S", a, b, "S"] and ref.segs[0].n == 3 + i % 5 and ref.segs[3].n == 1
        for s in ref.segs[1:3]:
            m = s.r if s.kind == "Z" else (s.k + 1 if s.kind == "V" else s.n)
            assert (m == ho.LONG or 5 <= m <= 20) if s.kind in ho.MFMA else 2 <= m <= 9, (a, b, s.kind, m)
            w8 |= s.kind == "W" and s.n == 8
            v8 |= s.kind == "V" and s.k == 7
            long_p |= s.kind == "P" and s.n == ho.LONG
            long_i |= s.kind == "I" and s.n == ho.LONG
        assert len(ref.toks) < ho.CAP - 2
    print(f"{name}: {n_must} tokens the GPU must reproduce, smallest lead {low:.2f} bars")
    assert low >= ho.GAP_BARS
    assert long_p and long_i and (("W" not in cfg.kinds) or (w8 and v8))


def test_every_ordered_pair_is_run_or_refused():
    run, out = ho.coverage()
    per = {c.name: len(ho.pairs(c)) for c in ho.CONFIGS.values()}
    print(f"pairs of kinds run on at least one configuration: {len(run)} of {len(ho.KINDS) ** 2}; excluded by a refusal: {len(out)}; "
          f"cases per configuration: {per}")
    assert len(run) + len(out) == len(ho.KINDS) ** 2 and not (run & set(out))
    for cfg in ho.CONFIGS.values():     # a configuration leaves a kind out only with the refusal that forbids it
        assert set(cfg.kinds) | set(cfg.refused) == set(ho.KINDS) and not set(cfg.kinds) & set(cfg.refused)
    assert set(ho.CONTRACT) == set(ho.KINDS)
