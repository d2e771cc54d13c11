"""What tests/test_gpu_scale_sweep.py rests on, re-measured on the CPU on every run (tests/scale_models.py holds the rescalings).

For tiny-llama and tiny-llama-d128 (weights seed 21, std 0.05, floored at 2^-12; sequence 0 of scale_models.seq_tokens, 16 tokens) and
every group, at every exponent of the group's sweep:

  1. the oracle on the rescaled weights is BIT-IDENTICAL to the oracle on the floored base (head_in: after the exact undo), so the GPU
     test needs one expected vector per step.  (resid is not exact - RMSNorm's eps - and is compared with its own walk.)
  2. the float32 restatement of the wide batch's arithmetic, against the decode bar 5e-4 * max(1, max|logit|):
       hi + 2^-11 lo as stated                      under HALF the bar at every exponent;
       hi only (a lost plane)                       over the WHOLE bar at at least one exponent of every group;
       the split with fp16 subnormals flushed       over the WHOLE bar at every exponent |k| >= 10 at which the group scales an fp16
       (weights and both planes)                    operand DOWN (head_in and resid: the negative ones; the others: both signs).
     The GPU test therefore tells the three apart.
  3. DRIFT: the largest difference between the restatement's own base run and any of its rescaled runs, as a fraction of the bar.
     Only the subnormal behaviour of the split moves it.  The GPU test's self-consistency bound is 4 DRIFT.
  4. Quantised models (Q4_K_M mix, Q5_K_M mix, all Q8_0; headers floored at 2^-6): the oracle on the dequantised rescaled blocks is
     bit-identical to the base at the exponents at which the header products are exact.
  5. The prefill (GEMV inputs and q / K / V rows rounded to fp16) and an fp16 KV cache (K / V rows rounded to fp16): the exponents at
     which their restatements stay under half of 2e-2 * max(1, max|logit|) and their hidden state and K / V rows within the GPU test's
     2e-2 tolerance: PREFILL_RANGE and KV16_RANGE.  (tiny-llama-d128 at -17 in qkv_in / gateup_in: the prefill's subnormal fp16 inputs
     put the state 2.5 - 4 tolerances off; its lower end is -12.)

Measured: see the tables printed by the tests; the worst values are asserted below."""
import functools

import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth

import scale_models as sm

try:   # the restatement's products are small: one BLAS thread does them as fast as many, without spinning the others
    import threadpoolctl
    _one_thread = threadpoolctl.threadpool_limits(1)
except ImportError:
    pass

MODELS = [synth.TINY, synth.TINY_D128]
BY_NAME = {d.name: d for d in MODELS}
BAR, BAR16 = 5e-4, 2e-2

# the largest |restatement at k - restatement at 0| / bar over both models, every exact group and every exponent (asserted below)
DRIFT = 0.008
# the same for the restatements of the prefill and of an fp16 KV cache, as fractions of THEIR bar, 2e-2 * max(1, max|logit|)
# (the prefill: at -17, where its fp16 inputs are subnormal, and from -12 up)
DRIFT_PREFILL_17, DRIFT_PREFILL = 0.35, 0.065
DRIFT_KV16 = 0.011

# (model, group) -> (lowest, highest) exponent of the sweep at which the restatement stays under half of the 2e-2 bar (asserted below)
# Every exponent of every sweep is kept: the worst are 0.34 (prefill, tiny-llama qkv_in at -17) and 0.04 (fp16 cache) of the bar.
KV16_GROUPS = ("q_k", "v_wo", "resid")
PREFILL_RANGE = {(n, g): (-17 if g in ("qkv_in", "gateup_in", "head_in") else -12, 17 if g == "resid" else 12)
                 for n in ("tiny-llama", "tiny-llama-d128") for g in sm.GROUPS}
PREFILL_RANGE[("tiny-llama-d128", "up_down")] = (-12, 11)
PREFILL_RANGE[("tiny-llama-d128", "qkv_in")] = PREFILL_RANGE[("tiny-llama-d128", "gateup_in")] = (-12, 12)   # -17: the state is 2.5 - 4 x off
KV16_RANGE = {key: r for key, r in PREFILL_RANGE.items() if key[1] in KV16_GROUPS}


def bar_of(want, scale):
    return scale * max(1.0, float(np.abs(want).max()))


@functools.lru_cache(maxsize=None)
def base(name):
    """(floored weights, maxima over the 16 sequences the GPU test uses, largest |weight|, sequence 0, its oracle logits)."""
    dims = BY_NAME[name]
    w = sm.floor_weights(synth.make_weights(dims, seed=21, std=0.05))
    maxima = sm.activation_maxima(dims, w, [sm.seq_tokens(dims, s) for s in range(16)])
    toks = sm.seq_tokens(dims, 0)
    return w, maxima, sm.wmax_of(w), toks, sm.oracle_walk(dims, w, toks)[0]


def walk(dims, w, toks, arith, rows="", state=None):
    """The restatement's logits per step; `state` (a list) also receives (hidden state per step, K caches, V caches)."""
    r = sm.Walk(dims, w, arith, rows, cap=len(toks))
    out, hidden = [], []
    for t in toks:
        out.append(r.step(t))
        hidden.append(r.x.copy())
    if state is not None:
        state += [hidden, r.K, r.V]
    return out


def state_error(state, ref, group, k):
    """The largest error of the hidden states and of the K / V rows against the oracle walk `ref` on the same weights, as a fraction of
    the GPU test's absolute tolerance for an fp16 path: 2e-2 times the power of two the group writes that quantity at."""
    fk, fv, fh = sm.state_factors(group, k)
    (hidden, K, V), (_, hidden0, K0, V0) = state, ref
    e = max(float(np.abs(a - b).max()) for a, b in zip(hidden, hidden0)) / fh
    e = max(e, max(float(np.abs(a - b).max()) for a, b in zip(K, K0)) / fk, max(float(np.abs(a - b).max()) for a, b in zip(V, V0)) / fv)
    return e / BAR16


def worst(got, want, f, scale):
    """max over the steps of |got / f - want / f| / bar(want / f)."""
    return max(float(np.abs(g / f - w / f).max()) / bar_of(w / f, scale) for g, w in zip(got, want))


@functools.lru_cache(maxsize=None)
def measure(name, group):
    """Per exponent of the sweep: oracle bit-identity and the restatements' errors as fractions of their bars."""
    dims = BY_NAME[name]
    w, maxima, wmax, toks, want0 = base(name)
    ks = sm.sweep(group, maxima, wmax)
    split0 = walk(dims, w, toks, "split")
    out = {}
    for k in ks:
        wk = sm.rescale(w, dims, group, k)
        f = np.float32(sm.logit_factor(dims, group, k))
        ref = sm.oracle_walk(dims, wk, toks)
        want = ref[0]
        identical = all(np.array_equal((a / f).view(np.uint32), b.view(np.uint32)) for a, b in zip(want, want0))
        w32 = {n: np.asarray(a, np.float32) for n, a in wk.items()}   # widened once for the five walks
        runs = {a: walk(dims, w32, toks, a) for a in ("split", "hi", "flush")}
        st = {"prefill": [], "kv16": []}
        runs16 = {"prefill": walk(dims, w32, toks, "hi", "qkv", st["prefill"]), "kv16": walk(dims, w32, toks, "split", "kv", st["kv16"])}
        if k == 0:
            base16 = runs16

        def drift(run, run0, scale):
            if group == "resid":
                return 0.0
            return max(float(np.abs(g / f - g0).max()) / bar_of(w0, scale) for g, g0, w0 in zip(run, run0, want0))

        out[k] = dict(identical=identical, **{a: worst(runs[a], want, f, BAR) for a in runs},
                      **{a: worst(runs16[a], want, f, BAR16) for a in runs16},
                      **{a + "_state": state_error(st[a], ref, group, k) for a in st}, drift=drift(runs["split"], split0, BAR), runs16=runs16)
    for k in ks:
        for a in ("prefill", "kv16"):
            f = np.float32(sm.logit_factor(dims, group, k))
            out[k]["drift_" + a] = 0.0 if group == "resid" else max(
                float(np.abs(g / f - g0).max()) / bar_of(w0, BAR16) for g, g0, w0 in zip(out[k]["runs16"][a], base16[a], want0))
        del out[k]["runs16"]
    return out


def kept(m, what):
    return [k for k in sorted(m) if m[k][what] < 0.5 and m[k][what + "_state"] < 1.0]


CASES = [pytest.param(d.name, g, id=f"{d.name}-{g}") for d in MODELS for g in sm.GROUPS]


@pytest.mark.parametrize("name,group", CASES)
def test_oracle_is_bit_identical_and_the_bar_separates_the_three(name, group):
    m = measure(name, group)
    _, maxima, wmax, _, _ = base(name)
    print(f"{name} {group}: sweep {sorted(m)} (top {max(m)}); maxima " + " ".join(f"{k} {v:.2f}" for k, v in sorted(maxima.items()))
          + f"; max|W| {wmax:.3f}")
    for k in sorted(m):
        r = m[k]
        print(f"  k {k:+3d}: oracle {'bit-identical' if r['identical'] else 'own walk'}  split {r['split']:.4f}  hi only {r['hi']:.2f}  "
              f"flushed {r['flush']:.2f}  drift {r['drift']:.4f}  | of the 2e-2 bar: prefill {r['prefill']:.3f} (state {r['prefill_state']:.3f})  "
              f"kv16 {r['kv16']:.3f} (state {r['kv16_state']:.3f})")
    down_sides = (lambda k: k < 0) if group in ("head_in", "resid") else (lambda k: True)
    for k, r in m.items():
        assert r["identical"] == (group != "resid" or k == 0), (k, r)
        assert r["split"] < 0.5, (k, r)
        assert r["drift"] <= DRIFT, (k, r)
        if abs(k) >= 10 and down_sides(k):
            assert r["flush"] > 1.0, (k, r)
    assert max(r["hi"] for r in m.values()) > 1.0, m
    assert {-6, 0, 6, 10} <= set(m) and min(m) <= -12 and max(m) >= 11, sorted(m)


def test_the_tops_are_derived_from_the_maxima():
    """One binade under 65504: the top of a sweep is the last exponent at which max |x| 2^k <= 32768 for every fp16-fed vector of the
    group, and one more breaks it (or the exactness of a matrix scaled down by 2^-12)."""
    for dims in MODELS:
        _, maxima, wmax, _, _ = base(dims.name)
        tops = {g: max(sm.sweep(g, maxima, wmax)) for g in sm.GROUPS}
        print(f"{dims.name}: tops {tops}")
        for g, top in tops.items():
            assert sm.allowed(g, maxima, wmax, top) and not sm.allowed(g, maxima, wmax, top + 1)
            for kind, sign in sm._FED[g]:
                assert maxima[kind] * 2.0 ** (sign * top) <= sm.CEILING
    with pytest.raises(ValueError):   # a matrix scaled below its floor is refused, not rounded
        sm.rescale(base("tiny-llama")[0], synth.TINY, "q_k", -17)


def test_drift_constant():
    """Over the exponents the GPU test runs (the prefill's: PREFILL_RANGE)."""
    for what, stated, pick in (("drift", DRIFT, lambda k: True), ("drift_prefill", DRIFT_PREFILL_17, lambda k: k == -17),
                               ("drift_prefill", DRIFT_PREFILL, lambda k: k > -17), ("drift_kv16", DRIFT_KV16, lambda k: True)):
        seen = max(r[what] for d in MODELS for g in sm.EXACT_GROUPS for k, r in measure(d.name, g).items()
                   if pick(k) and (what != "drift_prefill" or PREFILL_RANGE[(d.name, g)][0] <= k <= PREFILL_RANGE[(d.name, g)][1]))
        print(f"{what} measured {seen:.5f}, stated {stated}")
        assert stated / 2 <= seen <= stated


@pytest.mark.parametrize("name,group", CASES)
def test_prefill_and_fp16_cache_ranges(name, group):
    m = measure(name, group)
    for what, table in (("prefill", PREFILL_RANGE), ("kv16", KV16_RANGE)):
        if what == "kv16" and group not in KV16_GROUPS:
            continue
        ks = kept(m, what)
        print(f"{name} {group} {what}: kept {ks} of {sorted(m)}")
        lo, hi = table[(name, group)]
        assert ks == [k for k in sorted(m) if lo <= k <= hi], (what, ks, lo, hi)
        assert 0 in ks


def ranged(table, name, group, ks):
    lo, hi = table[(name, group)]
    return [k for k in ks if lo <= k <= hi]


@pytest.mark.parametrize("mix", sm.QUANT_MIXES)
@pytest.mark.parametrize("dims", MODELS, ids=lambda d: d.name)
def test_quantised_oracle_is_bit_identical_under_header_rescaling(dims, mix):
    wq, wref, sweeps = sm.quant_base(dims, mix)   # the sweeps keep only exact products and fed vectors at or below 32768
    toks = sm.seq_tokens(dims, 0)[:sm.N_TOK]
    want0 = sm.oracle_walk(dims, wref, toks)[0]
    for group in sm.EXACT_GROUPS:
        ks = sweeps[group]
        assert {-6, 0, 6} <= set(ks), (group, ks)   # matrices: the header floor; a group that scales only a gain down goes further
        for k in ks:
            f = np.float32(sm.logit_factor(dims, group, k))
            want = sm.oracle_walk(dims, sm.dequantised(sm.rescale(wq, dims, group, k), (wq, wref)), toks)[0]
            assert all(np.array_equal((a / f).view(np.uint32), b.view(np.uint32)) for a, b in zip(want, want0)), (group, k)
    print(f"{dims.name} {mix}: bit-identical at {sweeps}")
