"""Every decode path and the prefill on the GPU under exact power-of-two rescalings of the model (tests/scale_models.py): a producer
times 2^k and its consumers times 2^-k leave the fp32 oracle unchanged BIT FOR BIT (tests/test_scale_sweep.py shows it on the CPU),
so one oracle walk is the expected result at every exponent while the magnitudes the kernels see move by 2^+-k: activations from
2^-17 to one binade under fp16's 65504, fp16 weights down into the subnormals.

Models: tiny-llama and tiny-llama-d128 (weights seed 21, std 0.05, floored at 2^-12; quantised mixes with headers floored at 2^-6),
sequences scale_models.seq_tokens (16 tokens, the first 12 decoded; the prefill test decodes the last 4), KV capacity 32.  One test
per (path, group, model); the exponents of the group's sweep run inside it, 0 first.  Batch members start staggered by two tokens
(member s after 2 (s mod 6) tokens of its own sequence through its own path), then 4 batch steps.

At every exponent:
  * logits (divided by the exact 2^k that head_in / a tied resid put on them) within the path's bar of the oracle: 5e-4 *
    max(1, max|logit|); 2e-2 for the prefill and an fp16 KV cache.  The ArgMax is the first index of the maximum of the returned
    logits and, on the 5e-4 paths, the oracle's unless the oracle's two largest are within twice the tolerance (at most one such step
    per sequence, asserted).  On the 2e-2 paths (prefill, fp16 cache) the ArgMax is NOT compared with the oracle's, as in
    tests/test_gpu_batch_decode.py: twice that tolerance is 4 % of the largest logit, which these random models rarely clear.
    resid moves RMSNorm's eps relative to the stream, so it is compared with an oracle walk of its own per exponent.  At ONE point,
    tiny-llama-d128 resid k = -12, that walk's logits are all under 0.02: the logit bar is the absolute 5e-4, 13 of 16 steps are
    near-ties by the oracle alone, and the logit and ArgMax checks are vacuous there (a lost plane is 0.01 of the bar); only the
    scaled hidden / K / V checks bite.  The near-tie count is waived exactly where every checked oracle logit is under 1.
  * the first and last K and V rows the path wrote and the hidden state, at the scale they are written at: the absolute tolerances
    1e-3 / 2e-2 of the other model tests times 2^-k for K in q_k, 2^k for V in v_wo and for the hidden state in resid.
  * self-consistency: |logits at k - logits at 0| <= 4 DRIFT of the bar, DRIFT being what the CPU restatement of that arithmetic
    moves by over the exponents run (tests/test_scale_sweep.py: 0.008; fp16 cache 0.011; prefill 0.065, at -17 0.35, of their
    bar); whether the run is bit-identical to the one at 0 is printed, not asserted.
Nothing runs above 32768 in an fp16-fed vector: the documented overflow at 65504 is not provoked.

Measured on an MI355X (every test prints one SWEEP line per exponent; this is their worst per path and exponent):
    max|d| / bar, then drift / bar; worst over both models and the groups that run that exponent; '=': every run bit-identical to k = 0
    path                       -17     -12      -6      +0      +6     +10     +11     +12     +17
    all_q8_0 batch4         0.0077  0.0077  0.0077  0.0077  0.0096  0.0085       -  0.0085       -
      drift =               0.0000  0.0000  0.0000  0.0000  0.0000  0.0000       -  0.0000       -
    all_q8_0 single         0.0062  0.0062  0.0062  0.0062  0.0062  0.0072       -  0.0072       -
      drift =               0.0000  0.0000  0.0000  0.0000  0.0000  0.0000       -  0.0000       -
    all_q8_0 window4        0.0071  0.0071  0.0071  0.0071  0.0074  0.0086       -  0.0086       -
      drift =               0.0000  0.0000  0.0000  0.0000  0.0000  0.0000       -  0.0000       -
    f16 batch3              0.0069  0.0069  0.0069  0.0069  0.0096  0.0093  0.0069  0.0069  0.0093
      drift =               0.0000  0.0000  0.0000  0.0000  0.0000  0.0000  0.0000  0.0000  0.0000
    f16 batch3-kv16              -  0.0314  0.0358  0.0314  0.0351  0.0345       -  0.0323  0.0345
      drift                      -  0.0102  0.0007  0.0000  0.0028  0.0032       -  0.0071  0.0000
    f16 batch8              0.0115  0.0115  0.0115  0.0115  0.0119  0.0115  0.0115  0.0115  0.0093
      drift =               0.0000  0.0000  0.0000  0.0000  0.0000  0.0000  0.0000  0.0000  0.0000
    f16 engine              0.0124  0.0124  0.0124  0.0124  0.0124  0.0124  0.0124  0.0124  0.0111
      drift =               0.0000  0.0000  0.0000  0.0000  0.0000  0.0000  0.0000  0.0000  0.0000
    f16 prefill             0.1615  0.0642  0.0642  0.0642  0.0642  0.0642  0.0547  0.0642  0.0423
      drift                 0.1610  0.0580  0.0265  0.0000  0.0000  0.0235  0.0194  0.0377  0.0000
    f16 single              0.0122  0.0122  0.0122  0.0122  0.0122  0.0122  0.0122  0.0122  0.0110
      drift =               0.0000  0.0000  0.0000  0.0000  0.0000  0.0000  0.0000  0.0000  0.0000
    f16 single-kv16              -  0.0346  0.0321  0.0321  0.0322  0.0329       -  0.0321  0.0329
      drift                      -  0.0102  0.0007  0.0000  0.0014  0.0033       -  0.0053  0.0000
    f16 unfused             0.0133  0.0133  0.0133  0.0133  0.0133  0.0133  0.0133  0.0133  0.0107
      drift =               0.0000  0.0000  0.0000  0.0000  0.0000  0.0000  0.0000  0.0000  0.0000
    f16 wide16              0.0117  0.0107  0.0105  0.0103  0.0115  0.0110  0.0105  0.0110  0.0097
      drift                 0.0092  0.0017  0.0012  0.0000  0.0008  0.0012  0.0010  0.0014  0.0000
    f16 wide9               0.0117  0.0107  0.0105  0.0103  0.0115  0.0110  0.0105  0.0107  0.0097
      drift                 0.0074  0.0016  0.0012  0.0000  0.0008  0.0012  0.0009  0.0014  0.0000
    f16 wide9-kv16               -  0.0433  0.0433  0.0432  0.0435  0.0443       -  0.0434  0.0350
      drift                      -  0.0111  0.0014  0.0000  0.0026  0.0042       -  0.0073  0.0000
    f16 window4             0.0120  0.0120  0.0120  0.0120  0.0120  0.0120  0.0120  0.0120  0.0108
      drift =               0.0000  0.0000  0.0000  0.0000  0.0000  0.0000  0.0000  0.0000  0.0000
    f16 window4-kv16             -  0.0343  0.0323  0.0323  0.0323  0.0329       -  0.0323  0.0329
      drift                      -  0.0100  0.0015  0.0000  0.0016  0.0032       -  0.0055  0.0000
    f16 window8             0.0119  0.0119  0.0119  0.0119  0.0119  0.0119  0.0119  0.0119  0.0107
      drift =               0.0000  0.0000  0.0000  0.0000  0.0000  0.0000  0.0000  0.0000  0.0000
    q4_k_m batch4           0.0075  0.0075  0.0075  0.0075  0.0080  0.0083       -  0.0083       -
      drift =               0.0000  0.0000  0.0000  0.0000  0.0000  0.0000       -  0.0000       -
    q4_k_m single           0.0072  0.0072  0.0072  0.0072  0.0073  0.0074       -  0.0074       -
      drift =               0.0000  0.0000  0.0000  0.0000  0.0000  0.0000       -  0.0000       -
    q4_k_m window4          0.0063  0.0063  0.0063  0.0063  0.0078  0.0072       -  0.0072       -
      drift =               0.0000  0.0000  0.0000  0.0000  0.0000  0.0000       -  0.0000       -
    q5_k_m batch4           0.0072  0.0072  0.0072  0.0072  0.0077  0.0079       -  0.0079       -
      drift =               0.0000  0.0000  0.0000  0.0000  0.0000  0.0000       -  0.0000       -
    q5_k_m single           0.0083  0.0083  0.0083  0.0083  0.0083  0.0083       -  0.0083       -
      drift =               0.0000  0.0000  0.0000  0.0000  0.0000  0.0000       -  0.0000       -
    q5_k_m window4          0.0074  0.0074  0.0074  0.0074  0.0074  0.0074       -  0.0074       -
      drift =               0.0000  0.0000  0.0000  0.0000  0.0000  0.0000       -  0.0000       -
The fp16 MFMA takes subnormal A (weights) and B (planes) operands at full value: a core flushing them would be 50 - 3200 bars off
(tests/test_scale_sweep.py).  No path failed; nothing in the kernels had to change.
"""
import functools

import numpy as np
import pytest

from nfai_amd import synth

import scale_models as sm
from test_gpu_batch_decode import check_step, logit_tol
from test_scale_sweep import DRIFT, DRIFT_KV16, DRIFT_PREFILL, DRIFT_PREFILL_17, KV16_GROUPS, KV16_RANGE, PREFILL_RANGE, ranged

pytestmark = pytest.mark.gpu

MODELS = [synth.TINY, synth.TINY_D128]
BY_NAME = {d.name: d for d in MODELS}
STEPS = 4   # batch steps behind the staggered start


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


def ddict(d):
    return dict(E=d.E, L=d.L, H=d.H, Hkv=d.Hkv, D=d.D, F=d.F, V=d.V, eps=1e-5, rope_dims=d.D, rope_base=500000.0)


def alone(s):
    return 2 * (s % 6)


@functools.lru_cache(maxsize=None)
def base(name, mix):
    """(what the model loads, what the oracle computes on, the exponents of every group)."""
    dims = BY_NAME[name]
    if mix is None:
        w = sm.floor_weights(synth.make_weights(dims, seed=21, std=0.05))
        maxima = sm.activation_maxima(dims, w, [sm.seq_tokens(dims, s) for s in range(16)])
        return w, w, {g: sm.sweep(g, maxima, sm.wmax_of(w)) for g in sm.GROUPS}
    return sm.quant_base(dims, mix)   # sweeps: exact header products, fed vectors of sequences 0 .. 3 at or below 32768


@functools.lru_cache(maxsize=None)
def reference(name, mix, group, k, s):
    """Sequence s through the oracle: on the base for the exact groups (k is then always 0), on the rescaled weights for resid."""
    dims = BY_NAME[name]
    wdev, wref, _ = base(name, mix)
    if group == "resid" and k != 0:
        wref = sm.dequantised(sm.rescale(wdev, dims, group, k), (wdev, wref)) if mix else sm.rescale(wdev, dims, group, k)
    return sm.oracle_walk(dims, wref, sm.seq_tokens(dims, s))


def model(mgr, dims, wdev, mix, **kw):
    from nfai_amd.llama_model import LlamaModel
    if mix:
        kw.setdefault("dims", ddict(dims))
    return LlamaModel(mgr, synth.make_metadata(dims), wdev, sm.CAP, **kw)


# ---- the paths: each returns [(sequence, first position, logits [steps][V], argmax [steps], model)] and what to dispose ----------------
def run_single(mgr, dims, wdev, mix, **kw):
    m = model(mgr, dims, wdev, mix, **kw)
    out = [m.Step(t) for t in sm.seq_tokens(dims, 0)[:sm.N_TOK]]
    return [(0, 0, np.stack([lg for lg, _ in out]), [am for _, am in out], m)], [m]


def run_batch(mgr, dims, wdev, mix, n, wide=False, **kw):
    from nfai_amd.llama_model import LlamaBatch
    ms = [model(mgr, dims, wdev, mix, **kw)]
    ms += [model(mgr, dims, wdev, mix, share_from=ms[0], **kw) for _ in range(1, n)]
    toks = [sm.seq_tokens(dims, s) for s in range(n)]
    for s in range(n):
        for t in toks[s][:alone(s)]:
            ms[s].Step(t, want_logits=False)
    batch = LlamaBatch(ms, wide=True) if wide else LlamaBatch(ms, quantized=bool(mix), any_quant=bool(mix))
    lgs, ams = [], []
    for i in range(STEPS):
        lg, am = batch.Step([toks[s][alone(s) + i] for s in range(n)])
        lgs.append(lg)
        ams.append(am)
    return [(s, alone(s), np.stack([lg[s] for lg in lgs]), [int(am[s]) for am in ams], ms[s]) for s in range(n)], [batch] + ms[::-1]


def run_window(mgr, dims, wdev, mix, T, **kw):
    from nfai_amd.llama_model import LlamaWindow
    m = model(mgr, dims, wdev, mix, **kw)
    toks = sm.seq_tokens(dims, 0)
    for t in toks[:4]:
        m.Step(t, want_logits=False)
    win = LlamaWindow(m, T, quantized=bool(mix), any_quant=bool(mix))
    lgs, ams = [], []
    for p in range(4, sm.N_TOK, T):
        lg, am = win.Step(toks[p:p + T])
        lgs.append(lg)
        ams += [int(a) for a in am]
    return [(0, 4, np.concatenate(lgs), ams, m)], [win, m]


def run_prefill(mgr, dims, wdev, mix, **kw):
    m = model(mgr, dims, wdev, mix, max_batch=64, **kw)
    toks = sm.seq_tokens(dims, 0)
    lgs = [m.Prefill(toks[:sm.N_TOK])]
    ams = [int(np.argmax(lgs[0]))]   # (the prefill returns no token)
    for t in toks[sm.N_TOK:]:
        lg, am = m.Step(t)
        lgs.append(lg)
        ams.append(am)
    return [(0, sm.N_TOK - 1, np.stack(lgs), ams, m)], [m]


FP16_PATHS = {
    "single": (run_single, {}), "unfused": (run_single, dict(unfused=True)), "engine": (run_single, dict(engine=True)),
    "batch3": (run_batch, dict(n=3)), "batch8": (run_batch, dict(n=8)),
    "wide9": (run_batch, dict(n=9, wide=True)), "wide16": (run_batch, dict(n=16, wide=True)),
    "window4": (run_window, dict(T=4)), "window8": (run_window, dict(T=8)), "prefill": (run_prefill, {}),
}
KV16_PATHS = ("single", "batch3", "wide9", "window4")
QUANT_PATHS = {"single": (run_single, {}), "batch4": (run_batch, dict(n=4)), "window4": (run_window, dict(T=4))}


def sweep_path(mgr, name, mix, group, path, runner, kw, ks, scale, drift, atol):
    """drift: the restatement's, a number or a function of the exponent."""
    dims = BY_NAME[name]
    wdev, _, _ = base(name, mix)
    assert 0 in ks
    at0, worst = {}, (0.0, 0.0)
    for k in [0] + [k for k in ks if k != 0]:
        wk = sm.rescale(wdev, dims, group, k)
        f = np.float32(sm.logit_factor(dims, group, k))
        fk, fv, fh = sm.state_factors(group, k)
        runs, owned = runner(mgr, dims, wk, mix, **kw)
        try:
            e_max = d_max = 0.0
            same = True
            for s, first, lg, am, m in runs:
                own = group == "resid"   # compared with the oracle's walk on the rescaled weights, which carries the factors itself
                want, hidden, K, V = reference(name, mix, group, k if own else 0, s)
                lg = lg / f
                excluded = [0]
                for i in range(len(lg)):
                    w = want[first + i] / f if own else want[first + i]
                    e_max = max(e_max, float(np.abs(lg[i] - w).max()) / logit_tol(w, scale))
                    check_step([lg[i]], [am[i]], [w], scale, f"{path} {group} k {k:+d} seq {s} pos {first + i}",
                               oracle_argmax=scale == 5e-4, excluded=excluded)
                    if group != "resid":
                        if k == 0:
                            at0[(s, i)] = lg[i].copy()
                        d = float(np.abs(lg[i] - at0[(s, i)]).max()) / logit_tol(w, scale)
                        d_max = max(d_max, d)
                        same = same and np.array_equal(lg[i].view(np.uint32), at0[(s, i)].view(np.uint32))
                # The one waiver, decided by the oracle alone: resid far down is RMSNorm's eps over a vanishing stream, and where
                # every checked logit of the oracle is under 1 the tolerance is the absolute 5e-4 and nearly every step is a near-tie.
                vacuous = own and max(float(np.abs(want[first + i]).max()) / float(f) for i in range(len(lg))) < 1.0
                assert excluded[0] <= 1 or vacuous, (path, group, k, s, excluded)
                last = first + len(lg) - 1
                assert m.Pos == last + 1
                for l in range(dims.L):
                    for p in (first, last):   # the first and the last row the path wrote
                        np.testing.assert_allclose(m.ReadKV(l, False, p), K[l][p] * np.float32(fk), rtol=0, atol=atol * fk)
                        np.testing.assert_allclose(m.ReadKV(l, True, p), V[l][p] * np.float32(fv), rtol=0, atol=atol * fv)
                np.testing.assert_allclose(m.Read(0, dims.E), hidden[last] * np.float32(1.0 if own else fh), rtol=0, atol=atol * fh)
        finally:
            for o in owned:
                o.Dispose()
        print(f"SWEEP {name} {mix or 'f16'} {path} {group} k {k:+3d}: max|d|/bar {e_max:.4f}  drift/bar {d_max:.5f}"
              + ("" if group == "resid" else f"  bit-identical to k = 0: {'yes' if same else 'no'}"))
        bound = 4 * (drift(k) if callable(drift) else drift)
        assert d_max <= bound, (path, group, k, d_max, bound)
        worst = (max(worst[0], e_max), max(worst[1], d_max))
    print(f"WORST {name} {mix or 'f16'} {path} {group}: max|d|/bar {worst[0]:.4f}  drift/bar {worst[1]:.5f}")


CASES = [pytest.param(d.name, g, id=f"{d.name}-{g}") for d in MODELS for g in sm.GROUPS]


@pytest.mark.parametrize("name,group", CASES)
@pytest.mark.parametrize("path", list(FP16_PATHS))
def test_fp16_paths(mgr, path, name, group):
    runner, kw = FP16_PATHS[path]
    ks = base(name, None)[2][group]
    if path == "prefill":
        sweep_path(mgr, name, None, group, path, runner, kw, ranged(PREFILL_RANGE, name, group, ks), 2e-2,
                   lambda k: DRIFT_PREFILL_17 if k == -17 else DRIFT_PREFILL, 2e-2)
    else:
        sweep_path(mgr, name, None, group, path, runner, kw, ks, 5e-4, DRIFT, 1e-3)


@pytest.mark.parametrize("name,group", [c for c in CASES if c.values[1] in KV16_GROUPS])
@pytest.mark.parametrize("path", KV16_PATHS)
def test_fp16_paths_with_an_fp16_kv_cache(mgr, path, name, group):
    runner, kw = FP16_PATHS[path]
    ks = ranged(KV16_RANGE, name, group, base(name, None)[2][group])
    sweep_path(mgr, name, None, group, path + "-kv16", runner, dict(kw, kv_f16=True), ks, 2e-2, DRIFT_KV16, 2e-2)


@pytest.mark.parametrize("name,group", CASES)
@pytest.mark.parametrize("path", list(QUANT_PATHS))
@pytest.mark.parametrize("mix", sm.QUANT_MIXES)
def test_quantised_paths(mgr, mix, path, name, group):
    runner, kw = QUANT_PATHS[path]
    sweep_path(mgr, name, mix, group, path, runner, kw, base(name, mix)[2][group], 5e-4, DRIFT, 1e-3)
