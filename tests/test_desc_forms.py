"""CPU side of tests/test_gpu_desc_forms.py: the oracle alone under the descriptor forms of tests/desc_forms.py.

1. For every form, on tiny-llama and tiny-llama-d128, the C oracle (fp32) and oracle.np_oracle (fp64) agree at the tolerance of
   tests/test_oracle.py::test_whole_model_vs_fp64, 2e-4 * max|logit|, at every position of the run (48 / 100 positions, the token
   counts of the GPU test), and in the K rows of the last position.
2. Sensitivity, between oracles only: each wrong model of desc_forms.mutants (the switch ignored; rope_dims replaced by D; the
   frequencies formed with D / 2; eps replaced by 1e-5; the full table) must move the quantities the GPU test compares, the
   logits and the K row of every block at the last position of the run, by at least 5 of the GPU test's bars.  There are two sets
   of bars: the fp32-KV decode's (5e-4 * max(1, max|logit|) on logits, 1e-3 on K rows) and the fp16-KV / prefill ones (2e-2 *
   max(1, max|logit|) on logits, 2e-2 on K rows).  For K rows the margin is the smallest over the blocks.  Every margin is printed.
   5 bars are required of every one of them, against both sets of bars.

Forms changed because a margin failed, never the bar (tests/desc_forms.py states each with its figures): six carries eps = 1e-3, not
1e-6; cut carries base 1000, not 500000; ref32 carries base 10000, not 500000.  The smallest margins now: 5.7 bars (six, the
frequencies formed with D / 2, fp16-KV / prefill logits on tiny-llama) and 9.8 (none, eps, the same bar); DESIGN.md lists all.
The weights are the GPU test's: make_weights(seed 21, std 0.05); the tokens desc_forms.tokens."""
import functools

import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth

import desc_forms as df

MODELS = [synth.TINY, synth.TINY_D128]
BY_NAME = {d.name: d for d in MODELS}
BARS = {"decode": (5e-4, 1e-3), "kv16/prefill": (2e-2, 2e-2)}   # (logit scale, K row atol) of the GPU paths
NEED = 5.0


@functools.lru_cache(maxsize=None)
def weights(name):
    return synth.make_weights(BY_NAME[name], seed=21, std=0.05)


@functools.lru_cache(maxsize=None)
def np_walk(name, form, mutation):
    """(logits [N][V], K rows of the last position [L][Hkv D]) of the fp64 model: the form itself (mutation None) or a mutant."""
    dims = BY_NAME[name]
    rd, freqs, eps = df.exact(form, dims) if mutation is None else df.mutants(form, dims)[mutation]
    toks = df.tokens(dims)
    m = df.NpModel(dims, weights(name), len(toks), rd, freqs, eps)
    logits = np.stack([m.step(t) for t in toks])
    return logits, np.stack([m.K[l][len(toks) - 1] for l in range(dims.L)])


CASES = [pytest.param(d.name, f, id=f"{d.name}-{f}") for d in MODELS for f in df.forms_for(d)]


@pytest.mark.parametrize("name,form", CASES)
def test_c_oracle_agrees_with_fp64_under_the_form(name, form):
    dims = BY_NAME[name]
    toks = df.tokens(dims)
    want, wantK = np_walk(name, form, None)
    ref = orc.OracleLlama(df.odesc(dims, form, len(toks)), weights(name))
    worst = 0.0
    for i, t in enumerate(toks):
        lg = ref.step(t)
        tol = 2e-4 * float(np.abs(want[i]).max())
        worst = max(worst, float(np.abs(lg - want[i]).max()) / tol)
        np.testing.assert_allclose(lg, want[i], rtol=0, atol=tol, err_msg=f"position {i}")
        assert orc.argmax(lg) == int(np.argmax(want[i])) or np.partition(want[i], -2)[-1] - np.partition(want[i], -2)[-2] <= 2 * tol, i
    for l in range(dims.L):
        got = ref.kcache(l)[len(toks) - 1]
        np.testing.assert_allclose(got, wantK[l], rtol=0, atol=2e-4 * float(np.abs(wantK[l]).max()))
    ref.close()
    print(f"AGREE {name} {form}: worst |d logit| / (2e-4 max|logit|) {worst:.3f} over {len(toks)} positions")


def margins(name, form, mutation):
    """{bar class: (logit margin, K margin)} of one mutant, in bars, at the last position of the run."""
    want, wantK = np_walk(name, form, None)
    got, gotK = np_walk(name, form, mutation)
    out = {}
    for cls, (scale, atol) in BARS.items():
        bar = scale * max(1.0, float(np.abs(want[-1]).max()))
        out[cls] = (float(np.abs(got[-1] - want[-1]).max()) / bar, min(float(np.abs(gotK[l] - wantK[l]).max()) for l in range(len(wantK))) / atol)
    return out


@pytest.mark.parametrize("name,form", CASES)
def test_every_wrong_model_moves_what_the_gpu_test_compares(name, form):
    dims = BY_NAME[name]
    muts = df.mutants(form, dims)
    rd, nf, base, eps = df.resolve(form, dims)
    assert "default" in muts and ("eps" in muts) == (eps != 1e-5) and ("full" in muts) == (nf < rd // 2)
    assert ("denom_D" in muts) == (0 < rd < dims.D) and ("dims_D" in muts) == (rd < dims.D)
    low = []
    for mutation in muts:
        for cls, (ml, mk) in margins(name, form, mutation).items():
            print(f"MARGIN {name} {form} {mutation:8s} {cls:12s}: logits {ml:9.1f} bars   K rows (smallest block) {mk:9.1f} bars")
            if mk < NEED or ml < NEED:
                low.append((mutation, cls, round(ml, 2), round(mk, 2)))
    assert not low, low
