"""Scoring a token sequence, the part that needs no GPU: the fp64 reference of tests/score_cases.py on hand-made rows, what the MFMA
head's fp16 operands cost against the log-probability bar, the pinned share of every GPU case, and the entry points themselves (header,
exports, a dead handle).

Bar measurement (the way tests/test_prefill_rows_bar.py re-measures its bar).  The GPU bar on a log-probability of the MFMA path is
2 * 2e-2 * max(1, max|logit|).  The head alone, restated in NumPy on the oracle's hidden rows (row rounded to fp16 behind the norm, fp16
weights, fp32 accumulation), must stay under HALF of it on every row of every fixture tests/test_gpu_score.py uses; the figures are
printed.  Measured, largest error / (max(1, max|logit|)) over the rows, target and maximum: below 2e-3 on every fixture (the half
bar is 2e-2), so the bar stands as the issue states it.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import score_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_on_hand_made_rows():
    V = 1000
    # all equal: every probability is 1 / V, the first index wins
    lp, am, lpm = sc.score_rows_ref(np.full((1, V), 3.25), [17])
    assert am[0] == 0 and abs(lp[0] + np.log(V)) < 1e-12 and abs(lpm[0] + np.log(V)) < 1e-12
    # one logit at +80, the rest at -80: the maximum has probability 1 - (V - 1) e^-160, the others e^-160 of it
    row = np.full((2, V), -80.0)
    row[:, 123] = 80.0
    lp, am, lpm = sc.score_rows_ref(row, [123, 5])
    assert list(am) == [123, 123]
    assert abs(lp[0]) < 1e-12 and abs(lpm[1]) < 1e-12 and abs(lp[1] + 160.0) < 1e-9
    # ties: the first index of the maximum; both tied columns hold half of what the rest leaves
    row = np.zeros((1, V))
    row[0, [700, 40, 999]] = 9.0
    lp, am, lpm = sc.score_rows_ref(row, [999])
    assert am[0] == 40 and lp[0] == lpm[0]
    assert abs(lp[0] - (9.0 - np.log(3 * np.exp(9.0) + (V - 3)))) < 1e-12
    # no target
    lp, _, _ = sc.score_rows_ref(row, [sc.NO_TARGET])
    assert lp[0] == 0.0


FIXTURES = sorted({(c.dims, c.enc) for c in sc.CASES}, key=lambda de: (de[0].name, de[1]))


@pytest.mark.parametrize("dims,enc", FIXTURES, ids=[f"{d.name}-{e}" for d, e in FIXTURES])
def test_mfma_head_stays_under_half_the_logprob_bar(dims, enc):
    (lp64, am64, lpm64), (lp16, _, lpm16), l64 = sc.head_restated(dims, enc)
    w = sc.walk(dims, enc)
    scale = np.maximum(1.0, np.abs(w.logits).max(axis=1))
    # the hidden rows are the ones in front of the output norm: the fp64 head on them gives the oracle's logits
    assert np.abs(l64 - w.logits).max() <= 5e-4 * scale.max()
    err_t, err_m = float((np.abs(lp16 - lp64) / scale).max()), float((np.abs(lpm16 - lpm64) / scale).max())
    print(f"{dims.name} {enc}: MFMA head restated, logprob error / max(1, max|logit|): target {err_t:.2e}, maximum {err_m:.2e} "
          f"(half bar {sc.LOOSE:.0e})")
    assert err_t < sc.LOOSE and err_m < sc.LOOSE        # half of 2 * LOOSE


@pytest.mark.parametrize("c", sc.CASES, ids=[c.id for c in sc.CASES])
def test_pinned_share(c):
    _, _, _, _, lg = sc.case_rows(c)
    share = float(sc.pinned(c, lg).mean())
    assert share >= c.pin_share, f"{c.id}: {share:.0%} of the rows pinned, needs {c.pin_share:.0%}: reseed ({c.dims.name}, {c.enc}) in score_cases.RESEED"


def test_pinned_share_at_the_documented_seeds():
    """48 tokens of seeds 99 and 7 on the default fp16 weights: the decode bar pins nearly every row, the prefill bar more than half."""
    import oracle as orc
    from nfai_amd import synth
    for dims in (synth.TINY, synth.TINY_D128):
        for seed in (99, 7):
            toks = synth.make_tokens(dims, 48, seed=seed)
            ref = orc.OracleLlama(orc.LlamaDesc(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, C=48), synth.make_weights(dims))
            lg = np.stack([np.array(ref.step(int(t)), np.float32) for t in toks])
            ref.close()
            tight = sc.pinned(sc.Case(dims, "f16", False, 0, 48), lg).mean()
            loose = sc.pinned(sc.Case(dims, "f16", False, 128, 48), lg).mean()
            print(f"{dims.name} seed {seed}: pinned {tight:.0%} at the decode bar, {loose:.0%} at the prefill bar")
            assert tight >= sc.PIN_TIGHT and loose >= sc.PIN_LOOSE


# ---- the entry points (these fail without the feature) -----------------------------------------------------------------------------
def test_header_declares_both_entry_points():
    src = open(os.path.join(ROOT, "include", "nfai_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int32_t\s+nfai_hip_score_rows\s*\(", code)
    assert re.search(r"int32_t\s+nfai_hip_llama_score\s*\(", code)
    assert re.search(r"#define\s+NFAI_SCORE_NO_TARGET\s+0xFFFFFFFFu", src)
    assert "SamplingUtils.cs:35-41" in src and "SamplingUtils.cs:55-56" in src


def test_library_exports_and_refuses_a_dead_handle():
    from nfai_amd import build as hb, _lib
    hb.build()
    raw = ctypes.CDLL(os.path.join(ROOT, "nfai_amd", "csrc", "libnfai_hip.so"))
    assert hasattr(raw, "nfai_hip_score_rows") and hasattr(raw, "nfai_hip_llama_score")
    lib = _lib.load()
    toks = (ctypes.c_uint32 * 2)(1, 2)
    rc = lib.nfai_hip_llama_score(987654321, toks, 2, None, None, None, None)
    assert rc == _lib.ERR_INVALID and b"invalid model handle" in lib.nfai_hip_last_error()
    assert lib.nfai_hip_score_rows(12345, 0, 1, 1, 1, 0, 0, 0, 0, 0) == _lib.ERR_INVALID
    assert _lib.SCORE_NO_TARGET == sc.NO_TARGET == 0xFFFFFFFF


def test_perplexity_tool_counts_drafter_acceptance():
    """tools/perplexity.py: on a periodic text a model that always predicts the next token accepts every draft the n-gram drafter makes,
    a model that never does accepts none."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import perplexity as ppl
    toks = [5, 6, 7, 8] * 6
    right = np.array(toks[1:] + [0])
    acc, prop, pos = ppl.drafter_acceptance(toks, right, 3, 4)
    assert prop > 0 and acc == prop and pos > 0
    acc, prop, _ = ppl.drafter_acceptance(toks, np.zeros(len(toks), np.int64), 3, 4)
    assert prop > 0 and acc == 0


def test_python_host_has_score_and_perplexity():
    from nfai_amd.llama_model import LlamaModel
    assert callable(LlamaModel.Score) and callable(LlamaModel.Perplexity)
