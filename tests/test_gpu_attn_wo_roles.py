"""The fused attention + Wo launch (k_attn_wo) with its two roles in workgroups of their own: the first Hkv x 32 workgroups run
the KV slices, the nbw workgroups behind them stream Wo and wait for the merged attention output.  Everything here runs the model
against the CPU oracle at the suite's decode tolerance (logits max|d| <= 5e-4 * max(1, max|logit|), tests/test_gpu_model.py) and
shows, with a profile step, that the fused launch is what ran: a case must not pass on the two-launch path unnoticed.
"""
from dataclasses import replace

import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth

pytestmark = pytest.mark.gpu

# the test head shape of kAttnWoShapes: 4/2 heads of 128, E = H*D = 512 (Wo over 128 workgroups behind 64 slice workgroups)
ROLES = synth.LlamaDims("roles-d128", 512, 2, 4, 2, 128, 512, 256, True)


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


def odesc(d, C):
    return orc.LlamaDesc(E=d.E, L=d.L, H=d.H, Hkv=d.Hkv, D=d.D, F=d.F, V=d.V, C=C)


def logit_tol(want):
    return 5e-4 * max(1.0, float(np.abs(want).max()))


def fused_step(m, ref, tok, L):
    """One token as a profile step (launch by launch): the attention class holds one launch per block and the Wo class none."""
    prof = m.ProfileStep(int(tok))
    ref.step(int(tok), want_logits=False)
    assert prof["attn"][1] == L and prof["wo"][1] == 0, prof


def check_step(m, ref, tok, where):
    lg, am = m.Step(int(tok))
    want = ref.step(int(tok))
    err = float(np.abs(lg - want).max())
    assert err <= logit_tol(want), (where, err)
    assert am == orc.argmax(want), where


@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_slice_transitions(mgr, mode):
    """Every position of a 2048-position context, two blocks: S = 1 (single-slice path), 32 -> 33 and 64 -> 65 (another slice opens),
    1024 -> 1025 (the chunk grows past 32 positions) and the last position of the capacity, each against the oracle."""
    from nfai_amd.llama_model import LlamaModel
    C = 2048
    w = synth.make_weights(ROLES, seed=41, std=0.05)
    m = LlamaModel(mgr, synth.make_metadata(ROLES), w, C, graph=mode == "graph")
    ref = orc.OracleLlama(odesc(ROLES, C), w)
    toks = synth.make_tokens(ROLES, C, seed=14)
    profiled = {40, 1500}  # positions stepped launch by launch instead (not compared: a profile step returns no logits)
    for i, t in enumerate(toks):
        if i in profiled:
            fused_step(m, ref, t, ROLES.L)
        else:
            check_step(m, ref, t, i)
    assert m.Pos == C
    m.Dispose()


@pytest.mark.parametrize("dims,n_pos", [(synth.LLAMA_32_3B, 524), (synth.LLAMA_32_1B, 524), (replace(ROLES, E=128, name="roles-e128"), 70)],
                         ids=["3b", "1b", "e128"])
def test_grid_of_both_roles(mgr, dims, n_pos):
    """One block at the 3B shape (24/8 heads of 128, E = 3072) and the 1B shape (32/8 heads of 64, E = 2048): as many slice
    workgroups as Wo workgroups (256 on a 256-CU device); and the test head shape with E = 128: 64 slice workgroups in front of 32
    Wo workgroups, whatever the device.  Positions 0 .. n_pos - 1, so 33 and 520 among them (F and V thin: the oracle stays fast)."""
    from nfai_amd.llama_model import LlamaModel
    d1 = replace(dims, L=1, F=512, V=512, tied=True, name=dims.name + "-1blk")
    C = n_pos + 4
    w = synth.make_weights(d1, seed=43)
    m = LlamaModel(mgr, synth.make_metadata(d1), w, C)
    ref = orc.OracleLlama(odesc(d1, C), w)
    toks = synth.make_tokens(d1, n_pos, seed=15)
    for i, t in enumerate(toks):
        if i == 34 or i == n_pos - 2:
            fused_step(m, ref, t, 1)
        else:
            check_step(m, ref, t, i)
    m.Dispose()


def test_two_models_alternating(mgr):
    """Two models of one shape, different weights, stepped alternately on one context: both count their token epochs from the
    same start, so the tag of a launch of one is the tag the other's launch has just left in the granules of ITS workspace and in
    the LDS arrival words of the Wo workgroups.  Neither may ever take the other's for its own: each against its own oracle."""
    from nfai_amd.llama_model import LlamaModel
    C = 48
    ms, refs, toks = [], [], []
    for k, seed in enumerate((51, 52)):
        w = synth.make_weights(ROLES, seed=seed, std=0.05)
        ms.append(LlamaModel(mgr, synth.make_metadata(ROLES), w, C))
        refs.append(orc.OracleLlama(odesc(ROLES, C), w))
        toks.append(synth.make_tokens(ROLES, 40, seed=16 + k))
    for i in range(40):
        for k in (0, 1):
            if i == 36:
                fused_step(ms[k], refs[k], toks[k][i], ROLES.L)
            else:
                check_step(ms[k], refs[k], toks[k][i], (k, i))
    for m in ms:
        m.Dispose()
