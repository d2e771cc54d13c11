"""CPU-side checks of the wide batch (nfai_hip_llama_batch_create_wide, kernels_gemv_wide.hip): the entry point is exported, declared,
bound in ctypes and in the C# P/Invoke surface; bad arguments are error codes with a message, never a crash; _batch_create keeps its
limit of 8.  And the construction of EQUAL maxima for the GPU module (tests/test_gpu_batch_wide.py), placed by the wide lm_head's own
row dealing, with the margin asserted on the CPU oracle alone.  No GPU needed.

Dealing of the wide lm_head (kernels_gemv_wide.hip::plan_wgemv and k_wgemv, KS = 1 at V > 32768): a tile is 16 rows; a workgroup is
16 waves and takes 16 consecutive tiles (256 rows) per pass, wave w tile w; grid = min(n_cu, ceil(tiles / 16)); group g of 16 tiles
belongs to workgroup g % grid and is its pass g // grid.  Row r of a tile sits in lane group r // 4, accumulator register r % 4.  A
column's best (value, index) is carried by a lane from pass to pass, merged over the four lane groups of a wave, over the 16 waves
in LDS, and over the workgroups by the last one (lane l reads the partials of workgroups l, l + 64, ...)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from nfai_amd import synth

from test_batch_vocab import V_REAL, batch_columns, check_tied_columns, oracle_columns, tie_dims, weights, with_copied_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = "nfai_hip_llama_batch_create_wide"
WIDE_MAX = 16
CU_COUNTS = (256, 304, 128)


@pytest.fixture(scope="module")
def lib():
    from nfai_amd import build as hb, _lib
    hb.build()
    return _lib.load()


def _err(lib):
    return lib.nfai_hip_last_error().decode("utf-8", "replace")


def test_symbol_exported_declared_bound_and_in_csharp(lib):
    from nfai_amd import _lib
    src = open(os.path.join(ROOT, "include", "nfai_hip.h")).read()
    assert re.search(r"#define\s+NFAI_BATCH_WIDE_MAX\s+16\b", src)
    assert _lib.BATCH_WIDE_MAX == WIDE_MAX
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b" + WIDE + r"\s*\(([^;{]*?)\)\s*;", plain)
    assert m and m.group(1).count(",") + 1 == 4, m
    raw = C.CDLL(os.path.join(ROOT, "nfai_amd", "csrc", "libnfai_hip.so"))
    assert hasattr(raw, WIDE), f"{WIDE} is not exported"
    assert len(_lib.SIGNATURES[WIDE]) == 4
    cs = open(os.path.join(ROOT, "csharp", "NFAI.HIP", "NativeMethods.g.cs")).read()
    m = re.search(r"\b" + WIDE + r"\(([^)]*)\)", cs)
    assert m and m.group(1).count(",") + 1 == 4, m
    assert WIDE in open(os.path.join(ROOT, "csharp", "NFAI.HIP", "HipLlamaBatch.cs")).read()


def test_generated_csharp_is_current():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_csharp_bindings.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert WIDE in open(os.path.join(ROOT, "csharp", "NFAI.HIP", "NativeMethods.g.cs")).read()


def test_python_host_takes_wide():
    import inspect
    from nfai_amd.llama_model import LlamaBatch
    assert "wide" in inspect.signature(LlamaBatch.__init__).parameters
    assert "wide" in inspect.signature(LlamaBatch.RunTokens).parameters
    assert "wide" in inspect.signature(LlamaBatch.RunAsync).parameters
    with pytest.raises(ValueError, match="fp16"):
        LlamaBatch([], quantized=True, wide=True)


def test_bad_arguments_are_errors_not_crashes(lib):
    from nfai_amd import _lib
    h = _lib.H()
    dead = (_lib.H * 17)(*([987654321] * 17))
    fn = getattr(lib, WIDE)
    for models, n, flags, what, word in ((dead, 0, 0, "n = 0", "invalid n = 0"), (dead, 17, 0, "n = 17", "invalid n = 17"),
                                         (None, 2, 0, "NULL list", "null"), (dead, 1, 0, "dead handle", "invalid model handle"),
                                         (dead, 16, 0, "16 dead handles", "invalid model handle"), (dead, 2, 1, "flags 1", "invalid flags"),
                                         (dead, 2, 4, "flags 4", "invalid flags"), (dead, 2, 0x80000000, "flags bit 31", "invalid flags")):
        rc = fn(models, n, flags, C.byref(h))
        assert rc == _lib.ERR_INVALID, (what, rc)
        assert word in _err(lib) and "batch_create_wide" in _err(lib), (what, _err(lib))
    rc = fn(dead, 1, 0, None)
    assert rc == _lib.ERR_INVALID and "null" in _err(lib)
    assert "1 to 16" in (fn(dead, 17, 0, C.byref(h)), _err(lib))[1]


def test_batch_create_still_refuses_nine(lib):
    from nfai_amd import _lib
    h = _lib.H()
    dead = (_lib.H * 9)(*([987654321] * 9))
    rc = lib.nfai_hip_llama_batch_create(dead, 9, C.byref(h))
    assert rc == _lib.ERR_INVALID and _err(lib) == "batch_create: invalid n = 9 (a batch holds 1 to 8 models)", _err(lib)
    rc = lib.nfai_hip_llama_batch_create_ex(dead, 9, 1, C.byref(h))
    assert rc == _lib.ERR_INVALID and _err(lib) == "batch_create_ex: invalid n = 9 (a batch holds 1 to 8 models)", _err(lib)


# ---- equal maxima for sixteen columns -------------------------------------------------------------------------------------------------
class WideDeal:
    """Row -> (pass, workgroup, wave, lane group, register) of the wide lm_head at KS = 1."""

    def __init__(self, V, n_cu):
        self.V, self.n_cu = int(V), int(n_cu)
        self.tiles = -(-self.V // 16)
        assert self.tiles * 2 > 4096, "KS = 1"
        self.groups = -(-self.tiles // 16)
        self.grid = min(self.n_cu, self.groups)

    def place(self, row):
        tile = row // 16
        g = tile // 16
        return g // self.grid, g % self.grid, tile % 16, (row % 16) // 4, row % 4

    def row(self, pas, wg, wave, lg, reg):
        if pas < 0 or not (0 <= wg < self.grid) or not (0 <= wave < 16) or not (0 <= lg < 4) or not (0 <= reg < 4):
            return -1
        r = (((pas * self.grid + wg) * 16 + wave) * 16) + lg * 4 + reg
        return r if r < self.V else -1


# one placement per column: what decides between the winner and its copy
WIDE_TIE_KINDS = ("same-lane", "other-lane-group", "other-wave", "later-pass", "earlier-pass", "next-workgroup", "previous-workgroup",
                  "same-merge-lane", "row-0", "row-last", "same-lane", "other-lane-group", "other-wave", "later-pass", "next-workgroup",
                  "same-merge-lane")


def wide_tie_row(deal, r, kind, taken, second):
    """`second`: the second column of this kind takes the other direction first."""
    p, g, w, lg, reg = deal.place(r)
    cand = {
        "same-lane": [(p, g, w, lg, (reg + 1) % 4), (p, g, w, lg, (reg + 3) % 4)],
        "other-lane-group": [(p, g, w, (lg + 1) % 4, reg), (p, g, w, (lg + 3) % 4, reg)],
        "other-wave": [(p, g, (w + 5) % 16, lg, reg), (p, g, (w + 11) % 16, lg, reg)],
        "later-pass": [(p + 1, g, w, lg, reg), (p - 1, g, w, lg, reg)],
        "earlier-pass": [(p - 1, g, w, lg, reg), (p + 1, g, w, lg, reg)],
        "next-workgroup": [(p, g + 1, w, lg, reg), (p, g - 1, w, lg, reg)],
        "previous-workgroup": [(p, g - 1, w, lg, reg), (p, g + 1, w, lg, reg)],
        "same-merge-lane": [(p, g + 64, w, lg, reg), (p, g - 64, w, lg, reg)],
    }
    if kind == "row-0":
        return (0, "row 0") if r != 0 and 0 not in taken else (-1, "none")
    if kind == "row-last":
        return (deal.V - 1, "row V - 1") if r != deal.V - 1 and deal.V - 1 not in taken else (-1, "none")
    c = cand[kind][::-1] if second else cand[kind]
    for pos in c + [(p, (g + 3) % deal.grid, w, lg, reg)]:
        x = deal.row(*pos)
        if x >= 0 and x != r and x not in taken:
            return x, f"{kind}: {deal.place(r)} -> {pos}"
    return -1, "none"


WIDE_TIE_SEEDS = (21, 400)   # weights, tokens: chosen with the oracle alone (sixteen distinct winners, the margin at every CU count below)
_WIDE_BASE = {}


def wide_ties(n_cu):
    """(dims, weights with the copies, alone, step, winners, sets, expected tokens, the oracle's logits) for sixteen columns at V = 128256."""
    dims = tie_dims()
    wseed, tseed = WIDE_TIE_SEEDS
    wdev, wref = weights(dims, False, wseed)
    alone, step = batch_columns(dims, tseed, n=WIDE_MAX)
    if "winners" not in _WIDE_BASE:
        from oracle import argmax
        _WIDE_BASE["winners"] = [argmax(lg) for lg in oracle_columns(dims, wref, alone, step)]
    winners = _WIDE_BASE["winners"]
    assert len(set(winners)) == WIDE_MAX, winners
    deal = WideDeal(dims.V, n_cu)
    taken, sets, seen = set(int(r) for r in winners), [], set()
    for r, kind in zip(winners, WIDE_TIE_KINDS):
        x, what = wide_tie_row(deal, int(r), kind, taken, kind in seen)
        assert x >= 0, (kind, r)
        seen.add(kind)
        taken.add(x)
        sets.append((x, what))
    wdev2, wref2 = with_copied_rows(dims, False, wdev, wref, [(x, r) for (x, _), r in zip(sets, winners)])
    logits = oracle_columns(dims, wref2, alone, step)
    expect = check_tied_columns(logits, winners, sets, f"wide ties n_cu={n_cu}")
    return dims, wdev2, alone, step, winners, sets, expect, logits


@pytest.mark.parametrize("n_cu", CU_COUNTS)
def test_wide_tie_sets(n_cu):
    """Disjoint sets, the margin (check_tied_columns), and copies on both sides of their winners."""
    dims, _, _, _, winners, sets, expect, _ = wide_ties(n_cu)
    print(f"n_cu={n_cu} winners {winners} copies {sets} expected {expect}")
    deal = WideDeal(dims.V, n_cu)
    assert deal.grid == min(n_cu, 501) and dims.V == V_REAL
    own = sum(1 for b in range(WIDE_MAX) if expect[b] == winners[b])
    assert own >= 3 and WIDE_MAX - own >= 3, (expect, winners)
    for b, kind in enumerate(WIDE_TIE_KINDS):
        a, c = deal.place(winners[b]), deal.place(sets[b][0])
        if kind == "same-lane":
            assert a[:4] == c[:4] and a[4] != c[4]
        elif kind == "other-lane-group":
            assert a[:3] == c[:3] and a[3] != c[3]
        elif kind == "other-wave":
            assert a[:2] == c[:2] and a[2] != c[2]
        elif kind in ("later-pass", "earlier-pass"):
            assert (a[1:] == c[1:] and a[0] != c[0]) or a[1] != c[1]   # (a workgroup without a second pass: the fallback, another workgroup)
