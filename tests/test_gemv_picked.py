"""The case table of the picked fp16 / fp32 GEMV (tests/gemv_cases.py) against the planner itself, on the CPU.

nfai_hip_debug_gemv_plan is gemv_plan of kernels_gemv.hip — the function launch_gemv launches from — with n_cu taken from the
argument, so the sweep below asks the real pickers, not a restatement of them.  At n_cu = 256 the full grid

    modes PLAIN, RESIDUAL, q|k|v, gate|up  x  fp16, fp32  x  norm off, on  x  fused ArgMax off, on (PLAIN)
    K   every multiple of 8 up to 1024 and every multiple of 256 up to 40960
    NU  1 .. 4200, 8192, 16384, 34816, 128256

returns 258 classes (kernel, w_type, mode, norm, UPW | CH, U | RW, guard) in 21 (kernel, UPW | CH, U | RW, guard) families; 12 of
them are first reached above 128 MB of weights (gemv_cases.EXCLUDED), the other 246 have cases.  The full grid is 24 M planner calls,
about a minute; the test sweeps its two thinned halves, which return the same 258 classes and the same smallest shape for each
excluded class (checked once against the full grid):

    every K  x  NU in 1 .. 33, every multiple of 256 up to 4200 with its two neighbours, 4085 .. 4200 in steps of 5, 4097, 4100 and the four large ones
    every NU x  K in 8, 264, 520, 1000, 256, 512, 768, 1024, 1536, 2048, 4352, 5376, 8192, 8704, 10752, 16384, 17408, 32768

The class fp16 PLAIN without norm at k_gemv UPW = 2, U = 4 — the form an fp16 lm_head of 34816 x 4096 (285 MB) takes — needs no
exemption from the 128 MB cap: with the fused ArgMax the planner reaches it at 8192 x 2048 (32 MB), where the split-K form would
need more than 1024 workgroups.  Both shapes are cases.

Dispatch arms the default pickers cannot return:
  dispatch_sk (1, 8)                    RW = 8 needs CH = 2 (16 / CH above 60 MB, else 4); CH = 1 gets 16 or 4.  NFAI_GEMV_SK_RW only.
  split-K in q|k|v or gate|up mode      plan_gemv_sk serves the modes of NFAI_GEMV_SK_MODES, by default PLAIN and RESIDUAL.
  k_gemv with UPW * RPU * U > 8         plan_gemv keeps the loads per lane and step at NFAI_GEMV_MAXLD = 8.
The forms only the environment reaches (NFAI_GEMV_SK_MODES, _SK_RW, _WPB*, _BPC*, _MAXLD) are not swept: the pickers read
NFAI_GEMV_* once per process, so with any of them set the sweep runs in a child process without them.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gemv_cases as gc

K_ALL = sorted(set(range(8, 1025, 8)) | set(range(256, 40961, 256)))
NU_ALL = list(range(1, 4201)) + [8192, 16384, 34816, 128256]
K_THIN = [8, 264, 520, 1000, 256, 512, 768, 1024, 1536, 2048, 4352, 5376, 8192, 8704, 10752, 16384, 17408, 32768]
NU_THIN = sorted((set(range(1, 34)) | {m + d for m in range(256, 4201, 256) for d in (-1, 0, 1)} | set(range(4085, 4201, 5)) | {4097, 4100} |
                  {8192, 16384, 34816, 128256}) & set(NU_ALL))


def collect():
    """{"classes": [[class, bytes, NU, K], ...] (smallest shape per class over the swept grid), "cases": [descriptor or None per case]}."""
    plan = gc.load_plan()
    small = {}
    for wt in (gc.F16, gc.F32):
        for mode in range(4):
            for norm in (0, 1):
                for am in ((0, 1) if mode == gc.PLAIN else (0,)):
                    for Ks, NUs in ((K_ALL, NU_THIN), (K_THIN, NU_ALL)):
                        for K in Ks:
                            for NU in NUs:
                                r = (NU, 0, 0) if mode < 2 else ((2 * NU, 0, 0) if mode == gc.QKV else (NU, NU, 0))
                                d = plan(wt, mode, *r, K, gc.N_CU, norm, am)
                                if d is None:      # what launch_gemv refuses
                                    continue
                                assert d[12] == NU and d[13] == K
                                c, b = gc.desc_cls(d), gc.weight_bytes(wt, mode, NU, K)
                                if c not in small or b < small[c][0]:
                                    small[c] = (b, NU, K)
    cases = [plan(c.wt, c.mode, *gc.seg_rows(c), c.K, gc.N_CU, c.norm, c.argmax) for c in gc.CASES]
    return {"classes": [[list(c)] + list(v) for c, v in sorted(small.items())], "cases": cases}


@pytest.fixture(scope="module")
def swept():
    dirty = sorted(k for k in os.environ if k.startswith("NFAI_GEMV_"))
    if dirty:
        env = {k: v for k, v in os.environ.items() if k not in dirty}
        here = os.path.dirname(os.path.abspath(__file__))
        code = f"import sys, json; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_gemv_picked as t; print(json.dumps(t.collect()))"
        out = subprocess.run([sys.executable, "-c", code], env=env, check=True, capture_output=True, text=True).stdout
        got = json.loads(out.strip().splitlines()[-1])
    else:
        got = collect()
    classes = {tuple(r[0]): (r[1], r[2], r[3]) for r in got["classes"]}
    cases = [None if d is None else tuple(d) for d in got["cases"]]
    return classes, cases


def test_every_case_is_what_the_planner_returns(swept):
    _, descs = swept
    assert len(descs) == len(gc.CASES)
    for c, d in zip(gc.CASES, descs):
        assert d is not None, (gc.case_id(c), "the planner refuses the shape")
        assert gc.desc_cls(d) == gc.cls(c), (gc.case_id(c), d)
        assert (d[9], d[10], d[12], d[13], d[14]) == (c.threads, c.grid, c.NU, c.K, c.argmax), (gc.case_id(c), d)
        assert d[4] == 0 and d[5] == 0 and d[15] == 0, (gc.case_id(c), d)          # no begin, no dealing, no prefetch-only launch at op level
    assert len({gc.case_id(c) for c in gc.CASES}) == len(gc.CASES)


def test_cases_and_excluded_are_exactly_the_reachable_classes(swept):
    classes, _ = swept
    named = {gc.cls(c) for c in gc.CASES}
    print(f"{len(classes)} classes reachable, {len(named)} with cases, {len(gc.EXCLUDED)} excluded; "
          f"{len({(c[0], c[4], c[5], c[6]) for c in classes})} (kernel, UPW | CH, U | RW, guard) families")
    assert not named & set(gc.EXCLUDED)
    assert named | set(gc.EXCLUDED) == set(classes), (sorted(set(classes) - named - set(gc.EXCLUDED)), sorted((named | set(gc.EXCLUDED)) - set(classes)))
    for c, shape in sorted(gc.EXCLUDED.items()):
        b, NU, K = classes[c]
        print(f"excluded {c}: smallest swept shape NU = {NU}, K = {K}, {b / 2**20:.0f} MB of weights")
        assert b > gc.CAP_BYTES, (c, NU, K, b)
        assert (NU, K) == shape, (c, NU, K)
    for c in gc.CASES:                 # and no case spends more than the cap, but the lm_head form of 34816 x 4096
        if gc.weight_bytes(c.wt, c.mode, c.NU, c.K) > gc.CAP_BYTES:
            assert (gc.cls(c), c.NU, c.K) == ((0, gc.F16, gc.PLAIN, 0, 2, 4, 0), 34816, 4096), gc.case_id(c)


def test_launch_shapes_of_the_table():
    for wt in (gc.F16, gc.F32):
        sk = [c for c in gc.CASES if c.kernel == 1 and c.wt == wt]
        kg = [c for c in gc.CASES if c.kernel == 0 and c.wt == wt]
        waves = {ch: {c.threads // 64 for c in sk if c.a == ch} for ch in (1, 2, 4)}
        assert waves[1] == set(range(2, 17)), waves[1]
        assert waves[2] == set(range(9, 17)) and waves[4] == set(range(9, 17)), waves
        for norm in (0, 1):
            assert {c.threads // 64 for c in kg if c.norm == norm} == {4, 5, 6, 7, 8}, (wt, norm)
        rules = {"ceil" if (c.NU < 4 * gc.N_CU and c.grid == -(-c.NU // 4)) else c.grid for c in kg}
        assert rules == {"ceil", gc.N_CU, 2 * gc.N_CU}, rules
        # split-K: below one workgroup, a partial last workgroup, an exact multiple — per class, where 60 MB allow it
        for k in {gc.cls(c) for c in sk}:
            upg = k[5] // gc.rpu(k[2])
            kinds = {"below" if c.NU < upg else ("exact" if c.NU % upg == 0 else "partial") for c in sk if gc.cls(c) == k}
            assert kinds == ({"below", "partial", "exact"} if k[5] == 4 else {"partial", "exact"}), (k, kinds)
        # k_gemv: a partial last group wherever whole heads leave one
        for k in {gc.cls(c) for c in kg if c.a > 1}:
            if not (k[2] == gc.QKV and k[4] in (2, 4)):
                assert any(c.NU % c.a for c in kg if gc.cls(c) == k), k
        rem = {(c.K % (512 if wt == gc.F16 else 256)) for c in kg if c.guard}
        assert {8, 264 % (512 if wt == gc.F16 else 256), 1000 % (512 if wt == gc.F16 else 256)} <= rem, rem


@pytest.mark.parametrize("c", [c for c in gc.CASES if c.argmax and gc.weight_bytes(c.wt, c.mode, c.NU, c.K) <= 16 << 20], ids=gc.case_id)
def test_argmax_cases_have_a_clear_winner(c):
    """The fused ArgMax is compared with the float64 argmax: the reference's top two must lie more than twice the bar apart (the GPU
    test asserts the same for every ArgMax case, the larger ones included)."""
    want, bar = gc.reference(c, *gc.inputs(c))
    _, gap, b = gc.argmax_gap(want, bar)
    assert gap > 2 * b, (gap, b)
