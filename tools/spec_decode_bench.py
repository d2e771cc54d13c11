"""The window (nfai_hip_llama_window_*: up to 8 consecutive positions of ONE sequence per pass over the weights) against the paths
that exist without it, in the same run.  The method of tools/batch_decode_bench.py: alternating windows, medians, spread reported.

Llama-3.2-3B and -1B, weights built in HBM (bench.gen_weights_hbm), fp32 KV caches, 8 models over one copy of the weights, each after
a --depth-token _ingest of its own prompt (512 by default; --depth 8192 is the deep-context run) and 5 tokens of its own decode path.
For T in {2, 4, 8}:

  step cost    a blocking window step of T tokens (LlamaWindow.Step on member 0) against a blocking LlamaBatch.Step of T members at
               the same depths: the batch is the existing path doing the same GEMV work; what differs is the attention launch (one
               cache read once for all columns against T caches) and the lm_head tail.  Every step is timed on its own (the window
               is put back to the batch's depth between steps, untimed), >= 3 alternating windows of --steps steps.  Reported: ms per
               step of each (median, spread), the ratio, whether the window is slower than the batch by more than the batch's own
               spread, and per kernel class the eager hipEvent time per launch of one step of each (_profile_step).
  end to end   tokens/s of LlamaWindow.Verify loops against decode_greedy of the batch-1 path over the same positions, at the two bounds
               that need no real text: every draft right (the drafts are the continuation recorded by a plain greedy run — k = 0
               — through the window from the same state) and every draft wrong (the recorded token + 1 mod V).
  break-even   the mean number of tokens a verify pass must emit to match the batch-1 path: window step ms / batch-1 step ms.

What is NOT measured: how often an n-gram drafter is right on real text.  The weights are synthetic; no acceptance rate is quoted.

    python tools/spec_decode_bench.py --out profiles/spec_decode.json
    python tools/spec_decode_bench.py --quant q4_k_m --out profiles/spec_decode_q4_k_m.json
    python tools/spec_decode_bench.py --depth 8192 --only llama-3.2-3b --out profiles/spec_decode_deep.json

--quant q5_k_m | q8_0 | q4_0 | q3_k_m | iq4_xs: the weights of tools/q5_k_bench.py / tools/q8_0_bench.py / tools/q4_0_bench.py / tools/q3_k_bench.py /
tools/iq4_xs_bench.py, window and batch made with any_quant=True.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

WARM, NMAX, E2E_TOKENS = 5, 8, 256
CLASSES = ["qkv", "attn", "wo", "gateup", "down", "lmhead", "other"]


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def per_launch(prof):
    return {c: {"us_per_launch": prof[c][0] * 1e3 / prof[c][1], "launches_per_step": prof[c][1]} for c in CLASSES if prof[c][1]}


def run_model(torch, dims, depth, steps, windows, quant):
    from batch_decode_bench import ANY_QUANT, gen_weights
    from nfai_amd import synth
    from nfai_amd.hip import HipBufferManager
    from nfai_amd.llama_model import LlamaBatch, LlamaModel, LlamaWindow
    weights = gen_weights(torch, dims, quant)
    any_quant = quant in ANY_QUANT
    C = depth + WARM + E2E_TOKENS + 32
    mgr = HipBufferManager(0)
    dd = dict(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, eps=1e-5, rope_dims=dims.D, rope_base=500000.0)
    md = synth.make_metadata(dims)
    wt = {k: (t.data_ptr(), ty, r, c) for k, (t, ty, r, c) in weights.items()}
    members = [LlamaModel(mgr, md, wt, C, max_batch=512, dims=dd)]
    for _ in range(1, NMAX):
        members.append(LlamaModel(mgr, md, wt, C, max_batch=512, dims=dd, share_from=members[0]))
    first = []
    for s, m in enumerate(members):
        prompt = synth.make_tokens(dims, depth, seed=99 + s)
        prompt[0] = 128000 % dims.V
        m.Ingest(prompt)
        tok = int(prompt[-1])
        for _ in range(WARM):
            _, tok = m.Step(tok, want_logits=False)
        first.append(tok)
    p0 = depth + WARM
    m0 = members[0]
    win = LlamaWindow(m0, NMAX, quantized=quant != "f16", any_quant=any_quant)
    out = {"model": dims.name, "weights": quant, "kv_cache": "f32", "first_position": p0, "steps_per_window": steps, "by_T": {}}

    # the batch-1 path over the positions of the end-to-end runs, and the plain greedy continuation through the window (k = 0)
    def greedy_window():
        m0.SetPos(p0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        toks = m0.Greedy(first[0], E2E_TOKENS)
        return time.perf_counter() - t0, toks

    greedy_window()
    m0.SetPos(p0)
    rec, tok = [], first[0]
    for _ in range(E2E_TOKENS + NMAX):
        tok = int(win.Verify(tok, [])[1][0])
        rec.append(tok)
    out["window_greedy_equals_decode_greedy"] = bool(np.array_equal(np.asarray(rec[:E2E_TOKENS], np.uint32), greedy_window()[1]))

    for T in (2, 4, 8):
        ms = members[:T]
        batch = LlamaBatch(ms, quantized=quant != "f16", any_quant=any_quant)
        cols = [int(t) for t in synth.make_tokens(dims, T, seed=7 + T)]

        def batch_window():
            for m in ms:
                m.SetPos(p0)
            acc = 0.0
            for _ in range(steps):
                t0 = time.perf_counter()
                batch.Step(cols, want_logits=False)
                acc += time.perf_counter() - t0
            return acc / steps * 1e3

        def window_window():
            acc = 0.0
            for s in range(steps):
                m0.SetPos(p0 + s)            # the batch's depth at its step s (untimed)
                t0 = time.perf_counter()
                win.Step(cols, want_logits=False)
                acc += time.perf_counter() - t0
            return acc / steps * 1e3

        def verify_window(right):
            m0.SetPos(p0)
            tok, i, emitted, passes = first[0], 0, 0, 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            while emitted < E2E_TOKENS:
                draft = rec[i:i + T - 1] if right else [(t + 1) % dims.V for t in rec[i:i + T - 1]]
                got = win.Verify(tok, draft)[1]
                emitted += len(got)
                i += len(got)
                passes += 1
                tok = int(got[-1])
            return emitted / (time.perf_counter() - t0), emitted / passes

        batch_window(); window_window(); verify_window(True); verify_window(False)   # untimed: graph capture, code objects
        bt, wn, gr, vr, vw, acc_r, acc_w = [], [], [], [], [], [], []
        for _ in range(windows):   # alternating
            bt.append(batch_window())
            wn.append(window_window())
            gr.append(E2E_TOKENS / greedy_window()[0])
            tps, per = verify_window(True)
            vr.append(tps); acc_r.append(per)
            tps, per = verify_window(False)
            vw.append(tps); acc_w.append(per)
        for m in ms:
            m.SetPos(p0)
        batch.ProfileStep(cols)
        for m in ms:
            m.SetPos(p0)
        prof_b = batch.ProfileStep(cols)
        m0.SetPos(p0)
        win.ProfileStep(cols)
        m0.SetPos(p0)
        prof_w = win.ProfileStep(cols)
        m0.SetPos(p0)
        bytes_w = win.BytesPerStep(T)
        bytes_b = batch.BytesPerToken()
        med_b, med_w, med_g = statistics.median(bt), statistics.median(wn), statistics.median(gr)
        out["by_T"][str(T)] = {
            "window_ms_per_step": med_w, "window_windows_ms": wn, "window_spread": spread(wn),
            "batch_ms_per_step": med_b, "batch_windows_ms": bt, "batch_spread": spread(bt),
            "window_over_batch": med_w / med_b, "window_slower_than_batch_by_more_than_its_spread": med_w > med_b * (1 + spread(bt)),
            "window_bytes_per_step": bytes_w, "batch_bytes_per_step": bytes_b,
            "kernel_classes_window": per_launch(prof_w), "kernel_classes_batch": per_launch(prof_b),
            "decode_greedy_tokens_per_s": med_g, "decode_greedy_spread": spread(gr),
            "all_drafts_right_tokens_per_s": statistics.median(vr), "all_drafts_right_spread": spread(vr),
            "all_drafts_right_tokens_per_verify": statistics.median(acc_r),
            "all_drafts_wrong_tokens_per_s": statistics.median(vw), "all_drafts_wrong_spread": spread(vw),
            "all_drafts_wrong_tokens_per_verify": statistics.median(acc_w),
            "break_even_tokens_per_verify": med_w / (1e3 / med_g),
        }
        print(f"{dims.name} {quant} depth {depth} T={T}: window {med_w:.3f} ms, batch {med_b:.3f} ms", file=sys.stderr, flush=True)
        batch.Dispose()
    win.Dispose()
    for m in reversed(members):
        m.Dispose()
    mgr.Dispose()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--depth", type=int, default=512, help="tokens ingested before the measurement (8192: the deep-context run)")
    ap.add_argument("--only", default="", metavar="MODEL", help="one model, e.g. llama-3.2-3b")
    ap.add_argument("--quant", default="f16", choices=["f16", "q4_k_m", "q5_k_m", "q8_0", "q4_0", "q3_k_m", "iq4_xs"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from nfai_amd import synth
    torch.cuda.set_device(0)
    out = {"tool": "spec_decode_bench", "weights": a.quant, "depth": a.depth, "models": [],
           "not_measured": "the acceptance of the n-gram drafter on real text (synthetic weights): no acceptance rate is quoted"}
    for dims in (synth.LLAMA_32_3B, synth.LLAMA_32_1B):
        if a.only and a.only != dims.name:
            continue
        out["models"].append(run_model(torch, dims, a.depth, a.steps, max(3, a.windows), a.quant))
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
