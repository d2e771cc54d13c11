"""Batched decode (nfai_hip_llama_batch_*) against the same sequences stepped one after another, in the same run.

Llama-3.2-3B and -1B, fp16 weights built in HBM (bench.gen_weights_hbm), 8 models over one copy of the weights (fp32 KV caches, the
library's default), each after a 512-token _ingest of its own prompt.  For n in {1, 2, 4, 8}, from position 517 of every member:

  batch        n members through _batch_greedy (one graph replay per step for all of them)
  sequential   the same n members through the existing _decode_enqueue path, one token each per round, round after round: how n
               sequences are served without the batch (that path's code is unchanged)

The two alternate window by window (>= 3 windows of --steps steps each, every window from the same positions, one untimed warm-up
window of each first); reported: the median and the relative spread (max - min) / median of each, the ratio, the algorithmic bytes
of one step (_batch_bytes_per_token) and of the n sequential steps, the fraction of the byte-model ratio reached, the step's
fraction of 8 TB/s, and per kernel class the eager hipEvent time per launch of one batch step (_batch_profile_step) with its
algorithmic bytes and fraction of the HBM roofline.  Parity: max |dlogit| of the batch against the members' own _decode_step at depth
(4 positions, n = 4, same run), and against the CPU oracle for n = 4 on the 1B model at shallow staggered depths (--no-check skips
the oracle, which takes about a minute of host time).  One JSON line; --out writes it to a file too.

    python tools/batch_decode_bench.py --out profiles/batch_decode.json
    python tools/batch_decode_bench.py --quant q4_k_m --out profiles/batch_decode_q4_k_m.json

--quant q4_k_m: the same run on llama.cpp's Q4_K_M tensor mix (bench.gen_weights_hbm's random K-quant super-blocks; Q4_K with Q6_K
for token_embd / output and for attn_v / ffn_down of the blocks llama.cpp keeps there), through the int8-MFMA batch
(LlamaBatch(..., quantized=True), nfai_hip_llama_batch_create_ex); the oracle walks the dequantised weights.

--quant q5_k_m | q8_0 | q4_0 | q3_k_m | iq4_xs: the same on the Q5_K_M mix of tools/q5_k_bench.py, the Q8_0 weights of tools/q8_0_bench.py, the
Q4_0 mix of tools/q4_0_bench.py, the Q3_K_M mix of tools/q3_k_bench.py and the IQ4_XS mix of tools/iq4_xs_bench.py (their generators), through LlamaBatch(..., quantized=True, any_quant=True) (NFAI_BATCH_QUANT | NFAI_BATCH_QUANT_ANY).

    python tools/batch_decode_bench.py --quant q5_k_m --out profiles/batch_decode_q5_k_m.json
    python tools/batch_decode_bench.py --quant q8_0 --out profiles/batch_decode_q8_0.json

--sampled: the reference's DEFAULT sampler on a batch (nfai_hip_llama_batch_step_topk) instead of the greedy comparison.  Same models
and members, n in {1, 2, 4, 8}, positions 517-580 (64 steps per window, >= 3 windows of each form alternating, one untimed first):

  step_topk_ms / step_ms    median wall time of one StepTopK call (temperature 0.5, top-40) and of one blocking
                            Step(want_logits=False) of the same batch: what the candidate launches and the 520 bytes per member add
  sampled batch             StepTopK, then the nucleus cut and the draw on the host per member, the drawn tokens fed back
  sampled sequential        the same n members as single models, LlamaModel.StepTopK + the host nucleus one after another
  logits to the host        Step(want_logits=True) of the batch, then SamplingUtils.TopP over V on the host per member: what a
                            sampling host had to do before _batch_step_topk

Aggregate tokens/s of the three (median over the windows, with their spreads) and the ratios.  Writes
profiles/batch_sampled[_<quant>].json unless --out names another file.

    python tools/batch_decode_bench.py --sampled
    python tools/batch_decode_bench.py --sampled --quant q4_k_m

--wide: the wide batch (nfai_hip_llama_batch_create_wide, LlamaBatch(..., wide=True); fp16 only) against the existing one.  16 members
prepared as above; the same windows and alternation over seven forms: n = 8 through the existing batch, n = 8 / 12 / 16 through the
wide one, and the same 8 / 12 / 16 members stepped sequentially.  Per form ms per step and aggregate tokens/s (median, the windows,
max - min); the bar: wide n = 16 exceeds the EXISTING path's n = 8 aggregate tokens/s by more than the two figures' spreads added
(wide n = 8 against existing n = 8 is recorded beside it).  Plus _batch_profile_step per class at n = 16, and parity in the run: wide
n = 16 against the members' own _decode_step at depth, and against the CPU oracle at 1B.  Writes profiles/batch_decode_wide.json
unless --out names another file.

    python tools/batch_decode_bench.py --wide
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

HBM_PEAK = 8.0e12
T, WARM, NMAX = 512, 5, 8
CLASSES = ["qkv", "attn", "wo", "gateup", "down", "lmhead", "other"]


def class_bytes(weights, dims, positions, kv_esz=4):
    """Algorithmic HBM bytes of ONE launch of each class of a batch step: the weights once, per member its KV rows."""
    KD = dims.Hkv * dims.D
    n = len(positions)
    def wb(name):
        t = weights[name][0]
        return t.numel() * t.element_size()
    def avg(*parts):
        return sum(wb(f"blk.{i}.{p}.weight") for i in range(dims.L) for p in parts) / dims.L
    head = "output.weight" if "output.weight" in weights else "token_embd.weight"
    return {"qkv": avg("attn_q", "attn_k", "attn_v") + n * 2 * KD * kv_esz, "attn": sum(2 * KD * kv_esz * (p + 1) for p in positions),
            "wo": avg("attn_output"), "gateup": avg("ffn_gate", "ffn_up"), "down": avg("ffn_down"), "lmhead": wb(head),
            "other": n * wb("token_embd.weight") // weights["token_embd.weight"][2]}


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


ANY_QUANT = ("q5_k_m", "q8_0", "q4_0", "q3_k_m", "iq4_xs")   # the encodings a batch takes with any_quant=True


def gen_weights(torch, dims, quant):
    """name -> (device tensor, ggml type, rows, cols) in the encoding `quant`."""
    if quant == "q5_k_m":
        import q5_k_bench
        return q5_k_bench.gen_q5_k_m_weights_hbm(torch, dims)
    if quant == "q8_0":
        import q8_0_bench
        return q8_0_bench.gen_q8_0_weights_hbm(torch, dims)
    if quant == "q4_0":
        import q4_0_bench
        return q4_0_bench.gen_q4_0_weights_hbm(torch, dims)
    if quant == "q3_k_m":
        import q3_k_bench
        return q3_k_bench.gen_q3_k_weights_hbm(torch, dims)
    if quant == "iq4_xs":
        import iq4_xs_bench
        return iq4_xs_bench.gen_iq4_xs_weights_hbm(torch, dims)
    import bench as B
    return B.gen_weights_hbm(torch, dims, (0, dims.L), True, True, quant=quant)


def host_weights(weights, quant):
    """What the oracle takes: every quantised matrix dequantised to fp32."""
    if quant == "q5_k_m":
        import q5_k_bench
        return {k: q5_k_bench.dequant(t, ty, r, c) for k, (t, ty, r, c) in weights.items()}
    if quant == "q4_0":
        import q4_0_bench
        return {k: q4_0_bench.dequant(t, ty, r, c) for k, (t, ty, r, c) in weights.items()}
    if quant == "q3_k_m":
        import q3_k_bench
        return {k: q3_k_bench.dequant(t, ty, r, c) for k, (t, ty, r, c) in weights.items()}
    if quant == "iq4_xs":
        import iq4_xs_bench
        return {k: iq4_xs_bench.dequant(t, ty, r, c) for k, (t, ty, r, c) in weights.items()}
    if quant == "q8_0":
        import q8_0_bench
        return {k: (q8_0_bench.dequant_q8_0(t.cpu().numpy(), r, c) if ty == q8_0_bench.Q8_0 else t.cpu().numpy()) for k, (t, ty, r, c) in weights.items()}
    import bench as B
    return B.host_weights(weights)


def run_model(torch, dims, steps, windows, quant="f16"):
    from nfai_amd import synth
    from nfai_amd.hip import HipBufferManager
    from nfai_amd.llama_model import LlamaBatch, LlamaModel
    weights = gen_weights(torch, dims, quant)
    C = T + WARM + steps + 16
    mgr = HipBufferManager(0)
    dd = dict(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, eps=1e-5, rope_dims=dims.D, rope_base=500000.0)
    md = synth.make_metadata(dims)
    wt = {k: (t.data_ptr(), ty, r, c) for k, (t, ty, r, c) in weights.items()}
    members = [LlamaModel(mgr, md, wt, C, max_batch=T, dims=dd)]
    for _ in range(1, NMAX):
        members.append(LlamaModel(mgr, md, wt, C, max_batch=T, dims=dd, share_from=members[0]))
    first = []
    for s, m in enumerate(members):   # every member its own prompt; the tokens of positions 512..516 through its own decode path
        prompt = synth.make_tokens(dims, T, seed=99 + s)
        prompt[0] = 128000 % dims.V
        m.Ingest(prompt)
        tok = int(prompt[-1])
        for _ in range(WARM):
            _, tok = m.Step(tok, want_logits=False)
        first.append(tok)
    p0 = T + WARM

    def rewind(ms):
        for m in ms:
            m.SetPos(p0)

    out = {"model": dims.name, "weights": quant, "kv_cache": "f32", "positions": [p0, p0 + steps - 1], "steps_per_window": steps, "by_n": {}}
    for n in (1, 2, 4, 8):
        ms = members[:n]
        batch = LlamaBatch(ms, quantized=quant != "f16", any_quant=quant in ANY_QUANT)

        def batch_window():
            rewind(ms)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            batch.Greedy(first[:n], steps)
            return time.perf_counter() - t0

        def seq_window():
            rewind(ms)
            for m, tok in zip(ms, first):
                m.SetToken(tok)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                for m in ms:
                    m.Enqueue(1)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        batch_window()   # untimed: graph capture, code objects, every shape of the window
        seq_window()
        bt, sq = [], []
        for _ in range(windows):   # alternating, same positions
            bt.append(batch_window())
            sq.append(seq_window())
        b_tps = [n * steps / t for t in bt]
        s_tps = [n * steps / t for t in sq]
        rewind(ms)
        for m in ms:   # the byte model at the middle of the window
            m.SetPos(p0 + steps // 2)
        bytes_batch = batch.BytesPerToken()
        bytes_seq = sum(m.BytesPerToken(p0 + steps // 2)[0] for m in ms)
        rewind(ms)
        prof = batch.ProfileStep(first[:n])   # eager, one step (it advances the members)
        prof = batch.ProfileStep(first[:n])
        cb = class_bytes(weights, dims, [p0 + 1] * n)
        classes = {}
        for c in CLASSES:
            ms_c, launches = prof[c]
            if not launches:
                continue
            us = ms_c * 1e3 / launches
            classes[c] = {"us_per_launch": us, "launches_per_step": launches, "bytes_per_launch": int(cb[c]),
                          "frac_hbm_roofline": cb[c] / HBM_PEAK / (us * 1e-6) if us > 0 else None}
        med_b, med_s = statistics.median(b_tps), statistics.median(s_tps)
        ms_step = statistics.median(bt) / steps * 1e3
        res = {"batch_ms_per_step": ms_step, "batch_tokens_per_s": med_b, "batch_windows_tokens_per_s": b_tps, "batch_spread": spread(b_tps),
               "sequential_tokens_per_s": med_s, "sequential_windows_tokens_per_s": s_tps, "sequential_spread": spread(s_tps),
               "speedup": med_b / med_s, "above_sequential_by_more_than_its_spread": med_b > med_s * (1 + spread(s_tps)),
               "batch_bytes_per_step": bytes_batch, "sequential_bytes_per_round": bytes_seq, "byte_model_ratio": bytes_batch / bytes_seq,
               "fraction_of_byte_model_reached": (med_b / med_s) / (bytes_seq / bytes_batch),
               "step_frac_of_8TBps": bytes_batch / (ms_step * 1e-3) / HBM_PEAK, "launches_per_step": sum(v[1] for v in prof.values()),
               "kernel_classes": classes}
        if n == 4:   # the batch against the members' own decode path at depth, 4 positions
            rewind(ms)
            cur, worst, top = list(first[:n]), 0.0, 0.0
            solo = []
            for i, m in enumerate(ms):
                tok, rows = first[i], []
                for _ in range(4):
                    lg, tok = m.Step(tok)
                    rows.append(lg)
                solo.append(rows)
            rewind(ms)
            for p in range(4):
                lg, am = batch.Step(cur)
                for i in range(n):
                    worst = max(worst, float(np.abs(lg[i] - solo[i][p]).max()))
                    top = max(top, float(np.abs(solo[i][p]).max()))
                cur = [int(np.argmax(solo[i][p])) for i in range(n)]
            res["parity_vs_decode_step_at_depth"] = {"positions": [p0, p0 + 3], "max_abs_logit_diff": worst, "max_abs_logit": top}
        out["by_n"][str(n)] = res
        batch.Dispose()
    for m in reversed(members):
        m.Dispose()
    mgr.Dispose()
    return out


def run_sampled(torch, dims, steps, windows, quant="f16"):
    """--sampled: see the module docstring."""
    from nfai_amd import synth
    from nfai_amd.hip import HipBufferManager
    from nfai_amd.llama_model import LlamaBatch, LlamaModel, SamplingUtils
    weights = gen_weights(torch, dims, quant)
    C = T + WARM + steps + 16
    mgr = HipBufferManager(0)
    dd = dict(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, eps=1e-5, rope_dims=dims.D, rope_base=500000.0)
    md = synth.make_metadata(dims)
    wt = {k: (t.data_ptr(), ty, r, c) for k, (t, ty, r, c) in weights.items()}
    members = [LlamaModel(mgr, md, wt, C, max_batch=T, dims=dd)]
    for _ in range(1, NMAX):
        members.append(LlamaModel(mgr, md, wt, C, max_batch=T, dims=dd, share_from=members[0]))
    first = []
    for s, m in enumerate(members):
        prompt = synth.make_tokens(dims, T, seed=99 + s)
        prompt[0] = 128000 % dims.V
        m.Ingest(prompt)
        tok = int(prompt[-1])
        for _ in range(WARM):
            _, tok = m.Step(tok, want_logits=False)
        first.append(tok)
    p0 = T + WARM
    out = {"model": dims.name, "weights": quant, "kv_cache": "f32", "positions": [p0, p0 + steps - 1], "steps_per_window": steps,
           "temperature": 0.5, "top_k": 40, "top_p": 0.95, "by_n": {}}
    for n in (1, 2, 4, 8):
        ms = members[:n]
        batch = LlamaBatch(ms, quantized=quant != "f16", any_quant=quant in ANY_QUANT)

        def window(step):
            """steps calls of step(tokens) -> next tokens, from the same positions: (seconds, seconds of every call)."""
            for m in ms:
                m.SetPos(p0)
            toks, each = list(first[:n]), []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                t1 = time.perf_counter()
                toks = step(toks)
                each.append(time.perf_counter() - t1)
            return time.perf_counter() - t0, each

        rng = np.random.Generator(np.random.PCG64(7))

        def step_topk_only(toks):
            ids, _ = batch.StepTopK(toks)
            return [int(i[0]) for i in ids]

        def step_only(toks):
            return [int(t) for t in batch.Step(toks, want_logits=False)[1]]

        def sampled_batch(toks):
            ids, probs = batch.StepTopK(toks)
            return [SamplingUtils.TopPFromCandidates(ids[i], probs[i], rng=rng) for i in range(n)]

        def sampled_sequential(toks):
            nxt = []
            for m, tok in zip(ms, toks):
                ids, probs = m.StepTopK(tok)
                nxt.append(SamplingUtils.TopPFromCandidates(ids, probs, rng=rng))
            return nxt

        def logits_host(toks):
            lg, _ = batch.Step(toks, want_logits=True)
            return [SamplingUtils.TopP(lg[i], rng=rng) for i in range(n)]

        forms = {"step_topk": step_topk_only, "step": step_only, "sampled_batch": sampled_batch,
                 "sampled_sequential": sampled_sequential, "logits_to_host": logits_host}
        for f in forms.values():   # untimed: graph capture, code objects
            window(f)
        secs = {k: [] for k in forms}
        calls = {k: [] for k in forms}
        for _ in range(windows):   # alternating, same positions
            for k, f in forms.items():
                t, each = window(f)
                secs[k].append(t)
                calls[k].extend(each)
        tps = {k: [n * steps / t for t in v] for k, v in secs.items()}
        med = {k: statistics.median(v) for k, v in tps.items()}
        topk_ms, step_ms = statistics.median(calls["step_topk"]) * 1e3, statistics.median(calls["step"]) * 1e3
        out["by_n"][str(n)] = {
            "step_topk_ms": topk_ms, "step_ms": step_ms, "step_topk_over_step": topk_ms / step_ms,
            "sampled_batch_tokens_per_s": med["sampled_batch"], "sampled_batch_spread": spread(tps["sampled_batch"]),
            "sampled_sequential_tokens_per_s": med["sampled_sequential"], "sampled_sequential_spread": spread(tps["sampled_sequential"]),
            "logits_to_host_tokens_per_s": med["logits_to_host"], "logits_to_host_spread": spread(tps["logits_to_host"]),
            "speedup_over_sequential": med["sampled_batch"] / med["sampled_sequential"],
            "speedup_over_logits_to_host": med["sampled_batch"] / med["logits_to_host"],
            "bytes_to_host_per_step": {"step_topk": n * 520 + 36, "logits_to_host": n * dims.V * 4 + 36}}
        batch.Dispose()
    for m in reversed(members):
        m.Dispose()
    mgr.Dispose()
    return out


def run_wide(torch, dims, steps, windows):
    """--wide: see the module docstring."""
    from nfai_amd import synth
    from nfai_amd.hip import HipBufferManager
    from nfai_amd.llama_model import LlamaBatch, LlamaModel
    NW = 16
    weights = gen_weights(torch, dims, "f16")
    C = T + WARM + steps + 16
    mgr = HipBufferManager(0)
    dd = dict(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, eps=1e-5, rope_dims=dims.D, rope_base=500000.0)
    md = synth.make_metadata(dims)
    wt = {k: (t.data_ptr(), ty, r, c) for k, (t, ty, r, c) in weights.items()}
    members = [LlamaModel(mgr, md, wt, C, max_batch=T, dims=dd)]
    for _ in range(1, NW):
        members.append(LlamaModel(mgr, md, wt, C, max_batch=T, dims=dd, share_from=members[0]))
    first = []
    for s, m in enumerate(members):
        prompt = synth.make_tokens(dims, T, seed=99 + s)
        prompt[0] = 128000 % dims.V
        m.Ingest(prompt)
        tok = int(prompt[-1])
        for _ in range(WARM):
            _, tok = m.Step(tok, want_logits=False)
        first.append(tok)
    p0 = T + WARM

    def rewind(ms):
        for m in ms:
            m.SetPos(p0)

    def batch_form(batch, n):
        def window():
            rewind(members[:n])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            batch.Greedy(first[:n], steps)
            return time.perf_counter() - t0
        return window

    def seq_form(n):
        def window():
            rewind(members[:n])
            for m, tok in zip(members[:n], first):
                m.SetToken(tok)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                for m in members[:n]:
                    m.Enqueue(1)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        return window

    batches = {"batch_8": (LlamaBatch(members[:8]), 8), "wide_8": (LlamaBatch(members[:8], wide=True), 8),
               "wide_12": (LlamaBatch(members[:12], wide=True), 12), "wide_16": (LlamaBatch(members, wide=True), 16)}
    forms = {k: (batch_form(b, n), n) for k, (b, n) in batches.items()}
    forms.update({f"sequential_{n}": (seq_form(n), n) for n in (8, 12, 16)})
    for f, _ in forms.values():   # untimed: graph capture, code objects, every shape of the window
        f()
    secs = {k: [] for k in forms}
    for _ in range(windows):      # alternating, same positions
        for k, (f, _) in forms.items():
            secs[k].append(f())
    out = {"model": dims.name, "weights": "f16", "kv_cache": "f32", "positions": [p0, p0 + steps - 1], "steps_per_window": steps, "forms": {}}
    for k, (_, n) in forms.items():
        tps = [n * steps / t for t in secs[k]]
        out["forms"][k] = {"n": n, "ms_per_step": statistics.median(secs[k]) / steps * 1e3, "tokens_per_s": statistics.median(tps),
                           "windows_tokens_per_s": tps, "spread_tokens_per_s": max(tps) - min(tps), "spread": spread(tps)}
    fm = out["forms"]
    for n in (8, 12, 16):
        fm[f"wide_{n}"]["speedup_over_sequential"] = fm[f"wide_{n}"]["tokens_per_s"] / fm[f"sequential_{n}"]["tokens_per_s"]
    gain = fm["wide_16"]["tokens_per_s"] - fm["batch_8"]["tokens_per_s"]
    out["bar"] = {"wide_16_over_batch_8": fm["wide_16"]["tokens_per_s"] / fm["batch_8"]["tokens_per_s"],
                  "wide_8_over_batch_8": fm["wide_8"]["tokens_per_s"] / fm["batch_8"]["tokens_per_s"],
                  "gain_tokens_per_s": gain, "spreads_added_tokens_per_s": fm["wide_16"]["spread_tokens_per_s"] + fm["batch_8"]["spread_tokens_per_s"],
                  "met": gain > fm["wide_16"]["spread_tokens_per_s"] + fm["batch_8"]["spread_tokens_per_s"]}
    # the byte model and the launch classes at n = 16
    w16 = batches["wide_16"][0]
    for m in members:
        m.SetPos(p0 + steps // 2)
    bytes16 = w16.BytesPerToken()
    for m in members[:8]:
        m.SetPos(p0 + steps // 2)
    bytes8 = batches["batch_8"][0].BytesPerToken()
    out["bytes_per_step"] = {"wide_16": bytes16, "batch_8": bytes8}
    out["step_frac_of_8TBps"] = {"wide_16": bytes16 / (fm["wide_16"]["ms_per_step"] * 1e-3) / HBM_PEAK,
                                 "batch_8": bytes8 / (fm["batch_8"]["ms_per_step"] * 1e-3) / HBM_PEAK}
    classes = {}
    for key, n in (("wide_16", 16), ("batch_8", 8)):
        b = batches[key][0]
        rewind(members[:n])
        b.ProfileStep(first[:n])   # eager, one step (it advances the members)
        prof = b.ProfileStep(first[:n])
        cb = class_bytes(weights, dims, [p0 + 1] * n)
        classes[key] = {}
        for c in CLASSES:
            ms_c, launches = prof[c]
            if launches:
                us = ms_c * 1e3 / launches
                classes[key][c] = {"us_per_launch": us, "launches_per_step": launches, "us_per_step": ms_c * 1e3, "bytes_per_launch": int(cb[c]),
                                   "frac_hbm_roofline": cb[c] / HBM_PEAK / (us * 1e-6) if us > 0 else None}
    out["kernel_classes"] = classes
    # wide n = 16 against the members' own decode path at depth, 4 positions
    rewind(members)
    solo = []
    for i, m in enumerate(members):
        tok, rows = first[i], []
        for _ in range(4):
            lg, tok = m.Step(tok)
            rows.append(lg)
        solo.append(rows)
    rewind(members)
    cur, worst, top = list(first), 0.0, 0.0
    for p in range(4):
        lg, am = w16.Step(cur)
        for i in range(NW):
            worst = max(worst, float(np.abs(lg[i] - solo[i][p]).max()))
            top = max(top, float(np.abs(solo[i][p]).max()))
        cur = [int(np.argmax(solo[i][p])) for i in range(NW)]
    out["parity_vs_decode_step_at_depth"] = {"n": NW, "positions": [p0, p0 + 3], "max_abs_logit_diff": worst, "max_abs_logit": top}
    for b, _ in batches.values():
        b.Dispose()
    for m in reversed(members):
        m.Dispose()
    mgr.Dispose()
    return out


def oracle_parity(torch, dims, n=4, quant="f16", wide=False):
    """n = 4 on full-size weights at shallow staggered depths (the oracle walks every earlier token on the host): max |dlogit| over 4 steps."""
    import oracle as orc
    from nfai_amd import synth
    from nfai_amd.hip import HipBufferManager
    from nfai_amd.llama_model import LlamaBatch, LlamaModel
    weights = gen_weights(torch, dims, quant)
    C = 32
    mgr = HipBufferManager(0)
    dd = dict(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, eps=1e-5, rope_dims=dims.D, rope_base=500000.0)
    md = synth.make_metadata(dims)
    wt = {k: (t.data_ptr(), ty, r, c) for k, (t, ty, r, c) in weights.items()}
    ms = [LlamaModel(mgr, md, wt, C, dims=dd)]
    for _ in range(1, n):
        ms.append(LlamaModel(mgr, md, wt, C, dims=dd, share_from=ms[0]))
    host = host_weights(weights, quant)   # quantised matrices dequantised
    toks = [synth.make_tokens(dims, 24, seed=400 + s) for s in range(n)]
    refs = []
    for s in range(n):
        ref = orc.OracleLlama(orc.LlamaDesc(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, C=C), host)
        for t in toks[s][:2 + (s if wide else 3 * s)]:
            ms[s].Step(int(t), want_logits=False)
            ref.step(int(t), want_logits=False)
        refs.append(ref)
    batch = LlamaBatch(ms, wide=True) if wide else LlamaBatch(ms, quantized=quant != "f16", any_quant=quant in ANY_QUANT)
    worst, top, same = 0.0, 0.0, []
    for i in range(4):
        st = [int(toks[s][2 + (s if wide else 3 * s) + i]) for s in range(n)]
        lg, am = batch.Step(st)
        for s in range(n):
            want = refs[s].step(st[s])
            worst = max(worst, float(np.abs(lg[s] - want).max()))
            top = max(top, float(np.abs(want).max()))
            same.append(int(orc.argmax(want)) == int(am[s]))
    batch.Dispose()
    for m in reversed(ms):
        m.Dispose()
    mgr.Dispose()
    return {"model": dims.name, "weights": quant, "n": n, "positions_of_member_0": [2, 5], "max_abs_logit_diff": worst, "max_abs_logit": top, "argmax_equal": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--only", default="", metavar="MODEL", help="one model, e.g. llama-3.2-3b")
    ap.add_argument("--quant", default="f16", choices=["f16", "q4_k_m", "q5_k_m", "q8_0", "q4_0", "q3_k_m", "iq4_xs"], help="weight encoding (all but f16: the int8-MFMA batch)")
    ap.add_argument("--sampled", action="store_true", help="the default sampler on a batch (StepTopK) instead of the greedy comparison")
    ap.add_argument("--wide", action="store_true", help="the wide batch (up to 16 members, fp16 MFMA) against the existing one")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from nfai_amd import synth
    torch.cuda.set_device(0)
    if a.wide:
        if a.quant != "f16":
            ap.error("--wide takes fp16 weights only")
        out = {"tool": "batch_decode_bench --wide", "weights": "f16", "models": []}
        for dims in (synth.LLAMA_32_3B, synth.LLAMA_32_1B):
            if a.only and a.only != dims.name:
                continue
            out["models"].append(run_wide(torch, dims, a.steps, max(3, a.windows)))
            torch.cuda.empty_cache()
        if not a.no_check:
            out["parity_vs_oracle"] = oracle_parity(torch, synth.LLAMA_32_1B, n=16, wide=True)
        line = json.dumps(out)
        print(line)
        path = a.out or os.path.join(ROOT, "profiles", "batch_decode_wide.json")
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")
        return
    if a.sampled:
        out = {"tool": "batch_decode_bench --sampled", "weights": a.quant, "models": []}
        for dims in (synth.LLAMA_32_3B, synth.LLAMA_32_1B):
            if a.only and a.only != dims.name:
                continue
            out["models"].append(run_sampled(torch, dims, 64, max(3, a.windows), a.quant))
            torch.cuda.empty_cache()
        line = json.dumps(out)
        print(line)
        path = a.out or os.path.join(ROOT, "profiles", "batch_sampled%s.json" % ("" if a.quant == "f16" else "_" + a.quant))
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")
        return
    out = {"tool": "batch_decode_bench", "weights": a.quant, "models": []}
    for dims in (synth.LLAMA_32_3B, synth.LLAMA_32_1B):
        if a.only and a.only != dims.name:
            continue
        out["models"].append(run_model(torch, dims, a.steps, max(3, a.windows), a.quant))
        torch.cuda.empty_cache()
    if not a.no_check:
        out["parity_vs_oracle"] = oracle_parity(torch, synth.LLAMA_32_1B, quant=a.quant)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
