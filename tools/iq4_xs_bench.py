"""IQ4_XS decode and prefill on synthetic Llama-3.2-3B / -1B weights built in HBM, next to the same models in Q4_K_M and Q4_0 in
the same run.

IQ4_XS: the tensor mix of synth.iq4_xs_type (IQ4_XS everywhere, attn_v in Q5_K when H / Hkv >= 4, ffn_down of the first
n_layer // 8 blocks in Q5_K, the tied lm_head Q6_K; --mix all_iq4_xs: every matrix IQ4_XS), random IQ4_XS blocks with fp16
d = 1.6e-5 (weights ~0.02 as bench.py's fp16 N(0, 0.02^2): ls - 32 and the code uniform), Q5_K blocks as tools/q5_k_bench.py's, Q6_K
as bench.py's; gains f32 1 + N(0, 0.1^2).  Q4_K_M: bench.gen_weights_hbm; Q4_0: tools/q4_0_bench.py's generator.  The three
encodings of a model are resident together and their timed windows ALTERNATE (window w of IQ4_XS, of Q4_K_M, of Q4_0, then window
w + 1 ...), so that drift of the card touches all three alike.  Per model and encoding: a 512-token ingest (bench.py's prompt, seed
99), five greedy steps, then greedy decode from position 517 in >= 3 windows of --steps tokens (tokens/s: median, min and max),
prefill ms, _bytes_per_token and its fraction of 8 TB/s, per-kernel-class us per launch from _profile_kernel with the algorithmic
bytes of one launch and its fraction of the HBM roofline, and (IQ4_XS) max |dlogit| and greedy-token equality against the oracle on
weights dequantised by synth.dequantize_iq4_xs (the restatement of ggml's block_iq4_xs) at 4 positions.  One JSON line; --out
writes it to a file too.

    python tools/iq4_xs_bench.py --out profiles/iq4_xs_bench.json
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

Q4_0, Q4_K, Q5_K, Q6_K, IQ4_XS = 2, 12, 13, 14, 23
HBM_PEAK = 8.0e12


def gen_iq4_xs_weights_hbm(torch, dims, seed=1234, d=1.6e-5, mix="iq4_xs"):
    """name -> (uint8 tensor of native IQ4_XS / Q5_K / Q6_K blocks | f32 gains, ggml type, rows, cols), generated on the device in
    the mix of synth.iq4_xs_type."""
    from nfai_amd.synth import iq4_xs_type
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    d4 = torch.tensor([d], dtype=torch.float16).view(torch.uint8).to("cuda")
    hdr5 = torch.tensor([5.0e-5, 8.0e-4], dtype=torch.float16).view(torch.uint8).to("cuda")
    d6 = torch.tensor([2.0e-5], dtype=torch.float16).view(torch.uint8).to("cuda")
    block = {IQ4_XS: 136, Q5_K: 176, Q6_K: 210}
    out = {}
    for name, shape in dims.shapes().items():
        if len(shape) == 1:
            out[name] = (1.0 + 0.1 * torch.randn(shape, device="cuda", dtype=torch.float32, generator=g), 0, 1, shape[0])
            continue
        ty = iq4_xs_type(name, dims, mix)
        t = torch.randint(0, 256, (shape[0] * shape[1] // 256, block[ty]), device="cuda", dtype=torch.uint8, generator=g)
        if ty == IQ4_XS:
            t[:, 0:2] = d4
        elif ty == Q5_K:
            t[:, 0:4] = hdr5
        else:
            t[:, 208:210] = d6
        out[name] = (t, ty, shape[0], shape[1])
    torch.cuda.synchronize()
    return out


def dequant(t, ty, rows, cols):
    import oracle as orc
    from nfai_amd.synth import dequantize_iq4_xs
    a = t.cpu().numpy()
    if ty == IQ4_XS:
        rb = cols // 256 * 136
        out = np.empty((rows, cols), np.float32)
        for r0 in range(0, rows, 4096):   # in row chunks
            r1 = min(rows, r0 + 4096)
            out[r0:r1] = dequantize_iq4_xs(a.reshape(-1)[r0 * rb:r1 * rb].tobytes(), r1 - r0, cols)
        return out
    if ty == Q5_K:
        import q5_k_bench
        return q5_k_bench.dequant_q5_k(a, rows, cols)
    if ty == Q6_K:
        return orc.dequant_q6k(a.reshape(-1), rows * cols).reshape(rows, cols)
    return a


CLASSES = ["qkv", "attn", "wo", "gateup", "down", "lmhead"]


def class_bytes(weights, dims, pos, kv_esz=4):
    """Algorithmic HBM bytes of ONE launch of each class at position pos, averaged over the blocks (weights once in their encoding;
    attention: K and V rows 0..pos of a block)."""
    KD = dims.Hkv * dims.D

    def wb(name):
        t = weights[name][0]
        return t.numel() * t.element_size()

    def avg(*parts):
        return sum(wb(f"blk.{i}.{p}.weight") for i in range(dims.L) for p in parts) / dims.L

    head = "output.weight" if "output.weight" in weights else "token_embd.weight"
    return {"qkv": avg("attn_q", "attn_k", "attn_v") + 2 * KD * kv_esz, "attn": 2 * KD * kv_esz * (pos + 1), "wo": avg("attn_output"),
            "gateup": avg("ffn_gate", "ffn_up"), "down": avg("ffn_down"), "lmhead": wb(head)}


def gen(torch, dims, quant, mix):
    import bench as B
    if quant == "iq4_xs":
        return gen_iq4_xs_weights_hbm(torch, dims, mix=mix)
    if quant == "q4_0":
        import q4_0_bench as QB
        return QB.gen_q4_0_weights_hbm(torch, dims)
    return B.gen_weights_hbm(torch, dims, (0, dims.L), True, True, quant=quant)


def run_dims(torch, dims, quants, steps, windows, check, mix):
    import oracle as orc
    from nfai_amd import synth
    from nfai_amd._lib import NfaiHipError
    from nfai_amd.hip import HipBufferManager
    from nfai_amd.llama_model import LlamaModel
    T, warm = 512, 5
    C = T + warm + steps * windows + 8
    dd = dict(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, eps=1e-5, rope_dims=dims.D, rope_base=500000.0)
    prompt = synth.make_tokens(dims, T, seed=99)
    prompt[0] = 128000 % dims.V
    mgr = HipBufferManager(0)
    runs = {}
    for quant in quants:   # the encodings of this model, resident together
        weights = gen(torch, dims, quant, mix)
        m = LlamaModel(mgr, synth.make_metadata(dims), {k: (t.data_ptr(), ty, r, c) for k, (t, ty, r, c) in weights.items()}, C,
                       max_batch=T, dims=dd)
        m.Prefill(prompt[:64])          # warm every prefill shape
        m.Reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first = m.Prefill(prompt)
        torch.cuda.synchronize()
        prefill_ms = (time.perf_counter() - t0) * 1e3
        tok = int(np.argmax(first))
        got, toks = [first], [tok]
        for _ in range(warm - 1):        # positions 512..515 -> the timed windows start at 517 (bench.py)
            lg, tok = m.Step(tok)
            got.append(lg)
            toks.append(tok)
        lg, tok = m.Step(tok)
        m.SetToken(tok)
        runs[quant] = dict(m=m, weights=weights, prefill_ms=prefill_ms, got=got, toks=toks, tok=tok, rates=[])
    for _ in range(windows):             # alternating windows
        for quant in quants:
            r = runs[quant]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r["m"].Enqueue(steps)
            torch.cuda.synchronize()
            r["rates"].append(steps / (time.perf_counter() - t0))
    results = []
    for quant in quants:
        r = runs[quant]
        m = r["m"]
        pos = m.Pos
        total, dom = m.BytesPerToken(pos)
        tps = statistics.median(r["rates"])
        cb = class_bytes(r["weights"], dims, pos)
        classes = {}
        prof = m.ProfileStep(r["tok"])
        for c in CLASSES:
            try:
                us = m.ProfileKernel(r["tok"], c, reps=8)
            except NfaiHipError:
                continue
            classes[c] = {"us_per_launch": us, "launches_per_token": int(prof[c][1]) if c in prof else (1 if c == "lmhead" else dims.L),
                          "bytes_per_launch": int(cb[c]), "frac_hbm_roofline": cb[c] / HBM_PEAK / (us * 1e-6) if us > 0 else None}
        res = {"model": dims.name, "weights": quant + (f":{mix}" if quant == "iq4_xs" and mix != "iq4_xs" else ""), "decode_tokens_per_s": tps,
               "windows_tokens_per_s": r["rates"], "spread_tokens_per_s": [min(r["rates"]), max(r["rates"])], "steps_per_window": steps,
               "positions": [T + warm, pos - 1], "prefill_ms_512": r["prefill_ms"], "bytes_per_token": total, "dominant_bytes": dom,
               "token_frac_of_8TBps": total * tps / HBM_PEAK, "kernel_classes": classes}
        m.Dispose()
        results.append(res)
    mgr.Dispose()
    if check and "iq4_xs" in runs:
        r = runs["iq4_xs"]
        host = {k: dequant(t, ty, rr, c) for k, (t, ty, rr, c) in r["weights"].items()}
        for q in quants:
            runs[q]["weights"] = None
        ref = orc.OracleLlama(orc.LlamaDesc(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, C=T + 8), host)
        for t in prompt[:-1]:
            ref.step(int(t), want_logits=False)
        wants = [ref.step(int(prompt[-1]))] + [ref.step(t) for t in r["toks"][:3]]
        results[quants.index("iq4_xs")]["parity_vs_oracle"] = {
            "positions": [T - 1, T, T + 1, T + 2],
            "max_abs_logit_diff": max(float(np.abs(g - w).max()) for g, w in zip(r["got"][:4], wants)),
            "max_abs_logit": max(float(np.abs(w).max()) for w in wants),
            "greedy_tokens_equal": [int(orc.argmax(w)) == t for w, t in zip(wants, r["toks"][:4])]}
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--mix", default="iq4_xs", choices=["iq4_xs", "all_iq4_xs"])
    ap.add_argument("--models", default="llama-3.2-3b,llama-3.2-1b")
    ap.add_argument("--check", default="llama-3.2-3b,llama-3.2-1b", help="models whose IQ4_XS run is compared with the oracle ('' = none)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from nfai_amd import synth
    torch.cuda.set_device(0)
    out = {"tool": "iq4_xs_bench", "models": []}
    for name in [n for n in a.models.split(",") if n]:
        dims = synth.BY_NAME[name]
        out["models"] += run_dims(torch, dims, ["iq4_xs", "q4_k_m", "q4_0"], a.steps, max(3, a.windows), name in a.check.split(","), a.mix)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
