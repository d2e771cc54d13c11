"""Q5_K_M decode and prefill on synthetic Llama-3.2-3B / -1B weights built in HBM, next to the same models in fp16 and Q4_K_M in the
same run.

Q5_K_M: the tensor mix of synth.q5_k_m_type (Q5_K, Q6_K for attn_v / ffn_down of the use_more_bits blocks and for the tied lm_head),
random codes and sub-scales with fixed fp16 d = 5e-5, dmin = 8e-4 (Q5_K; the magnitude of bench.py's Q4_K blocks with twice the
codes) and d = 2e-5 (Q6_K, as bench.py); gains f32 1 + N(0, 0.1^2).  fp16 and Q4_K_M: bench.gen_weights_hbm.  Per model: a 512-token
ingest (bench.py's prompt, seed 99), five greedy steps, then greedy decode from position 517 in >= 3 windows of --steps tokens
(tokens/s: their median), prefill ms, _bytes_per_token and its fraction of 8 TB/s, per-kernel-class us per launch from
_profile_kernel with the algorithmic bytes of one launch and its fraction of the HBM roofline, and (Q5_K_M) max |dlogit| against
the oracle on weights dequantised by this file's restatement of ggml's dequantize_row_q5_K at 4 positions.  One JSON line; --out
writes it to a file too.

    python tools/q5_k_bench.py --out q5_k_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

Q4_K, Q5_K, Q6_K = 12, 13, 14
HBM_PEAK = 8.0e12
BLOCK_BYTES = {Q4_K: 144, Q5_K: 176, Q6_K: 210}


def gen_q5_k_m_weights_hbm(torch, dims, seed=1234):
    """name -> (uint8 tensor of native Q5_K / Q6_K blocks | f32 gains, ggml type, rows, cols), generated on the device in the mix
    of synth.q5_k_m_type."""
    from nfai_amd.synth import q5_k_m_type
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    hdr5 = torch.tensor([5.0e-5, 8.0e-4], dtype=torch.float16).view(torch.uint8).to("cuda")
    d6 = torch.tensor([2.0e-5], dtype=torch.float16).view(torch.uint8).to("cuda")
    out = {}
    for name, shape in dims.shapes().items():
        if len(shape) == 1:
            out[name] = (1.0 + 0.1 * torch.randn(shape, device="cuda", dtype=torch.float32, generator=g), 0, 1, shape[0])
            continue
        ty = q5_k_m_type(name, dims)
        t = torch.randint(0, 256, (shape[0] * shape[1] // 256, BLOCK_BYTES[ty]), device="cuda", dtype=torch.uint8, generator=g)
        if ty == Q5_K:
            t[:, 0:4] = hdr5
        else:
            t[:, 208:210] = d6
        out[name] = (t, ty, shape[0], shape[1])
    torch.cuda.synchronize()
    return out


def dequant_q5_k(raw, rows, cols):
    """ggml dequantize_row_q5_K on native 176-byte blocks (fp16 d, fp16 dmin, scales[12], qh[32], qs[128]), in row chunks."""
    b = np.ascontiguousarray(raw, np.uint8).reshape(-1, 176)
    out = np.empty((b.shape[0], 256), np.float32)
    n4 = np.arange(4, dtype=np.uint8)[None, :, None]
    for c0 in range(0, b.shape[0], 1 << 16):
        x = b[c0:c0 + (1 << 16)]
        d = x[:, 0:2].copy().view(np.float16).astype(np.float32)
        dmin = x[:, 2:4].copy().view(np.float16).astype(np.float32)
        s = x[:, 4:16]
        sc = np.concatenate([s[:, 0:4] & 63, (s[:, 8:12] & 0xF) | ((s[:, 0:4] >> 6) << 4)], axis=1).astype(np.float32)
        mn = np.concatenate([s[:, 4:8] & 63, (s[:, 8:12] >> 4) | ((s[:, 4:8] >> 6) << 4)], axis=1).astype(np.float32)
        qh, qs = x[:, None, 16:48], x[:, 48:176].reshape(-1, 4, 32)
        q = np.empty((x.shape[0], 4, 2, 32), np.float32)
        q[:, :, 0] = (qs & 0xF) | (((qh >> (2 * n4)) & 1) << 4)
        q[:, :, 1] = (qs >> 4) | (((qh >> (2 * n4 + 1)) & 1) << 4)
        q = q.reshape(-1, 8, 32)
        out[c0:c0 + x.shape[0]] = ((d * sc)[:, :, None] * q - (dmin * mn)[:, :, None]).reshape(-1, 256)
    return out.reshape(rows, cols)


def dequant(t, ty, rows, cols):
    import oracle as orc
    a = t.cpu().numpy()
    if ty == Q5_K:
        return dequant_q5_k(a, rows, cols)
    if ty == Q6_K:
        return orc.dequant_q6k(a.reshape(-1), rows * cols).reshape(rows, cols)
    if ty == Q4_K:
        return orc.dequant_q4k(a.reshape(-1), rows * cols).reshape(rows, cols)
    return a


CLASSES = ["qkv", "attn", "wo", "gateup", "down", "lmhead"]


def class_bytes(weights, dims, pos, kv_esz=4):
    """Algorithmic HBM bytes of ONE launch of each class at position pos, averaged over the blocks (weights once in their encoding;
    attention: K and V rows 0..pos of a block)."""
    KD = dims.Hkv * dims.D
    def wb(name):
        t, ty, r, c = weights[name]
        return t.numel() * t.element_size()
    def avg(*parts):
        return sum(wb(f"blk.{i}.{p}.weight") for i in range(dims.L) for p in parts) / dims.L
    head = "output.weight" if "output.weight" in weights else "token_embd.weight"
    return {"qkv": avg("attn_q", "attn_k", "attn_v") + 2 * KD * kv_esz, "attn": 2 * KD * kv_esz * (pos + 1), "wo": avg("attn_output"),
            "gateup": avg("ffn_gate", "ffn_up"), "down": avg("ffn_down"), "lmhead": wb(head)}


def run_model(torch, dims, quant, steps, windows, check):
    import bench as B
    import oracle as orc
    from nfai_amd import synth
    from nfai_amd.hip import HipBufferManager
    from nfai_amd.llama_model import LlamaModel
    T, warm = 512, 5
    weights = gen_q5_k_m_weights_hbm(torch, dims) if quant == "q5_k_m" else B.gen_weights_hbm(torch, dims, (0, dims.L), True, True, quant=quant)
    C = T + warm + steps * windows + 8
    mgr = HipBufferManager(0)
    dd = dict(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, eps=1e-5, rope_dims=dims.D, rope_base=500000.0)
    m = LlamaModel(mgr, synth.make_metadata(dims), {k: (t.data_ptr(), ty, r, c) for k, (t, ty, r, c) in weights.items()}, C,
                   max_batch=T, dims=dd)
    prompt = synth.make_tokens(dims, T, seed=99)
    prompt[0] = 128000 % dims.V
    m.Prefill(prompt[:64])          # warm every prefill shape
    m.Reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    first = m.Prefill(prompt)
    torch.cuda.synchronize()
    prefill_ms = (time.perf_counter() - t0) * 1e3
    tok = int(np.argmax(first))
    got = [first]
    toks = [tok]
    for _ in range(warm - 1):        # positions 512..515 -> the timed windows start at 517 (bench.py)
        lg, tok = m.Step(tok)
        got.append(lg)
        toks.append(tok)
    lg, tok = m.Step(tok)
    rates = []
    m.SetToken(tok)
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.Enqueue(steps)
        torch.cuda.synchronize()
        rates.append(steps / (time.perf_counter() - t0))
    pos = m.Pos
    total, dom = m.BytesPerToken(pos)
    tps = statistics.median(rates)
    cb = class_bytes(weights, dims, pos)
    classes = {}
    from nfai_amd._lib import NfaiHipError
    for c in CLASSES:
        try:
            us = m.ProfileKernel(tok, c, reps=8)
        except NfaiHipError:   # fp16: Wo rides on the attention launch (no launch of class "wo"); its bytes are counted there
            continue
        by = cb[c] + (cb["wo"] if c == "attn" and quant == "f16" else 0)
        classes[c] = {"us_per_launch": us, "launches_per_token": 1 if c == "lmhead" else dims.L, "bytes_per_launch": int(by),
                      "frac_hbm_roofline": by / HBM_PEAK / (us * 1e-6) if us > 0 else None}
    res = {"model": dims.name, "weights": quant, "decode_tokens_per_s": tps, "windows_tokens_per_s": rates, "steps_per_window": steps,
           "positions": [T + warm, pos - 1], "prefill_ms_512": prefill_ms, "bytes_per_token": total, "dominant_bytes": dom,
           "token_frac_of_8TBps": total * tps / HBM_PEAK, "kernel_classes": classes}
    m.Dispose()
    mgr.Dispose()
    if check:
        host = {k: dequant(t, ty, r, c) for k, (t, ty, r, c) in weights.items()}
        del weights
        ref = orc.OracleLlama(orc.LlamaDesc(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, C=T + 8), host)
        for t in prompt[:-1]:
            ref.step(int(t), want_logits=False)
        wants = [ref.step(int(prompt[-1]))] + [ref.step(t) for t in toks[:3]]
        res["parity_vs_oracle"] = {
            "positions": [T - 1, T, T + 1, T + 2],
            "max_abs_logit_diff": max(float(np.abs(g - w).max()) for g, w in zip(got[:4], wants)),
            "max_abs_logit": max(float(np.abs(w).max()) for w in wants),
            "greedy_tokens_equal": [int(orc.argmax(w)) == t for w, t in zip(wants, toks[:4])]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="", metavar="MODEL:QUANT", help="one run, e.g. llama-3.2-3b:q5_k_m (for a profiler's kernel trace)")
    a = ap.parse_args()
    import torch
    from nfai_amd import synth
    torch.cuda.set_device(0)
    out = {"tool": "q5_k_bench", "models": []}
    for dims in (synth.LLAMA_32_3B, synth.LLAMA_32_1B):
        for quant in ("q5_k_m", "q4_k_m", "f16"):
            if a.only and a.only != f"{dims.name}:{quant}":
                continue
            out["models"].append(run_model(torch, dims, quant, a.steps, max(3, a.windows), quant == "q5_k_m" and not a.no_check))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
