"""Q8_0 decode and prefill on synthetic Llama-3.2-3B / -1B weights built in HBM, next to the same models in fp16 in the same run.

Q8_0: every matrix (and the tied token_embd) as random int8 codes with fp16 d = 2.7e-4 (weights ~0.02, as bench.py's fp16
N(0, 0.02^2)); gains f32 1 + N(0, 0.1^2).  Per model: a 512-token ingest (bench.py's prompt, seed 99), five greedy steps, then
greedy decode from position 517 in >= 3 windows of --steps tokens (tokens/s: their median), prefill ms, _bytes_per_token and its
fraction of 8 TB/s, per-kernel-class us per launch from _profile_kernel with the algorithmic bytes of one launch and its fraction of
the HBM roofline, and max |dlogit| against the oracle (its own block_q8_0 dequantiser, tests/test_gpu_q8_0.py's
restatement) at 4 positions.  One JSON line; --out writes it to a file too.

    python tools/q8_0_bench.py --out q8_0_bench.json
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

Q8_0 = 8
HBM_PEAK = 8.0e12


def gen_q8_0_weights_hbm(torch, dims, seed=1234, d=2.7e-4):
    """name -> (uint8 tensor of native Q8_0 blocks | f32 gains, ggml type, rows, cols), generated on the device."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    dh = torch.tensor([d], dtype=torch.float16).view(torch.uint8).to("cuda")
    out = {}
    for name, shape in dims.shapes().items():
        if len(shape) == 1:
            out[name] = (1.0 + 0.1 * torch.randn(shape, device="cuda", dtype=torch.float32, generator=g), 0, 1, shape[0])
            continue
        nblk = shape[0] * shape[1] // 32
        t = torch.randint(0, 256, (nblk, 34), device="cuda", dtype=torch.uint8, generator=g)
        t[:, 0:2] = dh
        out[name] = (t, Q8_0, shape[0], shape[1])
    torch.cuda.synchronize()
    return out


def dequant_q8_0(raw, rows, cols):
    b = np.ascontiguousarray(raw, np.uint8).reshape(rows * cols // 32, 34)
    dd = b[:, :2].copy().view(np.float16).astype(np.float32)[:, 0]
    q = b[:, 2:].copy().view(np.int8).astype(np.float32)
    return (dd[:, None] * q).reshape(rows, cols)


CLASSES = ["qkv", "attn", "wo", "gateup", "down", "lmhead"]


def class_bytes(dims, wbytes, pos, kv_esz=4):
    """Algorithmic HBM bytes of ONE launch of each class at position pos (weights once; attention: K and V rows 0..pos of a block)."""
    E, HD, KD, F, V = dims.E, dims.H * dims.D, dims.Hkv * dims.D, dims.F, dims.V
    return {"qkv": (HD + 2 * KD) * E * wbytes + 2 * KD * kv_esz, "attn": 2 * KD * kv_esz * (pos + 1),
            "wo": HD * E * wbytes, "gateup": 2 * F * E * wbytes, "down": E * F * wbytes, "lmhead": V * E * wbytes}


def run_model(torch, dims, quant, steps, windows, check):
    import bench as B
    import oracle as orc
    from nfai_amd import synth
    from nfai_amd.hip import HipBufferManager
    from nfai_amd.llama_model import LlamaModel
    T, warm = 512, 5
    weights = gen_q8_0_weights_hbm(torch, dims) if quant == "q8_0" else B.gen_weights_hbm(torch, dims, (0, dims.L), True, True, quant="f16")
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
    wb = 34 / 32 if quant == "q8_0" else 2.0
    cb = class_bytes(dims, wb, pos)
    classes = {}
    from nfai_amd._lib import NfaiHipError
    for c in CLASSES:
        try:
            us = m.ProfileKernel(tok, c, reps=8)
        except NfaiHipError:   # fp16: Wo rides on the attention launch (no launch of class "wo"); its bytes are counted there
            continue
        by = cb[c] + (cb["wo"] if c == "attn" and quant != "q8_0" else 0)
        classes[c] = {"us_per_launch": us, "launches_per_token": 1 if c == "lmhead" else dims.L, "bytes_per_launch": int(by),
                      "frac_hbm_roofline": by / HBM_PEAK / (us * 1e-6) if us > 0 else None}
    res = {"model": dims.name, "weights": quant, "decode_tokens_per_s": tps, "windows_tokens_per_s": rates, "steps_per_window": steps,
           "positions": [T + warm, pos - 1], "prefill_ms_512": prefill_ms, "bytes_per_token": total, "dominant_bytes": dom,
           "token_frac_of_8TBps": total * tps / HBM_PEAK, "kernel_classes": classes}
    m.Dispose()
    mgr.Dispose()
    if check:
        host = {k: (dequant_q8_0(t.cpu().numpy(), r, c) if ty == Q8_0 else t.cpu().numpy()) for k, (t, ty, r, c) in weights.items()}
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
    a = ap.parse_args()
    import torch
    from nfai_amd import synth
    torch.cuda.set_device(0)
    out = {"tool": "q8_0_bench", "models": []}
    for dims in (synth.LLAMA_32_3B, synth.LLAMA_32_1B):
        for quant in ("q8_0", "f16"):
            out["models"].append(run_model(torch, dims, quant, a.steps, max(3, a.windows), quant == "q8_0" and not a.no_check))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
