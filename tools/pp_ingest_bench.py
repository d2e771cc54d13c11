#!/usr/bin/env python3
"""The prompt phase of a layer pipeline, filled two ways, with every stage driven by ONE process on ONE card:

* token by token: the decode schedule (`run_schedule_in_process(..., n_slots=1)`), one stage step per token and stage — what a
  sharded model had before nfai_hip_llama_stage_ingest (and what bench.py's context fill still does);
* chunked: `run_prompt_schedule_in_process` — nfai_hip_llama_stage_ingest per stage, the MFMA prefill in chunks of max_batch rows,
  [T][E] fp32 rows handed on as device-to-device copies.

Configurations: Llama-3.1-8B Q4_K_M over 8 stages (BASELINE config 5) and Llama-3.2-3B fp16 over 2 stages, synthetic weights at
full depth and vocabulary, a 512-token prompt from an empty cache, median of --reps fills after one warm-up fill (the first chunked
call of a K-quant stage widens its matrices to fp16: `chunked_first_ms`).  One card runs the stages one after another; N cards
overlap different sequences' work but a single prompt's chunks still cross the stages in turn, so the chunked figure is the
single-sequence latency plus the hand-offs.  The hand-offs here are on-card copies (`handoff_copy_ms`); over xGMI they are not
measured by this tool.  Prints one JSON line.

    python tools/pp_ingest_bench.py [--tokens 512] [--chunk 512] [--reps 3] [--configs 8b-q4km-pp8,3b-f16-pp2] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {"8b-q4km-pp8": ("llama-3.1-8b", "q4_k_m", 8), "3b-f16-pp2": ("llama-3.2-3b", "f16", 2)}


def stage_weights(dev, dims, lb, le, first, last):
    out = {}
    for name, t in dev.items():
        if name.startswith("blk."):
            if lb <= int(name.split(".")[1]) < le:
                out[name] = t
        elif name == "token_embd.weight":
            if first or (last and dims.tied):
                out[name] = t
        elif last:
            out[name] = t
    return out


def run_config(torch, mgr, stream, key, n_tok, chunk, reps):
    import bench as B
    from nfai_amd import synth
    from nfai_amd.pipeline import HipStage, partition_layers, pipeline_costs, run_prompt_schedule_in_process, run_schedule_in_process
    model, quant, world = CONFIGS[key]
    dims = synth.BY_NAME[model]
    C = n_tok + 16
    ranges = partition_layers(dims.L, world, *pipeline_costs(dims, quant))
    copy = lambda dst, src: dst.copy_(src)  # noqa: E731
    prompt = [int(t) for t in synth.make_tokens(dims, n_tok, seed=99)]
    with torch.cuda.stream(stream):
        dev = B.gen_weights_hbm(torch, dims, (0, dims.L), True, True, quant=quant)
        stages = [HipStage(torch, mgr, dims, (lb, le), stage_weights(dev, dims, lb, le, r == 0, r == world - 1), 1, C, r, world,
                           max_batch=chunk) for r, (lb, le) in enumerate(ranges)]

        def reset():
            for st in stages:
                st.models[0].Reset()
            stream.synchronize()

        def timed(fn):
            reset()
            t0 = time.perf_counter()
            fn()
            stream.synchronize()
            return (time.perf_counter() - t0) * 1e3

        chunked = lambda: run_prompt_schedule_in_process(stages, [prompt], chunk, copy)  # noqa: E731
        tokenwise = lambda: run_schedule_in_process(stages, n_tok, [prompt[0]], copy, n_slots=1)  # noqa: E731
        first_ms = timed(chunked)                     # K-quant stages widen their matrices here
        ck = [timed(chunked) for _ in range(reps)]
        timed(tokenwise)                               # captures the stage graphs
        tw = [timed(tokenwise) for _ in range(reps)]
        # the hand-offs of one chunked fill, alone: world - 1 copies of [chunk][E] fp32 rows
        src = torch.zeros(chunk * dims.E, device="cuda")
        dst = torch.zeros_like(src)
        stream.synchronize()
        t0 = time.perf_counter()
        for _ in range(world - 1):
            dst.copy_(src)
        stream.synchronize()
        hand_ms = (time.perf_counter() - t0) * 1e3
        for st in stages:
            st.dispose()
        del dev
        torch.cuda.empty_cache()
    ck_ms, tw_ms = float(np.median(ck)), float(np.median(tw))
    return {"config": key, "model": model, "quant": quant, "stages": world, "layer_ranges": ranges, "prompt_tokens": n_tok,
            "chunk": chunk, "tokenwise_ms": round(tw_ms, 3), "chunked_ms": round(ck_ms, 3), "chunked_first_ms": round(first_ms, 3),
            "speedup": round(tw_ms / ck_ms, 2), "tokenwise_ms_per_stage_step": round(tw_ms / (n_tok * world), 4),
            "handoff_copy_ms": round(hand_ms, 4), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from nfai_amd.hip import HipBufferManager
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    mgr = HipBufferManager(0, stream=stream.cuda_stream)
    res = [run_config(torch, mgr, stream, k, a.tokens, a.chunk, a.reps) for k in a.configs.split(",")]
    mgr.Dispose()
    line = json.dumps({"tool": "pp_ingest_bench", "device": torch.cuda.get_device_name(0), "one_card": True,
                       "note": "all stages on one card, one after another; the xGMI hand-off between cards is not measured here",
                       "results": res})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
