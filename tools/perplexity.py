#!/usr/bin/env python3
"""Perplexity of a text under a GGUF model, at prefill speed (nfai_hip_llama_score: every position's log-probability in one call).

    tools/perplexity.py MODEL.gguf TEXT_OR_TOKENS [--context 512] [--max-batch 512] [--draft-k 4] [--ngram 3]
    tools/perplexity.py --synthetic llama-3.2-3b --quant q4_k_m [--tokens 512] [--json profiles/score.json]

TEXT_OR_TOKENS: a UTF-8 text file (tokenised with the file's own tokenizer, BOS in front), or a file of whitespace-separated token
ids (every word an integer).  The text is scored in windows of --context tokens, each from an empty cache.  Printed: the perplexity
exp(-mean log p(token i + 1 | tokens .. i)), the top-1 agreement of the ArgMax with the next token, and the share of the model's own
greedy tokens the n-gram drafter (nfai_amd/drafter.py) with --ngram / --draft-k would have had accepted on this text: at every
position the drafter proposes from the text so far, and a draft counts as accepted as far as it equals the model's ArgMax chain —
which on a scored text is known only where the text itself follows the ArgMax, so the run stops at the first position where the
text leaves it (a lower bound of the acceptance a greedy generation of the same text would see).

--synthetic NAME --quant Q runs on random weights generated in HBM (no file) and also times the call: _score against _prefill on the
same tokens, alternating in one process, median of --rounds, and beside them the lone [tokens x E] x [E x V] fp16 GEMM of the head
(nfai_hip_gemm_f16; fp16 weights whatever --quant is).  --json merges the figures into that file under "NAME/Q"."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def drafter_acceptance(tokens, argmax, ngram, k):
    """(drafts accepted, drafts proposed, positions with a proposal): at position i the history is tokens[..i]; the next tokens the
    model itself would emit are argmax[i], and argmax[i + 1] ... as long as the text follows them."""
    from nfai_amd.drafter import PromptLookupDrafter
    d = PromptLookupDrafter(ngram)
    tokens = [int(t) for t in tokens]
    acc = prop = pos = 0
    for i in range(1, len(tokens) - 1):
        draft = d.Propose(tokens[:i + 1], k)[:len(tokens) - 1 - i]   # drafts past the end of the text cannot be judged
        if not draft:
            continue
        pos += 1
        prop += len(draft)
        for j, t in enumerate(draft):
            if t != int(argmax[i + j]):
                break
            acc += 1
            if tokens[i + j + 1] != t:   # the text leaves the model's own chain here
                break
    return acc, prop, pos


def report(tokens, lp, am, ngram, k):
    n = len(tokens)
    ppl = float(np.exp(-np.mean(lp, dtype=np.float64))) if len(lp) else float("nan")
    agree = float(np.mean(am == tokens[1:])) if n > 1 else float("nan")
    acc, prop, pos = drafter_acceptance(tokens, np.append(am, 0), ngram, k)
    print(f"tokens scored        {len(lp)}")
    print(f"perplexity           {ppl:.4f}")
    print(f"top-1 agreement      {agree:.4f}")
    print(f"drafter (n-gram <= {ngram}, k = {k}): {acc} of {prop} drafted tokens accepted ({acc / prop if prop else 0.0:.3f}) at {pos} positions")
    return dict(tokens=len(lp), perplexity=ppl, top1_agreement=agree, drafter_accepted=acc, drafter_proposed=prop)


def score_windows(m, tokens, context):
    """log p and ArgMax of every predicted token: windows of `context` tokens, each from an empty cache (the last row of a window has
    no target inside it and is left out)."""
    lps, ams = [], []
    for s in range(0, len(tokens) - 1, context - 1):
        w = tokens[s:s + context]
        if len(w) < 2:
            break
        m.Reset()
        lp, am, _ = m.Score(w)
        lps.append(lp[:-1])
        ams.append(am[:-1])
    return np.concatenate(lps), np.concatenate(ams)


def median_ms(fn, mgr, rounds):
    ts = []
    for _ in range(rounds):
        mgr.Synchronize()
        t0 = time.perf_counter()
        fn()
        mgr.Synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def synthetic(a):
    import torch
    import bench as B
    from nfai_amd import _lib, synth
    from nfai_amd._lib import call
    from nfai_amd.hip import HipBufferManager, ShaderProperty
    from nfai_amd.llama_model import LlamaModel
    dims = synth.BY_NAME[a.synthetic]
    torch.cuda.set_device(0)
    w = B.gen_weights_hbm(torch, dims, (0, dims.L), True, True, quant=a.quant)
    mgr = HipBufferManager(0)
    m = LlamaModel(mgr, synth.make_metadata(dims), B.as_model_tensors(_lib, w), a.tokens + 8, max_batch=a.max_batch,
                   dims=dict(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, eps=1e-5, rope_dims=dims.D, rope_base=500000.0))
    toks = synth.make_tokens(dims, a.tokens, seed=99)
    out = {}

    def score():
        m.Reset()
        out["score"] = m.Score(toks)

    def prefill():
        m.Reset()
        m.Prefill(toks, want_logits=False)

    score()      # first calls: the workspaces, the fp16 copies of a quantised model's blocks
    prefill()
    s_ms, p_ms = [], []
    for _ in range(a.rounds):      # alternating, one process
        s_ms.append(median_ms(score, mgr, 1)[0])
        p_ms.append(median_ms(prefill, mgr, 1)[0])
    lp, am, _ = out["score"]
    res = report(np.asarray(toks), lp[:-1], am[:-1], a.ngram, a.draft_k)
    # the lone head GEMM [tokens x E] x [E x V], fp16, fp32 output
    T, N, K = a.tokens, dims.V // 64 * 64, dims.E
    pa, pw, pc = ShaderProperty(mgr, T * K, np.float16), ShaderProperty(mgr, N * K, np.float16), ShaderProperty(mgr, T * N, np.float32)
    r = np.random.Generator(np.random.PCG64(1))
    pa.SetValue(r.standard_normal(T * K).astype(np.float16))
    pw.SetValue((0.02 * r.standard_normal(N * K, dtype=np.float32)).astype(np.float16))
    gemm = lambda: call("nfai_hip_gemm_f16", mgr.handle, pa.handle, pw.handle, 0, pc.handle, T, N, K, 0)   # noqa: E731
    gemm()
    g_med, g_min = median_ms(gemm, mgr, a.rounds)
    res.update(score_ms_median=float(np.median(s_ms)), score_ms_min=float(np.min(s_ms)), prefill_ms_median=float(np.median(p_ms)),
               prefill_ms_min=float(np.min(p_ms)), head_gemm_ms_median=g_med, head_gemm_ms_min=g_min, rounds=a.rounds, max_batch=a.max_batch)
    print(f"_score  {res['score_ms_median']:.3f} ms (min {res['score_ms_min']:.3f})   _prefill {res['prefill_ms_median']:.3f} ms (min {res['prefill_ms_min']:.3f})   "
          f"lone head GEMM [{T} x {K}] x [{K} x {N}] {g_med:.3f} ms (min {g_min:.3f})")
    over = res["score_ms_median"] - (res["prefill_ms_median"] + 2 * g_med)
    print(f"_score - (_prefill + 2 x head GEMM) = {over:+.3f} ms")
    if a.json:
        doc = json.load(open(a.json)) if os.path.exists(a.json) else {}
        doc[f"{a.synthetic}/{a.quant}"] = res
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    m.Dispose()
    mgr.Dispose()


def from_file(a):
    from nfai_amd import gguf
    from nfai_amd.hip import HipBufferManager
    from nfai_amd.llama_model import LlamaModel
    md, tensors = gguf.Parser().Read(a.model)
    mgr = HipBufferManager(0)
    m = LlamaModel(mgr, md, tensors, a.context + 8, max_batch=a.max_batch)
    words = open(a.text, encoding="utf-8").read()
    if all(x.isdigit() for x in words.split()) and words.split():
        toks = np.array([int(x) for x in words.split()], np.uint32)
    else:
        if m.tokenizer is None:
            raise SystemExit("the GGUF file has no tokenizer: pass a file of token ids")
        toks = np.array(m.tokenizer.Tokenize(words, addBos=True), np.uint32)
    if toks.size < 2:
        raise SystemExit("at least two tokens are needed")
    lp, am = score_windows(m, toks, a.context)
    # the windows overlap by one token, so the scored targets are tokens[1 ..] in order
    report(toks[:len(lp) + 1], lp, am, a.ngram, a.draft_k)
    m.Dispose()
    mgr.Dispose()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model", nargs="?", help="GGUF file")
    ap.add_argument("text", nargs="?", help="UTF-8 text, or whitespace-separated token ids")
    ap.add_argument("--synthetic", choices=["llama-3.2-1b", "llama-3.2-3b", "llama-3.1-8b", "tiny-llama", "tiny-llama-d128"])
    ap.add_argument("--quant", default="f16", choices=["f16", "q4_k_m"])
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--context", type=int, default=512)
    ap.add_argument("--max-batch", type=int, default=512)
    ap.add_argument("--ngram", type=int, default=3)
    ap.add_argument("--draft-k", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--json", help="merge the synthetic run's figures into this JSON file")
    a = ap.parse_args()
    if a.synthetic:
        return synthetic(a)
    if not a.model or not a.text:
        ap.error("a GGUF file and a text or token file, or --synthetic NAME")
    from_file(a)


if __name__ == "__main__":
    main()
