"""What the logit bar of tests/test_gpu_batch_wide.py can and cannot tell apart, re-measured on the CPU on every run.

The wide batch (kernels_gemv_wide.hip) feeds every fp32 activation x to the fp16 MFMA as two operands, hi = half(x) and
lo = half((x - hi) * 2^11), accumulates both products in fp32 and combines them as acc_hi + 2^-11 acc_lo.  The GPU test holds its logits
within 5e-4 * max(1, max|logit|) of the oracle's fp32 path.  Here a NumPy restatement of that arithmetic — every GEMV of the model as
two float32 products of the fp16 weights with the hi and the scaled lo plane, everything else (RMSNorm, RoPE, attention, SiLU,
residuals) in float32 — walks whole sequences on the two tiny models of GPU test 1 (weights seed 21, std 0.05):

  * as stated it must stay under HALF the bar on every step: the arithmetic the kernel is entitled to leaves room;
  * with the lo plane dropped (hi only: activations rounded to fp16) it must exceed the WHOLE bar on at least one step of each model:
    the GPU test would catch a lost plane.

Measured (worst |d| / bar over 4 sequences of 19 .. 31 steps):     as stated     lo plane dropped
  tiny-llama                                                           0.004         2.12  (87 of 100 steps over the bar)
  tiny-llama-d128                                                      0.008         2.79  (all 100 steps over the bar)
"""
import numpy as np
import pytest

import oracle as orc
from oracle import np_oracle as npo
from nfai_amd import synth

SCALE = 5e-4
MODELS = [synth.TINY, synth.TINY_D128]
CAP = 96


def split(x):
    """x (float32) -> (hi, lo) float32 values of the two fp16 planes."""
    hi = x.astype(np.float16)
    lo = ((x - hi.astype(np.float32)) * np.float32(2048)).astype(np.float16)
    return hi.astype(np.float32), lo.astype(np.float32)


def gemv(W32, x, with_lo):
    hi, lo = split(np.asarray(x, np.float32))
    y = W32 @ hi
    if with_lo:
        y = y + (W32 @ lo) * np.float32(2.0 ** -11)
    return y.astype(np.float32)


class Restated:
    """One sequence through the model, float32 throughout, every matrix product through gemv()."""

    def __init__(self, d, w, with_lo, cap=CAP):
        self.d, self.with_lo = d, with_lo
        self.w = {k: np.asarray(v, np.float32) for k, v in w.items()}
        self.freqs = npo.rope_freqs(d.D).astype(np.float32)
        self.K = [np.zeros((cap, d.Hkv * d.D), np.float32) for _ in range(d.L)]
        self.V = [np.zeros((cap, d.Hkv * d.D), np.float32) for _ in range(d.L)]
        self.pos = 0

    def mm(self, name, x):
        """Every matrix product of the model (tests/scale_models.py records its inputs and restates it in other ways)."""
        return gemv(self.w[name], x, self.with_lo)

    def row(self, kind, v):
        """The q ("q"), K ("k") or V ("v") row as the attention reads it (tests/scale_models.py rounds them to fp16)."""
        return v

    def step(self, tok, eps=1e-5):
        d, w, p, f32 = self.d, self.w, self.pos, np.float32
        mm, row = self.mm, self.row
        x = w["token_embd.weight"][tok].copy()
        for l in range(d.L):
            b = f"blk.{l}."
            xn = npo.rmsnorm(x, w[b + "attn_norm.weight"], eps).astype(f32)
            q = row("q", npo.rope(mm(b + "attn_q.weight", xn), self.freqs, d.D, d.H, d.D, p).astype(f32))
            self.K[l][p] = row("k", npo.rope(mm(b + "attn_k.weight", xn), self.freqs, d.D, d.Hkv, d.D, p).astype(f32))
            self.V[l][p] = row("v", mm(b + "attn_v.weight", xn))
            att = npo.attention(q, self.K[l], self.V[l], d.H, d.Hkv, d.D, p + 1).astype(f32)
            h = (x + mm(b + "attn_output.weight", att)).astype(f32)
            hn = npo.rmsnorm(h, w[b + "ffn_norm.weight"], eps).astype(f32)
            act = (mm(b + "ffn_up.weight", hn) * npo.silu(mm(b + "ffn_gate.weight", hn)).astype(f32)).astype(f32)
            x = (h + mm(b + "ffn_down.weight", act)).astype(f32)
        xn = npo.rmsnorm(x, w["output_norm.weight"], eps).astype(f32)
        self.x = x
        self.pos += 1
        return mm("output.weight" if "output.weight" in w else "token_embd.weight", xn)


@pytest.mark.parametrize("dims", MODELS, ids=lambda d: d.name)
def test_the_bar_passes_the_split_and_catches_a_lost_plane(dims):
    w = synth.make_weights(dims, seed=21, std=0.05)
    worst = {True: 0.0, False: 0.0}
    over = 0
    for s in range(4):
        toks = synth.make_tokens(dims, 3 + 4 * s + 16, seed=100 + s)
        ref = orc.OracleLlama(orc.LlamaDesc(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, C=CAP), w)
        both, hi_only = Restated(dims, w, True), Restated(dims, w, False)
        for t in toks:
            want = ref.step(int(t))
            bar = SCALE * max(1.0, float(np.abs(want).max()))
            r2 = float(np.abs(both.step(int(t)) - want).max()) / bar
            r1 = float(np.abs(hi_only.step(int(t)) - want).max()) / bar
            worst[True], worst[False] = max(worst[True], r2), max(worst[False], r1)
            over += r1 > 1.0
        ref.close()
    print(f"{dims.name}: worst |d| / (5e-4 * max(1, max|logit|)): hi + scaled lo {worst[True]:.3f}, hi only {worst[False]:.3f} "
          f"({over} steps over the bar)")
    assert worst[True] < 0.5, worst
    assert worst[False] > 1.0 and over >= 1, worst
