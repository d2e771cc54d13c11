"""What the all-rows bar of tests/test_gpu_prefill_rows.py can and cannot tell apart, re-measured on the CPU on every run.

The GPU test holds EVERY K / V row the MFMA prefill writes within atol = 2e-2 of the oracle's token-by-token fp32 path.  Here a
float64 NumPy restatement of that prefill — whole prompt at once, with the prefill's fp16 rounding points: the normed rows (the
GEMMs' A operands), q / K / V as attention operands, the probabilities, the attention output and act = up * silu(gate) — is held
against the same oracle on the same two thin models, 512 rows:

  * unmutated it must stay under HALF the bar on every K / V row of both blocks (and its logits, at every position, under half of
    2e-2 * max(1, max|logit|)): the rounding the prefill is entitled to leaves room;
  * with one 64-deep K tile of block 0's Wdown dropped for ONE row, that row of block 1's K and V must each move by more than FIVE
    times the bar; so must block 0's K row when it is rotated at the neighbouring position.

Measured (max |d|; weights seed 61 at std 0.05, tokens seed 13; max|K|, max|V| = 3.6, 3.4 resp. 3.7, 3.6):
                  unmutated K/V   logits / scale   dropped tile: K / V of the row   RoPE at pos + 1
  thin-f8192         3.4e-3          1.8e-3               0.185 / 0.192                 0.900
  thin-h9-d128       3.2e-3          1.3e-3               0.531 / 0.657                 1.397
against half the bar = 1e-2 and five times the bar = 0.1.  If a model misses a margin, its std changes, never the bar.
"""
import numpy as np
import pytest

import oracle as orc
from oracle import np_oracle as npo
from nfai_amd import synth

BAR = 2e-2
T = 512
DROP_ROW, DROP_TILE = 200, 5        # row 200 of the chunk loses columns [320, 384) of block 0's Wdown product
ROPE_ROW = 131                       # block 0's K row 131 is rotated as position 132
MODELS = [(synth.THIN_F8192, 0.05), (synth.THIN_H9, 0.05)]


def r16(x):
    return x.astype(np.float16).astype(np.float64)


def _rms(x, g, eps):
    return x / np.sqrt(np.mean(x * x, axis=1, keepdims=True) + eps) * g


def _rope_rows(x, freqs, n_heads, D, pos):
    """np_oracle.rope on every row: pairs (2i, 2i + 1) of each head rotated by freqs[i] * pos[row]."""
    t = x.reshape(x.shape[0], n_heads, D // 2, 2)
    th = pos[:, None, None] * freqs[None, None, :]
    c, s = np.cos(th), np.sin(th)
    out = np.empty_like(t)
    out[..., 0] = c * t[..., 0] - s * t[..., 1]
    out[..., 1] = s * t[..., 0] + c * t[..., 1]
    return out.reshape(x.shape)


def restate(d, w, toks, drop=None, rope_shift=None, eps=1e-5):
    """K rows, V rows (per block, [T][Hkv*D], as stored in an fp32 cache) and logits [T][V] of the one-chunk prefill in float64 with its
    fp16 rounding points.  drop = (row, tile): block 0's Wdown skips K columns [64 tile, 64 tile + 64) for that row; rope_shift = row:
    block 0's K row is rotated at position row + 1."""
    W = {k: np.asarray(v, np.float64) for k, v in w.items()}
    n, G = len(toks), d.H // d.Hkv
    pos = np.arange(n, dtype=np.float64)
    freqs = npo.rope_freqs(d.D)
    causal = np.arange(n)[None, :] <= np.arange(n)[:, None]
    x = W["token_embd.weight"][np.asarray(toks, np.int64)]
    Ks, Vs = [], []
    for l in range(d.L):
        b = f"blk.{l}."
        xn = r16(_rms(x, W[b + "attn_norm.weight"], eps))
        q = _rope_rows(xn @ W[b + "attn_q.weight"].T, freqs, d.H, d.D, pos)
        kpos = pos.copy()
        if rope_shift is not None and l == 0:
            kpos[rope_shift] += 1
        k = _rope_rows(xn @ W[b + "attn_k.weight"].T, freqs, d.Hkv, d.D, kpos)
        v = xn @ W[b + "attn_v.weight"].T
        Ks.append(k)
        Vs.append(v)
        qh, kh, vh = r16(q).reshape(n, d.H, d.D), r16(k).reshape(n, d.Hkv, d.D), r16(v).reshape(n, d.Hkv, d.D)
        att = np.empty((n, d.H, d.D))
        for h in range(d.H):
            sc = np.where(causal, qh[:, h] @ kh[:, h // G].T / np.sqrt(d.D), -np.inf)
            p = np.exp(sc - sc.max(axis=1, keepdims=True))
            att[:, h] = (r16(p) @ vh[:, h // G]) / p.sum(axis=1, keepdims=True)
        h1 = x + r16(att.reshape(n, d.H * d.D)) @ W[b + "attn_output.weight"].T
        hn = r16(_rms(h1, W[b + "ffn_norm.weight"], eps))
        act = r16((hn @ W[b + "ffn_up.weight"].T) * npo.silu(hn @ W[b + "ffn_gate.weight"].T))
        down = act @ W[b + "ffn_down.weight"].T
        if drop is not None and l == 0:
            row, tile = drop
            cols = slice(64 * tile, 64 * tile + 64)
            down[row] -= act[row, cols] @ W[b + "ffn_down.weight"][:, cols].T
        x = h1 + down
    head = W.get("output.weight", W["token_embd.weight"])
    return Ks, Vs, _rms(x, W["output_norm.weight"], eps) @ head.T


def oracle_rows(d, w, toks):
    """The oracle's K / V rows of every block and its logits at every position: attention is causal, so they serve every prefix."""
    ref = orc.OracleLlama(orc.LlamaDesc(E=d.E, L=d.L, H=d.H, Hkv=d.Hkv, D=d.D, F=d.F, V=d.V, C=len(toks)), w)
    logits = np.stack([ref.step(int(t)) for t in toks])
    K = [ref.kcache(l).copy() for l in range(d.L)]
    V = [ref.vcache(l).copy() for l in range(d.L)]
    ref.close()
    return K, V, logits


@pytest.mark.parametrize("dims,std", MODELS, ids=[m[0].name for m in MODELS])
def test_all_rows_bar_separates_rounding_from_a_dropped_tile(dims, std):
    w = synth.make_weights(dims, seed=61, std=std)
    toks = synth.make_tokens(dims, T, seed=13)
    oK, oV, oL = oracle_rows(dims, w, toks)
    K, V, lg = restate(dims, w, toks)
    kv = max(float(np.abs(a - b).max()) for a, b in zip(K + V, oK + oV))
    scale = np.maximum(1.0, np.abs(oL).max(axis=1))
    lrel = float((np.abs(lg - oL).max(axis=1) / scale).max())
    print(f"{dims.name}: max|K|, max|V| = {max(np.abs(a).max() for a in oK):.2f}, {max(np.abs(a).max() for a in oV):.2f}")
    print(f"{dims.name}: unmutated K/V max|d| = {kv:.2e} (half bar {BAR / 2:.0e}); logits {lrel:.2e} of scale (half bar {BAR / 2:.0e})")
    assert kv < BAR / 2, kv
    assert lrel < BAR / 2, lrel

    mK, mV, _ = restate(dims, w, toks, drop=(DROP_ROW, DROP_TILE))
    dk = float(np.abs(mK[1][DROP_ROW] - oK[1][DROP_ROW]).max())
    dv = float(np.abs(mV[1][DROP_ROW] - oV[1][DROP_ROW]).max())
    print(f"{dims.name}: Wdown tile {DROP_TILE} dropped for row {DROP_ROW}: block 1 K row moves {dk:.3f}, V row {dv:.3f} (5 x bar = {5 * BAR:.2f})")
    assert dk > 5 * BAR and dv > 5 * BAR, (dk, dv)
    # the rows before the mutated one are untouched by it (causal), so they stay where the unmutated run put them
    assert np.array_equal(mK[1][:DROP_ROW], K[1][:DROP_ROW])

    rK, _, _ = restate(dims, w, toks, rope_shift=ROPE_ROW)
    dr = float(np.abs(rK[0][ROPE_ROW] - oK[0][ROPE_ROW]).max())
    print(f"{dims.name}: block 0 K row {ROPE_ROW} rotated at position {ROPE_ROW + 1}: moves {dr:.3f}")
    assert dr > 5 * BAR, dr
