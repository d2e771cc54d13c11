"""Synthetic Llama-3 shaped models (there is no network for checkpoints): SURVEY.md §8d recipe.

Weights ~ N(0, 0.02^2) rounded to fp16, norm gains 1 + N(0, 0.1^2) fp32, NumPy PCG64 seeded.
Tensor names and [N][K] row-major layout are the GGUF ones the reference looks up
(NFAI.Vulkan.Shaders/TransformerBlock.cs:41-101, NFAI.Models.Llama3/LlamaModel.cs:43,58).
"""
from __future__ import annotations

from dataclasses import dataclass, asdict

import numpy as np


@dataclass(frozen=True)
class LlamaDims:
    name: str
    E: int
    L: int
    H: int
    Hkv: int
    D: int
    F: int
    V: int
    tied: bool = True

    def shapes(self) -> dict:
        """GGUF tensor name -> (N, K) for matrices / (E,) for norm gains."""
        s = {"token_embd.weight": (self.V, self.E), "output_norm.weight": (self.E,)}
        if not self.tied:
            s["output.weight"] = (self.V, self.E)
        for l in range(self.L):
            b = f"blk.{l}."
            s[b + "attn_norm.weight"] = (self.E,)
            s[b + "attn_q.weight"] = (self.H * self.D, self.E)
            s[b + "attn_k.weight"] = (self.Hkv * self.D, self.E)
            s[b + "attn_v.weight"] = (self.Hkv * self.D, self.E)
            s[b + "attn_output.weight"] = (self.E, self.H * self.D)
            s[b + "ffn_norm.weight"] = (self.E,)
            s[b + "ffn_gate.weight"] = (self.F, self.E)
            s[b + "ffn_up.weight"] = (self.F, self.E)
            s[b + "ffn_down.weight"] = (self.E, self.F)
        return s

    def n_params_read_per_token(self) -> int:
        """Matrix weights read once per decoded token (embedding table counted via lm_head when
        tied; the embedding row itself is E more)."""
        per_layer = (self.H * self.D * self.E + 2 * self.Hkv * self.D * self.E
                     + self.E * self.H * self.D + 3 * self.F * self.E)
        return self.L * per_layer + self.V * self.E

    def as_dict(self):
        return asdict(self)


# Public Llama-3 configurations.
LLAMA_32_1B = LlamaDims("llama-3.2-1b", 2048, 16, 32, 8, 64, 8192, 128256, True)
LLAMA_32_3B = LlamaDims("llama-3.2-3b", 3072, 28, 24, 8, 128, 8192, 128256, True)
LLAMA_31_8B = LlamaDims("llama-3.1-8b", 4096, 32, 32, 8, 128, 14336, 128256, False)
# Small shapes for CPU-sized parity runs (all K multiples of 256 so K-quants apply).
TINY = LlamaDims("tiny-llama", 256, 2, 4, 2, 64, 512, 512, True)
TINY_D128 = LlamaDims("tiny-llama-d128", 512, 3, 4, 2, 128, 1024, 768, False)
# Thin two-block models whose prefill GEMMs take the tile configurations of the published widths (tests/test_gpu_prefill_rows.py):
# F = 8192 gives gate|up and Wdown the wide forms and the K splits; (H + 2 Hkv) D = 1920 is a multiple of 80 and of 48.
THIN_F8192 = LlamaDims("thin-f8192", 256, 2, 4, 2, 64, 8192, 512, True)
THIN_H9 = LlamaDims("thin-h9-d128", 256, 2, 9, 3, 128, 512, 512, True)
# Thin one-block models at the K-panel edges of the wide batched decode (kernels_gemv_wide.hip stages x in panels of 2048 k;
# tests/test_gpu_batch_wide.py): E = 3072 is one and a half panels (RMSNorm across them), E = 4096 two, F = 14336 seven.
THIN_E3072 = LlamaDims("thin-e3072", 3072, 1, 4, 2, 64, 512, 512, True)
THIN_E4096 = LlamaDims("thin-e4096", 4096, 1, 4, 2, 64, 512, 512, True)
THIN_F14336 = LlamaDims("thin-f14336", 256, 1, 4, 2, 64, 14336, 512, True)

BY_NAME ={d.name: d for d in (LLAMA_32_1B, LLAMA_32_3B, LLAMA_31_8B, TINY, TINY_D128)}


def make_weights(dims: LlamaDims, seed: int = 1234, std: float = 0.02) -> dict:
    """name -> ndarray; matrices float16, gains float32."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for name, shape in dims.shapes().items():
        if len(shape) == 1:
            out[name] = (1.0 + 0.1 * rng.standard_normal(shape, dtype=np.float32)).astype(np.float32)
        else:
            out[name] = (std * rng.standard_normal(shape, dtype=np.float32)).astype(np.float16)
    return out


def quantize_q8_0(W) -> bytes:
    """ggml quantize_row_q8_0_ref on every row of W [rows][cols] (cols % 32 == 0): per 32-block d = amax / 127, q = round(x / d)
    (roundf: halves away from zero), d stored as fp16; blocks of 34 bytes (fp16 d, int8 qs[32]), row-major."""
    x = np.asarray(W, dtype=np.float32).reshape(-1, 32)
    amax = np.abs(x).max(axis=1)
    d = amax / np.float32(127)
    inv = np.where(d != 0, np.float32(1) / np.where(d != 0, d, np.float32(1)), np.float32(0)).astype(np.float32)
    v = x * inv[:, None]
    t = np.trunc(v)
    q = (t + np.sign(v) * (np.abs(v - t) >= np.float32(0.5))).astype(np.int8)  # roundf; v - t is exact
    out = np.empty((x.shape[0], 34), np.uint8)
    out[:, :2] = d.astype(np.float16).view(np.uint8).reshape(-1, 2)
    out[:, 2:] = q.view(np.uint8)
    return out.tobytes()


def quantize_q4_0(W) -> bytes:
    """ggml quantize_row_q4_0_ref on every row of W [rows][cols] (cols % 32 == 0), restated from the format: per 32-block, max = the
    element of largest magnitude WITH its sign (the first one among equals), d = max / -8, id = 1 / d (0 when d is 0),
    q = min(15, int(x * id + 8.5)) (truncation; the argument is never negative), d stored as fp16; blocks of 18 bytes (fp16 d,
    qs[16]: qs[j] = q[j] | q[j + 16] << 4), row-major.  Weight j decodes as d * (q[j] - 8): the extreme lands on code 0."""
    x = np.asarray(W, dtype=np.float32).reshape(-1, 32)
    idx = np.argmax(np.abs(x), axis=1)
    mx = x[np.arange(x.shape[0]), idx]
    d = (mx / np.float32(-8)).astype(np.float32)
    inv = np.where(d != 0, np.float32(1) / np.where(d != 0, d, np.float32(1)), np.float32(0)).astype(np.float32)
    q = np.minimum(15, (x * inv[:, None] + np.float32(8.5)).astype(np.int32)).astype(np.uint8)
    out = np.empty((x.shape[0], 18), np.uint8)
    out[:, :2] = d.astype(np.float16).view(np.uint8).reshape(-1, 2)
    out[:, 2:] = q[:, :16] | (q[:, 16:] << 4)
    return out.tobytes()


def dequantize_q4_0(raw, rows: int, cols: int) -> np.ndarray:
    """ggml dequantize_row_q4_0 on native blocks: float32 [rows][cols], weight j = d * ((qs[j] & 0xF) - 8), weight j + 16 =
    d * ((qs[j] >> 4) - 8), the product rounded to fp32."""
    b = np.frombuffer(bytes(raw), np.uint8).reshape(-1, 18)
    d = b[:, :2].copy().view(np.float16).astype(np.float32)                      # [nb][1]
    qs = b[:, 2:]
    q = np.concatenate([qs & 0xF, qs >> 4], axis=1).astype(np.int32) - 8         # [nb][32]
    return (d * q.astype(np.float32)).astype(np.float32).reshape(rows, cols)


def q4_0_type(name: str, dims, mix: str = "q4_0") -> int:
    """ggml type of a matrix in a Q4_0 file: Q4_0 (2) for every matrix, except Q6_K (14) for the lm_head (output.weight, or a tied
    token_embd); an untied token_embd is Q4_0.  This is llama.cpp's rule for the file type as recalled: its source was not at hand
    when this was written, so check it against a real file before relying on the head's type.  mix="all_q4_0": every matrix Q4_0,
    the head and the embedding table too (so that the Q4_0 lm_head + ArgMax and embedding gather run)."""
    if mix == "all_q4_0":
        return 2
    if mix != "q4_0":
        raise ValueError(f"unknown Q4_0 mix {mix!r} (q4_0, all_q4_0)")
    if name == "output.weight" or (name == "token_embd.weight" and dims.tied):
        return 14
    return 2


def _q3_k_scales(b):
    """The sixteen 6-bit scales (0..63) of every Q3_K block in b [nb][110]: low nibble of scale i from scales[i] (i < 8) or the
    high nibble of scales[i - 8], its high two bits from bits 2 (i // 4) .. + 1 of scales[8 + i % 4]."""
    s = b[:, 96:108]
    lo = np.concatenate([s[:, 0:8] & 0xF, s[:, 0:8] >> 4], axis=1)                            # [nb][16]
    i = np.arange(16)
    hi = (s[:, 8 + i % 4] >> (2 * (i // 4))[None, :]) & 3
    return (lo | (hi << 4)).astype(np.int32)


def dequantize_q3_k(raw, rows: int, cols: int) -> np.ndarray:
    """ggml block_q3_K (hmask[32], qs[64], scales[12], fp16 d per 256 weights) dequantised as restated from the format: float32
    [rows][cols].  Element k = 128 n + 32 j + 16 lh + l has low bits (qs[32 n + 16 lh + l] >> 2 j) & 3, high bit
    (hmask[16 lh + l] >> (4 n + j)) & 1 and scale index 8 n + 2 j + lh; y = dl * q with dl = d * (scale - 32) and
    q = low + 4 high - 4, both products rounded to fp32.  The restatement was written without ggml's source at hand: check it
    against a real Q3_K file when one is available."""
    b = np.frombuffer(bytes(raw), np.uint8).reshape(-1, 110)
    nb = b.shape[0]
    d = b[:, 108:110].copy().view(np.float16).astype(np.float32)                              # [nb][1]
    dl = (d * (_q3_k_scales(b) - 32).astype(np.float32)).astype(np.float32)                   # [nb][16], index 8 n + 2 j + lh
    qs = b[:, 32:96].reshape(nb, 2, 1, 32)                                                    # [nb][n][.][16 lh + l]
    hm = b[:, 0:32].reshape(nb, 1, 1, 32)
    n = np.arange(2).reshape(1, 2, 1, 1)
    j = np.arange(4).reshape(1, 1, 4, 1)
    q = ((qs >> (2 * j)) & 3).astype(np.int32) + 4 * ((hm >> (4 * n + j)) & 1).astype(np.int32) - 4   # [nb][n][j][32]
    y = dl.reshape(nb, 2, 4, 2, 1) * q.reshape(nb, 2, 4, 2, 16).astype(np.float32)
    return y.astype(np.float32).reshape(rows, cols)


def quantize_q3_k(W) -> bytes:
    """Valid ggml block_q3_K for every row of W [rows][cols] (cols % 256 == 0): 110 bytes per 256 weights in the order hmask[32],
    qs[64], scales[12], fp16 d.  NOT llama.cpp's quantiser bit for bit (its scale search is not restated).  Per group of 16 the
    signed scale is s = -m / 4 with m the value of largest magnitude with its sign (the first among equals), so that the extreme
    lands on code 0 (q - 4 = -4); d = max|s| / 31 as the next fp16 at or above it; the 6-bit scale is s / d rounded AWAY from zero
    (never more than 31 in magnitude, as d was rounded up) + 32, and q = clip(rint(x / (d (sc - 32))), -4, 3) + 4.  With the step
    |d (sc - 32)| >= |s| every |x| of the group is at most 4 steps, so only code +4 is clipped and every weight decodes within one
    step |d (sc - 32)| of its value (nearest rounding of the scale would let a value of the extreme's magnitude and the other sign
    miss that bound).  An all-zero block stores d = 0.  A fixed point on its own output, dequantize(quantize(y)) == y for
    y = dequantize(quantize(W)), wherever every group has its extreme on code 0: that is every group whose scale is at least 8 in
    magnitude (|s| / step > 7 / 8), and the block's largest group always (scale 31: d comes back exactly)."""
    x = np.asarray(W, dtype=np.float32).reshape(-1, 16, 16)                                   # [nb][group 8 n + 2 j + lh][l]
    nb = x.shape[0]
    idx = np.argmax(np.abs(x), axis=2)
    m = np.take_along_axis(x, idx[:, :, None], axis=2)[:, :, 0]
    s = (m / np.float32(-4)).astype(np.float32)
    d = _f16_up(np.abs(s).max(axis=1) / np.float32(31))
    d32 = d.astype(np.float32)
    ok = d32 > 0
    k = np.where(ok[:, None], np.ceil(np.abs(s) / np.where(ok, d32, 1)[:, None]), 0).astype(np.float32)
    k = np.minimum(k + (d32[:, None] * k < np.abs(s)), 31)                                    # (a quotient rounded down onto an integer)
    sc = (np.sign(s) * k).astype(np.int32)
    step = d32[:, None] * sc.astype(np.float32)                                               # d * (sc - 32) as the decoder forms it
    q = np.where(step[:, :, None] != 0, np.rint(x / np.where(step != 0, step, 1)[:, :, None]), 0)
    q = (np.clip(q, -4, 3) + 4).astype(np.uint8)                                              # [nb][16][16], codes 0..7
    sc6 = (sc + 32).astype(np.uint8)
    out = np.zeros((nb, 110), np.uint8)
    q5 = q.reshape(nb, 2, 4, 2, 16)                                                           # [nb][n][j][lh][l]
    for n in range(2):
        for j in range(4):
            code = q5[:, n, j].reshape(nb, 32)                                                # index 16 lh + l
            out[:, 32 + 32 * n:64 + 32 * n] |= (code & 3) << (2 * j)
            out[:, 0:32] |= (code >> 2) << (4 * n + j)
    out[:, 96:104] = (sc6[:, 0:8] & 0xF) | ((sc6[:, 8:16] & 0xF) << 4)
    for i in range(16):
        out[:, 104 + i % 4] |= (sc6[:, i] >> 4) << (2 * (i // 4))
    out[:, 108:110] = d.view(np.uint8).reshape(nb, 2)
    return out.tobytes()


def q3_k_type(name: str, dims, mix: str = "q3_k_m", layer_offset: int = 0, n_layers_file: int | None = None) -> int:
    """ggml type of a matrix in a file of the Q3_K family.  mix="q3_k_m": attn_q, attn_k, ffn_gate, ffn_up in Q3_K (11); attn_v in
    Q5_K (13) in the first two blocks, else Q4_K (12); attn_output in Q4_K; ffn_down in Q5_K in the first n_layer // 16 blocks, else
    Q4_K; the lm_head (output.weight, or a tied token_embd) in Q6_K (14); an untied token_embd in Q3_K.  This is llama.cpp's rule
    for the file type as recalled: its source was not at hand when this was written, so check it against a real file before relying
    on it.  mix="q3_k_s": Q3_K everywhere but the Q6_K head.  mix="all_q3_k": every matrix Q3_K, the head and the embedding table
    too (so that the Q3_K lm_head + ArgMax and embedding gather run).  layer_offset / n_layers_file: a pipeline stage's blocks
    numbered within the whole file."""
    if mix == "all_q3_k":
        return 11
    if mix not in ("q3_k_m", "q3_k_s"):
        raise ValueError(f"unknown Q3_K mix {mix!r} (q3_k_m, q3_k_s, all_q3_k)")
    if name == "output.weight" or (name == "token_embd.weight" and dims.tied):
        return 14
    if mix == "q3_k_s" or not name.startswith("blk."):
        return 11
    layer, n_layer = int(name.split(".")[1]) + layer_offset, n_layers_file or dims.L
    if name.endswith("attn_v.weight"):
        return 13 if layer < 2 else 12
    if name.endswith("attn_output.weight"):
        return 12
    if name.endswith("ffn_down.weight"):
        return 13 if layer < n_layer // 16 else 12
    return 11


IQ4_KV = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], np.int8)   # the IQ4_XS / IQ4_NL codebook


def _iq4_xs_scales(b):
    """The eight 6-bit scales ls (0..63) of every IQ4_XS block in b [nb][136]: low nibble of scale ib from nibble ib % 2 of
    scales_l[ib // 2], its high two bits from bits 2 ib .. + 1 of the uint16 scales_h."""
    sh = b[:, 2:4].copy().view(np.uint16).astype(np.int32)                                    # [nb][1]
    sl = b[:, 4:8].astype(np.int32)
    ib = np.arange(8)
    lo = (sl[:, ib // 2] >> (4 * (ib % 2))[None, :]) & 0xF
    hi = (sh >> (2 * ib)[None, :]) & 3
    return lo | (hi << 4)


def dequantize_iq4_xs(raw, rows: int, cols: int) -> np.ndarray:
    """ggml block_iq4_xs (fp16 d, uint16 scales_h, scales_l[4], qs[128] per 256 weights: 136 bytes) dequantised as restated from
    the format: float32 [rows][cols].  Sub-block ib (32 weights) has the 6-bit scale ls of _iq4_xs_scales and dl = d * (ls - 32);
    weight 32 ib + j = dl * KV[qs[16 ib + j] & 0xF], weight 32 ib + 16 + j = dl * KV[qs[16 ib + j] >> 4] (j < 16) with the
    16-entry table IQ4_KV, both products rounded to fp32.  The restatement was written without ggml's source at hand: check it
    against a real IQ4_XS file when one is available."""
    b = np.frombuffer(bytes(raw), np.uint8).reshape(-1, 136)
    nb = b.shape[0]
    d = b[:, 0:2].copy().view(np.float16).astype(np.float32)                                  # [nb][1]
    dl = (d * (_iq4_xs_scales(b) - 32).astype(np.float32)).astype(np.float32)                 # [nb][8]
    qs = b[:, 8:136].reshape(nb, 8, 16)
    codes = np.concatenate([qs & 0xF, qs >> 4], axis=2)                                       # [nb][ib][32]
    y = dl[:, :, None] * IQ4_KV[codes].astype(np.float32)
    return y.astype(np.float32).reshape(rows, cols)


def quantize_iq4_xs(W) -> bytes:
    """Valid ggml block_iq4_xs for every row of W [rows][cols] (cols % 256 == 0): 136 bytes per 256 weights in the order fp16 d,
    uint16 scales_h, scales_l[4], qs[128].  NOT llama.cpp's quantiser (its search over scales is not restated).  Per sub-block of
    32 the signed step is s = m / -127 with m the value of largest magnitude with its sign (the first among equals), so that the
    extreme lands on code 0 (KV[0] = -127); d = max|s| / 31 as the next fp16 at or above it; ls - 32 = s / d rounded AWAY from
    zero and clipped to +-31; every weight takes the table entry nearest x / (d (ls - 32)) (the lower code among equals).  As the
    step |d (ls - 32)| is never below |s|, x / step lies in [-127, 127]; the largest half-gap of the table is 12 (between 89 and
    113) and a value above 113 is at most 14 from it, so every weight decodes within 14 steps |d (ls - 32)| of its value: a bound
    derived from the table, not measured.  A sub-block of zeros stores ls = 32 and code 8, an all-zero block d = 0.  A fixed point
    on its own output, dequantize(quantize(y)) == y for y = dequantize(quantize(W)), in every sub-block that holds code 0 (its
    extreme then decodes to -127 steps and gives the step back: d (ls - 32) has 16 significant bits, so 127 times it is exact
    in fp32); the block's largest sub-block always does (ls - 32 = +-31: d comes back exactly)."""
    x = np.asarray(W, dtype=np.float32).reshape(-1, 8, 32)                                    # [nb][ib][j]
    nb = x.shape[0]
    idx = np.argmax(np.abs(x), axis=2)
    m = np.take_along_axis(x, idx[:, :, None], axis=2)[:, :, 0]
    s = (m / np.float32(-127)).astype(np.float32)
    d = _f16_up(np.abs(s).max(axis=1) / np.float32(31))
    d32 = d.astype(np.float32)
    ok = d32 > 0
    k = np.where(ok[:, None], np.ceil(np.abs(s) / np.where(ok, d32, 1)[:, None]), 0).astype(np.float32)
    k = np.minimum(k + (d32[:, None] * k < np.abs(s)), 31)                                    # (a quotient rounded down onto an integer)
    ls = (np.sign(s) * k).astype(np.int32)                                                    # ls - 32
    step = d32[:, None] * ls.astype(np.float32)                                               # d * (ls - 32) as the decoder forms it
    t = np.where(step[:, :, None] != 0, x / np.where(step != 0, step, 1)[:, :, None], 0).astype(np.float32)
    codes = np.argmin(np.abs(t[..., None] - IQ4_KV.astype(np.float32)), axis=3).astype(np.uint8)   # [nb][8][32], first among equals
    ls6 = (ls + 32).astype(np.uint16)
    out = np.zeros((nb, 136), np.uint8)
    out[:, 0:2] = d.view(np.uint8).reshape(nb, 2)
    sh = np.zeros(nb, np.uint16)
    for ib in range(8):
        sh |= (ls6[:, ib] >> 4) << (2 * ib)
        out[:, 4 + ib // 2] |= ((ls6[:, ib] & 0xF) << (4 * (ib % 2))).astype(np.uint8)
    out[:, 2:4] = sh.view(np.uint8).reshape(nb, 2)
    out[:, 8:136] = (codes[:, :, :16] | (codes[:, :, 16:] << 4)).reshape(nb, 128)
    return out.tobytes()


def iq4_xs_type(name: str, dims, mix: str = "iq4_xs", layer_offset: int = 0, n_layers_file: int | None = None) -> int:
    """ggml type of a matrix in an IQ4_XS file.  mix="iq4_xs": IQ4_XS (23) for every matrix, except Q5_K (13) for attn_v when the
    model groups its heads H / Hkv >= 4, Q5_K for ffn_down in the first n_layer // 8 blocks, and Q6_K (14) for the lm_head
    (output.weight, or a tied token_embd); an untied token_embd is IQ4_XS.  This is llama.cpp's rule for the file type as
    recalled: its source was not at hand when this was written, so check it against a real file before relying on it.
    mix="all_iq4_xs": every matrix IQ4_XS, the head and the embedding table too (so that the IQ4_XS lm_head + ArgMax and embedding
    gather run).  layer_offset / n_layers_file: a pipeline stage's blocks numbered within the whole file."""
    if mix == "all_iq4_xs":
        return 23
    if mix != "iq4_xs":
        raise ValueError(f"unknown IQ4_XS mix {mix!r} (iq4_xs, all_iq4_xs)")
    if name == "output.weight" or (name == "token_embd.weight" and dims.tied):
        return 14
    if not name.startswith("blk."):
        return 23
    layer, n_layer = int(name.split(".")[1]) + layer_offset, n_layers_file or dims.L
    if name.endswith("attn_v.weight"):
        return 13 if dims.H // dims.Hkv >= 4 else 23
    if name.endswith("ffn_down.weight"):
        return 13 if layer < n_layer // 8 else 23
    return 23


def _f16_up(v):
    """The smallest fp16 values >= v (v >= 0, float32 array): a scale that a 6-bit code times it must still reach v."""
    h = np.asarray(v, np.float32).astype(np.float16)
    return np.where(h.astype(np.float32) < v, np.nextafter(h, np.float16(np.inf)), h).astype(np.float16)


def quantize_q5_k(W) -> bytes:
    """Valid ggml block_q5_K for every row of W [rows][cols] (cols % 256 == 0): 176 bytes per 256 weights, in the order fp16 d,
    fp16 dmin, 12 bytes of 6-bit scales / mins (get_scale_min_k4 packing), qh[32], qs[128]; weight = d * sc * q - dmin * m,
    q = 0..31.  Not llama.cpp's search: per sub-block of 32 the 6-bit min m is rounded up (dmin * m >= -min(x, 0)), then the
    6-bit scale up (the 31st code reaches max(x)), so every weight is within half a step d * sc of its code."""
    x = np.asarray(W, dtype=np.float32).reshape(-1, 8, 32)
    nb = x.shape[0]
    sub_min = np.maximum(-x.min(axis=2), 0).astype(np.float32)                  # [nb][8]
    dmin = _f16_up(sub_min.max(axis=1) / np.float32(63))                       # [nb]
    dm32 = dmin.astype(np.float32)
    m = np.where(dm32[:, None] > 0, np.ceil(sub_min / np.where(dm32 > 0, dm32, 1)[:, None]), 0).astype(np.int64)
    m = np.clip(m, 0, 63)
    off = dm32[:, None] * m.astype(np.float32)                                  # dmin * m, exactly as the decoder forms it
    need = np.maximum(x.max(axis=2) + off, 0) / np.float32(31)                  # step that reaches max(x) at code 31
    d = _f16_up(need.max(axis=1) / np.float32(63))
    d32 = d.astype(np.float32)
    sc = np.where(d32[:, None] > 0, np.ceil(need / np.where(d32 > 0, d32, 1)[:, None]), 0).astype(np.int64)
    sc = np.clip(sc, 0, 63)
    step = d32[:, None] * sc.astype(np.float32)
    q = np.where(step[:, :, None] > 0, np.rint((x + off[:, :, None]) / np.where(step > 0, step, 1)[:, :, None]), 0)
    q = np.clip(q, 0, 31).astype(np.uint8)                                      # [nb][8][32]
    out = np.zeros((nb, 176), np.uint8)
    out[:, 0:2] = d.view(np.uint8).reshape(nb, 2)
    out[:, 2:4] = dmin.view(np.uint8).reshape(nb, 2)
    sc8, m8 = sc.astype(np.uint8), m.astype(np.uint8)
    # get_scale_min_k4: j < 4: scales[j] = sc, scales[j + 4] = m (6 bits each); j >= 4: low nibbles in scales[j + 4], the two high
    # bits in the top bits of scales[j - 4] (sc) and scales[j] (m)
    out[:, 4:8] = sc8[:, :4] | ((sc8[:, 4:] >> 4) << 6)
    out[:, 8:12] = m8[:, :4] | ((m8[:, 4:] >> 4) << 6)
    out[:, 12:16] = (sc8[:, 4:] & 0xF) | ((m8[:, 4:] & 0xF) << 4)
    # pair n = sub-blocks 2n, 2n+1: qs[32n + l] = low nibble of q[2n][l] | high nibble of q[2n+1][l]; fifth bits: qh[l] bit 2n, 2n+1
    qh = np.zeros((nb, 32), np.uint8)
    for n in range(4):
        lo, hi = q[:, 2 * n], q[:, 2 * n + 1]
        out[:, 48 + 32 * n:80 + 32 * n] = (lo & 0xF) | ((hi & 0xF) << 4)
        qh |= ((lo >> 4) << (2 * n)) | ((hi >> 4) << (2 * n + 1))
    out[:, 16:48] = qh
    return out.tobytes()


def q5_k_m_type(name: str, dims, layer_offset: int = 0, n_layers_file: int | None = None) -> int:
    """ggml type of a matrix in a Q5_K_M file (llama.cpp's mix): Q5_K (13), except Q6_K (14) for attn_v / ffn_down of the
    use_more_bits blocks (bench.use_more_bits) and for the lm_head (output.weight, or a tied token_embd); an untied token_embd is
    Q5_K."""
    from bench import use_more_bits
    if name == "output.weight" or (name == "token_embd.weight" and dims.tied):
        return 14
    if name.startswith("blk.") and name.endswith(("attn_v.weight", "ffn_down.weight")):
        return 14 if use_more_bits(int(name.split(".")[1]) + layer_offset, n_layers_file or dims.L) else 13
    return 13


def make_tokens(dims: LlamaDims, n: int, seed: int = 99) -> np.ndarray:
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(0, dims.V, size=n, dtype=np.uint32)


def make_metadata(dims: LlamaDims, eps: float = 1e-5) -> dict:
    """The GGUF metadata keys LlamaModel reads (LlamaModel.cs:23-39)."""
    return {
        "general.architecture": "llama", "general.name": dims.name, "llama.block_count": dims.L,
        "llama.attention.head_count": dims.H, "llama.attention.head_count_kv": dims.Hkv,
        "llama.attention.key_length": dims.D, "llama.attention.value_length": dims.D,
        "llama.rope.dimension_count": dims.D, "llama.rope.freq_base": 500000.0,
        "llama.attention.layer_norm_rms_epsilon": eps, "llama.embedding_length": dims.E,
        "llama.feed_forward_length": dims.F, "llama.vocab_size": dims.V,
        "tokenizer.ggml.bos_token_id": 1, "tokenizer.ggml.eos_token_id": 2,
    }
