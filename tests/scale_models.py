"""Exact power-of-two rescalings of a Llama model, shared by tests/test_scale_sweep.py (CPU) and tests/test_gpu_scale_sweep.py.

A block computes the same function when a producer is multiplied by 2^k and its consumers by 2^-k.  While every scaled tensor stays
exactly representable and nothing overflows, every intermediate value of an fp32 evaluation moves by an exact power of two and the
logits do not move by a bit: ONE oracle walk is the expected result at every k, while the magnitudes a kernel sees move by 2^+-k.

Groups (applied to every block):
  qkv_in     attn_norm gain x 2^k        | attn_q, attn_k, attn_v x 2^-k        the q|k|v input moves
  q_k        attn_q x 2^k                | attn_k x 2^-k                        q and the K rows move, the scores do not
  v_wo       attn_v x 2^k                | attn_output x 2^-k                   the V rows and the Wo input move
  gateup_in  ffn_norm gain x 2^k         | ffn_gate, ffn_up x 2^-k              the gate|up input moves
  up_down    ffn_up x 2^k                | ffn_down x 2^-k                      the Wdown input moves
  head_in    output_norm gain x 2^k      | nothing: the logits are 2^k times the base's, undone exactly by the caller
  resid      token_embd, every attn_output and ffn_down x 2^k: the residual stream moves.  NOT exact (RMSNorm's eps does not move
             with it): this group gets an oracle walk of its own per k.  With a tied head the logits carry 2^k as well.

Matrices are fp16, or quantised blocks whose fp16 header fields (d of Q8_0 / Q6_K, d and dmin of Q4_K / Q5_K) are scaled; gains fp32.
floor_weights() first removes the low bits that a scaling down by up to 2^-s_up would lose (into the fp16 subnormals included), so
that every later scaling is exact; rescale() checks each product in float64 and raises ValueError where it is not."""
import functools

import numpy as np

from nfai_amd import synth
from oracle import np_oracle as npo

from test_batch_wide_bar import Restated, split

S_UP = 12          # fp16 matrices: exact down to 2^-12
S_UP_QUANT = 6     # quantised headers: exact down to 2^-6
CEILING = 32768.0  # no fp16-fed vector above it: one binade under the documented overflow at 65504
F16_MAX = 65504.0
F16_MIN_NORMAL = 2.0 ** -14
GROUPS = ("qkv_in", "q_k", "v_wo", "gateup_in", "up_down", "head_in", "resid")
EXACT_GROUPS = GROUPS[:-1]

Q8_0, Q4_K, Q5_K, Q6_K = 8, 12, 13, 14
# ggml type -> (block bytes, byte offsets of the fp16 header fields)
HEADERS = {Q8_0: (34, (0,)), Q4_K: (144, (0, 2)), Q5_K: (176, (0, 2)), Q6_K: (210, (208,))}

# group -> (tensors x 2^k, tensors x 2^-k) by their name inside a block ("" prefix: a global tensor)
_BLOCK = {
    "qkv_in": (("attn_norm",), ("attn_q", "attn_k", "attn_v")),
    "q_k": (("attn_q",), ("attn_k",)),
    "v_wo": (("attn_v",), ("attn_output",)),
    "gateup_in": (("ffn_norm",), ("ffn_gate", "ffn_up")),
    "up_down": (("ffn_up",), ("ffn_down",)),
    "head_in": ((), ()),
    "resid": (("attn_output", "ffn_down"), ()),
}
# group -> the fp16-fed vectors that move with it: (kind of activation_maxima, sign of the exponent)
_FED = {
    "qkv_in": (("qkv", 1),), "q_k": (("q", 1), ("k", -1)), "v_wo": (("v", 1), ("wo", 1)), "gateup_in": (("gateup", 1),),
    "up_down": (("down", 1),), "head_in": (("head", 1),), "resid": (),
}


def is_quant(t):
    return hasattr(t, "ggml_type")


def _exact(got, want64, what):
    if not (np.isfinite(got).all() and np.array_equal(np.asarray(got, np.float64), want64)):
        raise ValueError(f"{what}: the product is not exactly representable")
    return got


def scale_tensor(t, j, what="tensor"):
    """t x 2^j, asserted exact: an fp16 matrix, an fp32 gain vector, or a QuantTensor (its fp16 header fields)."""
    if j == 0:
        return t
    f = 2.0 ** j
    if is_quant(t):
        size, fields = HEADERS[t.ggml_type]
        b = np.array(t.data, np.uint8).reshape(-1, size)
        for o in fields:
            h = b[:, o:o + 2].copy().view(np.float16)
            b[:, o:o + 2] = _exact((h.astype(np.float64) * f).astype(np.float16), h.astype(np.float64) * f, what).view(np.uint8)
        return type(t)(b.reshape(-1), t.ggml_type, t.shape)
    a = np.asarray(t)
    return _exact((a.astype(np.float64) * f).astype(a.dtype), a.astype(np.float64) * f, what)


def floor_weights(w, s_up=S_UP):
    """Every matrix rounded to fp16 at 2^-s_up of its scale and multiplied back (a QuantTensor: its header fields); gains stay fp32.
    Every later scaling of a matrix by 2^j, j >= -s_up, is then exact."""
    out = {}
    for name, t in w.items():
        if is_quant(t):
            size, fields = HEADERS[t.ggml_type]
            b = np.array(t.data, np.uint8).reshape(-1, size)
            for o in fields:
                h = b[:, o:o + 2].copy().view(np.float16).astype(np.float32)
                low = (h * np.float32(2.0 ** -s_up)).astype(np.float16).astype(np.float32)
                b[:, o:o + 2] = (low * np.float32(2.0 ** s_up)).astype(np.float16).view(np.uint8)
            out[name] = type(t)(b.reshape(-1), t.ggml_type, t.shape)
        elif t.ndim == 1:
            out[name] = np.asarray(t, np.float32)
        else:
            low = (np.asarray(t, np.float32) * np.float32(2.0 ** -s_up)).astype(np.float16).astype(np.float32)
            out[name] = (low * np.float32(2.0 ** s_up)).astype(np.float16)
    return out


def rescale(w, dims, group, k):
    """The weights of `group` at exponent k (a new dict; untouched tensors are shared).  ValueError where a product is inexact."""
    up, down = _BLOCK[group]
    out = dict(w)
    for l in range(dims.L):
        for names, j in ((up, k), (down, -k)):
            for n in names:
                name = f"blk.{l}.{n}.weight"
                out[name] = scale_tensor(w[name], j, f"{name} x 2^{j}")
    if group == "head_in":
        out["output_norm.weight"] = scale_tensor(w["output_norm.weight"], k, f"output_norm x 2^{k}")
    if group == "resid":
        out["token_embd.weight"] = scale_tensor(w["token_embd.weight"], k, f"token_embd x 2^{k}")
    return out


def logit_factor(dims, group, k):
    """What the logits at exponent k carry over the base's (an exact power of two; divide it out before comparing)."""
    if group == "head_in" or (group == "resid" and dims.tied):
        return 2.0 ** k
    return 1.0


def state_factors(group, k):
    """(K rows, V rows, hidden state): the power of two each is written at, relative to the oracle walk it is compared with."""
    return (2.0 ** -k if group == "q_k" else 1.0, 2.0 ** k if group == "v_wo" else 1.0, 2.0 ** k if group == "resid" else 1.0)


def wmax_of(w):
    """Largest |weight| over the fp16 matrices."""
    return max(float(np.abs(np.asarray(a, np.float32)).max()) for a in w.values() if not is_quant(a) and a.ndim == 2)


# ---- the float32 restatement, with the ways a kernel could treat the two planes --------------------------------------------------------
def _flush(a):
    """fp16 subnormals -> 0 (the values are fp16 values held in float32)."""
    return np.where(np.abs(a) < np.float32(F16_MIN_NORMAL), np.float32(0), a)


class Walk(Restated):
    """tests/test_batch_wide_bar.py::Restated with a choice of GEMV arithmetic and of what the attention reads.
    arith: "split"  hi + 2^-11 lo, as kernels_gemv_wide.hip states it
           "hi"     the lo plane dropped: activations rounded to fp16
           "flush"  the split on a matrix core that flushes fp16 subnormal operands (weights and both planes) to zero
           "f32"    fp32 activations (the kernels off the matrix cores)
    rows:  ""  the attention reads fp32 rows; "kv" K / V rows rounded to fp16 (an fp16 KV cache); "qkv" q rows as well (the prefill)
    It records max |x| per GEMV kind and max |q|, |K|, |V| over the rows."""
    KINDS = {"attn_q": "qkv", "attn_k": "qkv", "attn_v": "qkv", "attn_output": "wo", "ffn_gate": "gateup", "ffn_up": "gateup",
             "ffn_down": "down", "token_embd": "head", "output": "head"}

    def __init__(self, d, w, arith="split", rows="", cap=32):
        super().__init__(d, w, arith != "hi", cap=cap)
        self.arith, self.rows, self.maxima = arith, rows, {}
        if arith == "flush":
            self.w = {k: (_flush(v) if v.ndim == 2 else v) for k, v in self.w.items()}

    def note(self, kind, v):
        self.maxima[kind] = max(self.maxima.get(kind, 0.0), float(np.abs(v).max()))

    def mm(self, name, x):
        self.note(self.KINDS[name.split(".")[-2]], x)
        W, x = self.w[name], np.asarray(x, np.float32)
        if self.arith == "f32":
            return (W @ x).astype(np.float32)
        hi, lo = split(x)
        if self.arith == "flush":
            hi, lo = _flush(hi), _flush(lo)
        y = W @ hi
        if self.arith != "hi":
            y = y + (W @ lo) * np.float32(2.0 ** -11)
        return y.astype(np.float32)

    def row(self, kind, v):
        self.note(kind, v)
        if kind in self.rows:
            return v.astype(np.float16).astype(np.float32)
        return v


def activation_maxima(dims, w, toks):
    """max |x| per GEMV kind (qkv, wo, gateup, down, head) and max |q|, |k|, |v| over the rows, from one walk of the float32
    restatement over `toks` (one sequence, or a list of sequences: the largest over all of them)."""
    seqs = toks if isinstance(toks[0], (list, tuple, np.ndarray)) else [toks]
    out = {}
    for seq in seqs:
        r = Walk(dims, w, "split", cap=len(seq))
        for t in seq:
            r.step(int(t))
        for kind, v in r.maxima.items():
            out[kind] = max(out.get(kind, 0.0), v)
    return out


def allowed(group, maxima, wmax, k, s_up=S_UP):
    """Whether exponent k keeps every fp16-fed vector of the group at or below CEILING and every scaled matrix exact and finite."""
    up, down = _BLOCK[group]
    mats = [1 for n in up if "norm" not in n] + [-1 for n in down] + ([1] if group == "resid" else [])
    for sign in mats:
        j = sign * k
        if j < -s_up or wmax * 2.0 ** j >= F16_MAX:
            return False
    return all(maxima[kind] * 2.0 ** (sign * k) <= CEILING for kind, sign in _FED[group])


def sweep(group, maxima, wmax, s_up=S_UP):
    """The exponents to run: -17 (or the lowest exact one), -12, -6, 0, +6, +10 and the top, the largest k at which every fp16-fed
    vector of the group stays at or below 32768 (derived from `maxima`) and every scaled matrix is exact and below 65504."""
    ok = [k for k in range(-17, 18) if allowed(group, maxima, wmax, k, s_up)]
    return sorted({k for k in (ok[0], -12, -6, 0, 6, 10, ok[-1]) if k in ok})


# ---- quantised models ------------------------------------------------------------------------------------------------------------------
QUANT_MIXES = ("q4_k_m", "q5_k_m", "all_q8_0")


def quant_model(dims, mix, seed=21, std=0.05):
    """{name: QuantTensor | gains} of one of QUANT_MIXES, as the batch tests quantise it (tests/test_gpu_batch_quant.py: the Q4_K_M
    mix; tests/test_gpu_batch_quant_any.py: the others), headers floored at 2^-6."""
    if mix == "q4_k_m":
        from test_gpu_batch_quant import quant_weights
        wq = quant_weights(synth.make_weights(dims, seed=seed, std=std))[0]
    else:
        from test_gpu_batch_quant_any import quant_weights
        wq = quant_weights(dims, mix, seed=seed, std=std)[0]
    return floor_weights(wq, S_UP_QUANT)


def dequantised(wq, base=None):
    """What the oracle computes on: every QuantTensor through the dequantiser the quant tests use for its type.  base = (wq0, its
    dequantised dict): tensors that rescale() left untouched (the same objects as in wq0) are taken from there."""
    import oracle as orc
    from test_gpu_batch_quant_any import dequant_q5_k, dequant_q8_0
    out = {}
    for name, t in wq.items():
        if not is_quant(t):
            out[name] = t
            continue
        if base is not None and base[0][name] is t:
            out[name] = base[1][name]
            continue
        n = int(np.prod(t.shape))
        if t.ggml_type == Q4_K:
            out[name] = orc.dequant_q4k(t.data, n).reshape(t.shape)
        elif t.ggml_type == Q6_K:
            out[name] = orc.dequant_q6k(t.data, n).reshape(t.shape)
        elif t.ggml_type == Q5_K:
            out[name] = np.ascontiguousarray(dequant_q5_k(t.data, *t.shape), np.float32)
        else:
            out[name] = np.ascontiguousarray(dequant_q8_0(t.data, *t.shape), np.float32)
    return out


def quant_sweep(wq, dims, group, maxima):
    """The exponents of the fp16 sweep list (-17, -12, -6, 0, +6, +10, +12) at which the header rescaling is exact (matrices are
    floored at 2^-6; a group that scales only a gain down goes further) and every fp16-fed vector of the group stays at or below
    32768 by `maxima` (activation_maxima on the dequantised model over the sequences the test runs)."""
    out = []
    for k in (-17, -12, -6, 0, 6, 10, 12):
        if any(maxima[kind] * 2.0 ** (sign * k) > CEILING for kind, sign in _FED[group]):
            continue
        try:
            rescale(wq, dims, group, k)
            out.append(k)
        except ValueError:
            pass
    return out


QUANT_SEQS = 4   # the quantised GPU paths run sequences 0 .. 3 (a batch of 4)


@functools.lru_cache(maxsize=None)
def quant_base(dims, mix):
    """(what the model loads, what the oracle computes on, the exponents of every group), shared by the CPU and the GPU test."""
    wq = quant_model(dims, mix)
    wref = dequantised(wq)
    maxima = activation_maxima(dims, wref, [seq_tokens(dims, s) for s in range(QUANT_SEQS)])
    return wq, wref, {g: quant_sweep(wq, dims, g, maxima) for g in GROUPS}


# ---- sequences and the oracle ----------------------------------------------------------------------------------------------------------
N_TOK, N_EXTRA, CAP = 12, 4, 32   # 12 tokens per sequence; the prefill test decodes 4 more; KV capacity 32


def seq_tokens(dims, s):
    return [int(t) for t in synth.make_tokens(dims, N_TOK + N_EXTRA, seed=100 + s)]


def oracle_walk(dims, w, toks, cap=CAP):
    """One oracle walk: (logits per step, hidden state per step, K caches, V caches)."""
    import oracle as orc
    ref = orc.OracleLlama(orc.LlamaDesc(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, C=cap), w)
    logits, hidden = [], []
    for t in toks:
        logits.append(ref.step(int(t)).copy())
        hidden.append(ref.hidden())
    K = [ref.kcache(l)[:len(toks)].copy() for l in range(dims.L)]
    V = [ref.vcache(l)[:len(toks)].copy() for l in range(dims.L)]
    ref.close()
    return logits, hidden, K, V
