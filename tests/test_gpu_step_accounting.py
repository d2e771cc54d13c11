"""What the profiling and byte-count entry points of the model, the batch and the window report, on the GPU.

1. nfai_hip_llama_profile_step / _batch_profile_step / _window_profile_step: the launch count of every kernel class, a time for every
   class that launched and none for the others, the position each call leaves behind, and that a profiled step IS a step: the next
   ordinary step matches the CPU oracle fed the same tokens (5e-4 * max(1, max|logit|), fp32 KV: tests/test_gpu_window_decode.py).
   Every profile call is made twice running, so the second one finds what the first left behind.
2. nfai_hip_llama_bytes_per_token / _batch_bytes_per_token / _window_bytes_per_step against a restatement of their formulas from the
   tensor shapes alone (every weight byte once per pass + the KV rows read and written), exactly.

Models: tiny-llama (tied head) in fp16 and in the Q4_K / Q6_K mix of tests/test_gpu_window_decode.py; the byte counts also on an untied
twin of it, where a quantised pass reads the embedding rows from a tensor of its own."""
import dataclasses

import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth
from test_gpu_window_decode import CAP, Q4_K, Q6_K, logit_tol, make_model, odesc, weights

pytestmark = pytest.mark.gpu

DIMS = synth.TINY
UNTIED = dataclasses.replace(synth.TINY, name="tiny-llama-untied", tied=False)
CLASSES = ("qkv", "attn", "wo", "gateup", "down", "lmhead", "other", "engine")
WARM = 5


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


def column_counts(dims, quant):
    """Launches of one batched or windowed token: the embedding rows, five per block, the head; a quantised q|k|v is two launches
    where attn_v (Q6_K on even blocks) and attn_q (Q4_K) differ."""
    split = sum(1 for l in range(dims.L) if l % 2 == 0) if quant else 0
    return dict(other=1, qkv=dims.L + split, attn=dims.L, wo=dims.L, gateup=dims.L, down=dims.L, lmhead=1, engine=0)


def check_times(prof, where):
    print(where, {k: (round(ms, 4), n) for k, (ms, n) in prof.items()})
    assert set(prof) == set(CLASSES)
    for k, (ms, n) in prof.items():
        if n:
            assert ms > 0.0, (where, k, ms, n)
        else:
            assert ms == 0.0, (where, k, ms, n)


def check_logits(lg, am, want, where):
    tol = logit_tol(want, 5e-4)
    err = float(np.abs(lg - want).max())
    print(f"{where}: max|dlogit| {err:.3e} tol {tol:.3e}")
    assert err <= tol, (where, err, tol)
    assert int(am) == int(np.argmax(lg)), (where, int(am))


@pytest.mark.parametrize("quant", [False, True], ids=["f16", "q4km"])
def test_model_profile_step_counts_and_is_a_step(mgr, quant):
    wdev, wref = weights(DIMS, quant)
    m = make_model(mgr, DIMS, wdev, quant)
    ref = orc.OracleLlama(odesc(DIMS, CAP), wref)
    toks = [int(t) for t in synth.make_tokens(DIMS, 16, seed=141)]
    try:
        for t in toks[:WARM]:
            m.Step(t, want_logits=False)
            ref.step(t)
        for j in range(2):
            prof = m.ProfileStep(toks[WARM + j])
            ref.step(toks[WARM + j])
            check_times(prof, f"model call {j}")
            n = {k: v[1] for k, v in prof.items()}
            assert n["lmhead"] == 1 and n["gateup"] == DIMS.L and n["down"] == DIMS.L, n
            assert n["attn"] + n["wo"] + n["qkv"] >= 2 * DIMS.L, n    # attention + Wo may be one launch (the shape table decides)
            assert m.Pos == WARM + j + 1
        lg, am = m.Step(toks[WARM + 2])
        check_logits(lg, am, ref.step(toks[WARM + 2]), "decode_step behind two profiled steps")
        assert m.Pos == WARM + 3
    finally:
        m.Dispose()


@pytest.mark.parametrize("quant", [False, True], ids=["f16", "q4km"])
def test_batch_profile_step_counts_and_is_a_step(mgr, quant):
    from nfai_amd.llama_model import LlamaBatch
    N = 3
    wdev, wref = weights(DIMS, quant)
    mem = [make_model(mgr, DIMS, wdev, quant)]
    mem += [make_model(mgr, DIMS, wdev, quant, share_from=mem[0]) for _ in range(N - 1)]
    refs = [orc.OracleLlama(odesc(DIMS, CAP), wref) for _ in range(N)]
    toks = [[int(t) for t in synth.make_tokens(DIMS, 16, seed=151 + i)] for i in range(N)]
    bt = LlamaBatch(mem, quantized=quant)
    try:
        for i in range(N):
            for t in toks[i][:WARM]:
                mem[i].Step(t, want_logits=False)
                refs[i].step(t)
        for j in range(2):
            prof = bt.ProfileStep([toks[i][WARM + j] for i in range(N)])
            for i in range(N):
                refs[i].step(toks[i][WARM + j])
            check_times(prof, f"batch call {j}")
            assert {k: v[1] for k, v in prof.items()} == column_counts(DIMS, quant)
            assert [m.Pos for m in mem] == [WARM + j + 1] * N
        lg, am = bt.Step([toks[i][WARM + 2] for i in range(N)])
        for i in range(N):
            check_logits(lg[i], am[i], refs[i].step(toks[i][WARM + 2]), f"batch_step member {i} behind two profiled steps")
        assert [m.Pos for m in mem] == [WARM + 3] * N
    finally:
        bt.Dispose()
        for m in reversed(mem):
            m.Dispose()


@pytest.mark.parametrize("quant", [False, True], ids=["f16", "q4km"])
def test_window_profile_step_counts_and_is_a_step(mgr, quant):
    from nfai_amd.llama_model import LlamaWindow
    T = 3
    wdev, wref = weights(DIMS, quant)
    m = make_model(mgr, DIMS, wdev, quant)
    ref = orc.OracleLlama(odesc(DIMS, CAP), wref)
    toks = [int(t) for t in synth.make_tokens(DIMS, 32, seed=161)]
    win = LlamaWindow(m, 8, quantized=quant)
    try:
        for t in toks[:WARM]:
            m.Step(t, want_logits=False)
            ref.step(t)
        cur = WARM
        for j in range(2):
            prof = win.ProfileStep(toks[cur:cur + T])
            for t in toks[cur:cur + T]:
                ref.step(t)
            cur += T
            check_times(prof, f"window call {j}")
            assert {k: v[1] for k, v in prof.items()} == column_counts(DIMS, quant)
            assert m.Pos == cur
        lg, am = win.Step(toks[cur:cur + T])
        for i in range(T):
            check_logits(lg[i], am[i], ref.step(toks[cur + i]), f"window_step column {i} behind two profiled steps")
        assert m.Pos == cur + T
    finally:
        win.Dispose()
        m.Dispose()


# ---- 2: byte counts ------------------------------------------------------------------------------------------------------------------
def matrix_bytes(t):
    """fp16: 2 bytes per weight; Q4_K: 144 bytes per 256 weights; Q6_K: 210."""
    rows, cols = t.shape
    if isinstance(t, np.ndarray):
        assert t.dtype == np.float16
        return rows * cols * 2
    return rows * cols // 256 * {Q4_K: 144, Q6_K: 210}[t.ggml_type]


class Bytes:
    """The formulas of the three counters from the shapes of what the model loaded."""

    def __init__(self, dims, wdev, quant, kv_f16):
        self.d, self.quant = dims, quant
        blk = lambda l, names: sum(matrix_bytes(wdev[f"blk.{l}.{n}.weight"]) for n in names)
        self.qkv = [blk(l, ("attn_q", "attn_k", "attn_v")) for l in range(dims.L)]
        self.gu = [blk(l, ("ffn_gate", "ffn_up")) for l in range(dims.L)]
        self.blocks = sum(self.qkv) + sum(self.gu) + sum(blk(l, ("attn_output", "ffn_down")) for l in range(dims.L))
        self.untied = "output.weight" in wdev
        self.head = matrix_bytes(wdev["output.weight" if self.untied else "token_embd.weight"])
        self.emb_row = matrix_bytes(wdev["token_embd.weight"]) // dims.V
        self.gains = (2 * dims.L + 1) * dims.E * 4
        self.kv_row = 2 * dims.Hkv * dims.D * (2 if kv_f16 else 4)

    def once(self):
        """Every weight byte once per pass of a batch or a window; a quantised pass counts the norm gains too."""
        return self.blocks + self.head + (self.gains if self.quant else 0)

    def rows(self, n):
        """n embedding rows: a quantised pass over a tied table has them in the head's bytes already."""
        return n * self.emb_row if (not self.quant or self.untied) else 0

    def model(self, pos):
        return self.blocks + self.d.L * self.kv_row * (pos + 2) + self.emb_row + self.head, max(self.qkv + self.gu)

    def batch(self, positions):
        return self.once() + self.rows(len(positions)) + sum(self.d.L * self.kv_row * (p + 2) for p in positions)

    def window(self, pos, t):
        return self.once() + self.rows(t) + self.d.L * self.kv_row * (pos + t * (t + 1) // 2 + t)


@pytest.mark.parametrize("kv_f16", [False, True], ids=["kv32", "kv16"])
@pytest.mark.parametrize("quant", [False, True], ids=["f16", "q4km"])
@pytest.mark.parametrize("dims", [DIMS, UNTIED], ids=["tied", "untied"])
def test_byte_counts_are_the_formulas_on_the_tensor_shapes(mgr, dims, quant, kv_f16):
    from nfai_amd.llama_model import LlamaBatch, LlamaWindow
    wdev, _ = weights(dims, quant)
    assert ("output.weight" in wdev) == (not dims.tied)
    want = Bytes(dims, wdev, quant, kv_f16)
    mem = [make_model(mgr, dims, wdev, quant, kv_f16=kv_f16)]
    mem += [make_model(mgr, dims, wdev, quant, kv_f16=kv_f16, share_from=mem[0]) for _ in range(2)]
    toks = [int(t) for t in synth.make_tokens(dims, 8, seed=171)]
    bt = LlamaBatch(mem, quantized=quant)
    win = LlamaWindow(mem[0], 8, quantized=quant)
    try:
        positions = [5, 6, 7]
        for m, p in zip(mem, positions):
            for t in toks[:p]:
                m.Step(t, want_logits=False)
        assert [m.Pos for m in mem] == positions
        assert bt.BytesPerToken() == want.batch(positions)
        for t in (1, 3, 8):
            assert win.BytesPerStep(t) == want.window(5, t), t
        for pos in (0, 5, 37):
            assert mem[0].BytesPerToken(pos) == want.model(pos), pos
    finally:
        win.Dispose()
        bt.Dispose()
        for m in reversed(mem):
            m.Dispose()
