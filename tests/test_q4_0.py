"""Q4_0 weights on CPU: the GGUF reader / writer, the C ABI's byte count, the synthetic quantiser, the file mix and the pipeline
cost model.  Every Q4_0 value here is decoded by this file's own restatement of ggml's block_q4_0 (fp16 d, then qs[16]; weight j =
d * ((qs[j] & 0xF) - 8), weight j + 16 = d * ((qs[j] >> 4) - 8)), and the known answers are written out by hand."""
import ctypes
import os
import re

import numpy as np
import pytest

from nfai_amd import gguf, synth
from nfai_amd.llama_model import QuantTensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q4_0 = 2


def dequant_q4_0(raw, rows, cols):
    b = np.frombuffer(bytes(raw), np.uint8).reshape(rows * cols // 32, 18)
    d = b[:, :2].copy().view(np.float16).astype(np.float32)[:, 0]
    out = np.empty((b.shape[0], 32), np.float32)
    for j in range(16):
        out[:, j] = d * (np.float32(1) * ((b[:, 2 + j] & 0xF).astype(np.int32) - 8)).astype(np.float32)
        out[:, j + 16] = d * (np.float32(1) * ((b[:, 2 + j] >> 4).astype(np.int32) - 8)).astype(np.float32)
    return out.reshape(rows, cols)


def q4_bytes(rows, cols, seed):
    rng = np.random.default_rng(seed)
    return np.frombuffer(synth.quantize_q4_0(rng.standard_normal((rows, cols)).astype(np.float32)), np.uint8).copy()


def write_one(tmp_path, name, raw, shape, ty=Q4_0):
    w = gguf.GGUFWriter()
    w.add("general.architecture", "llama")
    w.add_tensor(name, QuantTensor(raw, ty, shape))
    path = str(tmp_path / f"{name}.gguf")
    w.write(path)
    return path


@pytest.mark.parametrize("shape", [(16, 256), (32, 512)])
def test_gguf_reads_q4_0_as_quant_tensor_and_round_trips(tmp_path, shape):
    raw = q4_bytes(*shape, seed=shape[0])
    assert raw.size == shape[0] * shape[1] // 32 * 18
    _, t = gguf.Parser().Read(write_one(tmp_path, "w", raw, shape))
    qt = t["w"]
    assert isinstance(qt, QuantTensor) and qt.ggml_type == Q4_0 and qt.shape == shape
    np.testing.assert_array_equal(qt.data, raw)
    w = gguf.GGUFWriter()
    w.add_tensor("again", qt)
    path = str(tmp_path / "again.gguf")
    w.write(path)
    _, t2 = gguf.Parser().Read(path)
    assert t2["again"].shape == shape and t2["again"].ggml_type == Q4_0
    np.testing.assert_array_equal(t2["again"].data, raw)


@pytest.mark.parametrize("shape", [(1, 32), (16, 32), (15, 256), (16, 288), (16, 512 + 256 * 127)])
def test_gguf_rejects_q4_0_outside_the_shape_rules(tmp_path, shape):
    raw = q4_bytes(*shape, seed=3)
    with pytest.raises(ValueError, match=r"Unsupported data type Q4_0.*" + re.escape(gguf.Q4_0_RULE)):
        gguf.Parser().Read(write_one(tmp_path, "w", raw, shape))
    assert "rows % 16 == 0" in gguf.Q4_0_RULE and "cols % 256 == 0" in gguf.Q4_0_RULE and "cols <= 32768" in gguf.Q4_0_RULE


def test_gguf_still_refuses_q5_1(tmp_path):
    with pytest.raises(ValueError, match="Unsupported data type Q5_1"):
        gguf.Parser().Read(write_one(tmp_path, "w", np.zeros(16 * 8 * 24, np.uint8), (16, 256), ty=7))


@pytest.fixture(scope="module")
def lib():
    from nfai_amd import build as hb, _lib
    hb.build()
    return _lib.load()


def test_weight_bytes_q4_0_through_the_c_abi(lib):
    from nfai_amd import _lib
    assert _lib.Q4_0 == 2
    n = ctypes.c_uint64()
    _lib.call("nfai_hip_weight_bytes", _lib.Q4_0, 16, 256, ctypes.byref(n))
    assert n.value == 16 * 8 * 18
    _lib.call("nfai_hip_weight_bytes", _lib.Q4_0, 128256, 3072, ctypes.byref(n))
    assert n.value == 128256 * 3072 // 32 * 18
    for rows, cols in ((1, 32), (16, 32), (15, 256), (16, 288), (16, 512 + 256 * 127)):
        with pytest.raises(_lib.NfaiHipError) as e:
            _lib.call("nfai_hip_weight_bytes", _lib.Q4_0, rows, cols, ctypes.byref(n))
        assert e.value.code == _lib.ERR_UNSUPPORTED
        assert "Q4_0 needs rows % 16 == 0, cols % 256 == 0 and cols <= 32768" in str(e.value)
    with pytest.raises(_lib.NfaiHipError) as e:   # Q5_1 stays without a kernel
        _lib.call("nfai_hip_weight_bytes", 7, 16, 256, ctypes.byref(n))
    assert e.value.code == _lib.ERR_UNSUPPORTED


def test_q4_0_type_ids_in_the_header_and_csharp():
    cs = open(os.path.join(ROOT, "csharp", "NFAI.HIP", "Native.cs")).read()
    assert re.search(r"enum GgmlType\s*\{[^}]*\bQ4_0 = 2\b", cs)
    h = open(os.path.join(ROOT, "include", "nfai_hip.h")).read()
    assert re.search(r"enum nfai_dtype\s*\{[^}]*\bNFAI_Q4_0 = 2\b", h)
    assert gguf.GGML_Q4_0 == 2 and gguf.GGML_BLOCK[2] == (32, 18)


def block(d16, codes):
    """18 bytes written by hand: fp16 d, then qs[j] = codes[j] | codes[j + 16] << 4."""
    c = np.asarray(codes, np.uint8)
    assert c.size == 32 and c.max() <= 15
    return np.float16(d16).tobytes() + (c[:16] | (c[16:] << 4)).astype(np.uint8).tobytes()


def test_quantize_q4_0_known_answers():
    # the extreme is negative: max = -8, d = -8 / -8 = 1 (positive); x = k - 8 for code k, x * id + 8.5 = k + 0.5 -> k
    codes = np.array([0] + [(3 * j) % 16 for j in range(1, 32)])
    x = (codes.astype(np.float32) - 8).reshape(1, 32)
    assert x.min() == -8 and np.abs(x).max() == 8 and x.max() == 7
    raw = synth.quantize_q4_0(x)
    assert raw == block(1.0, codes)
    np.testing.assert_array_equal(dequant_q4_0(raw, 1, 32), x)
    # the extreme is positive: max = +4, d = 4 / -8 = -0.5 (negative); the extreme lands on code 0 and decodes as -0.5 * -8 = 4;
    # x = -0.5 * (k - 8): -3.5 -> code 15, 0 -> code 8
    x = np.zeros((1, 32), np.float32)
    x[0, :4] = [4.0, -3.5, 1.0, -1.5]
    raw = synth.quantize_q4_0(x)
    assert raw == block(-0.5, [0, 15, 6, 11] + [8] * 28)
    np.testing.assert_array_equal(dequant_q4_0(raw, 1, 32), x)
    # the clamp at 15: the extreme is +8 (d = -1), and -8 would be code 16: it is stored as 15 and decodes as -7
    x = np.zeros((1, 32), np.float32)
    x[0, 0], x[0, 1] = 8.0, -8.0   # the FIRST element of largest magnitude gives the sign
    raw = synth.quantize_q4_0(x)
    assert raw == block(-1.0, [0, 15] + [8] * 30)
    assert list(dequant_q4_0(raw, 1, 32)[0, :3]) == [8.0, -7.0, 0.0]
    # an all-zero block: max = 0, d = 0 / -8 (zero, with the sign the division gives it: -0.0), id = 0, every code int(8.5) = 8
    raw = synth.quantize_q4_0(np.zeros((1, 64), np.float32))
    assert np.frombuffer(raw[:2], np.float16)[0] == 0.0
    assert raw == block(-0.0, [8] * 32) * 2
    assert not dequant_q4_0(raw, 1, 64).any()
    # d is rounded to fp16 for storage, the codes come from the fp32 d: max = -1 -> d = 0.125 exactly; max = -0.8 -> d = 0.1 in
    # fp32, 0.0999755859375 in fp16
    x = np.zeros((1, 32), np.float32)
    x[0, :3] = [-0.8, 0.7, 0.05]   # 0.7 * 10 + 8.5 = 15.5 -> 15; 0.05 * 10 + 8.5 = 9.0 -> 9 (or 8.99.. -> 8: checked below)
    raw = synth.quantize_q4_0(x)
    d32 = np.float32(-0.8) / np.float32(-8)
    assert np.frombuffer(raw[:2], np.float16)[0] == np.float16(d32) and np.float32(np.float16(d32)) != d32
    idv = np.float32(1) / d32
    want = [min(15, int(np.float32(v) * idv + np.float32(8.5))) for v in x[0]]
    assert want[0] == 0 and want[1] == 15 and want[3:] == [8] * 29
    assert raw[2:] == block(0.0, want)[2:]
    np.testing.assert_array_equal(dequant_q4_0(raw, 1, 32)[0, :2], np.float32(np.float16(d32)) * np.float32([-8, 7]))
    # nibble order: qs[j] holds weight j in its low and weight j + 16 in its high nibble
    x = np.zeros((1, 32), np.float32)
    x[0, 0], x[0, 5], x[0, 21] = -8.0, 3.0, -2.0
    raw = synth.quantize_q4_0(x)
    qs = np.frombuffer(raw[2:], np.uint8)
    assert qs[0] == (0 | 8 << 4) and qs[5] == (11 | 6 << 4) and all(qs[j] == 0x88 for j in range(16) if j not in (0, 5))
    # rows are independent and row-major: two rows of 64
    x = np.random.default_rng(5).standard_normal((2, 64)).astype(np.float32)
    raw = synth.quantize_q4_0(x)
    assert raw[:36] == synth.quantize_q4_0(x[:1]) and raw[36:] == synth.quantize_q4_0(x[1:])


def test_numpy_dequantiser_gives_d_times_q_minus_8():
    rng = np.random.default_rng(11)
    b = rng.integers(0, 256, (24, 18), dtype=np.uint8)
    b[:, :2] = (0.01 * rng.standard_normal(24)).astype(np.float16).view(np.uint8).reshape(-1, 1, 2)[:, 0]
    b[3, :2] = np.float16(-0.0).tobytes()[0], np.float16(-0.0).tobytes()[1]
    got = synth.dequantize_q4_0(b.tobytes(), 3, 256)
    assert got.dtype == np.float32 and got.shape == (3, 256)
    np.testing.assert_array_equal(got, dequant_q4_0(b.tobytes(), 3, 256))
    # and against the quantiser: every weight within half a step of its code, the extreme exact up to the fp16 rounding of d
    x = rng.standard_normal((4, 256)).astype(np.float32)
    y = synth.dequantize_q4_0(synth.quantize_q4_0(x), 4, 256)
    step = np.abs(x.reshape(-1, 32)).max(axis=1) / 8
    # (code 16 clamps to 15: one whole step; the fp16 rounding of d moves a weight by at most 8 codes * 2^-11)
    assert (np.abs(x - y).reshape(-1, 32) <= (1.0 + 8 * 2.0 ** -11) * step[:, None] + 1e-7).all()


@pytest.mark.parametrize("dims", [synth.LLAMA_32_1B, synth.LLAMA_32_3B, synth.LLAMA_31_8B], ids=lambda d: d.name)
def test_pipeline_costs_q4_0_against_a_hand_sum(dims):
    from nfai_amd.pipeline import pipeline_costs
    E, F, HD, KD, V = dims.E, dims.F, dims.H * dims.D, dims.Hkv * dims.D, dims.V
    per_block = (HD * E + 2 * KD * E + E * HD + 3 * F * E) * 18 / 32      # 4.5 bits per weight
    blk, head = pipeline_costs(dims, "q4_0")
    assert blk == pytest.approx(per_block, rel=1e-12)
    assert head == pytest.approx(V * E * 210 / 256, rel=1e-12)            # output.weight or the tied token_embd: Q6_K


def test_q4_0_type_for_tied_and_untied_models():
    tied, untied = synth.LLAMA_32_1B, synth.LLAMA_31_8B
    assert tied.tied and not untied.tied
    assert synth.q4_0_type("token_embd.weight", tied) == 14
    assert synth.q4_0_type("token_embd.weight", untied) == 2
    assert synth.q4_0_type("output.weight", untied) == 14
    for n in ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down"):
        for d in (tied, untied):
            assert synth.q4_0_type(f"blk.3.{n}.weight", d) == 2
            assert synth.q4_0_type(f"blk.3.{n}.weight", d, "all_q4_0") == 2
    assert synth.q4_0_type("token_embd.weight", tied, "all_q4_0") == 2 and synth.q4_0_type("output.weight", untied, "all_q4_0") == 2
    with pytest.raises(ValueError):
        synth.q4_0_type("output.weight", tied, "q4_1")


def test_python_hosts_argument_checks():
    """The checks LlamaBatch makes before it touches the library, and the bookkeeping that picks any_quant for a Q4_0 model."""
    from nfai_amd import _lib
    from nfai_amd.llama_model import LlamaBatch, LlamaModel
    with pytest.raises(ValueError, match="any_quant=True widens quantized=True"):
        LlamaBatch([], quantized=False, any_quant=True)
    with pytest.raises(ValueError, match="wide=True takes fp16 models only"):
        LlamaBatch([], quantized=True, any_quant=True, wide=True)

    calls = []

    class Probe(LlamaModel):   # SetTensor's bookkeeping without a library behind it
        def __init__(self):
            self.handle, self._quantized, self._any_quant = None, False, False

    import nfai_amd.llama_model as lm
    saved = lm.call
    lm.call = lambda *a: calls.append(a)
    try:
        p = Probe()
        p.SetTensor("blk.0.attn_q.weight", QuantTensor(np.zeros(16 * 8 * 18, np.uint8), Q4_0, (16, 256)))
        assert p._quantized and p._any_quant
        assert calls[-1][0] == "nfai_hip_llama_set_tensor" and calls[-1][3:6] == (Q4_0, 16, 256)
        p = Probe()
        p.SetTensor("blk.0.attn_q.weight", (0x1000, _lib.Q4_0, 16, 256))
        assert p._quantized and p._any_quant
        p = Probe()
        p.SetTensor("blk.0.attn_q.weight", QuantTensor(np.zeros(16 * 144, np.uint8), 12, (16, 256)))
        assert p._quantized and not p._any_quant   # Q4_K alone needs no BATCH_QUANT_ANY
    finally:
        lm.call = saved
