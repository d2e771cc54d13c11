"""Q8_0 weights on CPU: the GGUF reader / writer, the C ABI's byte count, the synthetic quantiser and the pipeline cost model.
Every Q8_0 value here is decoded by this file's own restatement of ggml's block_q8_0 (fp16 d, then int8 qs[32]; weight = d * q),
not by anything in nfai_amd."""
import ctypes
import os
import re

import numpy as np
import pytest

from nfai_amd import gguf, synth
from nfai_amd.llama_model import QuantTensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q8_0 = 8


def dequant_q8_0(raw, rows, cols):
    """ggml dequantize_row_q8_0: block i of a row = bytes [34 i, 34 i + 34): d = fp16 at +0, qs = int8 at +2 .. +34."""
    b = np.frombuffer(bytes(raw), np.uint8).reshape(rows * cols // 32, 34)
    d = b[:, :2].copy().view(np.float16).astype(np.float32)[:, 0]
    q = b[:, 2:].copy().view(np.int8).astype(np.float32)
    return (d[:, None] * q).reshape(rows, cols)


def q8_bytes(rows, cols, seed):
    rng = np.random.default_rng(seed)
    return np.frombuffer(synth.quantize_q8_0(rng.standard_normal((rows, cols)).astype(np.float32)), np.uint8).copy()


def write_one(tmp_path, name, raw, shape):
    w = gguf.GGUFWriter()
    w.add("general.architecture", "llama")
    w.add_tensor(name, QuantTensor(raw, Q8_0, shape))
    path = str(tmp_path / f"{name}.gguf")
    w.write(path)
    return path


@pytest.mark.parametrize("shape", [(16, 256), (32, 512)])
def test_gguf_reads_q8_0_as_quant_tensor_and_round_trips(tmp_path, shape):
    raw = q8_bytes(*shape, seed=shape[0])
    assert raw.size == shape[0] * shape[1] // 32 * 34
    _, t = gguf.Parser().Read(write_one(tmp_path, "w", raw, shape))
    qt = t["w"]
    assert isinstance(qt, QuantTensor) and qt.ggml_type == Q8_0 and qt.shape == shape
    np.testing.assert_array_equal(qt.data, raw)
    # writer -> reader again, from the QuantTensor the reader returned
    w = gguf.GGUFWriter()
    w.add_tensor("again", qt)
    path = str(tmp_path / "again.gguf")
    w.write(path)
    _, t2 = gguf.Parser().Read(path)
    assert t2["again"].shape == shape and t2["again"].ggml_type == Q8_0
    np.testing.assert_array_equal(t2["again"].data, raw)


@pytest.mark.parametrize("shape", [(1, 32), (16, 32), (15, 256), (16, 288)])
def test_gguf_rejects_q8_0_outside_the_shape_rules(tmp_path, shape):
    raw = q8_bytes(*shape, seed=3)
    with pytest.raises(ValueError, match="Unsupported data type Q8_0.*rows % 16 == 0"):
        gguf.Parser().Read(write_one(tmp_path, "w", raw, shape))


@pytest.fixture(scope="module")
def lib():
    from nfai_amd import build as hb, _lib
    hb.build()
    return _lib.load()


def test_weight_bytes_q8_0_through_the_c_abi(lib):
    from nfai_amd import _lib
    assert _lib.Q8_0 == 8
    n = ctypes.c_uint64()
    _lib.call("nfai_hip_weight_bytes", _lib.Q8_0, 16, 256, ctypes.byref(n))
    assert n.value == 16 * 8 * 34
    _lib.call("nfai_hip_weight_bytes", _lib.Q8_0, 128256, 2048, ctypes.byref(n))
    assert n.value == 128256 * 2048 // 32 * 34
    for rows, cols in ((15, 256), (16, 288), (16, 32), (16, 32768 + 256)):
        with pytest.raises(_lib.NfaiHipError) as e:
            _lib.call("nfai_hip_weight_bytes", _lib.Q8_0, rows, cols, ctypes.byref(n))
        assert e.value.code == _lib.ERR_UNSUPPORTED and "Q8_0 needs rows % 16 == 0" in str(e.value)


def block(d16, codes):
    return np.float16(d16).tobytes() + np.asarray(codes, np.int8).tobytes()


def test_quantize_q8_0_known_answers():
    # d = 0.5: a row whose amax is 63.5 = 127 * 0.5 and whose values are exact multiples of 0.5
    codes = np.arange(-127, 128, dtype=np.int32)  # 255 codes ... padded to 256 with a 0
    codes = np.concatenate([codes, [0]]).reshape(8, 32)
    codes[:, 0] = 127  # every block reaches amax = 63.5 so that d = 0.5 in each
    x = (codes.astype(np.float32) * 0.5).reshape(1, 256)
    raw = synth.quantize_q8_0(x)
    assert raw == b"".join(block(0.5, c) for c in codes)
    np.testing.assert_array_equal(dequant_q8_0(raw, 1, 256), x)
    # code -128 does not come out of the quantiser (|q| <= 127), but the decoder takes it: d * -128
    assert dequant_q8_0(block(0.5, [-128] + [0] * 31), 1, 32)[0, 0] == -64.0
    # an all-zero row: d = 0, every code 0
    raw = synth.quantize_q8_0(np.zeros((1, 64), np.float32))
    assert raw == block(0.0, [0] * 32) * 2
    assert not dequant_q8_0(raw, 1, 64).any()
    # amax = 1.0: d = 1/127 = 0.007874016 in fp32 -> fp16 0.007873535 (rounded); the codes are rounded with the fp32 d
    x = np.zeros((1, 32), np.float32)
    x[0, :4] = [1.0, -0.5, 0.25, 0.003937008]  # the last is just over half a step: rounds up to 1
    raw = synth.quantize_q8_0(x)
    d = np.float32(1.0) / np.float32(127)
    assert np.frombuffer(raw[:2], np.float16)[0] == np.float16(d) and np.float16(d) != d
    q = np.frombuffer(raw[2:], np.int8)
    assert list(q[:4]) == [127, -64, 32, 1] and not q[4:].any()
    np.testing.assert_array_equal(dequant_q8_0(raw, 1, 32)[0, :4], np.float32(np.float16(d)) * np.float32([127, -64, 32, 1]))


def test_csharp_ggml_type_matches_the_header():
    cs = open(os.path.join(ROOT, "csharp", "NFAI.HIP", "Native.cs")).read()
    assert re.search(r"enum GgmlType\s*\{[^}]*\bQ8_0 = 8\b", cs)
    h = open(os.path.join(ROOT, "include", "nfai_hip.h")).read()
    assert re.search(r"enum nfai_dtype\s*\{[^}]*\bNFAI_Q8_0 = 8\b", h)


def test_pipeline_costs_q8_0_is_8_5_bits_per_weight():
    from nfai_amd.pipeline import pipeline_costs
    dims = synth.LLAMA_32_1B
    E, F, KD, V = dims.E, dims.F, dims.Hkv * dims.D, dims.V
    per_block = (E * dims.H * dims.D + 2 * E * KD + dims.H * dims.D * E + 3 * E * F) * 34 / 32
    blk, head = pipeline_costs(dims, "q8_0")
    assert blk == pytest.approx(per_block, rel=1e-12)
    assert head == pytest.approx(V * E * 34 / 32, rel=1e-12)
