"""Q5_K weights on CPU: the NumPy restatement of ggml's dequantize_row_q5_K, the synthetic quantiser, the GGUF reader / writer, the
C ABI's byte count, the header / C# type ids and the pipeline cost model.

No ggml or `gguf` package is installed here, so the restatement below is the pin: it is parity against ggml's published block
definition (block_q5_K: fp16 d, fp16 dmin, u8 scales[12], u8 qh[32], u8 qs[128]; 176 bytes per 256 weights) and its
dequantize_row_q5_K, not against the reference, which has no Q5_K path at all (Parser.cs:111-114 throws "Unsupported data type").
Every Q5_K value in this file is decoded by that restatement, not by anything in nfai_amd."""
import ctypes
import os
import re

import numpy as np
import pytest

from nfai_amd import gguf, synth
from nfai_amd.llama_model import QuantTensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q5_K = 13


def scale_min_k4(j, s):
    """ggml get_scale_min_k4(j, scales): (sc, m) of sub-block j."""
    if j < 4:
        return s[j] & 63, s[j + 4] & 63
    return (s[j + 4] & 0xF) | ((s[j - 4] >> 6) << 4), (s[j + 4] >> 4) | ((s[j] >> 6) << 4)


def dequant_q5_k(raw, rows, cols):
    """ggml dequantize_row_q5_K, block by block: for pair n = 0..3 (u1 = 1 << 2n, u2 = 2 << 2n) and l = 0..31
         y[64n + l]      = d * sc[2n]   * ((qs[32n + l] & 0xF) + (16 if qh[l] & u1 else 0)) - dmin * m[2n]
         y[64n + 32 + l] = d * sc[2n+1] * ((qs[32n + l] >> 4)  + (16 if qh[l] & u2 else 0)) - dmin * m[2n+1]"""
    b = np.frombuffer(bytes(raw), np.uint8).reshape(rows * cols // 256, 176)
    y = np.empty((b.shape[0], 256), np.float32)
    for i, blk in enumerate(b):
        d = np.float32(blk[0:2].view(np.float16)[0])
        dmin = np.float32(blk[2:4].view(np.float16)[0])
        scales, qh, qs = blk[4:16], blk[16:48], blk[48:176]
        for n in range(4):
            u1, u2 = 1 << (2 * n), 2 << (2 * n)
            sc1, m1 = scale_min_k4(2 * n, scales)
            sc2, m2 = scale_min_k4(2 * n + 1, scales)
            d1, mm1 = d * np.float32(sc1), dmin * np.float32(m1)
            d2, mm2 = d * np.float32(sc2), dmin * np.float32(m2)
            for l in range(32):
                q = qs[32 * n + l]
                y[i, 64 * n + l] = d1 * np.float32((q & 0xF) + (16 if qh[l] & u1 else 0)) - mm1
                y[i, 64 * n + 32 + l] = d2 * np.float32((q >> 4) + (16 if qh[l] & u2 else 0)) - mm2
    return y.reshape(rows, cols)


def make_block(d, dmin, sc, m, q):
    """One block_q5_K from its fields: sc, m = eight 6-bit values each, q = 256 codes 0..31 in weight order."""
    s = np.zeros(12, np.uint8)
    for j in range(8):
        if j < 4:
            s[j] |= sc[j]
            s[j + 4] |= m[j]
        else:
            s[j + 4] |= (sc[j] & 0xF) | ((m[j] & 0xF) << 4)
            s[j - 4] |= (sc[j] >> 4) << 6
            s[j] |= (m[j] >> 4) << 6
    q = np.asarray(q, np.int64).reshape(8, 32)
    qh = np.zeros(32, np.uint8)
    qs = np.zeros(128, np.uint8)
    for n in range(4):
        qs[32 * n:32 * n + 32] = (q[2 * n] & 0xF) | ((q[2 * n + 1] & 0xF) << 4)
        qh |= (((q[2 * n] >> 4) & 1) << (2 * n)).astype(np.uint8) | (((q[2 * n + 1] >> 4) & 1) << (2 * n + 1)).astype(np.uint8)
    return np.float16(d).tobytes() + np.float16(dmin).tobytes() + s.tobytes() + qh.tobytes() + qs.tobytes()


def raw_block(d, dmin, scales, qh, qs):
    return np.float16(d).tobytes() + np.float16(dmin).tobytes() + bytes(scales) + bytes(qh) + bytes(qs)


def test_single_qh_bit_moves_exactly_one_weight():
    scales = [1] * 4 + [0] * 4 + [0x01] * 4  # sc = 1, m = 0 for all eight sub-blocks
    assert all(scale_min_k4(j, scales) == (1, 0) for j in range(8))
    qs = bytes(range(128))
    base = dequant_q5_k(raw_block(0.5, 0.25, scales, bytes(32), qs), 1, 256)[0]
    for n in range(4):
        for l in (0, 5, 17, 31):
            for hi in (0, 1):
                qh = bytearray(32)
                qh[l] = 1 << (2 * n + hi)
                y = dequant_q5_k(raw_block(0.5, 0.25, scales, qh, qs), 1, 256)[0]
                moved = np.nonzero(y != base)[0]
                assert list(moved) == [64 * n + 32 * hi + l], (n, l, hi, moved)
                assert y[moved[0]] - base[moved[0]] == 16 * 0.5 * 1  # 16 * d * sc


def test_scales_and_mins_below_and_above_four():
    sc = [1, 2, 3, 4, 17, 33, 47, 63]
    m = [5, 6, 7, 8, 20, 40, 55, 62]
    q = np.zeros(256, np.int64)
    raw = make_block(1.0, 1.0, sc, m, q)
    s = np.frombuffer(raw[4:16], np.uint8)
    assert [scale_min_k4(j, s) for j in range(8)] == list(zip(sc, m))
    y = dequant_q5_k(raw, 1, 256)[0].reshape(8, 32)
    np.testing.assert_array_equal(y, -np.float32(m)[:, None] * np.ones((1, 32), np.float32))  # q = 0: only -dmin * m
    q = np.full(256, 31)
    y = dequant_q5_k(make_block(1.0, 0.0, sc, m, q), 1, 256)[0].reshape(8, 32)
    np.testing.assert_array_equal(y[:, 0], 31 * np.float32(sc))


def test_d_and_dmin_are_fp16():
    d = 0.1  # not an fp16 value: the block stores 0.0999755859375
    raw = make_block(d, d, [1] * 8, [1] * 8, np.full(256, 3))
    assert np.frombuffer(raw[:2], np.float16)[0] == np.float16(d) and float(np.float16(d)) != d
    y = dequant_q5_k(raw, 1, 256)[0]
    d16 = np.float32(np.float16(d))
    np.testing.assert_array_equal(y, np.full(256, d16 * np.float32(3) - d16, np.float32))


def test_quantize_q5_k_round_trip():
    rng = np.random.default_rng(5)
    W = (0.02 * rng.standard_normal((32, 512))).astype(np.float32)
    W[0, :32] = 0.0                  # an all-zero sub-block
    W[1, :256] = np.abs(W[1, :256])  # a super-block without negative values (m = 0)
    W[2, 256:] = -np.abs(W[2, 256:]) # ... and one without positive values
    raw = synth.quantize_q5_k(W)
    assert len(raw) == 32 * 512 // 256 * 176
    b = np.frombuffer(raw, np.uint8).reshape(-1, 176)
    y = dequant_q5_k(raw, 32, 512)
    # codes: every one 0..31 (five bits), and the whole range is used
    codes = []
    for blk in b:
        qh, qs = blk[16:48], blk[48:176]
        for n in range(4):
            codes.append((qs[32 * n:32 * n + 32] & 0xF) | (((qh >> (2 * n)) & 1) << 4))
            codes.append((qs[32 * n:32 * n + 32] >> 4) | (((qh >> (2 * n + 1)) & 1) << 4))
    codes = np.concatenate(codes)
    assert codes.min() == 0 and codes.max() == 31
    # error: at most half a step d * sc of the sub-block (d, dmin are the stored fp16 values; fp32 arithmetic adds a few ulp)
    d = b[:, 0:2].copy().view(np.float16).astype(np.float32)[:, 0]
    step = np.array([[d[i] * np.float32(scale_min_k4(j, b[i, 4:16])[0]) for j in range(8)] for i in range(b.shape[0])])
    step = np.repeat(step.reshape(32, 2, 8), 32, axis=2).reshape(32, 512)
    err = np.abs(y - W)
    assert (err <= 0.5 * step + 1e-6 * (np.abs(W) + 0.02)).all(), float((err - 0.5 * step).max())
    np.testing.assert_array_equal(y[0, :32], 0.0)


def q5_bytes(rows, cols, seed):
    rng = np.random.default_rng(seed)
    return np.frombuffer(synth.quantize_q5_k(0.02 * rng.standard_normal((rows, cols)).astype(np.float32)), np.uint8).copy()


def write_one(tmp_path, name, raw, shape):
    w = gguf.GGUFWriter()
    w.add("general.architecture", "llama")
    w.add_tensor(name, QuantTensor(raw, Q5_K, shape))
    path = str(tmp_path / f"{name}.gguf")
    w.write(path)
    return path


@pytest.mark.parametrize("shape", [(16, 256), (32, 512)])
def test_gguf_reads_q5_k_as_quant_tensor_and_round_trips(tmp_path, shape):
    raw = q5_bytes(*shape, seed=shape[0])
    assert raw.size == shape[0] * shape[1] // 256 * 176
    _, t = gguf.Parser().Read(write_one(tmp_path, "w", raw, shape))
    qt = t["w"]
    assert isinstance(qt, QuantTensor) and qt.ggml_type == Q5_K and qt.shape == shape
    np.testing.assert_array_equal(qt.data, raw)
    w = gguf.GGUFWriter()
    w.add_tensor("again", qt)
    path = str(tmp_path / "again.gguf")
    w.write(path)
    _, t2 = gguf.Parser().Read(path)
    assert t2["again"].shape == shape and t2["again"].ggml_type == Q5_K
    np.testing.assert_array_equal(t2["again"].data, raw)


@pytest.mark.parametrize("shape", [(15, 256), (16, 512 + 256 * 127), (1, 256)])
def test_gguf_rejects_q5_k_outside_the_shape_rules(tmp_path, shape):
    raw = q5_bytes(*shape, seed=3)
    with pytest.raises(ValueError, match=r"Unsupported data type Q5_K.*" + re.escape(gguf.Q5_K_RULE)):
        gguf.Parser().Read(write_one(tmp_path, "w", raw, shape))


@pytest.fixture(scope="module")
def lib():
    from nfai_amd import build as hb, _lib
    hb.build()
    return _lib.load()


def test_weight_bytes_q5_k_through_the_c_abi(lib):
    from nfai_amd import _lib
    assert _lib.Q5_K == 13
    n = ctypes.c_uint64()
    _lib.call("nfai_hip_weight_bytes", _lib.Q5_K, 16, 256, ctypes.byref(n))
    assert n.value == 16 * 176
    for rows, cols in ((128256, 3072), (14336, 4096), (4096, 14336)):
        _lib.call("nfai_hip_weight_bytes", _lib.Q5_K, rows, cols, ctypes.byref(n))
        assert n.value == rows * cols // 256 * 176
    for rows, cols in ((15, 256), (16, 288), (16, 32), (16, 32768 + 256)):
        with pytest.raises(_lib.NfaiHipError) as e:
            _lib.call("nfai_hip_weight_bytes", _lib.Q5_K, rows, cols, ctypes.byref(n))
        assert e.value.code == _lib.ERR_UNSUPPORTED and "Q5_K needs rows % 16 == 0" in str(e.value)


def test_q5_k_type_ids_in_the_header_and_csharp():
    cs = open(os.path.join(ROOT, "csharp", "NFAI.HIP", "Native.cs")).read()
    assert re.search(r"enum GgmlType\s*\{[^}]*\bQ5_K = 13\b", cs)
    h = open(os.path.join(ROOT, "include", "nfai_hip.h")).read()
    assert re.search(r"enum nfai_dtype\s*\{[^}]*\bNFAI_Q5_K = 13\b", h)
    assert gguf.GGML_Q5_K == 13 and gguf.GGML_BLOCK[13] == (256, 176)


@pytest.mark.parametrize("dims", [synth.LLAMA_32_1B, synth.LLAMA_32_3B, synth.LLAMA_31_8B])
def test_pipeline_costs_q5_k_m_against_a_hand_sum(dims):
    from nfai_amd.pipeline import pipeline_costs
    E, F, HD, KD, V, L = dims.E, dims.F, dims.H * dims.D, dims.Hkv * dims.D, dims.V, dims.L
    q5, q6 = 176 / 256, 210 / 256

    def more(i):  # llama.cpp's use_more_bits, written out
        return i < L // 8 or i >= 7 * L // 8 or (i - L // 8) % 3 == 2

    tot = 0.0
    for i in range(L):
        tot += (HD * E + KD * E + HD * E + 2 * F * E) * q5            # q, k, o, gate, up
        tot += (KD * E + E * F) * (q6 if more(i) else q5)              # v, down
    blk, head = pipeline_costs(dims, "q5_k_m")
    assert blk == pytest.approx(tot / L, rel=1e-12)
    assert head == pytest.approx(V * E * q6, rel=1e-12)                # output.weight or the tied token_embd: Q6_K
    assert synth.q5_k_m_type("token_embd.weight", dims) == (14 if dims.tied else 13)
