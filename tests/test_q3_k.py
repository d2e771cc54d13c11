"""Q3_K weights on CPU: the GGUF reader / writer, the C ABI's byte count, the synthetic quantiser and dequantiser, the file mixes and
the pipeline cost model.

The reference throws for every quantised type (NFAI.GGUF/Parser.cs:111-114), so parity is UNPINNED by it.  The format is ggml's
block_q3_K restated from memory (no ggml source was at hand): 110 bytes per 256 weights in the order hmask[32], qs[64], scales[12],
fp16 d; element k = 128 n + 32 j + 16 lh + l has low bits (qs[32 n + 16 lh + l] >> 2 j) & 3, high bit (hmask[16 lh + l] >> (4 n + j)) & 1
and 6-bit scale index 8 n + 2 j + lh; weight = (d * (scale - 32)) * (low + 4 high - 4).  `scalar_dequant` below is that loop written
out; check the restatement against a real Q3_K file when one is at hand."""
import ctypes
import os
import re

import numpy as np
import pytest

from nfai_amd import gguf, synth
from nfai_amd.llama_model import QuantTensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q3_K, Q4_K, Q5_K, Q6_K = 11, 12, 13, 14
BAD_SHAPES = [(1, 256), (15, 256), (16, 32), (16, 288), (16, 512 + 256 * 127)]


def scale_of(scales, i):
    lo = (scales[i] & 0xF) if i < 8 else (scales[i - 8] >> 4)
    hi = (scales[8 + i % 4] >> (2 * (i // 4))) & 3
    return int(lo) | (int(hi) << 4)


def scalar_dequant(blk):
    """One 110-byte block -> 256 float32, element by element as the module docstring states it."""
    blk = np.frombuffer(bytes(blk), np.uint8)
    hmask, qs, scales = blk[0:32], blk[32:96], blk[96:108]
    d = np.float32(blk[108:110].copy().view(np.float16)[0])
    y = np.zeros(256, np.float32)
    for n in range(2):
        for j in range(4):
            for lh in range(2):
                for l in range(16):
                    lo = (int(qs[32 * n + 16 * lh + l]) >> (2 * j)) & 3
                    hb = (int(hmask[16 * lh + l]) >> (4 * n + j)) & 1
                    dl = np.float32(d * np.float32(scale_of(scales, 8 * n + 2 * j + lh) - 32))
                    y[128 * n + 32 * j + 16 * lh + l] = np.float32(dl * np.float32(lo + 4 * hb - 4))
    return y


def pack_scales(sc):
    """Sixteen 6-bit scales -> the 12 scale bytes."""
    out = np.zeros(12, np.uint8)
    for i, v in enumerate(sc):
        assert 0 <= v <= 63
        if i < 8:
            out[i] |= v & 0xF
        else:
            out[i - 8] |= (v & 0xF) << 4
        out[8 + i % 4] |= (v >> 4) << (2 * (i // 4))
    return out


def write_one(tmp_path, name, raw, shape, ty=Q3_K):
    w = gguf.GGUFWriter()
    w.add("general.architecture", "llama")
    w.add_tensor(name, QuantTensor(raw, ty, shape))
    path = str(tmp_path / f"{name}.gguf")
    w.write(path)
    return path


@pytest.mark.parametrize("shape", [(16, 256), (32, 512)])
def test_gguf_reads_q3_k_as_quant_tensor_and_round_trips(tmp_path, shape):
    raw = np.frombuffer(synth.quantize_q3_k(np.random.default_rng(shape[0]).standard_normal(shape).astype(np.float32)), np.uint8).copy()
    assert raw.size == shape[0] * shape[1] // 256 * 110
    _, t = gguf.Parser().Read(write_one(tmp_path, "w", raw, shape))
    qt = t["w"]
    assert isinstance(qt, QuantTensor) and qt.ggml_type == Q3_K and qt.shape == shape
    np.testing.assert_array_equal(qt.data, raw)
    w = gguf.GGUFWriter()
    w.add_tensor("again", qt)
    path = str(tmp_path / "again.gguf")
    w.write(path)
    _, t2 = gguf.Parser().Read(path)
    assert t2["again"].shape == shape and t2["again"].ggml_type == Q3_K
    np.testing.assert_array_equal(t2["again"].data, raw)


@pytest.mark.parametrize("shape", BAD_SHAPES)
def test_gguf_rejects_q3_k_outside_the_shape_rules(tmp_path, shape):
    rows, cols = shape
    assert rows * cols % 256 == 0   # whole blocks: the refusal is about the shape, not the byte count
    raw = np.zeros(rows * cols // 256 * 110, np.uint8)
    with pytest.raises(ValueError, match=r"Unsupported data type Q3_K.*" + re.escape(gguf.Q3_K_RULE)):
        gguf.Parser().Read(write_one(tmp_path, "w", raw, shape))
    assert "rows % 16 == 0" in gguf.Q3_K_RULE and "cols % 256 == 0" in gguf.Q3_K_RULE and "cols <= 32768" in gguf.Q3_K_RULE


def test_gguf_still_refuses_q5_1(tmp_path):
    with pytest.raises(ValueError, match="Unsupported data type Q5_1"):
        gguf.Parser().Read(write_one(tmp_path, "w", np.zeros(16 * 8 * 24, np.uint8), (16, 256), ty=7))


@pytest.fixture(scope="module")
def lib():
    from nfai_amd import build as hb, _lib
    hb.build()
    return _lib.load()


def test_weight_bytes_q3_k_through_the_c_abi(lib):
    from nfai_amd import _lib
    assert _lib.Q3_K == 11
    n = ctypes.c_uint64()
    _lib.call("nfai_hip_weight_bytes", _lib.Q3_K, 16, 256, ctypes.byref(n))
    assert n.value == 1760
    _lib.call("nfai_hip_weight_bytes", _lib.Q3_K, 128256, 3072, ctypes.byref(n))
    assert n.value == 128256 * 12 * 110
    for rows, cols in BAD_SHAPES:
        with pytest.raises(_lib.NfaiHipError) as e:
            _lib.call("nfai_hip_weight_bytes", _lib.Q3_K, rows, cols, ctypes.byref(n))
        assert e.value.code == _lib.ERR_UNSUPPORTED
        assert "Q3_K needs rows % 16 == 0, cols % 256 == 0 and cols <= 32768" in str(e.value)
    with pytest.raises(_lib.NfaiHipError) as e:   # Q5_1 stays without a kernel
        _lib.call("nfai_hip_weight_bytes", 7, 16, 256, ctypes.byref(n))
    assert e.value.code == _lib.ERR_UNSUPPORTED


def test_q3_k_type_ids_in_the_header_csharp_lib_and_gguf():
    from nfai_amd import _lib
    cs = open(os.path.join(ROOT, "csharp", "NFAI.HIP", "Native.cs")).read()
    assert re.search(r"enum GgmlType\s*\{[^}]*\bQ3_K = 11\b", cs)
    h = open(os.path.join(ROOT, "include", "nfai_hip.h")).read()
    assert re.search(r"enum nfai_dtype\s*\{[^}]*\bNFAI_Q3_K = 11\b", h)
    assert _lib.Q3_K == 11 and gguf.GGML_Q3_K == 11 and gguf.GGML_BLOCK[11] == (256, 110)


# sixteen distinct scales: 0 (-> -32), 32 (-> 0) and 63 (-> +31) among them; indices below and above 8 take the low and the high
# nibble of scales[0..8); the high two bits take the shifts 0, 2, 4, 6 of scales[8..12) with values 0..3 at every shift
HAND_SCALES = [0, 17, 32, 63, 5, 22, 41, 58, 9, 26, 47, 48, 15, 16, 35, 60]


def hand_block():
    assert len(set(HAND_SCALES)) == 16 and {0, 32, 63} <= set(HAND_SCALES)
    for grp in range(4):   # every value of the high two bits at every shift
        assert sorted(v >> 4 for v in HAND_SCALES[4 * grp:4 * grp + 4]) == [0, 1, 2, 3]
    blk = np.zeros(110, np.uint8)
    blk[0:32] = [1 << ((3 * i + 1) % 8) for i in range(32)]          # hmask: one bit per byte, its place varying
    blk[32:96] = [(37 * i + 11) % 256 for i in range(64)]            # qs: a counting pattern (stride 37: every 2-bit field varies)
    blk[96:108] = pack_scales(HAND_SCALES)
    blk[108:110] = np.frombuffer(np.float16(0.5).tobytes(), np.uint8)
    return blk


def test_dequantize_q3_k_known_answers():
    blk = hand_block()
    assert [scale_of(blk[96:108], i) for i in range(16)] == HAND_SCALES
    want = scalar_dequant(blk)
    got = synth.dequantize_q3_k(blk.tobytes(), 1, 256)
    assert got.dtype == np.float32 and got.shape == (1, 256)
    np.testing.assert_array_equal(got[0], want)
    # every field matters: the values written out for a few elements by hand
    # k = 0: n = 0, j = 0, lh = 0, l = 0: low = 11 & 3 = 3, hmask[0] = 1 << 1 -> bit 0 clear, scale[0] = 0 -> 0.5 * -32 * (3 - 4) = 16
    assert got[0, 0] == 16.0
    # k = 32 + 1 (j = 1, l = 1): qs[1] = 48 -> (48 >> 2) & 3 = 0; hmask[1] = 1 << 4: bit 1 clear; scale[2] = 32 -> weight 0
    assert got[0, 33] == 0.0
    # k = 96 + 16 + 2 (n = 0, j = 3, lh = 1, l = 2): qs[18] = (37 * 18 + 11) % 256 = 165 -> (165 >> 6) & 3 = 2; hmask[18] = 1 << 7:
    # bit 3 clear; scale[2 * 3 + 1] = 58 -> 0.5 * 26 * (2 - 4) = -26
    assert got[0, 114] == -26.0
    # k = 128 + 0 + 16 + 1 (n = 1, j = 0, lh = 1, l = 1): qs[32 + 16 + 1] = (37 * 49 + 11) % 256 = 32 -> 0; hmask[17] = 1 << 4: bit
    # 4 n + j = 4 SET -> q = 4 - 4 = 0
    assert got[0, 145] == 0.0
    # the scales reach every group: group g = 8 n + 2 j + lh covers k = 128 n + 32 j + 16 lh .. + 16
    for g in range(16):
        n, j, lh = g >> 3, (g >> 1) & 3, g & 1
        seg = got[0, 128 * n + 32 * j + 16 * lh:][:16]
        assert (np.abs(seg) <= 0.5 * abs(HAND_SCALES[g] - 32) * 4).all() and (seg / 0.5 % 1 == 0).all()
        if HAND_SCALES[g] == 32:
            assert not seg.any()
    # flipping one hmask bit moves exactly one weight, by 4 steps of its group
    b2 = blk.copy()
    b2[5] ^= 1 << 6   # hmask[5] bit 6: n = 1, j = 2, lh = 0, l = 5 -> k = 128 + 64 + 5
    diff = synth.dequantize_q3_k(b2.tobytes(), 1, 256)[0] - got[0]
    assert np.flatnonzero(diff).tolist() == [197] and abs(diff[197]) == 0.5 * abs(HAND_SCALES[8 + 4] - 32) * 4
    # several blocks and rows, random bytes: the vectorised dequantiser against the scalar loop
    rng = np.random.default_rng(3)
    b = rng.integers(0, 256, (6, 110), dtype=np.uint8)
    b[:, 108:110] = (0.01 * rng.standard_normal(6)).astype(np.float16).view(np.uint8).reshape(-1, 2)
    got = synth.dequantize_q3_k(b.tobytes(), 2, 768)
    np.testing.assert_array_equal(got, np.stack([scalar_dequant(x) for x in b]).reshape(2, 768))


def _fields(raw):
    b = np.frombuffer(bytes(raw), np.uint8).reshape(-1, 110)
    sc = np.array([[scale_of(x[96:108], i) for i in range(16)] for x in b])
    d = b[:, 108:110].copy().view(np.float16).astype(np.float32)[:, 0]
    codes = np.zeros((b.shape[0], 256), np.int32)
    for n in range(2):
        for j in range(4):
            lo = (b[:, 32 + 32 * n:64 + 32 * n] >> (2 * j)) & 3
            hb = (b[:, 0:32] >> (4 * n + j)) & 1
            codes[:, 128 * n + 32 * j:128 * n + 32 * j + 32] = lo + 4 * hb
    return d, sc, codes


def test_quantize_q3_k_round_trip_bound_codes_and_fixed_point():
    rng = np.random.default_rng(7)
    rows, cols = 16, 1024
    W = (0.02 * rng.standard_normal((rows, cols))).astype(np.float32)
    W[3, 256:512] = 0                          # an all-zero block inside a row
    W[5, :16] *= 40                            # one loud group: its neighbours get small scales
    raw = synth.quantize_q3_k(W)
    assert len(raw) == rows * cols // 256 * 110
    d, sc, codes = _fields(raw)
    assert codes.min() >= 0 and codes.max() <= 7 and set(np.unique(codes)) == set(range(8))
    assert sc.min() >= 0 and sc.max() <= 63
    y = synth.dequantize_q3_k(raw, rows, cols)
    # every weight within one step |d (sc - 32)| of its group (the quantiser's docstring says why one step and not half of one)
    step = np.abs(d[:, None] * (sc - 32).astype(np.float32))                                    # [nb][16], group 8 n + 2 j + lh
    err = np.abs(y - W).reshape(-1, 2, 4, 2, 16)                                                 # [nb][n][j][lh][l]
    assert (err <= step.reshape(-1, 2, 4, 2)[..., None]).all(), float((err - step.reshape(-1, 2, 4, 2)[..., None]).max())
    blk0 = (3 * (cols // 256) + 1)
    assert d[blk0] == 0 and not y[3, 256:512].any()
    # an all-zero tensor
    z = synth.quantize_q3_k(np.zeros((16, 256), np.float32))
    assert not synth.dequantize_q3_k(z, 16, 256).any()
    assert all(np.frombuffer(z, np.uint8).reshape(-1, 110)[:, 108:110].view(np.float16)[:, 0] == 0)
    # a fixed point on its own output (wherever every group has its extreme on code 0: checked, so that the claim is not empty)
    V = (0.02 * rng.standard_normal((rows, cols))).astype(np.float32)
    rawv = synth.quantize_q3_k(V)
    _, scv, cv = _fields(rawv)
    assert (cv.reshape(-1, 2, 4, 2, 16).min(axis=4) == 0).all() and np.abs(scv - 32).min() >= 8
    yv = synth.dequantize_q3_k(rawv, rows, cols)
    again = synth.quantize_q3_k(yv)
    np.testing.assert_array_equal(synth.dequantize_q3_k(again, rows, cols), yv)
    # rows are independent and row-major
    assert raw[:cols // 256 * 110] == synth.quantize_q3_k(W[:1])


def table(dims, mix):
    return {name: synth.q3_k_type(name, dims, mix) for name, shape in dims.shapes().items() if len(shape) == 2}


@pytest.mark.parametrize("dims", [synth.TINY_D128, synth.LLAMA_32_3B], ids=lambda d: d.name)
def test_q3_k_type_tensor_by_tensor(dims):
    first_q5_down = dims.L // 16                 # TINY_D128: 0 blocks, LLAMA_32_3B (28 blocks): 1
    assert first_q5_down == (1 if dims is synth.LLAMA_32_3B else 0)
    m, s, a = table(dims, "q3_k_m"), table(dims, "q3_k_s"), table(dims, "all_q3_k")
    assert set(m) == set(s) == set(a) == {k for k, v in dims.shapes().items() if len(v) == 2}
    assert set(a.values()) == {Q3_K}
    head = "token_embd.weight" if dims.tied else "output.weight"
    for name in m:
        if name == head:
            assert m[name] == s[name] == Q6_K
            continue
        assert s[name] == Q3_K
        if name == "token_embd.weight":
            assert m[name] == Q3_K               # untied: the table is Q3_K
            continue
        layer, kind = int(name.split(".")[1]), name.split(".")[2]
        want = {"attn_q": Q3_K, "attn_k": Q3_K, "ffn_gate": Q3_K, "ffn_up": Q3_K, "attn_output": Q4_K,
                "attn_v": Q5_K if layer < 2 else Q4_K, "ffn_down": Q5_K if layer < first_q5_down else Q4_K}[kind]
        assert m[name] == want, name
    # a pipeline stage numbers its blocks within the file
    assert synth.q3_k_type("blk.0.attn_v.weight", dims, "q3_k_m", layer_offset=2, n_layers_file=dims.L) == Q4_K
    assert synth.q3_k_type("blk.0.ffn_down.weight", synth.TINY_D128, "q3_k_m", layer_offset=0, n_layers_file=32) == Q5_K
    assert synth.q3_k_type("blk.2.ffn_down.weight", synth.TINY_D128, "q3_k_m", layer_offset=0, n_layers_file=32) == Q4_K
    with pytest.raises(ValueError):
        synth.q3_k_type("output.weight", dims, "q3_k_l")


@pytest.mark.parametrize("dims", [synth.LLAMA_32_1B, synth.LLAMA_32_3B, synth.LLAMA_31_8B, synth.TINY_D128], ids=lambda d: d.name)
def test_pipeline_costs_q3_k_m_is_the_sum_over_the_type_table(dims):
    from nfai_amd.pipeline import pipeline_costs
    blocks = 0
    for name, shape in dims.shapes().items():
        if name.startswith("blk.") and len(shape) == 2:
            be, bb = gguf.GGML_BLOCK[synth.q3_k_type(name, dims, "q3_k_m")]
            blocks += shape[0] * shape[1] // be * bb
    blk, head = pipeline_costs(dims, "q3_k_m")
    assert blk == pytest.approx(blocks / dims.L, rel=1e-12)
    assert head == pytest.approx(dims.V * dims.E * 210 / 256, rel=1e-12)   # output.weight or the tied token_embd: Q6_K


def test_python_host_picks_any_quant_for_q3_k():
    from nfai_amd import _lib
    from nfai_amd.llama_model import LlamaModel
    calls = []

    class Probe(LlamaModel):   # SetTensor's bookkeeping without a library behind it
        def __init__(self):
            self.handle, self._quantized, self._any_quant = None, False, False

    import nfai_amd.llama_model as lm
    saved = lm.call
    lm.call = lambda *a: calls.append(a)
    try:
        p = Probe()
        p.SetTensor("blk.0.attn_q.weight", QuantTensor(np.zeros(16 * 110, np.uint8), Q3_K, (16, 256)))
        assert p._quantized and p._any_quant
        assert calls[-1][0] == "nfai_hip_llama_set_tensor" and calls[-1][3:6] == (Q3_K, 16, 256)
        p = Probe()
        p.SetTensor("blk.0.attn_q.weight", (0x1000, _lib.Q3_K, 16, 256))
        assert p._quantized and p._any_quant
    finally:
        lm.call = saved
