"""IQ4_XS weights on CPU: the GGUF reader / writer, the C ABI's byte count, the synthetic quantiser and dequantiser, the file mixes
and the pipeline cost model.

The reference names the type (NFAI.GGUF/Parser.cs:285) and throws for every quantised type (Parser.cs:111-114), so parity is
UNPINNED by it.  The format is ggml's block_iq4_xs restated from memory (no ggml source was at hand): 136 bytes per 256 weights in
the order fp16 d, uint16 scales_h, scales_l[4], qs[128]; sub-block ib of 32 weights has the 6-bit scale
ls = ((scales_l[ib / 2] >> 4 (ib % 2)) & 0xF) | (((scales_h >> 2 ib) & 3) << 4) and dl = d * (ls - 32); weight 32 ib + j =
dl * KV[qs[16 ib + j] & 0xF], weight 32 ib + 16 + j = dl * KV[qs[16 ib + j] >> 4].  `scalar_dequant` below is that loop written
out; check the restatement against a real IQ4_XS file when one is at hand."""
import ctypes
import os
import re

import numpy as np
import pytest

from nfai_amd import gguf, synth
from nfai_amd.llama_model import QuantTensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IQ4_XS, Q5_K, Q6_K = 23, 13, 14
KV = [-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113]
BAD_SHAPES = [(1, 256), (15, 256), (16, 32), (16, 288), (16, 512 + 256 * 127)]


def scale_of(blk, ib):
    scales_h = int(blk[2]) | (int(blk[3]) << 8)
    scales_l = blk[4:8]
    return ((int(scales_l[ib // 2]) >> (4 * (ib % 2))) & 0xF) | (((scales_h >> (2 * ib)) & 3) << 4)


def scalar_dequant(blk):
    """One 136-byte block -> 256 float32, element by element as the module docstring states it."""
    blk = np.frombuffer(bytes(blk), np.uint8)
    d = np.float32(blk[0:2].copy().view(np.float16)[0])
    qs = blk[8:136]
    y = np.zeros(256, np.float32)
    for ib in range(8):
        dl = np.float32(d * np.float32(scale_of(blk, ib) - 32))
        for j in range(16):
            y[32 * ib + j] = np.float32(dl * np.float32(KV[int(qs[16 * ib + j]) & 0xF]))
            y[32 * ib + 16 + j] = np.float32(dl * np.float32(KV[int(qs[16 * ib + j]) >> 4]))
    return y


def pack_block(d, ls, codes):
    """fp16 d, eight 6-bit scales, 256 codes (0..15, in weight order) -> one 136-byte block, field by field."""
    blk = np.zeros(136, np.uint8)
    blk[0:2] = np.frombuffer(np.float16(d).tobytes(), np.uint8)
    sh = 0
    for ib, v in enumerate(ls):
        assert 0 <= v <= 63
        sh |= (v >> 4) << (2 * ib)
        blk[4 + ib // 2] |= (v & 0xF) << (4 * (ib % 2))
    blk[2], blk[3] = sh & 0xFF, sh >> 8
    codes = np.asarray(codes, np.uint8).reshape(8, 32)
    assert codes.max() <= 15
    blk[8:136] = (codes[:, :16] | (codes[:, 16:] << 4)).reshape(128)
    return blk


def _fields(raw):
    b = np.frombuffer(bytes(raw), np.uint8).reshape(-1, 136)
    ls = np.array([[scale_of(x, ib) for ib in range(8)] for x in b])
    d = b[:, 0:2].copy().view(np.float16).astype(np.float32)[:, 0]
    qs = b[:, 8:136].reshape(-1, 8, 16)
    codes = np.concatenate([qs & 0xF, qs >> 4], axis=2).astype(np.int32)            # [nb][ib][32]
    return d, ls, codes


def write_one(tmp_path, name, raw, shape, ty=IQ4_XS):
    w = gguf.GGUFWriter()
    w.add("general.architecture", "llama")
    w.add_tensor(name, QuantTensor(raw, ty, shape))
    path = str(tmp_path / f"{name}.gguf")
    w.write(path)
    return path


def test_codebook_is_the_one_the_format_states():
    assert synth.IQ4_KV.dtype == np.int8 and synth.IQ4_KV.tolist() == KV


def test_dequantize_iq4_xs_against_the_scalar_loop():
    rng = np.random.default_rng(3)
    b = rng.integers(0, 256, (6, 136), dtype=np.uint8)
    b[:, 0:2] = (0.01 * rng.standard_normal(6)).astype(np.float16).view(np.uint8).reshape(-1, 2)
    got = synth.dequantize_iq4_xs(b.tobytes(), 2, 768)
    assert got.dtype == np.float32 and got.shape == (2, 768)
    np.testing.assert_array_equal(got, np.stack([scalar_dequant(x) for x in b]).reshape(2, 768))
    # a block whose 256 nibbles run through all 16 codes in every sub-block (sub-block ib starts at code ib: each code meets each nibble place)
    codes = np.array([[(ib + j) % 16 for j in range(32)] for ib in range(8)])
    ls = [0, 31, 32, 33, 63, 17, 40, 58]
    blk = pack_block(0.5, ls, codes)
    assert [scale_of(blk, ib) for ib in range(8)] == ls
    want = scalar_dequant(blk)
    got = synth.dequantize_iq4_xs(blk.tobytes(), 1, 256)[0]
    np.testing.assert_array_equal(got, want)
    for ib in range(8):
        for j in range(32):
            assert got[32 * ib + j] == 0.5 * (ls[ib] - 32) * KV[(ib + j) % 16], (ib, j)
        assert set(codes[ib]) == set(range(16))
    assert not got[64:96].any()                       # ls = 32: a zero scale
    # values written out by hand: sub-block 0 (ls 0 -> -32), weight 0 = code 0: 0.5 * -32 * -127; weight 16 (high nibble of qs[0]) = code 0
    assert got[0] == 2032.0 and got[16] == 0.5 * -32 * KV[0] and got[1] == 0.5 * -32 * -104
    # flipping one nibble moves exactly one weight: the high nibble of qs[16 * 5 + 3] is weight 32 * 5 + 16 + 3
    b2 = blk.copy()
    b2[8 + 16 * 5 + 3] ^= 0x10
    diff = synth.dequantize_iq4_xs(b2.tobytes(), 1, 256)[0] - got
    assert np.flatnonzero(diff).tolist() == [32 * 5 + 19]


@pytest.mark.parametrize("value", [0, 31, 32, 33, 63])
def test_packing_of_ls_at_its_edges(value):
    blk = pack_block(1.0, [value] * 8, np.full(256, 8))      # code 8 = +1: the weight is the scale itself
    assert [scale_of(blk, ib) for ib in range(8)] == [value] * 8
    y = synth.dequantize_iq4_xs(blk.tobytes(), 1, 256)[0]
    assert (y == value - 32).all()
    np.testing.assert_array_equal(synth._iq4_xs_scales(blk.reshape(1, 136))[0], [value] * 8)
    if value == 63:
        assert blk[2] == 0xFF and blk[3] == 0xFF and (blk[4:8] == 0xFF).all()
    if value == 32:
        assert blk[2] == 0xAA and blk[3] == 0xAA and not blk[4:8].any()


def test_packing_of_ls_eight_distinct_values_per_block():
    ls = [0, 63, 32, 17, 46, 5, 58, 27]                      # every value of the high two bits twice, at different shifts
    assert len(set(ls)) == 8 and sorted(v >> 4 for v in ls) == [0, 0, 1, 1, 2, 2, 3, 3]
    blk = pack_block(2.0, ls, np.full(256, 8))
    np.testing.assert_array_equal(synth._iq4_xs_scales(blk.reshape(1, 136))[0], ls)
    y = synth.dequantize_iq4_xs(blk.tobytes(), 1, 256)[0].reshape(8, 32)
    for ib in range(8):
        assert (y[ib] == 2.0 * (ls[ib] - 32)).all()
    # scales_h alone and scales_l alone
    only_h = blk.copy(); only_h[4:8] = 0
    only_l = blk.copy(); only_l[2:4] = 0
    assert [scale_of(only_h, ib) for ib in range(8)] == [v & 0x30 for v in ls]
    assert [scale_of(only_l, ib) for ib in range(8)] == [v & 0xF for v in ls]
    np.testing.assert_array_equal(synth.dequantize_iq4_xs(only_h.tobytes(), 1, 256)[0], scalar_dequant(only_h))
    np.testing.assert_array_equal(synth.dequantize_iq4_xs(only_l.tobytes(), 1, 256)[0], scalar_dequant(only_l))


def check_quantised(W, raw):
    """Valid blocks, and every weight within 14 steps |d (ls - 32)| of its value (the bound synth.quantize_iq4_xs derives from the
    table; compared in float64, with the rounding of the decoder's own product dl * KV, half an ulp of fp32, beside it)."""
    rows, cols = W.shape
    assert len(raw) == rows * cols // 256 * 136
    d, ls, codes = _fields(raw)
    assert codes.min() >= 0 and codes.max() <= 15 and ls.min() >= 0 and ls.max() <= 63 and np.isfinite(d).all()
    y = synth.dequantize_iq4_xs(raw, rows, cols)
    step = np.abs(d[:, None].astype(np.float64) * (ls - 32))                                    # [nb][8]
    err = np.abs(y.astype(np.float64) - W.astype(np.float64)).reshape(-1, 8, 32)
    bound = 14.0 * step[:, :, None] + 2.0 ** -24 * np.abs(y.astype(np.float64)).reshape(-1, 8, 32)
    assert (err <= bound).all(), float((err - bound).max())
    return d, ls, codes, y


def check_fixed_point(raw, rows, cols):
    """dequantize(quantize(y)) == y in every sub-block that holds code 0 (its extreme then sits there), and at least the block's
    largest sub-block does."""
    _, ls, codes = _fields(raw)
    y = synth.dequantize_iq4_xs(raw, rows, cols)
    again = synth.dequantize_iq4_xs(synth.quantize_iq4_xs(y), rows, cols)
    has0 = (codes == 0).any(axis=2)                                                             # [nb][8]
    live = np.abs(ls - 32).max(axis=1) > 0
    assert has0[live].any(axis=1).all() and (np.abs(ls - 32).max(axis=1)[live] == 31).all()
    same = (again.reshape(-1, 8, 32) == y.reshape(-1, 8, 32)).all(axis=2)
    assert same[has0].all()
    assert same[~live].all()
    return has0


def test_quantize_iq4_xs_gaussian_rows():
    rng = np.random.default_rng(7)
    rows, cols = 16, 1024
    W = (0.02 * rng.standard_normal((rows, cols))).astype(np.float32)
    W[3, 256:512] = 0                          # an all-zero block inside a row
    W[5, :32] *= 40                            # one loud sub-block: its neighbours get small scales
    raw = synth.quantize_iq4_xs(W)
    d, ls, codes, y = check_quantised(W, raw)
    assert set(np.unique(codes)) == set(range(16))
    blk0 = 3 * (cols // 256) + 1
    assert d[blk0] == 0 and not y[3, 256:512].any()
    has0 = check_fixed_point(raw, rows, cols)
    assert has0.mean() > 0.5                   # (so that the fixed-point claim is not empty)
    # rows are independent and row-major
    assert raw[:cols // 256 * 136] == synth.quantize_iq4_xs(W[:1])


def test_quantize_iq4_xs_one_outlier_per_sub_block():
    rng = np.random.default_rng(11)
    rows, cols = 16, 512
    W = (0.01 * rng.standard_normal((rows, cols))).astype(np.float32)
    sub = W.reshape(-1, 32)
    at = rng.integers(0, 32, sub.shape[0])
    sub[np.arange(sub.shape[0]), at] = rng.choice([-1.0, 1.0], sub.shape[0]).astype(np.float32) * rng.uniform(0.5, 2.0, sub.shape[0]).astype(np.float32)
    # the worst case of the bound: a weight of the extreme's magnitude and the other sign (x / step = +127, 14 above the table's top)
    sub[0, (at[0] + 1) % 32] = -sub[0, at[0]]
    raw = synth.quantize_iq4_xs(W)
    d, ls, codes, y = check_quantised(W, raw)
    c = codes.reshape(-1, 32)
    assert (c[np.arange(c.shape[0]), at] == 0).mean() > 0.5 and c[0, (at[0] + 1) % 32] == 15
    check_fixed_point(raw, rows, cols)


def test_quantize_iq4_xs_all_zero_block():
    z = synth.quantize_iq4_xs(np.zeros((16, 256), np.float32))
    d, ls, codes, y = check_quantised(np.zeros((16, 256), np.float32), z)
    assert not y.any() and (d == 0).all() and (ls == 32).all()
    assert not np.signbit(d).any()
    check_fixed_point(z, 16, 256)


@pytest.mark.parametrize("shape", [(16, 256), (32, 512)])
def test_gguf_reads_iq4_xs_as_quant_tensor_and_round_trips(tmp_path, shape):
    raw = np.frombuffer(synth.quantize_iq4_xs(np.random.default_rng(shape[0]).standard_normal(shape).astype(np.float32)), np.uint8).copy()
    assert raw.size == shape[0] * shape[1] // 256 * 136
    _, t = gguf.Parser().Read(write_one(tmp_path, "w", raw, shape))
    qt = t["w"]
    assert isinstance(qt, QuantTensor) and qt.ggml_type == IQ4_XS and qt.shape == shape
    np.testing.assert_array_equal(qt.data, raw)
    w = gguf.GGUFWriter()
    w.add_tensor("again", qt)
    path = str(tmp_path / "again.gguf")
    w.write(path)
    _, t2 = gguf.Parser().Read(path)
    assert t2["again"].shape == shape and t2["again"].ggml_type == IQ4_XS
    np.testing.assert_array_equal(t2["again"].data, raw)


@pytest.mark.parametrize("shape", BAD_SHAPES)
def test_gguf_rejects_iq4_xs_outside_the_shape_rules(tmp_path, shape):
    rows, cols = shape
    assert rows * cols % 256 == 0   # whole blocks: the refusal is about the shape, not the byte count
    raw = np.zeros(rows * cols // 256 * 136, np.uint8)
    with pytest.raises(ValueError, match=r"Unsupported data type IQ4_XS.*" + re.escape(gguf.IQ4_XS_RULE)):
        gguf.Parser().Read(write_one(tmp_path, "w", raw, shape))
    assert gguf.IQ4_XS_RULE.startswith("IQ4_XS needs a 2-D tensor")
    assert "rows % 16 == 0" in gguf.IQ4_XS_RULE and "cols % 256 == 0" in gguf.IQ4_XS_RULE and "cols <= 32768" in gguf.IQ4_XS_RULE


def test_gguf_still_refuses_q5_1(tmp_path):
    with pytest.raises(ValueError, match="Unsupported data type Q5_1"):
        gguf.Parser().Read(write_one(tmp_path, "w", np.zeros(16 * 8 * 24, np.uint8), (16, 256), ty=7))


@pytest.fixture(scope="module")
def lib():
    from nfai_amd import build as hb, _lib
    hb.build()
    return _lib.load()


def test_weight_bytes_iq4_xs_through_the_c_abi(lib):
    from nfai_amd import _lib
    assert _lib.IQ4_XS == 23
    n = ctypes.c_uint64()
    _lib.call("nfai_hip_weight_bytes", _lib.IQ4_XS, 16, 256, ctypes.byref(n))
    assert n.value == 16 * 136
    _lib.call("nfai_hip_weight_bytes", _lib.IQ4_XS, 128256, 3072, ctypes.byref(n))
    assert n.value == 128256 * 12 * 136
    for rows, cols in BAD_SHAPES:
        with pytest.raises(_lib.NfaiHipError) as e:
            _lib.call("nfai_hip_weight_bytes", _lib.IQ4_XS, rows, cols, ctypes.byref(n))
        assert e.value.code == _lib.ERR_UNSUPPORTED
        assert "IQ4_XS needs rows % 16 == 0, cols % 256 == 0 and cols <= 32768" in str(e.value)
    with pytest.raises(_lib.NfaiHipError) as e:   # Q5_1 stays without a kernel
        _lib.call("nfai_hip_weight_bytes", 7, 16, 256, ctypes.byref(n))
    assert e.value.code == _lib.ERR_UNSUPPORTED


def test_iq4_xs_type_ids_in_the_header_csharp_lib_and_gguf():
    from nfai_amd import _lib
    cs = open(os.path.join(ROOT, "csharp", "NFAI.HIP", "Native.cs")).read()
    assert re.search(r"enum GgmlType\s*\{[^}]*\bIQ4_XS = 23\b", cs)
    h = open(os.path.join(ROOT, "include", "nfai_hip.h")).read()
    assert re.search(r"enum nfai_dtype\s*\{[^}]*\bNFAI_IQ4_XS = 23\b", h)
    c = open(os.path.join(ROOT, "nfai_amd", "csrc", "common.h")).read()
    assert re.search(r"\bNFAI_IQ4_XS_T16 = 123\b", c)
    assert _lib.IQ4_XS == 23 and gguf.GGML_IQ4_XS == 23 and gguf.GGML_BLOCK[23] == (256, 136) and gguf.GGML_NAME[23] == "IQ4_XS"


def table(dims, mix):
    return {name: synth.iq4_xs_type(name, dims, mix) for name, shape in dims.shapes().items() if len(shape) == 2}


def file_bytes(dims, types):
    total = 0
    for name, shape in dims.shapes().items():
        if len(shape) == 2:
            be, bb = gguf.GGML_BLOCK[types[name]]
            total += shape[0] * shape[1] // be * bb
        else:
            total += shape[0] * 4
    return total


@pytest.mark.parametrize("dims", [synth.LLAMA_32_1B, synth.LLAMA_32_3B, synth.LLAMA_31_8B], ids=lambda d: d.name)
def test_iq4_xs_type_tensor_by_tensor_and_the_file_size_that_follows(dims):
    m, a = table(dims, "iq4_xs"), table(dims, "all_iq4_xs")
    assert set(m) == set(a) == {k for k, v in dims.shapes().items() if len(v) == 2}
    assert set(a.values()) == {IQ4_XS}
    head = "token_embd.weight" if dims.tied else "output.weight"
    grouped = dims.H / dims.Hkv >= 4             # 1B: 32 / 8, 8B: 32 / 8 -> Q5_K attn_v; 3B: 24 / 8 = 3 -> IQ4_XS
    assert grouped == (dims is not synth.LLAMA_32_3B)
    first = dims.L // 8                          # 1B: 2 of 16, 3B: 3 of 28, 8B: 4 of 32
    assert first == {synth.LLAMA_32_1B.name: 2, synth.LLAMA_32_3B.name: 3, synth.LLAMA_31_8B.name: 4}[dims.name]
    n5v = n5d = 0
    for name in m:
        if name == head:
            assert m[name] == Q6_K
            continue
        if name == "token_embd.weight":
            assert m[name] == IQ4_XS             # untied: the table is IQ4_XS
            continue
        layer, kind = int(name.split(".")[1]), name.split(".")[2]
        want = IQ4_XS
        if kind == "attn_v" and grouped:
            want, n5v = Q5_K, n5v + 1
        if kind == "ffn_down" and layer < first:
            want, n5d = Q5_K, n5d + 1
        assert m[name] == want, name
    assert n5v == (dims.L if grouped else 0) and n5d == first
    # the file size that follows from the table: every matrix at 136 bytes per 256 weights, the listed ones at 176 (Q5_K) / 210 (Q6_K)
    mats = {k: v for k, v in dims.shapes().items() if len(v) == 2}
    base = sum(r * c // 256 * 136 for r, c in mats.values()) + sum(v[0] * 4 for v in dims.shapes().values() if len(v) == 1)
    assert file_bytes(dims, a) == base
    Hkv_rows = dims.Hkv * dims.D
    extra = n5v * Hkv_rows * dims.E // 256 * (176 - 136) + n5d * dims.E * dims.F // 256 * (176 - 136) + dims.V * dims.E // 256 * (210 - 136)
    assert file_bytes(dims, m) == base + extra
    # a pipeline stage numbers its blocks within the file
    assert synth.iq4_xs_type("blk.0.ffn_down.weight", dims, "iq4_xs", layer_offset=first, n_layers_file=dims.L) == IQ4_XS
    assert synth.iq4_xs_type("blk.0.ffn_down.weight", dims, "iq4_xs", layer_offset=first - 1, n_layers_file=dims.L) == Q5_K
    assert synth.iq4_xs_type("blk.0.ffn_down.weight", synth.TINY_D128, "iq4_xs", layer_offset=0, n_layers_file=32) == Q5_K
    assert synth.iq4_xs_type("blk.0.ffn_down.weight", synth.TINY_D128, "iq4_xs") == IQ4_XS   # 3 blocks: 3 // 8 = 0
    with pytest.raises(ValueError):
        synth.iq4_xs_type("output.weight", dims, "iq4_nl")


@pytest.mark.parametrize("dims", [synth.LLAMA_32_1B, synth.LLAMA_32_3B, synth.LLAMA_31_8B, synth.TINY_D128], ids=lambda d: d.name)
def test_pipeline_costs_iq4_xs_is_the_sum_over_the_type_table(dims):
    from nfai_amd.pipeline import pipeline_costs
    blocks = 0
    for name, shape in dims.shapes().items():
        if name.startswith("blk.") and len(shape) == 2:
            be, bb = gguf.GGML_BLOCK[synth.iq4_xs_type(name, dims, "iq4_xs")]
            blocks += shape[0] * shape[1] // be * bb
    blk, head = pipeline_costs(dims, "iq4_xs")
    assert blk == pytest.approx(blocks / dims.L, rel=1e-12)
    assert head == pytest.approx(dims.V * dims.E * 210 / 256, rel=1e-12)   # output.weight or the tied token_embd: Q6_K


def test_python_host_picks_any_quant_for_iq4_xs():
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
        p.SetTensor("blk.0.attn_q.weight", QuantTensor(np.zeros(16 * 136, np.uint8), IQ4_XS, (16, 256)))
        assert p._quantized and p._any_quant
        assert calls[-1][0] == "nfai_hip_llama_set_tensor" and calls[-1][3:6] == (IQ4_XS, 16, 256)
        p = Probe()
        p.SetTensor("blk.0.attn_q.weight", (0x1000, _lib.IQ4_XS, 16, 256))
        assert p._quantized and p._any_quant
    finally:
        lm.call = saved
