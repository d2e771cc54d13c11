"""Whole-model parity on the GPU: the fused hipGraph path, the 1:1 C++ chain and the Python op-class
chain against the CPU oracle, on synthetic tiny-Llama models (the oracle finishes in seconds) and on
one full-width block of each BASELINE model.

Stated tolerances (fp32 activations, fp16 weights, fp32 KV): logits max|d| <= 5e-4 * max(1, max|logit|) (tightened in round 4: 4e-5 observed at full size)
end to end and identical greedy tokens; with an fp16 KV cache 2e-2 (the "stated fp16 tolerance").
"""
import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


def odesc(d, C, nfreq=None):
    return orc.LlamaDesc(E=d.E, L=d.L, H=d.H, Hkv=d.Hkv, D=d.D, F=d.F, V=d.V, C=C, rope_n_freqs=nfreq)


def logit_tol(want, scale=5e-4):
    return scale * max(1.0, float(np.abs(want).max()))


def kv_rows(m, layer, is_v, pos, n):
    """[n][Hkv*D] fp32 rows of one block's K or V cache in one synchronising call (test hook nfai_hip_debug_read_kv_rows)."""
    import ctypes as C
    from nfai_amd import _lib
    lib = _lib.load()
    lib.nfai_hip_debug_read_kv_rows.argtypes = [_lib.H, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
    lib.nfai_hip_debug_read_kv_rows.restype = C.c_int32
    out = np.empty((n, m.dims["Hkv"] * m.dims["D"]), np.float32)
    _lib.call("nfai_hip_debug_read_kv_rows", m.handle, layer, int(is_v), pos, n, out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


def gemm_last():
    """The descriptors of the prefill GEMM launches since the last call (test hook nfai_hip_debug_gemm_last), 16 words each: BM, BN,
    WM, WN, BK, stages, weight-ring stages, KS, pipelined, LDS-staged, epilogue, batch, ksplit, M, N, K."""
    import ctypes as C
    from nfai_amd import _lib
    lib = _lib.load()
    lib.nfai_hip_debug_gemm_last.argtypes = [C.POINTER(C.c_uint32), C.c_uint32]
    lib.nfai_hip_debug_gemm_last.restype = C.c_uint32
    buf = (C.c_uint32 * (16 * 256))()
    n = lib.nfai_hip_debug_gemm_last(buf, 256)
    return [tuple(buf[16 * i:16 * i + 16]) for i in range(n)]


@pytest.mark.parametrize("dims", [synth.TINY, synth.TINY_D128], ids=lambda d: d.name)
@pytest.mark.parametrize("mode", ["graph", "eager", "unfused"])
def test_decode_matches_oracle(mgr, dims, mode):
    from nfai_amd.llama_model import LlamaModel
    w = synth.make_weights(dims, seed=21, std=0.05)
    C = 48
    m = LlamaModel(mgr, synth.make_metadata(dims), w, C, unfused=mode == "unfused", graph=mode == "graph")
    ref = orc.OracleLlama(odesc(dims, C), w)
    toks = synth.make_tokens(dims, 40, seed=3)
    for i, t in enumerate(toks):
        lg, am = m.Step(int(t))
        want = ref.step(int(t))
        assert np.abs(lg - want).max() <= logit_tol(want), (i, np.abs(lg - want).max())
        assert am == orc.argmax(want)
    # intermediate state: hidden vector and this token's K/V rows of every layer
    np.testing.assert_allclose(m.Read(0, dims.E), ref.hidden(), rtol=0, atol=1e-3)
    for l in range(dims.L):
        np.testing.assert_allclose(m.ReadKV(l, False, 39), ref.kcache(l)[39], rtol=0, atol=1e-3)
        np.testing.assert_allclose(m.ReadKV(l, True, 17), ref.vcache(l)[17], rtol=0, atol=1e-3)
    assert m.Pos == 40
    m.Dispose()


def test_greedy_loop_on_device_and_reset(mgr):
    """Token fed back on the device through the graph (no host round trip) == host-driven greedy ==
    oracle greedy (ArgMax in place of the stochastic TopP, SamplingUtils.cs:43-57)."""
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY_D128
    w = synth.make_weights(dims, seed=22, std=0.05)
    m = LlamaModel(mgr, synth.make_metadata(dims), w, 64)
    ref = orc.OracleLlama(odesc(dims, 64), w)
    want, tok = [], 5
    for _ in range(24):
        tok = orc.argmax(ref.step(tok))
        want.append(tok)
    got = m.Greedy(5, 24)
    assert got.tolist() == want
    m.Reset()
    assert m.Pos == 0
    tok, host = 5, []
    for _ in range(24):
        _, tok = m.Step(tok, want_logits=False)
        host.append(tok)
    assert host == want
    # two runs bit-equal (determinism: no atomics on the value path)
    m.Reset()
    a, _ = m.Step(9)
    m.Reset()
    b, _ = m.Step(9)
    np.testing.assert_array_equal(a, b)
    m.Dispose()


def test_fused_vs_unfused_vs_opchain(mgr):
    """Every fused kernel against its unfused chain at model scale (same device, same inputs), and the
    Python op-class chain (TransformerBlock wired with BindShaderProprty as TransformerBlock.cs:41-124)
    against the C++ 1:1 chain: those two run the same kernels in the same order."""
    from nfai_amd.llama_model import ChainLlamaModel, LlamaModel
    dims = synth.TINY
    w = synth.make_weights(dims, seed=23, std=0.05)
    md = synth.make_metadata(dims)
    fused = LlamaModel(mgr, md, w, 32)
    unf = LlamaModel(mgr, md, w, 32, unfused=True)
    chain = ChainLlamaModel(mgr, md, w, 32, ropeTableEntries=None)
    for t in synth.make_tokens(dims, 20, seed=4):
        a, _ = fused.Step(int(t))
        b, _ = unf.Step(int(t))
        c = chain.Step(int(t))
        np.testing.assert_allclose(b, c, rtol=0, atol=1e-4)  # same kernels; only the host-built RoPE table may differ by an ulp
        assert np.abs(a - b).max() <= 1e-3 * max(1.0, np.abs(b).max())
    fused.Dispose()
    unf.Dispose()


def test_reference_rope_truncation_mode(mgr):
    """rope_n_freqs = 32 reproduces the reference's 32-entry frequency upload (TransformerBlock.cs:66):
    for D = 128 the pairs 32..63 are not rotated.  The op-class chain defaults to that behaviour."""
    from nfai_amd.llama_model import ChainLlamaModel, LlamaModel
    dims = synth.TINY_D128
    w = {k: v for k, v in synth.make_weights(dims, seed=24, std=0.05).items() if k != "output.weight"}  # the reference ties lm_head
    md = synth.make_metadata(dims)
    m = LlamaModel(mgr, md, w, 64, rope_n_freqs=32)
    chain = ChainLlamaModel(mgr, md, w, 64)  # ropeTableEntries = 32 as the reference
    ref = orc.OracleLlama(odesc(dims, 64, nfreq=32), w)
    spec = orc.OracleLlama(odesc(dims, 64), w)
    for t in synth.make_tokens(dims, 60, seed=12):
        lg, _ = m.Step(int(t))
        want = ref.step(int(t))
        spec.step(int(t), want_logits=False)
        assert np.abs(lg - want).max() <= logit_tol(want)
        assert np.abs(chain.Step(int(t)) - want).max() <= logit_tol(want)
    # the truncated pairs are the LOW frequencies, so the defect shows in late K rows, dims 64..127
    k_got = m.ReadKV(0, False, 59).reshape(dims.Hkv, dims.D)
    k_ref = ref.kcache(0)[59].reshape(dims.Hkv, dims.D)
    k_spec = spec.kcache(0)[59].reshape(dims.Hkv, dims.D)
    np.testing.assert_allclose(k_got, k_ref, rtol=0, atol=1e-3)
    np.testing.assert_allclose(k_got[:, :64], k_spec[:, :64], rtol=0, atol=1e-3)
    assert np.abs(k_got[:, 64:] - k_spec[:, 64:]).max() > 1e-2  # the switch does something
    m.Dispose()


def test_kv_f16_option(mgr):
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY_D128
    w = synth.make_weights(dims, seed=25, std=0.05)
    m = LlamaModel(mgr, synth.make_metadata(dims), w, 128, kv_f16=True)
    ref = orc.OracleLlama(odesc(dims, 128), w)
    for t in synth.make_tokens(dims, 100, seed=6):  # up to four KV slices: the fp16-KV form of the fused attention + Wo launch
        lg, am = m.Step(int(t))
        want = ref.step(int(t))
        assert np.abs(lg - want).max() <= logit_tol(want, 2e-2)
    m.Dispose()


def test_kv_capacity_is_a_hard_error(mgr):
    from nfai_amd._lib import KVCacheFull
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY
    m = LlamaModel(mgr, synth.make_metadata(dims), synth.make_weights(dims, seed=26), 4)
    for t in range(4):
        m.Step(t)
    with pytest.raises(KVCacheFull):
        m.Step(1)
    with pytest.raises(KVCacheFull):
        m.Greedy(1, 2)
    m.Reset()
    m.Step(1)
    m.Dispose()


def test_missing_and_misshaped_tensors(mgr):
    from nfai_amd._lib import NfaiHipError
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY
    w = synth.make_weights(dims, seed=27)
    md = synth.make_metadata(dims)
    bad = dict(w)
    del bad["blk.1.ffn_up.weight"]
    with pytest.raises(NfaiHipError, match="never set"):
        LlamaModel(mgr, md, bad, 8)
    bad = dict(w)
    bad["blk.0.attn_k.weight"] = bad["blk.0.attn_k.weight"][:-2]
    with pytest.raises(NfaiHipError, match="expected"):
        LlamaModel(mgr, md, bad, 8)
    bad = dict(w)
    bad["blk.0.bogus.weight"] = np.zeros(4, np.float32)
    with pytest.raises(NfaiHipError, match="unknown tensor"):
        LlamaModel(mgr, md, bad, 8)


def test_pipeline_stages_bit_identical_to_single(mgr):
    """Layer ranges as pipeline stages on one GPU (hidden state handed over in device memory):
    logits bit-identical to the single-stage run."""
    from nfai_amd.hip import ShaderProperty
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY_D128
    w = synth.make_weights(dims, seed=28, std=0.05)
    md = synth.make_metadata(dims)
    whole = LlamaModel(mgr, md, w, 16, graph=False)
    s0 = LlamaModel(mgr, md, w, 16, layer_range=(0, 1))
    s1 = LlamaModel(mgr, md, w, 16, layer_range=(1, 2))
    s2 = LlamaModel(mgr, md, w, 16, layer_range=(2, 3))
    h01, h12 = ShaderProperty(mgr, dims.E), ShaderProperty(mgr, dims.E)
    for t in (4, 8, 15, 16, 23, 42):
        want, am = whole.Step(t)
        s0.StageStep(t, None, h01.buffer.device_ptr)
        s1.StageStep(0, h01.buffer.device_ptr, h12.buffer.device_ptr)
        lg, am2 = s2.StageStep(0, h12.buffer.device_ptr, None, want_logits=True)
        np.testing.assert_array_equal(lg, want)
        assert am == am2
    for m in (whole, s0, s1, s2):
        m.Dispose()


@pytest.mark.parametrize("dims", [synth.LLAMA_32_1B, synth.LLAMA_32_3B, synth.LLAMA_31_8B], ids=lambda d: d.name)
def test_one_full_width_block(mgr, dims):
    """One transformer block at the real widths of each BASELINE model (E, H, Hkv, D, F as published;
    vocabulary cut to 4096 rows so the oracle stays fast), 20 positions."""
    from dataclasses import replace
    from nfai_amd.llama_model import LlamaModel
    d1 = replace(dims, L=1, V=4096, name=dims.name + "-1blk")
    w = synth.make_weights(d1, seed=31)
    m = LlamaModel(mgr, synth.make_metadata(d1), w, 32)
    ref = orc.OracleLlama(odesc(d1, 32), w)
    for t in synth.make_tokens(d1, 20, seed=8):
        lg, am = m.Step(int(t))
        want = ref.step(int(t))
        assert np.abs(lg - want).max() <= logit_tol(want), np.abs(lg - want).max()
    m.Dispose()


@pytest.mark.parametrize("dims,n_pos,cap", [(synth.LLAMA_32_1B, 1100, 0), (synth.LLAMA_32_3B, 200, 0), (synth.LLAMA_31_8B, 200, 0),
                                            (synth.LLAMA_32_3B, 700, 2304)],
                         ids=["1b-1100", "3b-200", "8b-200", "3b-700-long-capacity"])
def test_attention_slices_full_width(mgr, dims, n_pos, cap):
    """The KV slices of the decode attention and their hand-off inside the launch ({value, tag} granules polled by the block of
    the last slice; tag = token epoch x blocks + block) at the head shapes of the BASELINE models: two blocks (two tags per
    token on one workspace), every position from 1 slice to the maximum of 32 (1B: 1100 positions), logits against the oracle
    at every step.  A KV capacity above 2048 selects the one-pass (online softmax) form of the kernel and two launches
    (attention, then Wo) instead of the fused one: same hand-off, same tolerance."""
    from dataclasses import replace
    from nfai_amd.llama_model import LlamaModel
    d2 = replace(dims, L=2, V=1024, name=dims.name + "-2blk")
    w = synth.make_weights(d2, seed=37)
    C = cap or n_pos + 4
    m = LlamaModel(mgr, synth.make_metadata(d2), w, C)
    ref = orc.OracleLlama(odesc(d2, C), w)
    worst = 0.0
    for i, t in enumerate(synth.make_tokens(d2, n_pos, seed=12)):
        lg, am = m.Step(int(t))
        want = ref.step(int(t))
        err = np.abs(lg - want).max()
        worst = max(worst, err / logit_tol(want))
        assert err <= logit_tol(want), (i, err)
    assert m.Pos == n_pos
    m.Dispose()


def test_bytes_per_token_accounting(mgr):
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY
    w = synth.make_weights(dims, seed=29)
    m = LlamaModel(mgr, synth.make_metadata(dims), w, 8)
    total, dom = m.BytesPerToken(3)
    mats = sum(v.nbytes for k, v in w.items() if v.ndim == 2)
    kv = dims.L * (2 * dims.Hkv * dims.D * 4 * 4 + 2 * dims.Hkv * dims.D * 4)
    assert total == mats + dims.E * 2 + kv
    assert dom == 2 * dims.F * dims.E * 2
    m.Dispose()


@pytest.mark.parametrize("dims", [synth.TINY, synth.TINY_D128], ids=lambda d: d.name)
def test_attention_handoff_failure_falls_back_to_the_ticket_form(mgr, dims, capfd):
    """The slices' workgroups of the attention launch wait for each other (bounded).  A test hook makes one slice publish
    nothing: the waits give up, the error word is set — and the step must re-run the token on the ticket hand-off, say so once,
    return the oracle's logits, and keep working (ticket form) afterwards.  One provoked failure, not a loop."""
    import ctypes as C
    from nfai_amd import _lib
    from nfai_amd.llama_model import LlamaModel
    w = synth.make_weights(dims, seed=71, std=0.06)
    m = LlamaModel(mgr, synth.make_metadata(dims), w, 96)
    ref = orc.OracleLlama(odesc(dims, 96), w)
    toks = synth.make_tokens(dims, 44, seed=5)
    for t in toks[:40]:                                  # 40 positions: two slices per kv head from here on
        lg, _ = m.Step(int(t))
        lr = ref.step(int(t))
    tol = 5e-4 * max(1.0, float(np.abs(lr).max()))
    assert np.abs(lg - lr).max() <= tol
    lib = _lib.load()
    lib.nfai_hip_debug_attn_withhold.argtypes = [_lib.H, C.c_uint32]
    lib.nfai_hip_debug_attn_withhold.restype = C.c_int32
    assert lib.nfai_hip_debug_attn_withhold(m.handle, 2) == 0      # slice 1 of kv head 0 stays silent
    capfd.readouterr()
    lg, am = m.Step(int(toks[40]))                       # fails inside, falls back, re-runs position 40
    lr = ref.step(int(toks[40]))
    err = capfd.readouterr().err
    assert "ticket hand-off" in err and "position 40" in err
    assert np.abs(lg - lr).max() <= tol and am == orc.argmax(lg) and m.Pos == 41
    for t in toks[41:]:                                  # the model stays on the ticket form (the hook only gags the granule form)
        lg, _ = m.Step(int(t))
        lr = ref.step(int(t))
        assert np.abs(lg - lr).max() <= tol
    assert "ticket hand-off" not in capfd.readouterr().err   # logged once
    m.Dispose()


def test_topk_sampling_path(mgr):
    """The reference's DEFAULT sampler (LlamaModel.cs:128-130,165: SamplingUtils.TopP) with its first half on the device:
    after every step nfai_hip_llama_decode_topk must return the candidates TopP forms from the oracle's logits, and the token
    drawn from them must be the oracle's for the same `rand`; the draws are fed back, so positions advance as in RunAsync."""
    from nfai_amd.llama_model import LlamaModel, SamplingUtils
    dims = synth.TINY
    w = synth.make_weights(dims, seed=61, std=0.08)
    m = LlamaModel(mgr, synth.make_metadata(dims), w, 32)
    ref = orc.OracleLlama(odesc(dims, 32), w)
    tok = 5
    rands = np.random.Generator(np.random.PCG64(9)).random(12, dtype=np.float32)
    for step, rand in enumerate(rands):
        ids, probs = m.StepTopK(tok, 0.5, 40)
        lg = ref.step(tok)
        want, ids_ref, probs_ref, _ = orc.topp(lg, 0.5, 0.95, 40, float(rand))
        # the GPU logits differ from the oracle's in the last bits (summation order): candidates whose probabilities are
        # closer than that may swap places, so compare as sets where the oracle's neighbours are within 1e-5 relative
        gaps = np.abs(np.diff(probs_ref)) / probs_ref[:-1]
        if (gaps > 1e-4).all():
            np.testing.assert_array_equal(ids, ids_ref)
        else:
            assert set(ids[:30].tolist()) <= set(ids_ref.tolist())
        np.testing.assert_allclose(np.sort(probs)[::-1], probs_ref, rtol=2e-4)
        got = SamplingUtils.TopPFromCandidates(ids, probs, 0.95, rand=float(rand))
        lgpu = m.Read(4, dims.V)
        own_tok, own_ids, own_probs, _ = orc.topp(lgpu, 0.5, 0.95, 40, float(rand))
        # on the GPU's own logits the candidate indices are exact: in order, unless two neighbours' probabilities coincide to the
        # last bits (then the device's and the oracle's sum of exponentials may round them to equal / unequal values differently)
        assert sorted(ids.tolist()) == sorted(own_ids.tolist())
        if (np.abs(np.diff(own_probs)) > 1e-6 * own_probs[:-1]).all():
            np.testing.assert_array_equal(ids, own_ids)
        assert got == own_tok
        tok = want if got != want else got
        assert m.Pos == step + 1
    # a rejected call (k > 64, k > V, temperature <= 0) must leave the model where it was: the same token can be retried
    from nfai_amd import _lib
    pos = m.Pos
    for bad_t, bad_k in ((0.5, 65), (0.5, 0), (0.0, 40), (-1.0, 40)):
        with pytest.raises(_lib.NfaiHipError):
            m.StepTopK(tok, bad_t, bad_k)
        assert m.Pos == pos
    ids, probs = m.StepTopK(tok, 0.5, 40)
    np.testing.assert_array_equal(np.sort(ids), np.sort(orc.topp(m.Read(4, dims.V), 0.5, 0.95, 40, 0.0)[1]))
    assert m.Pos == pos + 1
    # the blocking calls are one hipGraph each (token in, kernels, candidates out), re-captured when (temperature, k) change; a model
    # without graphs takes the eager form of the same sequence: identical candidates, step by step, also across a change of k
    e = LlamaModel(mgr, synth.make_metadata(dims), w, 32, graph=False)
    m.Reset()
    t2 = 9
    for step, (temp, k) in enumerate([(0.5, 40), (0.5, 40), (0.8, 8), (0.8, 8), (0.5, 40), (1.0, 64)]):
        gi, gp = m.StepTopK(t2, temp, k)
        ei, ep = e.StepTopK(t2, temp, k)
        np.testing.assert_array_equal(gi, ei)
        np.testing.assert_array_equal(gp, ep)
        lg, am = m.Step(int(gi[0]))                      # the plain blocking step (its own graph) in between
        le, ae = e.Step(int(gi[0]))
        assert am == ae and np.array_equal(lg, le) and m.Pos == e.Pos == 2 * step + 2
        t2 = am
    e.Dispose()
    m.Dispose()


def test_gguf_file_to_generation_end_to_end(mgr, tmp_path):
    """File -> Parser -> factory (AbstractModelFactory.TryCreate hook) -> LlamaModel.RunAsync with the
    reference's chat template and tokenizer -> greedy text; token ids identical to the oracle driven by
    the same prompt ids."""
    from nfai_amd import gguf
    from nfai_amd.llama_model import LlamaModelFactory, ModelOptions
    from nfai_amd.tokenizer import Tokenizer
    dims = synth.TINY
    w = synth.make_weights(dims, seed=51, std=0.05)
    specials = ["<|begin_of_text|>", "<|start_header_id|>", "<|end_header_id|>", "<|eot_id|>"]
    chars = list("abcdefghijklmnopqrstuvwxyzY.,!?'0123456789") + ["Ġ", "Ċ"]
    merges = ["h e", "l l", "he ll", "hell o", "Ġ w", "o r", "Ċ Ċ"]
    toks = specials + chars + [m.replace(" ", "") for m in merges]
    toks += [f"<pad{i}>" for i in range(dims.V - len(toks))]
    md = synth.make_metadata(dims)
    md.update({"tokenizer.ggml.tokens": toks, "tokenizer.ggml.merges": merges,
               "tokenizer.ggml.bos_token_id": 0, "tokenizer.ggml.eos_token_id": 3})
    path = str(tmp_path / "tiny.gguf")
    gguf.write_model(path, md, w)

    class Factory(LlamaModelFactory):  # share the test's device context instead of creating a second one
        def __init__(self, m):
            self.mgr = m

    model = gguf.Parser([Factory(mgr)]).Parse(ModelOptions(GGUFPath=path, KVCacheSize=128))
    assert model.ModelName == dims.name and model.C == 128
    # the factory gives the provider path its MFMA prefill workspace: RunAsync ingests the prompt (all tokens but the last) in ONE
    # call (nfai_hip_llama_ingest), the last prompt token goes through the sampled step
    assert model.promptPrefill
    calls = []
    orig_ingest, orig_step = model.Ingest, model.Step
    model.Ingest = lambda toks: (calls.append(("ingest", len(toks))), orig_ingest(toks))[1]
    model.Step = lambda tok, want_logits=True: (calls.append(("step", 1)), orig_step(tok, want_logits))[1]
    text = "".join(model.RunAsync("hello world", greedy=True, max_tokens=6))
    tk = Tokenizer(md)
    ids = tk.Tokenize("hello world", addBos=True)
    assert calls[0] == ("ingest", len(ids) - 1) and all(c == ("step", 1) for c in calls[1:])
    ref = orc.OracleLlama(odesc(dims, 128), w)
    lg = None
    for t in ids:
        lg = ref.step(t)
    first_logits = lg
    want = []
    for _ in range(6):
        t = orc.argmax(lg)
        if t == 3:
            break
        want.append(t)
        lg = ref.step(t)
    assert text == tk.Detokenize(want)
    # every prompt token and every generated token that was fed back advanced the position: the 6-token cap stops
    # before the 6th token is fed; an EOS stops after the (len(want)+1)-th sample without feeding it
    assert model.Pos == len(ids) + (5 if len(want) == 6 else len(want))
    # the first sampled step's logits behind the MFMA-prefilled cache, against the oracle's token-by-token fp32 path: the stated
    # fp16 tolerance of the prefill (2e-2 * max(1, max|logit|)); then the switch: promptPrefill = False is the M = 1 path bit for bit
    model.Reset()
    model.Ingest(ids[:-1])
    lg_pf, _ = orig_step(ids[-1])
    assert np.abs(lg_pf - first_logits).max() <= 2e-2 * max(1.0, float(np.abs(first_logits).max()))
    model.Reset()
    for t in ids[:-1]:
        orig_step(t, False)
    lg_tok, _ = orig_step(ids[-1])
    assert np.abs(lg_tok - first_logits).max() <= logit_tol(first_logits)
    model.Reset()
    model.firstInput = True
    model.promptPrefill = False
    calls.clear()
    text2 = "".join(model.RunAsync("hello world", greedy=True, max_tokens=6))
    assert text2 == text and not any(c[0] == "ingest" for c in calls)
    # the KV-capacity error is preserved on the prompt path: refused before anything runs
    from nfai_amd._lib import KVCacheFull
    model.SetPos(128 - 2)
    with pytest.raises(KVCacheFull):
        model.Ingest(ids[:-1])
    assert model.Pos == 128 - 2
    model.Dispose()


@pytest.mark.parametrize("dims,n,chunk", [(synth.TINY, 37, 64), (synth.TINY_D128, 100, 64), (synth.TINY_D128, 130, 128)],
                         ids=["tiny-37", "d128-100-chunked", "d128-130-chunked"])
def test_prefill_mfma_matches_token_by_token(mgr, dims, n, chunk):
    """Batched MFMA prefill (fp16 operands, fp32 accumulate) against the oracle's token-by-token fp32
    path (the reference feeds the prompt one token at a time, LlamaModel.cs:103-126).  Stated fp16
    tolerance: logits max|d| <= 2e-2 * max(1, max|logit|) (round 4: was 5e-2), same argmax; then decode continues from the
    prefilled KV cache within the same tolerance."""
    from nfai_amd.llama_model import LlamaModel
    w = synth.make_weights(dims, seed=71, std=0.05)
    m = LlamaModel(mgr, synth.make_metadata(dims), w, 160, max_batch=chunk)
    ref = orc.OracleLlama(odesc(dims, 160), w)
    toks = synth.make_tokens(dims, n, seed=13)
    want = None
    for t in toks:
        want = ref.step(int(t))
    got = m.Prefill(toks)
    assert m.Pos == n
    tol = 2e-2 * max(1.0, float(np.abs(want).max()))
    assert np.abs(got - want).max() <= tol, np.abs(got - want).max()
    assert int(np.argmax(got)) == orc.argmax(want)
    # K/V rows written by the prefill
    for l in (0, dims.L - 1):
        np.testing.assert_allclose(m.ReadKV(l, False, n - 1), ref.kcache(l)[n - 1], rtol=0, atol=2e-2)
        np.testing.assert_allclose(m.ReadKV(l, True, 3), ref.vcache(l)[3], rtol=0, atol=2e-2)
    # decode continues on the GEMV path from the prefilled cache
    tok = orc.argmax(want)
    for _ in range(8):
        lg, am = m.Step(tok)
        wl = ref.step(tok)
        assert np.abs(lg - wl).max() <= tol
        tok = orc.argmax(wl)
    m.Dispose()


# the q|k|v + RoPE launch each case is meant to reach: (BM, BN, BK, stages, KS, pipelined) as nfai_hip_debug_gemm_last reports them
@pytest.mark.parametrize("dims,chunk,rope_form", [(synth.LLAMA_32_3B, 512, (128, 80, 128, 3, 2, 1)), (synth.LLAMA_32_3B, 256, (128, 64, 128, 3, 2, 0)),
                                                  (synth.LLAMA_31_8B, 512, (128, 96, 64, 4, 2, 0)), (synth.LLAMA_32_1B, 512, (128, 48, 128, 3, 2, 0)),
                                                  (synth.LLAMA_32_3B, -39, (64, 80, 64, 4, 1, 0)), (synth.LLAMA_32_1B, -100, (128, 48, 128, 3, 2, 0)),
                                                  (synth.LLAMA_31_8B, -7, (64, 64, 64, 4, 1, 0))],
                         ids=["3b-512", "3b-2x256", "8b-512", "1b-512", "3b-short-39", "1b-short-100", "8b-short-7"])
def test_prefill_full_width_block(mgr, dims, chunk, rope_form):
    """BASELINE config 3's prefill leg at its real size: ONE block at the published widths (vocabulary cut to 4096 rows so the
    oracle stays fast), T = 512 prompt tokens through the MFMA prefill — here gemm_pick takes the 128 x 128 direct-to-LDS
    kernels with the SiLU*up / fp16 epilogues and the causal tile skipping that carry the headline prefill number — against the
    oracle's token-by-token fp32 path (LlamaModel.cs:103-126).  chunk = 256: the second chunk runs with pos0 = 256.
    Stated fp16 tolerance 2e-2 * max(1, max|logit|) (about 1e-1 absolute at these widths; round 4: was 5e-2), same argmax, EVERY K / V row of
    the block within 2e-2 (the 80- and 96-wide RoPE tiles of 3B / 8B at 512 rows, the 64-row ones of the short prompts: which one ran is
    asserted through nfai_hip_debug_gemm_last), then 8 decode tokens from the prefilled cache."""
    from dataclasses import replace
    from nfai_amd.llama_model import LlamaModel
    d1 = replace(dims, L=1, V=4096, name=dims.name + "-1blk")
    w = synth.make_weights(d1, seed=33)
    # chunk < 0: a SHORT prompt of -chunk tokens in one call (what the provider path's RunAsync hands to nfai_hip_llama_ingest): at <= 64 rows
    # the 64-row tiles, at <= 128 rows the K range of Wo / Wdown split over the chip + k_sum_slabs, at the published widths
    n = 512 if chunk > 0 else -chunk
    C = n + 16
    m = LlamaModel(mgr, synth.make_metadata(d1), w, C, max_batch=max(chunk, 128))
    ref = orc.OracleLlama(odesc(d1, C), w)
    toks = synth.make_tokens(d1, n, seed=14)
    for t in toks[:-1]:
        ref.step(int(t), want_logits=False)  # the oracle skips output norm + lm_head when no logits are asked for
    want = ref.step(int(toks[-1]))
    gemm_last()
    got = m.Prefill(toks)
    rope = {(r[0], r[1], r[4], r[5], r[7], r[8]) for r in gemm_last() if r[10] == 3}   # epilogue 3: q|k|v + RoPE + cache stores
    assert rope == {rope_form}, rope
    assert m.Pos == n
    tol = 2e-2 * max(1.0, float(np.abs(want).max()))
    assert np.abs(got - want).max() <= tol, np.abs(got - want).max()
    assert int(np.argmax(got)) == orc.argmax(want)
    for is_v, cache in ((False, ref.kcache(0)), (True, ref.vcache(0))):   # all n rows the prefill wrote
        err = np.abs(kv_rows(m, 0, is_v, 0, n) - cache[:n]).max(axis=1)
        assert err.max() <= 2e-2, ("V" if is_v else "K", int(err.argmax()), float(err.max()))
    # the hidden state of the last prompt token (what the output norm + lm_head consumed)
    tok = orc.argmax(want)
    for _ in range(8):
        lg, am = m.Step(tok)
        wl = ref.step(tok)
        assert np.abs(lg - wl).max() <= tol
        tok = orc.argmax(wl)
    m.Dispose()


@pytest.mark.parametrize("n", [256, 500], ids=["256-rows", "500-rows-ragged"])
def test_prefill_long_chunk_k_split_and_fused_combine(mgr, monkeypatch, n):
    """Chunks of >= 256 rows run Wdown (K >= 8192) as four K quarters on 256 x 128 tiles; the slabs are added up — residual + slab 0 + ... in
    order — either by k_sum_slabs or, fused, by the next block's attention norm (k_rmsnorm_rows_combine): the two must be bit-identical
    (NFAI_PREFILL_COMBINE_FUSED is read per call), over two blocks at the 3B widths (so that one combine is fused into a norm and the last
    one is the plain tail), and the logits must agree with the oracle's token-by-token path within the prefill tolerance.  Every row of
    block 1's K and V is compared, fused against unfused bit for bit and against the oracle at 2e-2: a slab not added for one row block
    shows in that block's rows."""
    from dataclasses import replace
    from nfai_amd.llama_model import LlamaModel
    d2 = replace(synth.LLAMA_32_3B, L=2, V=2048, name="llama-3.2-3b-2blk")
    w = synth.make_weights(d2, seed=35)
    C = n + 16   # (500 rows: four 128-row blocks, the last one ragged — rows past the chunk's end are neither stored nor added)
    toks = synth.make_tokens(d2, n, seed=16)
    outs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("NFAI_PREFILL_COMBINE_FUSED", fused)
        m = LlamaModel(mgr, synth.make_metadata(d2), w, C, max_batch=n)
        lg = m.Prefill(toks)
        outs.append((lg, m.Read(0, d2.E), [kv_rows(m, 1, v, 0, n) for v in (False, True)]))   # every row of block 1's K and V
        m.Dispose()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    for a, b in zip(outs[0][2], outs[1][2]):
        assert np.array_equal(a, b)
    ref = orc.OracleLlama(odesc(d2, C), w)
    for t in toks[:-1]:
        ref.step(int(t), want_logits=False)
    want = ref.step(int(toks[-1]))
    assert np.abs(outs[0][0] - want).max() <= 2e-2 * max(1.0, float(np.abs(want).max()))
    assert int(np.argmax(outs[0][0])) == orc.argmax(want)
    # block 1's K / V rows witness block 0's Wdown quarters and their combine for every row of the chunk
    for got, cache in zip(outs[0][2], (ref.kcache(1), ref.vcache(1))):
        err = np.abs(got - cache[:n]).max(axis=1)
        assert err.max() <= 2e-2, (int(err.argmax()), float(err.max()))


@pytest.mark.parametrize("dims,n,chunk,kv16", [(synth.TINY_D128, 130, 128, False), (synth.TINY_D128, 101, 64, True), (synth.TINY, 37, 64, False)],
                         ids=["d128-130", "d128-101-kvf16-unaligned-chunks", "tiny-d64"])
def test_prefill_rope_in_the_gemm_epilogue_is_bit_identical(mgr, dims, n, chunk, kv16, monkeypatch):
    """RoPE + the q / KV-cache / fp16 K / V^T stores in the q|k|v GEMM's epilogue (the default) against the same GEMM followed by
    k_rope_store_tiles (NFAI_PREFILL_ROPE_FUSED=0; the switch is read per call): same arithmetic in the same order, so logits and
    every K / V row must be IDENTICAL, also for a second chunk (pos0 > 0), a ragged last chunk and an fp16 KV cache."""
    from nfai_amd.llama_model import LlamaModel
    w = synth.make_weights(dims, seed=72, std=0.05)
    toks = synth.make_tokens(dims, n, seed=15)
    outs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("NFAI_PREFILL_ROPE_FUSED", fused)
        m = LlamaModel(mgr, synth.make_metadata(dims), w, 160, max_batch=chunk, kv_f16=kv16)
        lg = m.Prefill(toks)
        kv = [m.ReadKV(l, v, pos) for l in range(dims.L) for v in (False, True) for pos in (0, 1, chunk - 1, chunk, n - 1)]
        nxt, _ = m.Step(int(np.argmax(lg)))  # reads the fp32 / fp16 cache rows the prefill wrote
        outs.append((lg, kv, nxt))
        m.Dispose()
    assert np.array_equal(outs[0][0], outs[1][0])
    for a, b in zip(outs[0][1], outs[1][1]):
        assert np.array_equal(a, b)
    assert np.array_equal(outs[0][2], outs[1][2])


# ---- the weight-streaming engine: one launch per block (kernels_engine.hip) ---------------------------------------------
@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_engine_decode_matches_oracle(mgr, mode):
    """Wo -> gate|up -> Wdown -> next block's q|k|v in one launch per block (LDS-DMA weight ring, granule hand-offs) against the
    oracle, token by token, with the intermediate state; then against the five-launch path of the same library (same kernels'
    arithmetic, another summation tree): the stated end-to-end tolerance, identical greedy tokens."""
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY_D128  # E = HD = 512, F = 1024: every K is a multiple of 512
    w = synth.make_weights(dims, seed=91, std=0.05)
    C = 48
    m = LlamaModel(mgr, synth.make_metadata(dims), w, C, graph=mode == "graph", engine=True)
    five = LlamaModel(mgr, synth.make_metadata(dims), w, C, engine=False)
    ref = orc.OracleLlama(odesc(dims, C), w)
    for i, t in enumerate(synth.make_tokens(dims, 40, seed=5)):
        lg, am = m.Step(int(t))
        lf, _ = five.Step(int(t))
        want = ref.step(int(t))
        assert np.abs(lg - want).max() <= logit_tol(want), (i, np.abs(lg - want).max())
        assert np.abs(lg - lf).max() <= logit_tol(want)
        assert am == orc.argmax(want)
    np.testing.assert_allclose(m.Read(0, dims.E), ref.hidden(), rtol=0, atol=1e-3)
    for l in range(dims.L):
        np.testing.assert_allclose(m.ReadKV(l, False, 39), ref.kcache(l)[39], rtol=0, atol=1e-3)
        np.testing.assert_allclose(m.ReadKV(l, True, 17), ref.vcache(l)[17], rtol=0, atol=1e-3)
    # greedy on the device, reset, bit-reproducibility
    m.Reset()
    ref2 = orc.OracleLlama(odesc(dims, C), w)
    want, tok = [], 5
    for _ in range(24):
        tok = orc.argmax(ref2.step(tok))
        want.append(tok)
    assert m.Greedy(5, 24).tolist() == want
    m.Reset()
    a, _ = m.Step(9)
    m.Reset()
    b, _ = m.Step(9)
    np.testing.assert_array_equal(a, b)
    m.Dispose()
    five.Dispose()


@pytest.mark.parametrize("dims", [synth.LLAMA_32_1B, synth.LLAMA_32_3B, synth.LLAMA_31_8B], ids=lambda d: d.name)
def test_engine_two_full_width_blocks(mgr, dims):
    """Two blocks at the published widths of each BASELINE model (the first engine launch carries the second block's q|k|v,
    the last one ends with Wdown), vocabulary cut to 4096 rows, 16 positions, against the oracle."""
    from dataclasses import replace
    from nfai_amd.llama_model import LlamaModel
    d2 = replace(dims, L=2, V=4096, name=dims.name + "-2blk")
    w = synth.make_weights(d2, seed=93)
    m = LlamaModel(mgr, synth.make_metadata(d2), w, 24, engine=True)
    ref = orc.OracleLlama(odesc(d2, 24), w)
    for t in synth.make_tokens(d2, 16, seed=15):
        lg, am = m.Step(int(t))
        want = ref.step(int(t))
        assert np.abs(lg - want).max() <= logit_tol(want), np.abs(lg - want).max()
    np.testing.assert_allclose(m.Read(0, d2.E), ref.hidden(), rtol=0, atol=1e-3)
    m.Dispose()


def test_engine_pipeline_stages_and_fallback(mgr):
    """Layer ranges as stages with the engine on against the whole model with the engine on: the first block of a stage gets
    its q|k|v from the GEMV kernel instead of the previous block's engine launch (another summation tree), so the results agree
    to the summation-order tolerance rather than bit for bit.  A model the engine cannot take (K not a multiple of 512)
    silently runs the five-launch path."""
    from nfai_amd.hip import ShaderProperty
    from nfai_amd.llama_model import LlamaModel
    dims = synth.TINY_D128
    w = synth.make_weights(dims, seed=95, std=0.05)
    md = synth.make_metadata(dims)
    whole = LlamaModel(mgr, md, w, 16, engine=True)
    s0 = LlamaModel(mgr, md, w, 16, layer_range=(0, 2), engine=True)
    s1 = LlamaModel(mgr, md, w, 16, layer_range=(2, 3), engine=True)
    h01 = ShaderProperty(mgr, dims.E)
    for t in (4, 8, 15, 16, 23, 42):
        want, am = whole.Step(t)
        s0.StageStep(t, None, h01.buffer.device_ptr)
        lg, am2 = s1.StageStep(0, h01.buffer.device_ptr, None, want_logits=True)
        np.testing.assert_allclose(lg, want, rtol=0, atol=1e-4)
        assert am == am2
    for m in (whole, s0, s1):
        m.Dispose()
    tiny = synth.TINY  # E = 256
    wt = synth.make_weights(tiny, seed=96, std=0.05)
    a = LlamaModel(mgr, synth.make_metadata(tiny), wt, 8, engine=True)
    b = LlamaModel(mgr, synth.make_metadata(tiny), wt, 8, engine=False)
    np.testing.assert_array_equal(a.Step(3)[0], b.Step(3)[0])
    a.Dispose()
    b.Dispose()


@pytest.mark.parametrize("quant", ["f16", "q4_k_m"])
def test_full_size_parity_through_bench(quant, tmp_path):
    """The whole Llama-3.2-3B (BASELINE config 3: 28 blocks, vocabulary 128256, 6.4 GB of fp16 weights) at full size: `bench.py`
    runs the oracle on the same weights (its `cpu_baseline` leg, here 6 tokens) and compares EVERY position's full logit vector
    with the GPU's, and compares the 512-token MFMA prefill with the token-by-token decode path.  The tolerances are the
    end-to-end ones of this file; the line must also carry the contract's roofline fields.  Also as Q4_K_M (BASELINE config 4:
    Q4_K / Q6_K blocks; the oracle multiplies the dequantised weights).  The fp16 run is the default workload, so it also
    appends `configs[]` — BASELINE configs 4, 2 (the whole 16-block Llama-3.2-1B) and config 5's per-GPU share (four 8B blocks
    + the untied Q6_K lm_head), each in a child process with its own oracle comparison at full width and depth.  All of this is
    `bench.py --full`; the plain run of the same arguments (the headline only) must time the same steps on the same inputs: the
    same positions and KV capacity, and bit for bit the same last logits and token (the value path has no atomics)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}

    def bench(dump, *extra):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "16", "--warmup", "2", "--cpu-tokens", "6", "--quant", quant,
                            "--dump-outputs", dump, *extra], env=env, cwd=root, capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        return json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])

    dump = str(tmp_path / "outputs")
    d = bench(dump, "--full")
    plain_dump = str(tmp_path / "plain_outputs")
    p = bench(plain_dump)
    for k in ("metric", "unit", "n_gpus", "steps", "warmup", "higher_is_better", "dtype", "bytes_per_token"):
        assert p[k] == d[k], k
    assert p["value"] > 100 and abs(p["value"] - 1e3 / p["ms_per_step"]) < 1e-6 * p["value"]
    assert {k: p["config"][k] for k in ("workload", "positions", "kv_capacity")} == {k: d["config"][k] for k in ("workload", "positions", "kv_capacity")}
    assert not {"roofline", "prefill", "cpu_baseline", "short_context", "sampling_path", "configs"} & set(p), sorted(p)
    for name in ("logits", "token"):
        np.testing.assert_array_equal(np.load(os.path.join(plain_dump, name + ".npy")), np.load(os.path.join(dump, name + ".npy")))
    # --dump-outputs: what the last timed step returned, its greedy token being the argmax of its logits
    lg, tk = np.load(os.path.join(dump, "logits.npy")), np.load(os.path.join(dump, "token.npy"))
    assert lg.dtype == np.float32 and lg.shape == (synth.BY_NAME["llama-3.2-3b"].V,) and np.isfinite(lg).all()
    assert tk.dtype == np.float64 and tk.shape == (1,) and int(tk[0]) == int(np.argmax(lg))
    cb = d["cpu_baseline"]
    tol = 5e-4 * max(1.0, cb["max_abs_logit"])             # observed 4e-5 at 3B fp16 (logits are O(1) here), 2.3e-5 as Q4_K_M
    assert cb["kind"] == "port" and cb["max_abs_logit_diff_vs_gpu_token0"] <= tol
    # positions 0..5 through all 28 blocks (multi-position attention at full size), greedy tokens identical at every step
    assert cb["positions_compared"] == 6 and len(cb["max_abs_logit_diff_vs_gpu_by_position"]) == 6 and cb["max_abs_logit_diff_vs_gpu"] <= tol
    assert all(cb["greedy_tokens_equal_by_position"]) and cb["value_1core"] > 0
    chk = d["prefill"]["check"]
    assert chk["same_argmax"] and chk["max_abs_logit_diff"] <= chk["tolerance"]
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and 0.3 < rf["frac"] < 1.0   # (`traffic` is a committed offline PMC figure, labelled so: nothing to assert on)
    assert abs(rf["frac_of_measured_ceiling"] * rf["measured_ceiling"] - rf["frac"] * rf["peak"]) < 1e-6 * rf["achieved"]
    classes = {k["class"]: k for k in rf["kernels"]}
    assert {"qkv", "gateup", "down", "lmhead"} <= set(classes) and all(0.02 < k["frac"] < 1.0 for k in rf["kernels"]), rf["kernels"]
    assert sum(k["us_per_launch"] * k["launches_per_token"] for k in rf["kernels"]) <= 1.15e3 * d["ms_per_step"]   # the kernels fit the token (replay timing: a few % over)
    assert d["n_gpus"] == 1 and d["steps"] == 16 and d["value"] > 100
    sp = d["sampling_path"]
    assert sp["sampling_path_tokens_per_s"] > 50 and sp["blocking_greedy_tokens_per_s"] > 50
    assert d["short_context"]["tokens_per_s"] >= 0.9 * d["value"]    # a shorter context is never much slower (16 timed steps: noisy)
    if quant != "f16":
        assert "configs" not in d
        return
    cfgs = d["configs"]
    assert len(cfgs) == 3 and not any("error" in c for c in cfgs), [c.get("error") for c in cfgs]
    for c, needle, floor in zip(cfgs, ("llama-3.2-3b Q4_K_M", "llama-3.2-1b fp16", "llama-3.1-8b Q4_K_M"), (500, 700, 500)):
        assert needle in c["workload"] and c["value"] > floor and c["steps"] == 64, c["workload"]
        assert 0.05 < c["token_hbm_frac_of_peak"] < 1.0 and 0.05 < c["roofline"]["frac"] < 1.0
        assert abs(c["bytes_per_token"] / (c["ms_per_step"] * 1e-3) / 1e9 - c["token_hbm_gbps"]) < 1e-6 * c["token_hbm_gbps"]
        pv = c["parity_vs_oracle"]
        assert pv["positions_compared"] >= 4 and all(pv["greedy_tokens_equal_by_position"])
        assert pv["max_abs_logit_diff"] <= 5e-4 * max(1.0, pv["max_abs_logit"]), pv
        assert c["prefill"]["check"]["same_argmax"]
    assert "blocks [28,32) of 32" in cfgs[2]["workload"]


def _timed_region_run(quant, T=512, G=8):
    """The benchmark's timed region on the whole Llama-3.2-3B with bench.py's weights (same generator, same seed): a T-token
    prompt through the MFMA prefill, then G greedy tokens on the decode path.  -> (weights, prompt, [G + 1 logit vectors], tokens)."""
    import torch
    import bench as B
    from nfai_amd import _lib
    from nfai_amd.hip import HipBufferManager
    from nfai_amd.llama_model import LlamaModel
    dims = synth.LLAMA_32_3B
    torch.cuda.set_device(0)
    weights = B.gen_weights_hbm(torch, dims, (0, dims.L), True, True, quant=quant)
    mgr = HipBufferManager(0)
    C = T + G + 1
    m = LlamaModel(mgr, synth.make_metadata(dims), B.as_model_tensors(_lib, weights), C, max_batch=T,
                   dims=dict(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, eps=1e-5, rope_dims=dims.D, rope_base=500000.0))
    prompt = synth.make_tokens(dims, T, seed=99)
    prompt[0] = 128000 % dims.V
    got = [m.Prefill(prompt)]
    toks = [int(np.argmax(got[0]))]
    for _ in range(G):
        lg, am = m.Step(toks[-1])
        got.append(lg)
        toks.append(am)
    assert m.Pos == T + G
    m.Dispose()
    mgr.Dispose()
    return weights, prompt, got, toks


def _timed_region_child(quant, out_dir):
    """Child-process side of test_timed_region_full_depth_against_the_oracle (switches read once per process, e.g.
    NFAI_PREFILL_FUSED): the G + 1 logit vectors and the greedy tokens -> out_dir/logits.npy, tokens.npy."""
    import os
    weights, _, got, toks = _timed_region_run(quant)
    del weights
    np.save(os.path.join(out_dir, "logits.npy"), np.stack(got))
    np.save(os.path.join(out_dir, "tokens.npy"), np.array(toks, np.int64))


@pytest.mark.parametrize("quant", ["f16", "q4_k_m"])
def test_timed_region_full_depth_against_the_oracle(quant, tmp_path):
    """the benchmark's own timed region against the oracle at full depth — the whole Llama-3.2-3B (28 blocks,
    V = 128256), a 512-token prompt through the MFMA prefill, then 8 greedy tokens on the decode path (positions 512..519), against
    `OracleLlama` fed the same 520 tokens one by one in fp32 (the reference's loop, LlamaModel.cs:103-126; ~60 s on 16 host
    threads).  The prefill rounds its GEMM operands to fp16, so the bar is the stated fp16 tolerance on the logits
    (2e-2 * max(1, max|logit|), about 1e-1 absolute here) with identical greedy tokens at every step; the oracle skips the lm_head for the prompt.
    Also as Q4_K_M (bench.py --quant q4_k_m: the oracle multiplies the dequantised weights), in both prefill forms: the default one
    that widens each block's K-quant matrices to fp16 for the direct-to-LDS GEMMs (in this process) and the dequant-in-LDS GEMMs of
    NFAI_PREFILL_FUSED=1 (read once per process: a child process, running while this one computes the one oracle pass)."""
    import os
    import subprocess
    import sys
    import bench as B
    dims = synth.LLAMA_32_3B
    T, G = 512, 8
    C = T + G + 1
    weights, prompt, got, toks = _timed_region_run(quant, T, G)
    forms = {"default": (got, toks)}
    child = None
    if quant != "f16":
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
        env["NFAI_PREFILL_FUSED"] = "1"
        code = (f"import sys; sys.path[:0] = [{root!r}, {os.path.join(root, 'tests')!r}]; import test_gpu_model as t; "
                f"t._timed_region_child({quant!r}, {str(tmp_path)!r})")
        child = subprocess.Popen([sys.executable, "-c", code], env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    try:
        ref = orc.OracleLlama(odesc(dims, C), B.host_weights(weights))
        del weights
        for t in prompt[:-1]:
            ref.step(int(t), want_logits=False)
        wants = [ref.step(int(prompt[-1]))]
        for i in range(G):
            wants.append(ref.step(toks[i]))
    finally:
        if child is not None:
            try:
                out, _ = child.communicate(timeout=900)
            except subprocess.TimeoutExpired:
                child.kill()
                out = child.communicate()[0] + "\n(child killed at its 900 s limit)"
    if child is not None:
        assert child.returncode == 0, out[-4000:]
        forms["fused"] = (list(np.load(tmp_path / "logits.npy")), np.load(tmp_path / "tokens.npy").tolist())
    for form, (got, toks) in forms.items():
        worst = 0.0
        for i in range(G + 1):
            want = wants[i]
            err, scale = float(np.abs(got[i] - want).max()), max(1.0, float(np.abs(want).max()))
            worst = max(worst, err / scale)
            top2 = np.sort(want)[-2:]
            assert err <= 2e-2 * scale, (form, i, err, scale)
            assert orc.argmax(want) == toks[i], (form, i, orc.argmax(want), toks[i], "oracle top-1 / top-2 margin", float(top2[1] - top2[0]))
        print(f"full-depth timed region ({quant}, {form} prefill): worst max|dlogit| / max(1, max|logit|) over {G + 1} positions = {worst:.3g}")


@pytest.mark.parametrize("dims", [synth.LLAMA_32_3B, synth.LLAMA_32_1B], ids=lambda d: d.name)
def test_decode_is_bit_reproducible(mgr, dims):
    """The hand-offs inside the launches (attention slices, attention -> Wo) are ordered by data, not by arrival: the same 150
    tokens twice (after a reset) and on a second model instance must give bit-identical logits at every step — slice merges
    run in fixed slice order whatever block publishes first."""
    from dataclasses import replace
    from nfai_amd.llama_model import LlamaModel
    d2 = replace(dims, L=2, V=2048, name=dims.name + "-2blk")
    w = synth.make_weights(d2, seed=41)
    toks = synth.make_tokens(d2, 150, seed=17)
    m = LlamaModel(mgr, synth.make_metadata(d2), w, 160)
    first = [m.Step(int(t))[0].copy() for t in toks]
    m.Reset()
    for i, t in enumerate(toks):
        assert np.array_equal(m.Step(int(t))[0], first[i]), i
    m2 = LlamaModel(mgr, synth.make_metadata(d2), w, 160, graph=False)
    for i, t in enumerate(toks):
        assert np.array_equal(m2.Step(int(t))[0], first[i]), i
    m.Dispose()
    m2.Dispose()


def test_chunked_ingest_full_width_and_depth():
    """RunAsync's prompt sequence on the whole Llama-3.2-1B (16 blocks, fp16, V = 128256): a model with max_batch = 256 ingests the
    first 699 tokens of a 700-token prompt (nfai_hip_llama_ingest: chunks of 256, 256 and a ragged 187, the second and third
    attending across the K / V rows the earlier ones cached), steps the last prompt token, then 8 greedy tokens — against
    `OracleLlama` fed all 708 tokens one by one.  Logits of the 9 sampled steps within the stated fp16 bar (2e-2 * max(1,
    max|logit|)) with identical greedy tokens; K and V rows on both sides of the chunk edges and of the last prompt token, first
    and last layer, within the 2e-2 of test_prefill_mfma_matches_token_by_token."""
    import torch
    import bench as B
    from nfai_amd import _lib
    from nfai_amd.hip import HipBufferManager
    from nfai_amd.llama_model import LlamaModel
    dims = synth.LLAMA_32_1B
    torch.cuda.set_device(0)
    weights = B.gen_weights_hbm(torch, dims, (0, dims.L), True, True, quant="f16", seed=4321)
    n, G = 700, 8
    C = n + G + 4
    mgr = HipBufferManager(0)
    m = LlamaModel(mgr, synth.make_metadata(dims), B.as_model_tensors(_lib, weights), C, max_batch=256,
                   dims=dict(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, eps=1e-5, rope_dims=dims.D, rope_base=500000.0))
    prompt = synth.make_tokens(dims, n, seed=23)
    prompt[0] = 128000
    m.Ingest(prompt[:-1])
    assert m.Pos == n - 1
    got, toks = [], []
    tok = int(prompt[-1])
    for _ in range(G + 1):
        lg, tok = m.Step(tok)
        got.append(lg)
        toks.append(tok)
    assert m.Pos == n + G
    rows = (255, 256, 511, 512, n - 2)
    kv = {(l, v, p): m.ReadKV(l, v, p) for l in (0, dims.L - 1) for v in (False, True) for p in rows}
    m.Dispose()
    mgr.Dispose()
    ref = orc.OracleLlama(odesc(dims, C), B.host_weights(weights))
    del weights
    for t in prompt[:-1]:
        ref.step(int(t), want_logits=False)
    worst = 0.0
    for i, want in enumerate([ref.step(int(prompt[-1]))] + [None] * G):
        if want is None:
            want = ref.step(toks[i - 1])
        err, scale = float(np.abs(got[i] - want).max()), max(1.0, float(np.abs(want).max()))
        worst = max(worst, err / scale)
        top2 = np.sort(want)[-2:]
        assert err <= 2e-2 * scale, (i, err, scale)
        assert orc.argmax(want) == toks[i], (i, orc.argmax(want), toks[i], "oracle top-1 / top-2 margin", float(top2[1] - top2[0]))
    for (l, v, p), row in kv.items():
        np.testing.assert_allclose(row, (ref.vcache(l) if v else ref.kcache(l))[p], rtol=0, atol=2e-2, err_msg=f"layer {l} {'V' if v else 'K'} row {p}")
    print(f"chunked ingest (1B, 256-row chunks): worst max|dlogit| / max(1, max|logit|) over {G + 1} positions = {worst:.3g}")


def _xcd_lib():
    import ctypes as C
    from nfai_amd import _lib
    lib = _lib.load()
    lib.nfai_hip_debug_xcd_shares.argtypes = [_lib.H, C.POINTER(C.c_uint16)]
    lib.nfai_hip_debug_xcd_shares.restype = C.c_int32
    lib.nfai_hip_debug_gemv_dealt.argtypes = []
    lib.nfai_hip_debug_gemv_dealt.restype = C.c_uint64
    return lib


def test_lm_head_dealt_by_forced_shares_at_model_level():
    """The model's lm_head + ArgMax launch with its rows dealt by a forced, skewed share vector (nfai_hip_debug_xcd_shares before
    the model is finalised: the token graph captures the shares), whatever the box's own probe would pick: two blocks at the 3B
    widths with the full 128256-row vocabulary.  A twin on a context with dealing off must give bit-identical logits at 16
    positions and the same greedy tokens (the device loop), both within the end-to-end tolerance of the oracle."""
    import ctypes as C
    from dataclasses import replace
    from nfai_amd.hip import HipBufferManager
    from nfai_amd.llama_model import LlamaModel
    lib = _xcd_lib()
    skewed = (30, 50, 41, 40, 40, 40, 40, 39)
    d2 = replace(synth.LLAMA_32_3B, L=2, name="llama-3.2-3b-2blk-full-vocab")
    w = synth.make_weights(d2, seed=43)
    N, n_ctx = 16, 2 * 16 + 4
    mo, md = HipBufferManager(0), HipBufferManager(0)
    assert lib.nfai_hip_debug_xcd_shares(mo.handle, None) == 0
    assert lib.nfai_hip_debug_xcd_shares(md.handle, (C.c_uint16 * 8)(*skewed)) == 0
    assert mo.XcdShares()[0] == [0] * 8 and md.XcdShares()[0] == list(skewed)
    c0 = lib.nfai_hip_debug_gemv_dealt()
    off = LlamaModel(mo, synth.make_metadata(d2), w, n_ctx)
    g_off = off.Greedy(5, N)
    assert lib.nfai_hip_debug_gemv_dealt() == c0, "a context with dealing off dealt"
    dealt = LlamaModel(md, synth.make_metadata(d2), w, n_ctx)
    g_dealt = dealt.Greedy(5, N)
    assert lib.nfai_hip_debug_gemv_dealt() > c0, "the lm_head of the forced context did not take the XD path"
    ref = orc.OracleLlama(odesc(d2, n_ctx), w)
    tok, want_toks, wants = 5, [], []
    for _ in range(N):
        wants.append(ref.step(tok))
        tok = orc.argmax(wants[-1])
        want_toks.append(tok)
    assert g_dealt.tolist() == g_off.tolist() == want_toks
    off.Reset()
    dealt.Reset()
    for i, t in enumerate([5] + want_toks[:-1]):
        la, aa = off.Step(t)
        lb, ab = dealt.Step(t)
        assert np.array_equal(la, lb) and aa == ab, (i, np.flatnonzero(~(la == lb))[:16])
        assert np.abs(lb - wants[i]).max() <= logit_tol(wants[i]), (i, np.abs(lb - wants[i]).max())
    off.Dispose()
    dealt.Dispose()
    mo.Dispose()
    md.Dispose()
