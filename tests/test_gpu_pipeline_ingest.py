"""The prompt phase of the layer pipeline on the one card of the GPU box: `HipStage(..., max_batch)` x 2 / 3 / 8 driven through
`run_prompt_schedule_in_process` (nfai_hip_llama_stage_ingest: the MFMA prefill per stage, [T][E] hand-off rows), then the decode
schedule.  The K / V rows every stage leaves must match a whole model that ingested the same prompt (nfai_hip_llama_ingest), the
CPU oracle stepping the prompt token by token within the ingest tolerance; the greedy tokens that follow must equal the whole
model's and be the oracle's argmax within the ingest tolerance.
Also: the token-by-token fall-back (max_batch = 0) against n stage steps bit for bit, the whole model against _ingest bit for bit,
the argument errors, and the K-quant fp16 shadow shared by the slots of a stage."""
import ctypes as C

import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth

pytestmark = pytest.mark.gpu

Q4_K, Q6_K = 12, 14


@pytest.fixture(scope="module")
def env():
    import torch
    from nfai_amd.hip import HipBufferManager
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    mgr = HipBufferManager(0, stream=stream.cuda_stream)
    yield torch, stream, mgr
    mgr.Dispose()


def _device_weights(torch, dims, quant, seed=81):
    """name -> (device tensor, ggml type, rows, cols) as HipStage takes them, plus the host weights the oracle takes."""
    w = synth.make_weights(dims, seed=seed, std=0.05)
    dev, host = {}, {}
    for name, a in w.items():
        if a.ndim == 1:
            dev[name] = (torch.from_numpy(a).cuda(), 0, 1, a.shape[0])
            host[name] = a
        elif quant:
            qt = Q6_K if name.endswith(("attn_v.weight", "ffn_down.weight")) or name.startswith(("token_embd", "output.")) else Q4_K
            f = a.astype(np.float32)
            raw = orc.quantize_q4k(f) if qt == Q4_K else orc.quantize_q6k(f)
            deq = (orc.dequant_q4k if qt == Q4_K else orc.dequant_q6k)(raw, a.size).reshape(a.shape)
            dev[name] = (torch.from_numpy(np.ascontiguousarray(raw)).cuda(), qt, a.shape[0], a.shape[1])
            host[name] = deq
        else:
            dev[name] = (torch.from_numpy(a).cuda(), 1, a.shape[0], a.shape[1])
            host[name] = a
    return dev, host


def _stage_weights(dev, dims, lb, le, first, last):
    out = {}
    for name, t in dev.items():
        if name.startswith("blk."):
            if lb <= int(name.split(".")[1]) < le:
                out[name] = t
        elif name == "token_embd.weight":
            if first or (last and dims.tied):
                out[name] = t
        elif last:
            out[name] = t
    return out


def _desc(dims):
    return dict(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, eps=1e-5, rope_dims=dims.D, rope_base=500000.0)


def _whole(mgr, dims, dev, C, max_batch, share_from=None):
    from nfai_amd.llama_model import LlamaModel
    tens = {k: (t.data_ptr(), ty, rows, cols) for k, (t, ty, rows, cols) in dev.items()}
    return LlamaModel(mgr, {"general.name": dims.name}, tens, C, dims=_desc(dims), max_batch=max_batch, share_from=share_from)


def _stages(torch, mgr, dims, dev, ranges, n_slots, C, max_batch):
    from nfai_amd.pipeline import HipStage
    world = len(ranges)
    return [HipStage(torch, mgr, dims, (lb, le), _stage_weights(dev, dims, lb, le, r == 0, r == world - 1), n_slots, C, r, world,
                     max_batch=max_batch) for r, (lb, le) in enumerate(ranges)]


LENGTHS = [1, 63, 64, 65, 150]   # prompt tokens in front of the sampled one: one row, ragged and exact chunks of 64, three chunks


@pytest.mark.parametrize("quant", [False, True], ids=["f16", "q4_k_m"])
@pytest.mark.parametrize("world", [2, 3, 8])
def test_stage_prompts_equal_one_device(env, world, quant):
    torch, stream, mgr = env
    from dataclasses import replace
    from nfai_amd.pipeline import partition_layers, run_prompt_schedule_in_process, run_schedule_in_process
    dims = synth.TINY_D128
    if world == 8:
        dims = replace(dims, L=8, name=dims.name + "-8blk")
    n_slots, n_steps, mb = len(LENGTHS), 8, 64
    C = max(LENGTHS) + 1 + n_steps + 1
    rng = np.random.default_rng(world * 10 + int(quant))
    prompts = [[int(t) for t in rng.integers(0, dims.V, n + 1)] for n in LENGTHS]
    dec_slots = min(world, n_slots)      # the decode schedule keeps at most `world` sequences in flight
    with torch.cuda.stream(stream):
        dev, host = _device_weights(torch, dims, quant)
        ranges = partition_layers(dims.L, world)
        stages = _stages(torch, mgr, dims, dev, ranges, n_slots, C, mb)
        run_prompt_schedule_in_process(stages, [p[:-1] for p in prompts], mb, lambda dst, src: dst.copy_(src))
        for st in stages:
            assert [m.Pos for m in st.models] == LENGTHS
        stage_kv = {}
        for r, (lb, le) in enumerate(ranges):
            for s in range(n_slots):
                for l in range(lb, le):
                    for p in range(LENGTHS[s]):
                        stage_kv[(s, l, p)] = (stages[r].models[s].ReadKV(l, False, p), stages[r].models[s].ReadKV(l, True, p))
        run_schedule_in_process(stages, n_steps, [p[-1] for p in prompts[:dec_slots]], lambda dst, src: dst.copy_(src), n_slots=dec_slots)
        stream.synchronize()
        got = [stages[-1].models[s].FetchTokens(n_steps).tolist() for s in range(dec_slots)]
        whole = _whole(mgr, dims, dev, C, mb)
        want_dev = []
        for s, prompt in enumerate(prompts):
            whole.Reset()
            whole.Ingest(prompt[:-1])
            for l in range(dims.L):
                for p in range(LENGTHS[s]):
                    k, v = stage_kv[(s, l, p)]
                    np.testing.assert_allclose(k, whole.ReadKV(l, False, p), rtol=0, atol=1e-4, err_msg=f"slot {s} layer {l} pos {p} K")
                    np.testing.assert_allclose(v, whole.ReadKV(l, True, p), rtol=0, atol=1e-4, err_msg=f"slot {s} layer {l} pos {p} V")
            if s < dec_slots:
                want_dev.append(whole.Greedy(prompt[-1], n_steps).tolist())
        whole.Dispose()
        for st in stages:
            st.dispose()
    desc = orc.LlamaDesc(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, C=C)
    for s, prompt in enumerate(prompts):
        ref = orc.OracleLlama(desc, host)
        for t in prompt[:-1]:
            ref.step(t)
        for l in range(dims.L):
            kc, vc = ref.kcache(l), ref.vcache(l)
            for p in range(LENGTHS[s]):
                k, v = stage_kv[(s, l, p)]
                np.testing.assert_allclose(k, kc[p], rtol=0, atol=2e-2, err_msg=f"slot {s} layer {l} pos {p} K vs oracle")
                np.testing.assert_allclose(v, vc[p], rtol=0, atol=2e-2, err_msg=f"slot {s} layer {l} pos {p} V vs oracle")
        if s < dec_slots:
            # the stages decode exactly what the whole model decodes after its own _ingest; against the oracle (fp32, token by token)
            # each token must be the oracle's argmax up to the ingest tolerance (the oracle follows the device's tokens: a near-tie the
            # fp16 prompt rows resolve the other way is the documented precision trade of _ingest, not a stage error)
            assert got[s] == want_dev[s], (s, got[s], want_dev[s])
            tok = prompt[-1]
            for i, g in enumerate(got[s]):
                lg = ref.step(tok)
                tol = 2e-2 * max(1.0, float(np.abs(lg).max()))
                assert lg[g] >= lg.max() - tol, (s, i, g, orc.argmax(lg), float(lg.max() - lg[g]))
                tok = g


@pytest.mark.parametrize("model,quant", [("llama-3.2-3b", "f16"), ("llama-3.1-8b", "q4_k_m")])
def test_two_stages_full_width(env, model, quant):
    """Two stages at the real widths (four blocks, vocabulary cut to 2048), a 512-token prompt in chunks of 256 (the long-chunk
    K-split of Wdown whose combine the stage boundary finishes): K / V rows of the boundary layers against the whole model's
    _ingest, and the 8 greedy tokens that follow."""
    torch, stream, mgr = env
    from dataclasses import replace
    import bench as B
    from nfai_amd.pipeline import partition_layers, pipeline_costs, run_prompt_schedule_in_process, run_schedule_in_process
    dims = replace(synth.BY_NAME[model], L=4, V=2048, name=model + "-4blk")
    n_steps, mb, n = 8, 256, 512
    C = n + n_steps + 8
    ranges = partition_layers(dims.L, 2, *pipeline_costs(dims, quant))
    prompt = [int(t) for t in np.random.default_rng(3).integers(0, dims.V, n)]
    with torch.cuda.stream(stream):
        dev = B.gen_weights_hbm(torch, dims, (0, dims.L), True, True, seed=21, quant=quant)
        stages = _stages(torch, mgr, dims, dev, ranges, 1, C, mb)
        run_prompt_schedule_in_process(stages, [prompt[:-1]], mb, lambda dst, src: dst.copy_(src))
        layers = sorted({ranges[0][1] - 1, ranges[1][0], dims.L - 1})
        kv = {(l, p, v): stages[0 if l < ranges[0][1] else 1].models[0].ReadKV(l, v, p) for l in layers for p in range(n - 1) for v in (False, True)}
        run_schedule_in_process(stages, n_steps, [prompt[-1]], lambda dst, src: dst.copy_(src), n_slots=1)
        stream.synchronize()
        got = stages[-1].models[0].FetchTokens(n_steps).tolist()
        whole = _whole(mgr, dims, dev, C, mb)
        whole.Ingest(prompt[:-1])
        worst = 0.0
        for (l, p, v), row in kv.items():
            want = whole.ReadKV(l, v, p)
            err = float(np.abs(row - want).max()) / max(1.0, float(np.abs(want).max()))
            worst = max(worst, err)
            assert err <= 1e-4, (l, p, v, err)
        want_tok = whole.Greedy(prompt[-1], n_steps).tolist()
        whole.Dispose()
        for st in stages:
            st.dispose()
    assert got == want_tok, (got, want_tok)
    print(f"{model} {quant}: stages {ranges}, worst scaled |dK/V| = {worst:.3g}")


@pytest.mark.parametrize("quant", [False, True], ids=["f16", "q4_k_m"])
def test_fallback_is_n_stage_steps(env, quant):
    """max_batch = 0: stage ingest of n tokens computes exactly what n nfai_hip_llama_stage_step calls compute (K / V rows and the
    hidden rows handed on), on every stage of a 3-stage pipeline."""
    torch, stream, mgr = env
    from nfai_amd.pipeline import partition_layers
    dims, n, C = synth.TINY_D128, 7, 16
    toks = [int(t) for t in np.random.default_rng(5).integers(0, dims.V, n)]
    with torch.cuda.stream(stream):
        dev, _ = _device_weights(torch, dims, quant)
        ranges = partition_layers(dims.L, 3)
        stages = _stages(torch, mgr, dims, dev, ranges, 2, C, 0)
        g = torch.Generator(device="cuda")
        g.manual_seed(9)
        rows_in = torch.randn((n, dims.E), device="cuda", generator=g)
        for r, st in enumerate(stages):
            a, b = st.models                                       # a: one stage_ingest call, b: n stage steps
            last = r == len(stages) - 1
            out_a = None if last else torch.zeros((n, dims.E), device="cuda")
            out_b = None if last else torch.zeros((n, dims.E), device="cuda")
            if r == 0:
                a.StageIngest(toks, None, out_a.data_ptr())
                for i in range(n):
                    b.StageStep(toks[i], None, out_b[i].data_ptr())
            else:
                a.StageIngest(None, rows_in.data_ptr(), None if last else out_a.data_ptr(), n)
                for i in range(n):
                    b.StageStep(0, rows_in[i].data_ptr(), None if last else out_b[i].data_ptr())
            stream.synchronize()
            assert a.Pos == b.Pos == n
            if not last:
                assert np.array_equal(out_a.cpu().numpy(), out_b.cpu().numpy()), r
            lb, le = ranges[r]
            for l in range(lb, le):
                for p in range(n):
                    for v in (False, True):
                        assert np.array_equal(a.ReadKV(l, v, p), b.ReadKV(l, v, p)), (r, l, p, v)
        for st in stages:
            st.dispose()


@pytest.mark.parametrize("max_batch", [0, 64])
def test_whole_model_stage_ingest_is_ingest(env, max_batch):
    torch, stream, mgr = env
    dims, n, C = synth.TINY_D128, 90, 112
    toks = [int(t) for t in np.random.default_rng(6).integers(0, dims.V, n)]
    with torch.cuda.stream(stream):
        dev, _ = _device_weights(torch, dims, True)
        a = _whole(mgr, dims, dev, C, max_batch)
        b = _whole(mgr, dims, dev, C, max_batch, share_from=a)
        a.Ingest(toks)
        b.StageIngest(toks)
        assert a.Pos == b.Pos == n
        for l in range(dims.L):
            for p in range(n):
                for v in (False, True):
                    assert np.array_equal(a.ReadKV(l, v, p), b.ReadKV(l, v, p)), (l, p, v)
        assert a.Greedy(5, 6).tolist() == b.Greedy(5, 6).tolist()
        b.Dispose()
        a.Dispose()


def test_stage_ingest_errors(env):
    torch, stream, mgr = env
    from nfai_amd import _lib
    from nfai_amd.pipeline import partition_layers
    dims, C = synth.TINY_D128, 16
    with torch.cuda.stream(stream):
        dev, _ = _device_weights(torch, dims, False)
        stages = _stages(torch, mgr, dims, dev, partition_layers(dims.L, 3), 1, C, 64)
        first, mid, last = (st.models[0] for st in stages)
        rows = torch.zeros((C + 1, dims.E), device="cuda")
        first.StageIngest([1, 2, 3], None, rows.data_ptr())
        mid.StageIngest(None, rows.data_ptr(), rows.data_ptr(), 3)
        stream.synchronize()
        cases = [
            (first, _lib.KVCacheFull, lambda: first.StageIngest([1] * (C - 2), None, rows.data_ptr())),
            (first, _lib.NfaiHipError, lambda: first.StageIngest([1, dims.V], None, rows.data_ptr())),
            (first, _lib.NfaiHipError, lambda: first.StageIngest([1, 2], rows.data_ptr(), rows.data_ptr())),
            (mid, _lib.NfaiHipError, lambda: mid.StageIngest(None, None, rows.data_ptr(), 2)),
            (mid, _lib.NfaiHipError, lambda: mid.StageIngest([1, 2], rows.data_ptr(), rows.data_ptr())),
            (mid, _lib.NfaiHipError, lambda: mid.StageIngest(None, rows.data_ptr(), None, 2)),
            (last, _lib.NfaiHipError, lambda: last.StageIngest(None, rows.data_ptr(), rows.data_ptr(), 2)),
            (last, _lib.KVCacheFull, lambda: last.StageIngest(None, rows.data_ptr(), None, C + 1)),
        ]
        for m, exc, fn in cases:
            before = m.Pos
            with pytest.raises(exc) as ei:
                fn()
            assert ei.value.code == (_lib.ERR_KV_FULL if exc is _lib.KVCacheFull else _lib.ERR_INVALID)
            assert m.Pos == before
        last.StageIngest(None, rows.data_ptr(), None, 0)           # n == 0: nothing to do
        assert last.Pos == 0
        for st in stages:
            st.dispose()


def _shadow(m):
    from nfai_amd import _lib
    lib = _lib.load()
    lib.nfai_hip_debug_prefill_shadow.argtypes = [_lib.H, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.nfai_hip_debug_prefill_shadow.restype = C.c_int32
    p, b = C.c_void_p(), C.c_uint64()
    assert lib.nfai_hip_debug_prefill_shadow(m.handle, C.byref(p), C.byref(b)) == 0
    return p.value, b.value


def test_slots_share_the_kquant_shadow(env):
    """Two slots of a Q4_K_M stage over one donor's weights: after both ingest, both report the donor's fp16 copy (same address,
    same size) — the second slot widened nothing of its own."""
    torch, stream, mgr = env
    from nfai_amd.pipeline import partition_layers
    dims, C, n = synth.TINY_D128, 80, 70
    with torch.cuda.stream(stream):
        dev, _ = _device_weights(torch, dims, True)
        ranges = partition_layers(dims.L, 2)
        stages = _stages(torch, mgr, dims, dev, ranges, 2, C, 64)
        st = stages[1]
        a, b = st.models
        assert _shadow(a) == (None, 0) and _shadow(b) == (None, 0)
        rows = torch.randn((n, dims.E), device="cuda")
        a.StageIngest(None, rows.data_ptr(), None, n)
        b.StageIngest(None, rows.data_ptr(), None, n)
        stream.synchronize()
        pa, ba = _shadow(a)
        pb, bb = _shadow(b)
        blocks = ranges[1][1] - ranges[1][0]
        per_block = 2 * (dims.H * dims.D * dims.E + 2 * dims.Hkv * dims.D * dims.E + dims.E * dims.H * dims.D + 3 * dims.F * dims.E)
        assert pa and pa == pb and ba == bb and ba >= blocks * per_block
        for l in range(*ranges[1]):
            assert np.array_equal(a.ReadKV(l, False, n - 1), b.ReadKV(l, False, n - 1))
        for s in stages:
            s.dispose()
