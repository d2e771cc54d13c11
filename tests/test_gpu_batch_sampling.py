"""Sampled batched decode on the GPU: the row-batched candidate launch (nfai_hip_topk_rows), a batch step that returns every member's
TopP candidates (nfai_hip_llama_batch_step_topk) and the token loop of n conversations (LlamaBatch.RunTokens / RunAsync).

Bounds.  A row's candidates are BIT-IDENTICAL to nfai_hip_topk on the same vector: the rows launch runs the same device body with the
same range partition and the same order of sums, so no tolerance applies.  Against the oracle's restatement of SamplingUtils.TopP the
indices are exact and the probabilities agree to 1e-6 relative, the bound tests/test_gpu_ops.py::test_topk_candidates uses for the
single-vector launch (device expf and the order of the sum differ from the host's)."""
import ctypes as C

import numpy as np
import pytest

import oracle as orc
from nfai_amd import synth
from test_gpu_batch_decode import dispose, make_members, seq_tokens
from test_gpu_batch_quant import make_members as make_members_q
from test_gpu_batch_quant import quant_weights

pytestmark = pytest.mark.gpu

CAP = 96
U32P, F32P = C.POINTER(C.c_uint32), C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


def hval(h):
    return h.value if hasattr(h, "value") else int(h)


_props = {}


def prop(mgr, n, slot=0):
    """A device vector of n floats, kept per (n, slot) for the module."""
    from nfai_amd.hip import ShaderProperty
    key = (id(mgr), n, slot)
    if key not in _props:
        _props[key] = ShaderProperty(mgr, n)
    return _props[key]


def topk_single(mgr, v, temperature, k, slot=0):
    """nfai_hip_topk on the host vector v."""
    from nfai_amd._lib import call
    p = prop(mgr, v.size, slot)
    p.SetValue(v)
    ids, probs = np.empty(k, np.uint32), np.empty(k, np.float32)
    call("nfai_hip_topk", mgr.handle, p.handle, v.size, temperature, k, ids.ctypes.data_as(U32P), probs.ctypes.data_as(F32P))
    return ids, probs


def topk_rows(mgr, handles, n, temperature, k, rows=None):
    from nfai_amd import _lib
    from nfai_amd._lib import call
    rows = len(handles) if rows is None else rows
    hs = (_lib.H * max(len(handles), 1))(*[hval(h) for h in handles])
    ids, probs = np.empty((max(rows, 1), max(k, 1)), np.uint32), np.empty((max(rows, 1), max(k, 1)), np.float32)
    call("nfai_hip_topk_rows", mgr.handle, hs, rows, n, temperature, k, ids.ctypes.data_as(U32P), probs.ctypes.data_as(F32P))
    return ids, probs


def bit_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
DUP_ROW, DUP_OF, FLAT_ROW = 5, 2, 6   # in the 8-row cases row 5 names row 2's buffer; at n = 32000 and 128256 row 6 holds n equal values
LDS_CAP = 4096                        # candidates the last workgroup ranks in LDS (TOPK_LDS_CAP); more take the slow ranking path


def flat_candidates(n, k):
    """How many candidates a vector of n EQUAL values leaves, from the launch's range partition (topk_blocks, common.h): 256 threads
    of 8 logits per block, at least min(ceil(n / 256), 128) blocks, 4 waves per block, wave g owning [g cw, (g + 1) cw).  Every head
    is the first index of its range, the order is (value descending, index ascending), so tau is the head of range k - 1 and the
    candidates are the indices 0 .. (k - 1) cw."""
    blocks = min(1024, max(-(-n // 2048), min(-(-n // 256), 128), 1))
    nw = 4 * blocks
    cw = -(-n // nw)
    return n if nw < k else (k - 1) * cw + 1


def row_vector(n, r, seed):
    """3 N(0, 1) with the ties of test_topk_candidates, at indices that differ per row."""
    v = (3.0 * np.random.Generator(np.random.PCG64(1000 * seed + r)).standard_normal(n)).astype(np.float32)
    if n >= 1000:
        v[[n - 1 - r, 77 + r, n // 2 + 3 + r]] = v.max() + 0.75        # equal maxima in three different workgroups
        v[[5 + r, n // 3 + r, n // 3 + 1 + r]] = np.sort(v)[-20]      # a tie inside the top-k
    return v


@pytest.mark.parametrize("rows,n,k,temperature", [(1, 40, 40, 0.7), (3, 65, 1, 0.5), (8, 1000, 40, 0.5), (5, 4100, 40, 0.5),
                                                  (8, 32000, 40, 0.5), (2, 128256, 64, 1.0), (8, 128256, 40, 0.5)])
def test_rows_match_the_single_row_launch_and_the_oracle(mgr, rows, n, k, temperature):
    """Every row of one nfai_hip_topk_rows call is bit-identical to nfai_hip_topk on that row, and is what the oracle's TopP forms
    (indices exact, probabilities to 1e-6 relative); three rounds of two calls per shape on the same slices (slice 0's counters are
    only ever re-armed by the launch; the entry point zeroes those of the other slices, whose re-arming the batch steps of test 2 rely
    on: a batch zeroes its workspace once).  The rows are separate allocations; in the 8-row cases one buffer is named twice.  A row of n equal values: at n = 128256 (128
    blocks, 512 ranges of 251) it leaves 39 * 251 + 1 = 9790 candidates, past the LDS staging (4096), so that row's last workgroup
    takes the slow ranking path next to rows on the fast path; at n = 32000 (ranges of 64) it leaves 2497 and stays on the fast one."""
    from nfai_amd import _lib
    vs = [row_vector(n, r, rows) for r in range(rows)]
    if rows == 8 and n >= 5000:
        vs[FLAT_ROW] = np.full(n, 1.25, np.float32)
        assert flat_candidates(n, k) == {32000: 2497, 128256: 9790}[n]
        assert (flat_candidates(n, k) > LDS_CAP) == (n == 128256)   # the slow path runs in the (8, 128256) case
    owner = [DUP_OF if (rows == 8 and r == DUP_ROW) else r for r in range(rows)]
    for rep in range(3):
        for r in range(rows):
            if owner[r] == r:
                prop(mgr, n, 1 + r).SetValue(vs[r])
        handles = [prop(mgr, n, 1 + owner[r]).handle for r in range(rows)]
        ids, probs = topk_rows(mgr, handles, n, temperature, k)
        again = topk_rows(mgr, handles, n, temperature, k)   # back to back on the same slices
        assert np.array_equal(again[0], ids) and bit_equal(again[1], probs), rep
        for r in range(rows):
            v = vs[owner[r]]
            ids1, probs1 = topk_single(mgr, v, temperature, k)
            assert np.array_equal(ids[r], ids1) and bit_equal(probs[r], probs1), (rep, r)
            _, ids_ref, probs_ref, _ = orc.topp(v, temperature, 0.95, k, 0.0)
            np.testing.assert_array_equal(ids[r], ids_ref)
            np.testing.assert_allclose(probs[r], probs_ref, rtol=1e-6)
        vs = [np.roll(v, (12345 + 17 * r) % n) for r, v in enumerate(vs)]
    # the predicates of nfai_hip_topk, plus the row count, a dead buffer and a buffer shorter than n
    handles = [prop(mgr, n, 1 + owner[r]).handle for r in range(rows)]
    for bad_rows in (0, 9):
        with pytest.raises(_lib.NfaiHipError):
            topk_rows(mgr, (handles * 9)[:9], n, temperature, k, rows=bad_rows)
    for bad_t, bad_k in ((temperature, 0), (temperature, 65), (temperature, n + 1), (0.0, k), (-1.0, k)):
        with pytest.raises(_lib.NfaiHipError):
            topk_rows(mgr, handles, n, bad_t, bad_k)
    with pytest.raises(_lib.NfaiHipError, match="invalid buffer handle"):
        topk_rows(mgr, handles[:-1] + [987654321], n, temperature, k)
    with pytest.raises(_lib.NfaiHipError, match="needs"):
        topk_rows(mgr, handles, n + 1, temperature, min(k, n))
    ids2, probs2 = topk_rows(mgr, handles, n, temperature, k)   # and the next valid call is what it was
    assert np.array_equal(ids2, ids) and bit_equal(probs2, probs)


def test_rows_after_other_sizes_in_the_same_scratch(mgr):
    """The context's top-k scratch is shared by every n and by the single-vector entry point: rows of one n after rows of another
    n, and after a single-vector call whose lists covered the place of their slices, still find their counters armed."""
    for n, rows in ((128256, 8), (1000, 8), (4100, 5), (128256, 2), (1000, 3)):
        vs = [row_vector(n, r, 77) for r in range(rows)]
        for r in range(rows):
            prop(mgr, n, 1 + r).SetValue(vs[r])
        topk_single(mgr, row_vector(128256, 0, 78), 0.5, 40)     # the largest single-vector workspace in front of the rows
        ids, probs = topk_rows(mgr, [prop(mgr, n, 1 + r).handle for r in range(rows)], n, 0.5, 40)
        for r in range(rows):
            ids1, probs1 = topk_single(mgr, vs[r], 0.5, 40)
            assert np.array_equal(ids[r], ids1) and bit_equal(probs[r], probs1), (n, r)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
def staggered(ms, dims, n):
    """Member s takes its first 5 + 7 s tokens alone (tests/test_gpu_batch_decode.py)."""
    toks = [seq_tokens(dims, s) for s in range(n)]
    for s in range(n):
        for t in toks[s][:5 + 7 * s]:
            ms[s].Step(int(t), want_logits=False)
    return toks


def check_candidates(mgr, ms, V, ids, probs, temperature, k, where):
    """The batch's candidates are nfai_hip_topk's on every member's own logits, read back and uploaded again; -> those logits."""
    own = []
    for s, m in enumerate(ms):
        lg = m.Read(4, V)
        ids1, probs1 = topk_single(mgr, lg, temperature, k)
        assert np.array_equal(ids[s], ids1) and bit_equal(probs[s], probs1), (where, s)
        own.append(lg)
    return own


CASES = [(d, n, False) for d in (synth.TINY, synth.TINY_D128) for n in (1, 2, 5, 8)] + [(synth.TINY_D128, 3, True)]


@pytest.mark.parametrize("dims,n,quant", CASES, ids=lambda v: getattr(v, "name", str(v)))
def test_a_batch_steps_candidates_are_those_of_its_own_logits(mgr, dims, n, quant):
    """12 StepTopK(tokens, 0.5, 40) steps of a staggered batch (fp16, and a Q4_K / Q6_K mix of 3): after each, every member's
    candidates are bit-equal to nfai_hip_topk on its read-back logits, the token TopPFromCandidates draws for a fixed `rand` is the
    oracle's TopP on those logits, and its position advanced by one.  The drawn tokens are fed back, as RunTokens does."""
    from nfai_amd.llama_model import LlamaBatch, SamplingUtils
    w = synth.make_weights(dims, seed=21, std=0.05)
    ms = make_members_q(mgr, dims, quant_weights(w)[0], n, CAP) if quant else make_members(mgr, dims, w, n, CAP)
    toks = staggered(ms, dims, n)
    batch = LlamaBatch(ms, quantized=quant)
    feed = [int(toks[s][5 + 7 * s]) for s in range(n)]
    rands = np.random.Generator(np.random.PCG64(9)).random((12, n), dtype=np.float32)
    for i in range(12):
        ids, probs = batch.StepTopK(feed, 0.5, 40)
        assert ids.shape == (n, 40) and ids.dtype == np.uint32 and probs.shape == (n, 40) and probs.dtype == np.float32
        own = check_candidates(mgr, ms, dims.V, ids, probs, 0.5, 40, f"step {i}")
        for s in range(n):
            got = SamplingUtils.TopPFromCandidates(ids[s], probs[s], 0.95, rand=float(rands[i, s]))
            assert got == orc.topp(own[s], 0.5, 0.95, 40, float(rands[i, s]))[0], (i, s)
            assert ms[s].Pos == 5 + 7 * s + i + 1
            feed[s] = got
    dispose(batch, ms)


def test_step_greedy_and_changes_of_temperature_and_k_interleave(mgr):
    """The candidate graph sits beside the batch's other graphs and is re-captured when (temperature, k) change: between Step and
    Greedy calls, through (0.5, 40) -> (0.8, 8) -> (0.5, 40) -> (1.0, 64), the candidates stay bit-equal to nfai_hip_topk on the
    read-back logits.  A batch over graph-less members (graph=False) in the same state returns the same bits."""
    from nfai_amd.llama_model import LlamaBatch
    dims, n = synth.TINY, 3
    w = synth.make_weights(dims, seed=21, std=0.05)
    sets = [make_members(mgr, dims, w, n, CAP), make_members(mgr, dims, w, n, CAP, graph=False)]
    batches = []
    for ms in sets:
        staggered(ms, dims, n)
        batches.append(LlamaBatch(ms))
    toks = [seq_tokens(dims, s) for s in range(n)]
    feed = [int(toks[s][5 + 7 * s]) for s in range(n)]
    plan = [("topk", 0.5, 40), ("step",), ("topk", 0.5, 40), ("topk", 0.8, 8), ("greedy",), ("topk", 0.8, 8), ("topk", 0.5, 40),
            ("step",), ("topk", 1.0, 64), ("greedy",), ("topk", 1.0, 64)]
    pos = 0
    for at, op in enumerate(plan):
        got = []
        for ms, batch in zip(sets, batches):
            if op[0] == "topk":
                ids, probs = batch.StepTopK(feed, op[1], op[2])
                check_candidates(mgr, ms, dims.V, ids, probs, op[1], op[2], f"op {at}")
                got.append((ids, probs))
                nxt = [int(ids[s][at % op[2]]) for s in range(n)]   # some candidate, not always the best
            elif op[0] == "step":
                nxt = [int(t) for t in batch.Step(feed, want_logits=False)[1]]
            else:
                nxt = [int(t) for t in batch.Greedy(feed, 2)[-1]]
        if got:
            assert np.array_equal(got[0][0], got[1][0]) and bit_equal(got[0][1], got[1][1]), at
        pos += 2 if op[0] == "greedy" else 1
        for ms in sets:
            assert [m.Pos for m in ms] == [5 + 7 * s + pos for s in range(n)]
        feed = nxt
    for batch, ms in zip(batches, sets):
        dispose(batch, ms)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_move_nothing(mgr):
    from nfai_amd import _lib
    from nfai_amd.llama_model import LlamaBatch
    dims, n = synth.TINY, 3
    w = synth.make_weights(dims, seed=21, std=0.05)
    ms = make_members(mgr, dims, w, n, [CAP, 12, CAP])
    for s, m in enumerate(ms):
        for t in seq_tokens(dims, s)[:3 + 2 * s]:
            m.Step(int(t), want_logits=False)
    batch = LlamaBatch(ms)
    pos = [m.Pos for m in ms]
    good = [1, 2, 3]
    t = np.array(good, np.uint32)
    ids, probs = np.empty((n, 64), np.uint32), np.empty((n, 64), np.float32)

    def refused(code, tokens, temperature, k, ids_p, probs_p):
        tk = None if tokens is None else np.ascontiguousarray(tokens, np.uint32)
        with pytest.raises(_lib.NfaiHipError) as e:
            _lib.call("nfai_hip_llama_batch_step_topk", batch.handle, tk.ctypes.data_as(U32P) if tokens is not None else None,
                      temperature, k, ids_p, probs_p)
        assert e.value.code == code, (e.value.code, str(e.value))
        assert [m.Pos for m in ms] == pos

    ip, pp = ids.ctypes.data_as(U32P), probs.ctypes.data_as(F32P)
    for k in (0, 65, dims.V + 1):
        refused(_lib.ERR_INVALID, good, 0.5, k, ip, pp)
    for temperature in (0.0, -1.0, float("nan")):
        refused(_lib.ERR_INVALID, good, temperature, 40, ip, pp)
    refused(_lib.ERR_INVALID, [1, dims.V, 3], 0.5, 40, ip, pp)
    refused(_lib.ERR_INVALID, good, 0.5, 40, None, pp)
    refused(_lib.ERR_INVALID, good, 0.5, 40, ip, None)
    refused(_lib.ERR_INVALID, None, 0.5, 40, ip, pp)
    got_ids, got_probs = batch.StepTopK(good)                  # a valid call after the refusals
    check_candidates(mgr, ms, dims.V, got_ids, got_probs, 0.5, 40, "after refusals")
    pos = [p + 1 for p in pos]
    assert [m.Pos for m in ms] == pos
    while ms[1].Pos < 12:                                      # member 1 alone to its capacity
        ms[1].Step(4, want_logits=False)
    pos = [m.Pos for m in ms]
    refused(_lib.ERR_KV_FULL, good, 0.5, 40, ip, pp)
    with pytest.raises(_lib.KVCacheFull):
        batch.StepTopK(good)
    assert [m.Pos for m in ms] == pos
    ms[1].SetPos(6)                                            # room again: the same batch steps
    got_ids, got_probs = batch.StepTopK(good)
    check_candidates(mgr, ms, dims.V, got_ids, got_probs, 0.5, 40, "after KV_FULL")
    assert [m.Pos for m in ms] == [pos[0] + 1, 7, pos[2] + 1]
    dispose(batch, ms)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
def drive(mgr, models, lists, eos, greedy, max_tokens, rng):
    """The loop RunTokens states, written out on Step(want_logits=True) + nfai_hip_topk per member: -> [(member, token)]."""
    from nfai_amd.llama_model import LlamaBatch, SamplingUtils
    for m, tl in zip(models, lists):
        m.Ingest(tl[:-1])
    running = list(range(len(models)))
    last = {i: int(lists[i][-1]) for i in running}
    count = {i: 0 for i in running}
    out = []
    batch = LlamaBatch([models[i] for i in running])
    while running:
        lg, am = batch.Step([last[i] for i in running], want_logits=True)
        nxt = []
        for j, i in enumerate(running):                        # ascending member order: one draw each
            if greedy:
                tk = int(am[j])
            else:
                ids, probs = topk_single(mgr, lg[j], 0.5, 40)
                tk = SamplingUtils.TopPFromCandidates(ids, probs, rng=rng)
            count[i] += 1
            if tk == eos and count[i] > 1:
                continue                                       # a later EOS: not yielded, not fed, the stream ends
            out.append((i, tk))                                # (the first token is yielded whatever it is)
            if tk == eos or count[i] >= max_tokens:
                continue
            last[i] = tk
            nxt.append(i)
        if nxt != running:
            batch.Dispose()
            batch = LlamaBatch([models[i] for i in nxt]) if nxt else None
        running = nxt
    if batch is not None:
        batch.Dispose()
    return out


@pytest.mark.parametrize("greedy", [False, True], ids=["sampled", "greedy"])
def test_the_loop_is_the_written_out_loop(mgr, greedy):
    """RunTokens on one set of 4 members against the same loop driven by the test on an identical set: identical (member, token)
    streams and final positions.  EOS is the token member 1 emits at its 4th step in a first pass without EOS, so member 1 retires
    early, the batch shrinks, and member 1 is not advanced after its stream ended."""
    from nfai_amd.llama_model import LlamaBatch
    dims, n, seed = synth.TINY, 4, 31
    w = synth.make_weights(dims, seed=61, std=0.08)
    A, B = make_members(mgr, dims, w, n, CAP), make_members(mgr, dims, w, n, CAP)
    lists = [[int(t) for t in synth.make_tokens(dims, ln, seed=200 + s)] for s, ln in enumerate((3, 6, 4, 9))]
    batch = LlamaBatch(A)
    first = list(batch.RunTokens(lists, -1, greedy=greedy, max_tokens=12, rng=np.random.Generator(np.random.PCG64(seed))))
    assert [sum(1 for i, _ in first if i == s) for s in range(n)] == [12] * n
    assert [m.Pos for m in A] == [len(tl) - 1 + 12 for tl in lists]
    E = [tk for i, tk in first if i == 1][3]
    for m in A:
        m.Reset()
    got = list(batch.RunTokens(lists, E, greedy=greedy, max_tokens=12, rng=np.random.Generator(np.random.PCG64(seed))))
    want = drive(mgr, B, lists, E, greedy, 12, np.random.Generator(np.random.PCG64(seed)))
    assert got == want
    assert [m.Pos for m in A] == [m.Pos for m in B]
    mine = [tk for i, tk in got if i == 1]
    assert len(mine) <= 3 and E not in mine[1:]                # it ended at or before its 4th step, and EOS was not yielded
    # every token it was fed advanced it once: its prompt, then the tokens it emitted (EOS, emitted first, is not fed)
    assert A[1].Pos == len(lists[1]) + len(mine) - (1 if mine[0] == E else 0)
    assert A[1].Pos < len(lists[1]) - 1 + 12                   # short of where the pass without EOS left it
    assert max(sum(1 for i, _ in got if i == s) for s in (0, 2, 3)) > len(mine)   # and the batch went on without it
    dispose(batch, A)
    dispose(None, B)


def test_run_async_yields_the_detokenised_run_tokens_stream(mgr):
    """On the tokenizer fixture of tests/test_gpu_model.py::test_gguf_file_to_generation_end_to_end: RunAsync(prompts) of two members
    is RunTokens on the tokenised prompts, detokenised token by token."""
    from nfai_amd.llama_model import LlamaBatch, LlamaModel
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
    ms = [LlamaModel(mgr, md, w, 128)]
    ms.append(LlamaModel(mgr, md, w, 128, share_from=ms[0]))
    assert ms[0].tokenizer is not None
    prompts = ["hello world", "hello"]
    batch = LlamaBatch(ms)
    text = list(batch.RunAsync(prompts, max_tokens=6, rng=np.random.Generator(np.random.PCG64(5))))
    assert not ms[0].firstInput and not ms[1].firstInput
    pos = [m.Pos for m in ms]
    tk = Tokenizer(md)
    lists = [tk.Tokenize(p, addBos=True) for p in prompts]
    for m in ms:
        m.Reset()
    stream = list(batch.RunTokens(lists, tk.EosTokenId, max_tokens=6, rng=np.random.Generator(np.random.PCG64(5))))
    assert text == [(i, tk.Detokenize([t])) for i, t in stream] and len(text) >= 2
    assert [m.Pos for m in ms] == pos
    dispose(batch, ms)
