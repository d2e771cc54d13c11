"""CPU-side checks of sampled batched decode (nfai_hip_topk_rows, nfai_hip_llama_batch_step_topk, LlamaBatch.RunTokens / RunAsync):
the two entry points are exported, declared, bound in ctypes and present in the generated C# with matching parameter counts, and
called by the hand-written host class; their header comments cite the reference members they replace; dead and zero handles are
error codes with a message; the token loop's bookkeeping on a fake batch (NumPy stand-ins, no device).  The GPU side is
tests/test_gpu_batch_sampling.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = {"nfai_hip_topk_rows": 8, "nfai_hip_llama_batch_step_topk": 6}


@pytest.fixture(scope="module")
def lib():
    from nfai_amd import build as hb, _lib
    hb.build()
    return _lib.load()


def test_symbols_are_exported_declared_and_bound(lib):
    from nfai_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_csharp_bindings as gen
    raw = ctypes.CDLL(os.path.join(ROOT, "nfai_amd", "csrc", "libnfai_hip.so"))
    header = {name: params for name, _, params in gen.parse_header()}
    cs = open(os.path.join(ROOT, "csharp", "NFAI.HIP", "NativeMethods.g.cs")).read()
    for name, n_params in ENTRIES.items():
        assert hasattr(raw, name), name                                   # exported
        assert name in header and len(header[name]) == n_params, name     # declared
        assert len(_lib.SIGNATURES[name]) == n_params, name               # bound in ctypes
        m = re.search(r"internal static partial int %s\((.*?)\);" % name, cs)
        assert m and len(m.group(1).split(",")) == n_params, name         # generated C#
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_csharp_bindings.py"), "--check"]).returncode == 0
    # the hand-written host class calls the batch entry point, from StepTopK, and StepSampled finishes TopP per member
    host = open(os.path.join(ROOT, "csharp", "NFAI.HIP", "HipLlamaBatch.cs")).read()
    assert "Native.nfai_hip_llama_batch_step_topk(" in host
    assert re.search(r"public void StepTopK\(", host) and re.search(r"public void StepSampled\(", host)
    assert "HipLlamaModel.TopPFromCandidates(" in host and "Random.Shared.NextSingle()" in host


def _comment_in_front_of(src, name):
    """The comment block that ends where the declaration of `name` begins."""
    at = src.index("int32_t %s(" % name)
    start = src.rindex("/*", 0, at)
    assert src[src.index("*/", start) + 2:at].strip() == "", name   # nothing between the comment and the declaration
    return src[start:at]


def test_entries_cite_the_reference_members_they_replace():
    src = open(os.path.join(ROOT, "include", "nfai_hip.h")).read()
    rows = _comment_in_front_of(src, "nfai_hip_topk_rows")
    assert "SamplingUtils.cs:7-13" in rows
    step = _comment_in_front_of(src, "nfai_hip_llama_batch_step_topk")
    assert "LlamaModel.cs:116-125" in step and "SamplingUtils.cs" in step and "LlamaModel.cs:128-130,165" in step


def test_bad_handles_are_error_codes_with_a_message(lib):
    from nfai_amd import _lib
    H, u32, f32 = _lib.H, ctypes.c_uint32, ctypes.c_float
    toks, ids, probs = (u32 * 8)(), (u32 * 8 * 64)(), (f32 * 8 * 64)()
    bufs = (H * 8)()

    def refused(match, name, *args):
        with pytest.raises(_lib.NfaiHipError, match=match) as e:
            _lib.call(name, *args)
        assert e.value.code == _lib.ERR_INVALID, (name, e.value.code)

    for h in (H(0), H(987654321)):
        refused("invalid batch handle", "nfai_hip_llama_batch_step_topk", h, toks, 0.5, 40, ctypes.cast(ids, ctypes.POINTER(u32)),
                ctypes.cast(probs, ctypes.POINTER(f32)))
        refused("invalid context handle", "nfai_hip_topk_rows", h, bufs, 2, 1000, 0.5, 40, ctypes.cast(ids, ctypes.POINTER(u32)),
                ctypes.cast(probs, ctypes.POINTER(f32)))


# ---- the token loop on a fake batch ----------------------------------------------------------------------------------------------
EOS = 7


class FakeModel:
    def __init__(self, idx, prefill):
        self.idx, self.promptPrefill = idx, prefill
        self.ingested, self.stepped, self.fed = [], [], []   # prompt tokens by path | tokens fed by batch steps
        self.firstInput = True
        self.tokenizer = None

    def Ingest(self, tokens):
        self.ingested.append([int(t) for t in tokens])

    def Step(self, token, want_logits=True):
        assert want_logits is False
        self.stepped.append(int(token))
        return None, 0


class ScriptedRng:
    """Stands in for numpy's Generator: hands out the scripted draws and counts them."""

    def __init__(self, draws, log):
        self.draws, self.at, self.log = list(draws), 0, log

    def random(self, dtype=np.float64):
        self.log.append("draw")
        r = self.draws[self.at % len(self.draws)]
        self.at += 1
        return dtype(r)


def candidates(script, member, step):
    """Member `member`'s two candidates at its step `step`, each with probability 1/2: a draw below 0.5 takes the first."""
    return script.get((member, step), (1000 * (member + 1) + 10 * step, 1000 * (member + 1) + 10 * step + 1))


@pytest.fixture
def fake(monkeypatch):
    """LlamaBatch with its constructor, Step, StepTopK and Dispose replaced: `log` records batches made, steps (with the members that
    ran), draws and disposals, in order."""
    from nfai_amd import llama_model
    log, script = [], {}

    def init(self, models, quantized=False, any_quant=False):
        self.models, self.n, self.handle = list(models), len(models), None
        self._kw = dict(quantized=quantized, any_quant=any_quant)
        log.append(("batch", tuple(m.idx for m in self.models), quantized, any_quant))

    def feed(self, tokens):
        assert len(tokens) == self.n
        log.append(("step", tuple(m.idx for m in self.models)))
        cands = []
        for m, t in zip(self.models, tokens):
            cands.append(candidates(script, m.idx, len(m.fed)))
            m.fed.append(int(t))
        return cands

    def step_topk(self, tokens, temperature=0.5, topK=40):
        assert (temperature, topK) == (0.5, 40)   # the reference's defaults (SamplingUtils.cs:5)
        cands = feed(self, tokens)
        return np.array(cands, np.uint32), np.full((self.n, 2), 0.5, np.float32)

    def step(self, tokens, want_logits=True):
        assert want_logits is False
        return None, np.array([c[0] for c in feed(self, tokens)], np.uint32)

    monkeypatch.setattr(llama_model.LlamaBatch, "__init__", init)
    monkeypatch.setattr(llama_model.LlamaBatch, "StepTopK", step_topk)
    monkeypatch.setattr(llama_model.LlamaBatch, "Step", step)
    monkeypatch.setattr(llama_model.LlamaBatch, "Dispose", lambda self: log.append(("dispose", tuple(m.idx for m in self.models))))
    return llama_model.LlamaBatch, log, script


def test_run_tokens_bookkeeping_sampled(fake):
    LlamaBatch, log, script = fake
    ms = [FakeModel(0, True), FakeModel(1, False), FakeModel(2, True), FakeModel(3, True)]
    script[(2, 0)] = (EOS, EOS)         # member 2's FIRST token is EOS: yielded whatever it is, then its stream ends
    script[(1, 2)] = (555, EOS)         # member 1's third token is EOS on a draw >= 0.5: not yielded, never fed
    batch = LlamaBatch(ms, quantized=True, any_quant=True)
    prompts = [[11, 12, 13], [21, 22], [31], [41, 42, 43, 44]]
    draws = [0.1, 0.9, 0.3, 0.7,     # step 0: members 0, 1, 2, 3 in this order
             0.9, 0.2, 0.6,          # step 1: members 0, 1, 3
             0.4, 0.8, 0.1,          # step 2: members 0, 1 (EOS), 3
             0.9, 0.9]               # step 3: members 0, 3 (max_tokens = 4 ends both)
    rng = ScriptedRng(draws, log)
    out = list(batch.RunTokens(prompts, EOS, greedy=False, max_tokens=4, rng=rng))

    def tok(member, step, draw):
        return candidates(script, member, step)[0 if draw < 0.5 else 1]
    want = [(0, tok(0, 0, 0.1)), (1, tok(1, 0, 0.9)), (2, EOS), (3, tok(3, 0, 0.7)),
            (0, tok(0, 1, 0.9)), (1, tok(1, 1, 0.2)), (3, tok(3, 1, 0.6)),
            (0, tok(0, 2, 0.4)), (3, tok(3, 2, 0.1)),
            (0, tok(0, 3, 0.9)), (3, tok(3, 3, 0.9))]
    assert out == want
    assert rng.at == len(draws)   # exactly one draw per running member per step
    # prompt phase per member: Ingest(tokens[:-1]) with promptPrefill, token by token without
    assert ms[0].ingested == [[11, 12]] and ms[0].stepped == []
    assert ms[1].ingested == [] and ms[1].stepped == [21]
    assert ms[2].ingested == [[]] and ms[3].ingested == [[41, 42, 43]]
    # what each member was fed: its last prompt token, then its own emitted tokens, never EOS and nothing after its stream ended
    assert ms[0].fed == [13, want[0][1], want[4][1], want[7][1]]
    assert ms[1].fed == [22, want[1][1], want[5][1]]
    assert ms[2].fed == [31]
    assert ms[3].fed == [44, want[3][1], want[6][1], want[8][1]]
    assert all(EOS not in m.fed for m in ms)
    # the running set shrinks with a new batch over the members still running (made as the first was), disposed by the loop
    assert log == [("batch", (0, 1, 2, 3), True, True),
                   ("step", (0, 1, 2, 3)), "draw", "draw", "draw", "draw",
                   ("batch", (0, 1, 3), True, True),
                   ("step", (0, 1, 3)), "draw", "draw", "draw",
                   ("step", (0, 1, 3)), "draw", "draw", "draw",
                   ("batch", (0, 3), True, True),
                   ("step", (0, 3)), "draw", "draw",
                   ("dispose", (0, 1, 3)), ("dispose", (0, 3))]


def test_run_tokens_bookkeeping_greedy(fake):
    LlamaBatch, log, script = fake
    ms = [FakeModel(0, True), FakeModel(1, True)]
    script[(0, 1)] = (EOS, 1)           # member 0's second token is EOS
    batch = LlamaBatch(ms)
    out = list(batch.RunTokens([[5], [6, 7]], EOS, greedy=True, max_tokens=3))
    assert out == [(0, 1000), (1, 2000), (1, 2010), (1, 2020)]
    assert ms[0].fed == [5, 1000] and ms[1].fed == [7, 2000, 2010]
    assert "draw" not in log
    assert log == [("batch", (0, 1), False, False), ("step", (0, 1)), ("step", (0, 1)), ("batch", (1,), False, False), ("step", (1,)),
                   ("dispose", (1,))]


def test_run_tokens_max_tokens_counts_per_member_and_one_is_the_floor(fake):
    LlamaBatch, log, script = fake
    ms = [FakeModel(0, True), FakeModel(1, True)]
    out = list(LlamaBatch(ms).RunTokens([[1], [2]], EOS, greedy=True, max_tokens=1))
    assert out == [(0, 1000), (1, 2000)] and ms[0].fed == [1] and ms[1].fed == [2]
    assert [e for e in log if e[0] == "step"] == [("step", (0, 1))]


def test_run_tokens_refuses_a_length_mismatch(fake):
    LlamaBatch, log, script = fake
    ms = [FakeModel(0, True), FakeModel(1, True)]
    batch = LlamaBatch(ms)
    with pytest.raises(ValueError, match="1 prompts for 2 members"):
        list(batch.RunTokens([[1, 2]], EOS))
    with pytest.raises(ValueError):
        list(batch.RunTokens([[1, 2], []], EOS))
    ms[0].tokenizer = object()
    with pytest.raises(ValueError, match="3 prompts for 2 members"):
        list(batch.RunAsync(["a", "b", "c"]))
    assert all(m.fed == [] and m.ingested == [] for m in ms)   # nothing ran


def test_run_async_is_run_tokens_with_member_0s_tokenizer(fake):
    LlamaBatch, log, script = fake

    class Tok:
        EosTokenId = EOS
        calls = []

        def Tokenize(self, prompt, addBos):
            self.calls.append((prompt, addBos))
            return ([1] if addBos else []) + [ord(c) for c in prompt]

        def Detokenize(self, ids):
            return "<%d>" % ids[0]

    ms = [FakeModel(0, True), FakeModel(1, True)]
    ms[0].tokenizer = Tok()
    ms[1].firstInput = False
    out = list(LlamaBatch(ms).RunAsync(["ab", "c"], greedy=True, max_tokens=2))
    assert Tok.calls == [("ab", True), ("c", False)] and not ms[0].firstInput
    assert out == [(0, "<1000>"), (1, "<2000>"), (0, "<1010>"), (1, "<2010>")]
    assert ms[0].ingested == [[1, ord("a")]] and ms[0].fed[0] == ord("b") and ms[1].fed[0] == ord("c")
