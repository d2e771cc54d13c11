"""CPU-side checks of the window (greedy speculative decoding, nfai_hip_llama_window_*): the entry points are exported, declared,
bound in ctypes and present in the generated C# with matching parameter counts; bad arguments are error codes with a message; the
prompt-lookup drafter's known answers; RunAsync refuses speculative decoding without greedy.  No compute calls here (the GPU side
is tests/test_gpu_window_decode.py)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the C ABI block of the window: the handle type and its six entry points, with their parameter counts
WINDOW_TYPE = "nfai_window_t"
WINDOW_ENTRIES = {
    "nfai_hip_llama_window_create": 4,
    "nfai_hip_llama_window_destroy": 1,
    "nfai_hip_llama_window_step": 5,
    "nfai_hip_llama_window_verify": 7,
    "nfai_hip_llama_window_bytes_per_step": 3,
    "nfai_hip_llama_window_profile_step": 5,
}


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
    header_src = open(os.path.join(ROOT, "include", "nfai_hip.h")).read()
    assert re.search(r"typedef\s+uint64_t\s+%s\s*;" % WINDOW_TYPE, header_src)
    header = {name: params for name, _, params in gen.parse_header()}
    cs = open(os.path.join(ROOT, "csharp", "NFAI.HIP", "NativeMethods.g.cs")).read()
    for name, n_params in WINDOW_ENTRIES.items():
        assert hasattr(raw, name), name                                   # exported
        assert name in header and len(header[name]) == n_params, name     # declared
        assert len(_lib.SIGNATURES[name]) == n_params, name               # bound in ctypes
        m = re.search(r"internal static partial int %s\((.*?)\);" % name, cs)
        assert m and len(m.group(1).split(",")) == n_params, name         # generated C#
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_csharp_bindings.py"), "--check"]).returncode == 0
    # the hand-written host class calls every entry point
    host = open(os.path.join(ROOT, "csharp", "NFAI.HIP", "HipLlamaWindow.cs")).read()
    for name in WINDOW_ENTRIES:
        assert "Native." + name + "(" in host, name


def test_window_entries_cite_the_reference_loop():
    src = open(os.path.join(ROOT, "include", "nfai_hip.h")).read()
    block = src[src.index("---- window:"):src.index("---- layer pipeline")]
    assert "LlamaModel.cs:116-125" in block and "SamplingUtils.cs:43-57" in block


def test_bad_arguments_are_error_codes_with_a_message(lib):
    from nfai_amd import _lib
    H, u32, f32 = _lib.H, ctypes.c_uint32, ctypes.c_float
    out, n = H(), u32()
    toks = (u32 * 8)()
    ms, cnt = (f32 * 8)(), (u32 * 8)()
    total = ctypes.c_uint64()

    def refused(match, name, *args):
        with pytest.raises(_lib.NfaiHipError, match=match) as e:
            _lib.call(name, *args)
        assert e.value.code == _lib.ERR_INVALID, (name, e.value.code)

    # create: dead and zero model handles, max_tokens outside [2, 8], unknown flag bits, NULL output
    refused("invalid model handle", "nfai_hip_llama_window_create", H(0), 4, 0, ctypes.byref(out))
    refused("invalid model handle", "nfai_hip_llama_window_create", H(987654321), 4, 0, ctypes.byref(out))
    refused("max_tokens = 1", "nfai_hip_llama_window_create", H(0), 1, 0, ctypes.byref(out))
    refused("max_tokens = 9", "nfai_hip_llama_window_create", H(0), 9, 0, ctypes.byref(out))
    refused("invalid flags 0x2", "nfai_hip_llama_window_create", H(0), 4, 2, ctypes.byref(out))
    refused("null argument", "nfai_hip_llama_window_create", H(0), 4, 0, None)
    # every other entry point on dead and zero window handles
    for h in (H(0), H(987654321)):
        refused("invalid window handle", "nfai_hip_llama_window_destroy", h)
        refused("invalid window handle", "nfai_hip_llama_window_step", h, toks, 2, None, None)
        refused("invalid window handle", "nfai_hip_llama_window_verify", h, 1, toks, 2, None, toks, ctypes.byref(n))
        refused("invalid window handle", "nfai_hip_llama_window_bytes_per_step", h, 2, ctypes.byref(total))
        refused("invalid window handle", "nfai_hip_llama_window_profile_step", h, toks, 2, ms, cnt)
    assert out.value == 0


# ---- the drafter ------------------------------------------------------------------------------------------------------------------
def test_drafter_longest_ngram_wins():
    from nfai_amd.drafter import PromptLookupDrafter
    #        0  1  2  3   4  5  6   7  8  9
    hist = [1, 2, 3, 10, 7, 3, 20, 1, 2, 3]
    # the 3-gram (1, 2, 3) occurred at 0 -> 10 follows; the more recent 1-gram (3) at 5 would give 20
    assert PromptLookupDrafter(3).Propose(hist, 2) == [10, 7]
    assert PromptLookupDrafter(1).Propose(hist, 2) == [20, 1]


def test_drafter_most_recent_match_wins():
    from nfai_amd.drafter import PromptLookupDrafter
    hist = [5, 6, 11, 9, 5, 6, 12, 9, 5, 6]
    assert PromptLookupDrafter(2).Propose(hist, 3) == [12, 9, 5]


def test_drafter_proposal_is_cut_at_the_end_of_the_history():
    from nfai_amd.drafter import PromptLookupDrafter
    hist = [4, 8, 15, 16, 4, 8]
    assert PromptLookupDrafter(3).Propose(hist, 7) == [15, 16, 4, 8]
    assert PromptLookupDrafter(3).Propose([7, 7], 4) == [7]   # the match ends one token before the end


def test_drafter_no_match_is_an_empty_proposal():
    from nfai_amd.drafter import PromptLookupDrafter
    d = PromptLookupDrafter(3)
    assert d.Propose([1, 2, 3, 4], 4) == []
    assert d.Propose([9], 4) == [] and d.Propose([], 4) == []
    assert d.Propose([1, 2, 1], 0) == []
    with pytest.raises(ValueError):
        PromptLookupDrafter(0)


def test_run_async_refuses_speculative_sampling():
    """speculative > 0 verifies drafts against ArgMax: with greedy=False it is a ValueError at the call, before anything runs."""
    from nfai_amd.llama_model import LlamaModel
    m = LlamaModel.__new__(LlamaModel)   # no device needed: the arguments are checked first
    with pytest.raises(ValueError, match="greedy"):
        m.RunAsync("hello", greedy=False, speculative=2)
    with pytest.raises(ValueError):
        m.RunAsync("hello", greedy=True, speculative=8)


def _scan(hist, k, ngram_max):
    """The definition, statement by statement: the most recent earlier occurrence of the longest tail n-gram that occurs at all."""
    L = len(hist)
    if k <= 0 or L < 2:
        return []
    for n in range(min(ngram_max, L - 1), 0, -1):
        for start in range(L - n - 1, -1, -1):
            if hist[start:start + n] == hist[L - n:]:
                return hist[start + n:start + n + k]
    return []


def test_drafter_fed_a_growing_history_answers_as_a_fresh_scan():
    """RunAsync hands the drafter the same history, longer each time: the incremental index gives what a scan of the whole history
    gives, also when the history is replaced by an unrelated or a shorter one in between."""
    from nfai_amd.drafter import PromptLookupDrafter
    rng = np.random.default_rng(5)
    for ngram_max in (1, 2, 3):
        d = PromptLookupDrafter(ngram_max)
        hist = []
        for grow in rng.integers(1, 6, size=60):
            hist = hist + [int(t) for t in rng.integers(0, 4, size=grow)]   # a small alphabet: matches at every n
            assert d.Propose(hist, 5) == _scan(hist, 5, ngram_max), (ngram_max, hist)
        other = [int(t) for t in rng.integers(0, 4, size=40)]
        assert d.Propose(other, 5) == _scan(other, 5, ngram_max)
        assert d.Propose(other[:17], 5) == _scan(other[:17], 5, ngram_max)
        assert d.Propose(np.asarray(other[:29], np.uint32), 3) == _scan(other[:29], 3, ngram_max)


def test_drafter_cuts_the_proposal_in_front_of_the_stop_token():
    from nfai_amd.drafter import PromptLookupDrafter
    hist = [4, 8, 15, 99, 16, 4, 8]
    assert PromptLookupDrafter(3).Propose(hist, 4) == [15, 99, 16, 4]
    assert PromptLookupDrafter(3).Propose(hist, 4, stop=99) == [15]
    assert PromptLookupDrafter(3).Propose(hist, 4, stop=15) == []
    assert PromptLookupDrafter(3).Propose(hist, 4, stop=7) == [15, 99, 16, 4]


def test_a_model_given_block_encoded_matrices_on_the_device_opens_quantised_windows(monkeypatch):
    """RunAsync(speculative=k) picks the window's kernel family from what the model was given, a QuantTensor or a device tuple."""
    from nfai_amd import _lib, llama_model
    from nfai_amd.llama_model import LlamaModel
    monkeypatch.setattr(llama_model, "call", lambda *a, **k: None)
    m = LlamaModel.__new__(LlamaModel)
    m.handle, m._quantized = _lib.H(0), False
    m.SetTensor("blk.0.attn_norm.weight", (0, _lib.F32, 1, 256))
    m.SetTensor("blk.0.attn_q.weight", (0, _lib.F16, 256, 256))
    assert m._quantized is False
    m.SetTensor("blk.0.attn_k.weight", (0, _lib.Q4_K, 128, 256))
    assert m._quantized is True
