"""nfai_hip_llama_score against one oracle walk per model (tests/score_cases.py): the log-probabilities and the ArgMax of every row on
the M = 1 path and on the MFMA path (chunk edges, a lead-in, every weight encoding, both KV types, the real vocabulary across slab
boundaries), the state the call leaves — bit for bit a twin's that went through nfai_hip_llama_prefill (MFMA) or n _decode_step calls
(M = 1) — and the refusals.

Bars: both log-probabilities within twice the case's logit bar (5e-4 * max(1, max|logit|) on the M = 1 path with an fp32 cache, 2e-2 *
max(1, max|logit|) on the MFMA path or with an fp16 cache); the returned ArgMax's oracle logit within two logit bars of the oracle
maximum on every row and equal to the oracle's ArgMax on every pinned row."""
import ctypes as C

import numpy as np
import pytest

import score_cases as sc
from nfai_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


def kv_rows(m, layer, is_v, pos, n):
    from nfai_amd import _lib
    from nfai_amd._lib import call
    lib = _lib.load()
    lib.nfai_hip_debug_read_kv_rows.argtypes = [_lib.H, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
    lib.nfai_hip_debug_read_kv_rows.restype = C.c_int32
    out = np.empty((n, m.dims["Hkv"] * m.dims["D"]), np.float32)
    call("nfai_hip_debug_read_kv_rows", m.handle, layer, int(is_v), pos, n, out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


def token_word(mgr, m):
    from nfai_amd.hip import ShaderProperty
    p = ShaderProperty(mgr, 1, np.uint32)
    m.TokenToDevice(p.buffer.device_ptr)
    mgr.Synchronize()
    v = int(p.GetValue()[0])
    p.buffer.free()
    return v


def state(mgr, m, n_rows):
    d = m.dims
    return dict(pos=m.Pos, tok=token_word(mgr, m), hidden=m.Read(0, d["E"]), logits=m.Read(4, d["V"]),
                kv=[kv_rows(m, l, v, 0, n_rows) for l in range(d["L"]) for v in (False, True)])


def same_state(a, b, where):
    assert a["pos"] == b["pos"] and a["tok"] == b["tok"], (where, a["pos"], b["pos"], a["tok"], b["tok"])
    for k in ("hidden", "logits"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (where, k)
    for i, (x, y) in enumerate(zip(a["kv"], b["kv"])):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (where, "K / V rows", i)


def make(mgr, c, cap=None):
    from nfai_amd.llama_model import LlamaModel
    return LlamaModel(mgr, synth.make_metadata(c.dims), sc.weights(c.dims, c.enc)[0], cap or (sc.LEAD_MAX + sc.N_MAX + 2), dims=sc.ddict(c.dims),
                      max_batch=c.max_batch, kv_f16=c.kv_f16)


@pytest.mark.parametrize("c", sc.CASES, ids=[c.id for c in sc.CASES])
def test_score(mgr, c):
    lead, toks, targets, scored, lg = sc.case_rows(c)
    m, twin = make(mgr, c), make(mgr, c)
    try:
        for t in lead:
            m.Step(int(t))
            twin.Step(int(t))
        lp, am, lpm = m.Score(toks, targets)
        if c.max_batch > 0:
            twin.Prefill(toks)
        else:
            for t in toks:
                twin.Step(int(t))
        want_lp, want_am, want_lpm = sc.score_rows_ref(lg, scored)
        bars = sc.logit_bars(c, lg)
        e1, e2 = np.abs(lp - want_lp) / (2 * bars), np.abs(lpm - want_lpm) / (2 * bars)
        print(f"{c.id}: logprob error / bar: target {e1.max():.3f}, maximum {e2.max():.3f}; pinned {sc.pinned(c, lg).mean():.0%}")
        assert e1.max() <= 1.0 and e2.max() <= 1.0, (float(e1.max()), int(e1.argmax()), float(e2.max()), int(e2.argmax()))
        assert (lp[scored == sc.NO_TARGET] == 0.0).all()
        rows = np.arange(c.n)
        assert (am < c.dims.V).all()
        assert (lg.max(axis=1) - lg[rows, am] <= 2 * bars).all(), "a returned ArgMax lies more than two logit bars under the oracle's maximum"
        pin = sc.pinned(c, lg)
        assert np.array_equal(am[pin], want_am[pin]), np.nonzero(pin & (am != want_am))[0]
        # the state: bit for bit the twin's, and one further token agrees bit for bit
        end = c.lead + c.n
        same_state(state(mgr, m, end), state(mgr, twin, end), "behind the call")
        nxt = int(want_am[-1])
        la, aa = m.Step(nxt)
        lb, ab = twin.Step(nxt)
        assert aa == ab and np.array_equal(la.view(np.uint32), lb.view(np.uint32))
        same_state(state(mgr, m, end + 1), state(mgr, twin, end + 1), "one token later")
        if c.max_batch > 0 and not c.kv_f16 and c.n > 1:   # the MFMA path ran: fp16 operands, not the M = 1 path's bits
            ref = make(mgr, sc.Case(c.dims, c.enc, c.kv_f16, 0, c.n, c.lead))
            for t in list(lead) + list(toks):
                ref.Step(int(t))
            assert not np.array_equal(kv_rows(ref, c.dims.L - 1, False, c.lead, c.n), kv_rows(m, c.dims.L - 1, False, c.lead, c.n))
            ref.Dispose()
    finally:
        m.Dispose()
        twin.Dispose()


def test_perplexity_is_the_mean_of_the_scored_rows(mgr):
    c = sc.Case(synth.TINY, "f16", False, 16, 35)
    _, toks, _, scored, lg = sc.case_rows(c)
    m = make(mgr, c)
    got = m.Perplexity(toks)
    m.Dispose()
    want = float(np.exp(-np.mean(sc.score_rows_ref(lg, scored)[0][:-1])))
    bar = 2 * float(sc.logit_bars(c, lg).max())            # every row's log-probability is within it, so is their mean
    assert abs(np.log(got) - np.log(want)) <= bar, (got, want)


@pytest.mark.parametrize("max_batch", [0, 16], ids=["m1", "mfma"])
def test_refusals_leave_the_sequence_where_it_was(mgr, max_batch):
    from nfai_amd import _lib
    from nfai_amd.llama_model import LlamaModel
    c = sc.Case(synth.TINY, "f16", False, max_batch, 8, 3)
    lead, toks, _, _, _ = sc.case_rows(c)
    cap = 12
    m = make(mgr, c, cap)
    lib = _lib.load()
    for t in lead:
        m.Step(int(t))
    before = state(mgr, m, cap)
    u32p = C.POINTER(C.c_uint32)
    t8 = np.ascontiguousarray(toks, np.uint32)
    bad_tok = t8.copy()
    bad_tok[5] = c.dims.V
    bad_tgt = t8.copy()
    bad_tgt[2] = c.dims.V + 7
    long = np.ascontiguousarray(sc.walk(c.dims, c.enc).toks[:cap - len(lead) + 1], np.uint32)

    def call(tok, n, tgt=None):
        return lib.nfai_hip_llama_score(m.handle, None if tok is None else tok.ctypes.data_as(u32p), n,
                                        None if tgt is None else tgt.ctypes.data_as(u32p), None, None, None)
    for what, rc, want in (("NULL tokens", call(None, 8), _lib.ERR_INVALID), ("n = 0", call(t8, 0), _lib.ERR_INVALID),
                           ("token >= V", call(bad_tok, 8), _lib.ERR_INVALID), ("target >= V", call(t8, 8, bad_tgt), _lib.ERR_INVALID),
                           ("KV full", call(long, long.size), _lib.ERR_KV_FULL)):
        assert rc == want, (what, rc, lib.nfai_hip_last_error())
        same_state(before, state(mgr, m, cap), what)
    stage = LlamaModel(mgr, synth.make_metadata(c.dims), sc.weights(c.dims, c.enc)[0], cap, dims=sc.ddict(c.dims), max_batch=max_batch,
                       layer_range=(0, 1))
    assert lib.nfai_hip_llama_score(stage.handle, t8.ctypes.data_as(u32p), 8, None, None, None, None) == _lib.ERR_UNSUPPORTED
    assert stage.Pos == 0
    stage.Dispose()
    # all outputs NULL is a valid call (the K / V rows and the state are what it leaves); the sequence goes on from there
    assert call(t8, 8) == 0 and m.Pos == len(lead) + 8
    m.Dispose()


def test_second_call_reuses_the_workspace(mgr):
    """The workspace is allocated by the first call: a second one (longer, from position 0 again) takes no device memory."""
    import torch
    for enc in ("f16", "q4_k_m"):           # the quantised head adds the fp16 scratch of one slab
        c = sc.Case(synth.TINY_D128, enc, False, 16, 35)
        _, toks, _, _, _ = sc.case_rows(c)
        m = make(mgr, c)
        m.Score(toks[:5])
        mgr.Synchronize()
        free1 = torch.cuda.mem_get_info()[0]
        m.Reset()
        a = m.Score(toks)
        m.Reset()
        b = m.Score(toks)
        mgr.Synchronize()
        assert torch.cuda.mem_get_info()[0] >= free1      # device memory did not grow
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))   # deterministic
        m.Dispose()
