"""The prompt phase of the layer pipeline on CPU (nfai_amd.pipeline.schedule_prompt_ticks / run_prompt_schedule): the wavefront of
(slot, chunk) jobs checked on a recording stage for any world size, slot count, prompt lengths and chunk size, and the whole
prompt -> decode recipe over gloo with 2 and 3 ranks, each stage computed by the CPU oracle: the tokens must equal a
single-process oracle run of the same prompts followed by greedy decode."""
import os
import socket

import numpy as np
import pytest

from nfai_amd import synth
from nfai_amd.pipeline import partition_layers, run_prompt_schedule, run_schedule, schedule_prompt_ticks

E_FAKE = 4


class _Buf:
    """A stand-in for a hand-off view: which stage / slot / direction it belongs to and how many floats it holds."""

    def __init__(self, rank, slot, kind, n):
        self.rank, self.slot, self.kind, self.numel = rank, slot, kind, n * E_FAKE


class _RecordingStage:
    def __init__(self, rank, log):
        self.rank, self.log = rank, log

    def prompt_first(self, slot, begin, n, tokens):
        self.log.append((self.rank, slot, begin, n))

    def prompt_middle(self, slot, n):
        self.log.append((self.rank, slot, None, n))

    def prompt_last(self, slot, n):
        self.log.append((self.rank, slot, None, n))

    def p_in(self, slot, n):
        return _Buf(self.rank, slot, "in", n)

    def p_out(self, slot, n):
        return _Buf(self.rank, slot, "out", n)


def _check_schedule(world, lengths, chunk):
    log = []
    ticks = [[] for _ in range(world)]
    for r in range(world):
        st = _RecordingStage(r, log)
        for t, posted in enumerate(schedule_prompt_ticks(st, r, world, lengths, chunk)):
            ticks[r].append((len(log), posted))
    n_chunks = [(n + chunk - 1) // chunk for n in lengths]
    n_jobs = sum(n_chunks)
    assert all(len(tk) == n_jobs + world - 1 for tk in ticks)
    # every (slot, chunk) visits every stage exactly once; per stage the chunks of a slot run in order, covering the prompt
    for r in range(world):
        mine = [e for e in log if e[0] == r]
        assert len(mine) == n_jobs
        for s, n in enumerate(lengths):
            sizes = [e[3] for e in mine if e[1] == s]
            assert sizes == [min(chunk, n - c * chunk) for c in range(n_chunks[s])]
            if r == 0:
                assert [e[2] for e in mine if e[1] == s] == [c * chunk for c in range(n_chunks[s])]
        # every stage runs the jobs in the same order (so each job reaches stage r + 1 one tick after stage r)
        if r:
            assert [e[1:2] + e[3:] for e in mine] == [e[1:2] + e[3:] for e in log if e[0] == 0]
    # the exchange: every send has its receive in the same tick on the same link, of the same slot and size; never a 1-float buffer
    for t in range(n_jobs + world - 1):
        sends = [(r, b, dst) for r in range(world) for b, dst in ticks[r][t][1][0]]
        recvs = [(r, b, src) for r in range(world) for b, src in ticks[r][t][1][1]]
        assert len(sends) == len(recvs)
        for r, b, dst in sends:
            assert dst == r + 1 and b.kind == "out"
            m = [rb for rr, rb, src in recvs if rr == dst and src == r]
            assert len(m) == 1 and m[0].slot == b.slot and m[0].numel == b.numel and b.numel > 1
    # stage r has run exactly its first t - r + 1 jobs when it posts tick t's exchange (job j at tick j + r)
    for r in range(world):
        ran = [sum(1 for e in log[:cnt] if e[0] == r) for cnt, _ in ticks[r]]
        assert ran == [min(max(t - r + 1, 0), n_jobs) for t in range(n_jobs + world - 1)]


@pytest.mark.parametrize("seed", range(60))
def test_prompt_schedule_properties(seed):
    rng = np.random.default_rng(seed)
    world = int(rng.integers(1, 9))
    n_slots = int(rng.integers(1, world + 1))
    lengths = [int(x) for x in rng.integers(0, 301, n_slots)]
    if seed % 7 == 0:
        lengths[0] = 0
    chunk = int(rng.integers(1, 129))
    _check_schedule(world, lengths, chunk)


def test_prompt_schedule_tick_of_each_job():
    """Stage r runs job j at tick j + r: recorded per tick on a 3-stage pipeline with ragged prompts."""
    world, lengths, chunk = 3, [5, 0, 3], 2
    per_tick = {}
    for r in range(world):
        log = []
        st = _RecordingStage(r, log)
        for t, _ in enumerate(schedule_prompt_ticks(st, r, world, lengths, chunk)):
            per_tick[(r, t)] = list(log)
            log.clear()
    jobs = [(0, 2), (2, 2), (0, 2), (2, 1), (0, 1)]   # (slot, rows): round 0 of slots 0 and 2, round 1, then slot 0's last
    for r in range(world):
        for t in range(len(jobs) + world - 1):
            j = t - r
            want = [(jobs[j][0], jobs[j][1])] if 0 <= j < len(jobs) else []
            assert [(e[1], e[3]) for e in per_tick[(r, t)]] == want, (r, t)


class _OraclePromptStage:
    """A pipeline stage computed by the CPU oracle: the prompt phase token by token (what a stage's ingest computes up to the
    precision of the MFMA path), then the decode schedule of tests/test_pipeline.py."""

    def __init__(self, torch, dims, weights, lrange, n_slots, C):
        import oracle as orc
        self.torch, self.orc, self.dims, self.lrange, self.w = torch, orc, dims, lrange, weights
        desc = orc.LlamaDesc(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, C=C)
        self.models = [orc.OracleLlama(desc, weights) for _ in range(n_slots)]
        self._hin = [torch.zeros(dims.E) for _ in range(n_slots)]
        self._hout = [torch.zeros(dims.E) for _ in range(n_slots)]
        self._tok = [torch.zeros(1, dtype=torch.int32) for _ in range(n_slots)]
        self._pin = [torch.zeros(0) for _ in range(n_slots)]
        self._pout = [torch.zeros(0) for _ in range(n_slots)]
        self.tokens = [[] for _ in range(n_slots)]

    def _run(self, slot, hidden):
        m = self.models[slot]
        h = m.layers(hidden, *self.lrange)
        m.advance()
        return h

    # -- prompt phase
    def _rows(self, bufs, s, n):
        if bufs[s].numel() != n * self.dims.E:
            bufs[s] = self.torch.zeros(n * self.dims.E)
        return bufs[s]

    def p_in(self, s, n):
        return self._rows(self._pin, s, n)

    def p_out(self, s, n):
        return self._rows(self._pout, s, n)

    def prompt_first(self, slot, begin, n, tokens):
        out = self.p_out(slot, n).view(n, self.dims.E)
        for i, t in enumerate(tokens):
            out[i] = self.torch.from_numpy(self._run(slot, self.w["token_embd.weight"][int(t)].astype(np.float32)))

    def prompt_middle(self, slot, n):
        rows = self.p_in(slot, n).view(n, self.dims.E).numpy().copy()
        out = self.p_out(slot, n).view(n, self.dims.E)
        for i in range(n):
            out[i] = self.torch.from_numpy(self._run(slot, rows[i]))

    def prompt_last(self, slot, n):
        rows = self.p_in(slot, n).view(n, self.dims.E).numpy().copy()
        for i in range(n):
            self._run(slot, rows[i])

    # -- decode phase (schedule_ticks)
    def h_in(self, s):
        return self._hin[s]

    def h_out(self, s):
        return self._hout[s]

    def tok(self, s):
        return self._tok[s]

    def first(self, slot, token):
        if token is None:
            token = int(self._tok[slot].item())
        h = self.w["token_embd.weight"][token].astype(np.float32)
        self._hout[slot].copy_(self.torch.from_numpy(self._run(slot, h)))

    def middle(self, slot):
        self._hout[slot].copy_(self.torch.from_numpy(self._run(slot, self._hin[slot].numpy())))

    def last(self, slot):
        orc = self.orc
        h = self._run(slot, self._hin[slot].numpy())
        xn = orc.rmsnorm(h, self.w["output_norm.weight"], 1e-5)
        head = self.w.get("output.weight", self.w["token_embd.weight"])
        t = orc.argmax(orc.gemv_f16w(head, xn))
        self.tokens[slot].append(t)
        self._tok[slot][0] = t


class _CountingComm:
    def __init__(self, inner):
        self.inner, self.checks = inner, 0

    def exchange(self, sends, recvs):
        self.inner.exchange(sends, recvs)

    def check(self):
        self.checks += 1


def _prompts(world, V):
    rng = np.random.default_rng(17 + world)
    lengths = [7, 1, 12][:world]
    return [[int(t) for t in rng.integers(0, V, n)] for n in lengths]


def _worker(rank, world, port, n_steps, chunk, C, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from nfai_amd.pipeline import TorchComm
    dims = synth.TINY_D128
    w = synth.make_weights(dims, seed=41, std=0.05)
    ranges = partition_layers(dims.L, world)
    stage = _OraclePromptStage(torch, dims, w, ranges[rank], world, C)
    prompts = _prompts(world, dims.V)
    comm = _CountingComm(TorchComm(dist))
    run_prompt_schedule(stage, comm, rank, world, [p[:-1] for p in prompts], chunk)
    n_jobs = sum((len(p) - 1 + chunk - 1) // chunk for p in prompts)
    assert comm.checks == (n_jobs + world - 1) // world
    run_schedule(stage, comm, rank, world, n_steps, [p[-1] for p in prompts])
    dist.barrier()
    if rank == world - 1:
        q.put(stage.tokens)
    dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world", [2, 3])
def test_prompt_then_decode_gloo(world):
    import torch.multiprocessing as mp
    import oracle as orc
    n_steps, chunk, C = 5, 4, 24
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_steps, chunk, C, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = q.get(timeout=180)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    dims = synth.TINY_D128
    w = synth.make_weights(dims, seed=41, std=0.05)
    desc = orc.LlamaDesc(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, C=C)
    for s, prompt in enumerate(_prompts(world, dims.V)):
        ref = orc.OracleLlama(desc, w)
        for t in prompt[:-1]:
            ref.step(t)
        tok, want = prompt[-1], []
        for _ in range(n_steps):
            tok = orc.argmax(ref.step(tok))
            want.append(tok)
        assert got[s] == want, (s, got[s], want)
