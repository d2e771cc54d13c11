"""nfai_hip_score_rows (kernels_score.hip) against the fp64 reference of tests/score_cases.py: every vocabulary width at which the row
kernel takes another path (one column, under / at / over one wave, under / at / over 4 columns per lane, a row that is not 16-byte
aligned, the real vocabulary), one row / a few / 128 / 129 rows, one pass and passes of 64, 192 and 8192 columns (also where the slab
does not divide V), a leading dimension over V with NaN in the padding.

Bar on both log-probabilities: 1e-5 * max(1, max|logit|).  fp32 rounding of l - max contributes <= 6e-8 * |logit| per term, a 17-level
sum and the exp about 1.2e-6 to the log: more than 4x under the bar.  The ArgMax must be exact (first index of the maximum)."""
import ctypes as C

import numpy as np
import pytest

import score_cases as sc

pytestmark = pytest.mark.gpu
NO = sc.NO_TARGET
KINDS = 10
SENT_F, SENT_U = np.float32(-12345.5), np.uint32(0xDEADBEEF)


@pytest.fixture(scope="module")
def mgr():
    from nfai_amd.hip import HipBufferManager
    m = HipBufferManager(0)
    yield m
    m.Dispose()


def make_rows(V, T, slab, first_kind, seed):
    """logits [T][V] fp32 and targets [T]: row r is of kind (first_kind + r) % KINDS (see the module's list in the code below)."""
    r = np.random.Generator(np.random.PCG64(seed))
    b = slab if 0 < slab < V else max(1, V // 2)          # a slab boundary (or the middle of a single pass)
    lg = r.standard_normal((T, V)).astype(np.float32)
    tg = r.integers(0, V, T).astype(np.uint32)
    for i in range(T):
        kind = (first_kind + i) % KINDS
        row = lg[i]
        if kind == 1:                                      # Gaussian at scale 3e4
            row *= np.float32(3e4)
        elif kind == 2:                                    # all equal
            row[:] = np.float32(-7.5)
        elif kind == 3:                                    # one logit at +80, the rest at -80; the target is one of the rest
            row[:] = -80.0
            j = int(r.integers(0, V))
            row[j] = 80.0
            tg[i] = (j + 1) % V
        elif kind == 4:                                    # the maximum at several indices on both sides of a slab boundary
            top = np.float32(row.max() + 1.0)
            for j in {min(j, V - 1) for j in (b - 1, b, b + 1, b + 70, V - 1)}:
                row[j] = top
            tg[i] = min(b, V - 1)                          # a later copy of the maximum: the same log-probability, another index
        elif kind == 5:                                    # the target is the ArgMax
            tg[i] = int(np.argmax(row))
        elif kind == 6:                                    # the target in the last (partial) slab
            tg[i] = V - 1
        elif kind == 7:                                    # the maximum in the last slab, the target in the first
            row[V - 1] = row.max() + np.float32(3.0)
            tg[i] = 0
        elif kind == 8:                                    # the maximum in the first slab, the target in the last
            row[0] = row.max() + np.float32(3.0)
            tg[i] = V - 1
        elif kind == 9:                                    # no target
            tg[i] = NO
    return lg, tg


def run(mgr, lg, tg, V, ld, slab, expect_ok=True):
    """One call; returns (logprob, argmax, logprob_max, status).  Padding columns [V, ld) hold NaN; four sentinels behind every output."""
    from nfai_amd import _lib
    from nfai_amd.hip import ShaderProperty
    T = lg.shape[0]
    full = np.full((T, ld), np.nan, np.float32)
    full[:, :V] = lg
    flat = full.reshape(-1)[:(T - 1) * ld + V]             # the last row ends at its V-th column: nothing behind it is the buffer's
    pl, pt = ShaderProperty(mgr, flat.size), ShaderProperty(mgr, T, np.uint32)
    outs = [ShaderProperty(mgr, T + 4), ShaderProperty(mgr, T + 4, np.uint32), ShaderProperty(mgr, T + 4)]
    pl.SetValue(flat)
    pt.SetValue(tg)
    for p, s in zip(outs, (SENT_F, SENT_U, SENT_F)):
        p.SetValue(np.full(T + 4, s, p.dtype))
    rc = _lib.load().nfai_hip_score_rows(mgr.handle, pl.handle, T, V, ld, slab, pt.handle, outs[0].handle, outs[1].handle, outs[2].handle)
    got = [p.GetValue() for p in outs]
    for p in [pl, pt] + outs:
        p.buffer.free()
    for g, s in zip(got, (SENT_F, SENT_U, SENT_F)):
        assert (g[T:] == s).all(), "an output array was written past its T entries"
    return got[0][:T], got[1][:T], got[2][:T], rc


def check(mgr, V, T, slab, ld, first_kind, seed):
    lg, tg = make_rows(V, T, slab, first_kind, seed)
    lp, am, lpm, rc = run(mgr, lg, tg, V, ld, slab)
    assert rc == 0
    want_lp, want_am, want_lpm = sc.score_rows_ref(lg, tg)
    bar = 1e-5 * np.maximum(1.0, np.abs(lg).max(axis=1))
    assert np.isfinite(lp).all() and np.isfinite(lpm).all()
    where = f"V={V} T={T} slab={slab} ld={ld} kinds from {first_kind}"
    assert np.array_equal(am, want_am), (where, np.nonzero(am != want_am)[0][:8], am[am != want_am][:8], want_am[am != want_am][:8])
    e1, e2 = np.abs(lp - want_lp) / bar, np.abs(lpm - want_lpm) / bar
    assert e1.max() <= 1.0 and e2.max() <= 1.0, (where, float(e1.max()), int(e1.argmax()), float(e2.max()), int(e2.argmax()))
    assert (lp[tg == NO] == 0.0).all()


VS = [1, 63, 64, 65, 512, 1000, 4097, 128256]
SLABS = [0, 64, 192, 8192]


@pytest.mark.parametrize("slab", SLABS)
@pytest.mark.parametrize("V", VS)
def test_score_rows(mgr, V, slab):
    """T in {1, 3, 128, 129} (1, 3 and 8 at the real vocabulary); ld = V, V + 3 (rows off the 16-byte grid) and the next multiple of 4
    + 4 (aligned rows, padded); every row kind on every (V, slab), also at T = 1 and 3 (one launch per first kind)."""
    for T in ([1, 3, 8] if V > 100000 else [1, 3, 128, 129]):
        lds = [V, V + 3, (V + 3) // 4 * 4 + 4]
        if V > 100000:
            starts = [0, 3, 6] if T == 3 else ([4] if T == 1 else [2])   # T = 3: kinds 0..8; T = 1: the tie row; T = 8: kinds 2..9
        else:
            starts = range(0, KINDS, T) if T < KINDS else [T % KINDS]
        for k, first in enumerate(starts):
            check(mgr, V, T, slab, lds[(k + T) % 3], first, 1000 * V + 10 * T + k)


def test_score_rows_refusals(mgr):
    """Each refusal is NFAI_ERR_INVALID; a bad target is found on the device and leaves all three outputs unwritten."""
    from nfai_amd import _lib
    from nfai_amd.hip import ShaderProperty
    lib = _lib.load()
    lg, tg = make_rows(512, 3, 0, 0, 1)
    for V, T, ld, slab in ((0, 3, 512, 0), (512, 0, 512, 0), (512, 3, 511, 0), (512, 3, 512, 100), (512, 3, 512, 32)):
        pl, pt, po = ShaderProperty(mgr, 3 * 512), ShaderProperty(mgr, 3, np.uint32), ShaderProperty(mgr, 3)
        pu = ShaderProperty(mgr, 3, np.uint32)
        assert lib.nfai_hip_score_rows(mgr.handle, pl.handle, T, V, ld, slab, pt.handle, po.handle, pu.handle, po.handle) == _lib.ERR_INVALID, (V, T, ld, slab)
    # buffers too small: logits one float short, each of the others one entry short
    sizes = dict(l=3 * 512, t=3, p=3, a=3, m=3)
    for short in sizes:
        n = dict(sizes)
        n[short] -= 1
        b = dict(l=ShaderProperty(mgr, n["l"]), t=ShaderProperty(mgr, n["t"], np.uint32), p=ShaderProperty(mgr, n["p"]),
                 a=ShaderProperty(mgr, n["a"], np.uint32), m=ShaderProperty(mgr, n["m"]))
        rc = lib.nfai_hip_score_rows(mgr.handle, b["l"].handle, 3, 512, 512, 0, b["t"].handle, b["p"].handle, b["a"].handle, b["m"].handle)
        assert rc == _lib.ERR_INVALID, short
    for bad in (512, 0xFFFFFFFE):
        t2 = tg.copy()
        t2[1] = bad
        for slab in (0, 64):
            lp, am, lpm, rc = run(mgr, lg, t2, 512, 512, slab)
            assert rc == _lib.ERR_INVALID and b"target" in lib.nfai_hip_last_error()
            assert (lp == SENT_F).all() and (am == SENT_U).all() and (lpm == SENT_F).all()
    lp, am, lpm, rc = run(mgr, lg, tg, 512, 512, 64)      # the error word does not outlive the call
    assert rc == 0 and np.array_equal(am, np.argmax(lg, axis=1))
