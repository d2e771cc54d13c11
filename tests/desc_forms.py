"""Named forms of the four nfai_llama_desc values that change the arithmetic of every token (rope_dims, rope_n_freqs, rope_base, eps),
shared by tests/test_desc_forms.py (CPU) and tests/test_gpu_desc_forms.py.  Every other model in tests/ and tools/ sits at ONE point
(rope_dims = D, the full frequency table, base 500000, eps 1e-5), where no kernel takes the "do not rotate" side of its d < rope_dims
branch, a table of D / 2 entries cannot be told from one of rope_dims / 2, a frequency formed with the denominator D / 2 equals one
formed with rope_dims / 2, and eps is 0.4 % of the mean square it is added to.

Forms (for a LlamaDims with head size D):
  half   rope_dims = D / 2, full table, base 500000, eps = EPS_BIG
  six    rope_dims = 6, base 10000, eps = EPS_BIG: three frequencies; the rotate / don't-rotate boundary lies inside a 16-column
         block of the prefill epilogue and inside a 4-row group.  (It was to carry eps = 1e-6; against 1e-5 that moves a normalised
         vector by 0.2 %: 4 bars of the tightest path in the K rows, 0.1 of the loosest: a small eps cannot be told from the
         default by any test at these bars.  With eps = 1e-2 q and k shrink so far that the frequencies formed with D / 2 move
         the fp16-KV / prefill logits by 4.3 bars only; with 1e-3 it is 5.7.)
  cut    rope_dims = 24, rope_n_freqs = 5, base 1000, eps = 1e-5: truncation inside a partial rotation.  (It was to carry base
         500000, where the first truncated frequency is 4e-3: the full table in its place then moves the logits by 0.96 of the
         fp16-KV / prefill bar on tiny-llama; at base 10000 by 4.4; at base 1000, where that frequency is 0.06, by 10.7.)
  ref32  (D = 128 only) rope_dims = 128, rope_n_freqs = 32, base 10000: the table length of the model factory's reference-parity
         mode.  (At the factory's base 500000 the truncated frequencies are below 1.5e-3 and the full table in their place moves
         the fp16-KV / prefill logits by 2.7 bars at position 99, 4.0 at 199; at base 10000 they start at 0.01 and it is 14.9.)
  none   rope_dims = 0: no rotation at all (every kernel's table read is in bounds there: include/nfai_hip.h), eps = EPS_BIG

For each form: model_args() is what LlamaModel takes (the metadata, the dims= dict, which overrides the metadata, and the
rope_n_freqs / rope_base keywords: the form's values are in all of them, so whichever the harness reads carries them) and odesc()
the matching oracle descriptor.

EPS_BIG = 1e-3.  It was to start at 1e-3 and rise by powers of ten until tests/test_desc_forms.py shows the required sensitivity.
1e-3 already does: the mean square of these models' residual stream is 2.5e-3 (embedding rows ~ N(0, 0.05^2)), so eps = 1e-3 moves
a normalised vector by 15 %.  Measured with eps replaced by 1e-5, smallest over half / none and both models: logits 390 bars and
K rows 349 bars of the fp32-KV decode, logits 9.8 and K rows 17.5 bars of the fp16-KV / prefill paths.  DESIGN.md lists every margin.

mutants() gives the wrong models a kernel could compute instead, as (rope_dims, frequency table, eps) for oracle.np_oracle:
  default   the default descriptor: the switch ignored
  dims_D    rope_dims replaced by D with the same table length: every pair is rotated, and pair i takes entry i mod (rope_dims / 2)
            of the form's table of rope_dims / 2 entries (a table stride of rope_dims under an index that runs to D).  Two other
            readings were tried and are NOT mutations: a table padded with zeros past rope_dims / 2 (what the library uploads:
            llama.hip sizes it by D) rotates the extra pairs by angle 0 and IS the form; and the form's own formula continued
            past rope_dims / 2 gives frequencies below 1 / base, under 1e-3 rad at these positions (measured: 0.1 bar).
            For rope_dims = 0 the table is the default one.
  denom_D   the frequencies formed with the denominator D / 2 instead of rope_dims / 2
  eps       eps replaced by 1e-5 (the forms whose eps differs)
  full      the full table (the forms that truncate it)
A mutation that does not change the model (dims_D and denom_D where rope_dims = D; all three table mutations where rope_dims = 0,
except that dims_D then rotates with the default table) is left out."""
from dataclasses import dataclass

import numpy as np

from nfai_amd import synth

EPS_BIG = 1e-3
N_POS = {"tiny-llama": 48, "tiny-llama-d128": 100}   # positions of a decode run: several KV slices on the larger model
N_WALK = 134                                         # the longest sequence a path walks: a 130-token prompt and 4 decode steps


@dataclass(frozen=True)
class Form:
    name: str
    rope_dims: int | None      # None: D / 2
    rope_n_freqs: int | None   # None: the full table, rope_dims / 2
    rope_base: float
    eps: float
    only_d: int | None = None  # the head size the form exists for


FORMS = {f.name: f for f in (
    Form("half", None, None, 500000.0, EPS_BIG),
    Form("six", 6, None, 10000.0, EPS_BIG),
    Form("cut", 24, 5, 1000.0, 1e-5),
    Form("ref32", 128, 32, 10000.0, 1e-5, only_d=128),
    Form("none", 0, None, 500000.0, EPS_BIG),
)}
DEFAULT = Form("default", -1, None, 500000.0, 1e-5)   # rope_dims = D


def forms_for(dims, none=True):
    """The names of the forms that exist for this head size (none=False: without the rope_dims = 0 form)."""
    return [n for n, f in FORMS.items() if (f.only_d is None or f.only_d == dims.D) and (none or n != "none")]


def resolve(form, dims):
    """(rope_dims, rope_n_freqs, rope_base, eps) of a form (or its name) for this model."""
    f = form if isinstance(form, Form) else (DEFAULT if form == "default" else FORMS[form])
    rd = dims.D // 2 if f.rope_dims is None else (dims.D if f.rope_dims < 0 else f.rope_dims)
    nf = rd // 2 if f.rope_n_freqs is None else f.rope_n_freqs
    assert rd % 2 == 0 and rd <= dims.D and nf <= rd // 2, (f, dims.name)
    return rd, nf, f.rope_base, f.eps


def ddict(dims, form):
    """The dims= dict of LlamaModel (it overrides the metadata)."""
    rd, _, base, eps = resolve(form, dims)
    return dict(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, eps=eps, rope_dims=rd, rope_base=base)


def metadata(dims, form):
    rd, _, base, eps = resolve(form, dims)
    md = synth.make_metadata(dims, eps=eps)
    md["llama.rope.dimension_count"] = rd
    md["llama.rope.freq_base"] = base
    return md


def model_args(dims, form):
    """(metadata, keyword arguments) for LlamaModel(mgr, metadata, tensors, capacity, **keywords)."""
    _, nf, base, _ = resolve(form, dims)
    return metadata(dims, form), dict(dims=ddict(dims, form), rope_n_freqs=nf, rope_base=base)


def odesc(dims, form, cap):
    import oracle as orc
    rd, nf, base, eps = resolve(form, dims)
    return orc.LlamaDesc(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, C=cap, eps=eps, rope_base=base,
                         rope_dims=rd, rope_n_freqs=nf)


def table(rd, nf, base, denom, n):
    """n frequencies base^-(i / denom), zero at nf <= i < rd / 2 (the truncation), float64."""
    i = np.arange(n, dtype=np.float64)
    f = base ** (-(i / denom)) if denom else np.zeros(n)
    f[(i >= nf) & (i < rd // 2)] = 0.0
    return f


def exact(form, dims):
    """(rope_dims, frequency table, eps) of the form itself, for NpModel."""
    rd, nf, base, eps = resolve(form, dims)
    return rd, table(rd, nf, base, rd / 2, rd // 2), eps


def mutants(form, dims):
    """{mutation: (rope_dims, frequency table, eps)}: the wrong models of the module docstring that differ from the form."""
    rd, nf, base, eps = resolve(form, dims)
    D = dims.D
    out = {"default": exact(DEFAULT, dims)}
    if rd == 0:
        out["dims_D"] = (D, table(D, D // 2, base, D / 2, D // 2), eps)
    elif rd < D:
        out["dims_D"] = (D, np.resize(table(rd, nf, base, rd / 2, rd // 2), D // 2), eps)
        out["denom_D"] = (rd, table(rd, nf, base, D / 2, rd // 2), eps)
    if eps != 1e-5:
        out["eps"] = (rd, table(rd, nf, base, rd / 2, rd // 2), 1e-5)
    if nf < rd // 2:
        out["full"] = (rd, table(rd, rd // 2, base, rd / 2, rd // 2), eps)
    return out


def NpModel(dims, w, cap, rd, freqs, eps):
    """oracle.np_oracle.NpLlama (fp64) with rope_dims, the frequency table and eps given directly, so that it can also be a model
    no descriptor describes."""
    import oracle as orc
    from oracle import np_oracle as npo
    m = npo.NpLlama(orc.LlamaDesc(E=dims.E, L=dims.L, H=dims.H, Hkv=dims.Hkv, D=dims.D, F=dims.F, V=dims.V, C=cap, eps=eps), w)
    m.rd, m.freqs = rd, np.asarray(freqs, np.float64)
    return m


def tokens(dims, n=None):
    """The sequence every run walks: the first n (default: N_POS) of N_WALK tokens, so that one oracle walk serves every path."""
    return [int(t) for t in synth.make_tokens(dims, N_WALK, seed=77)[:N_POS[dims.name] if n is None else n]]
