"""CPU-side checks of the batched decode entry points (nfai_hip_llama_batch_*): exported, declared, bound in ctypes and in the
C# P/Invoke surface with matching parameter counts; bad arguments are error codes with a message, never a crash.  No GPU needed:
every call here is refused before it touches the device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BATCH_FUNCTIONS = {
    "nfai_hip_llama_batch_create": 3,
    "nfai_hip_llama_batch_destroy": 1,
    "nfai_hip_llama_batch_step": 4,
    "nfai_hip_llama_batch_greedy": 4,
    "nfai_hip_llama_batch_bytes_per_token": 2,
}


@pytest.fixture(scope="module")
def lib():
    from nfai_amd import build as hb, _lib
    hb.build()
    return _lib.load()


def _header_params():
    src = open(os.path.join(ROOT, "include", "nfai_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(nfai_hip_\w+)\s*\(([^;{]*?)\)\s*;", src):
        params = " ".join(m.group(2).split())
        out[m.group(1)] = 0 if params in ("", "void") else params.count(",") + 1
    return out


def test_symbols_exported_declared_and_bound(lib):
    from nfai_amd import _lib
    header = _header_params()
    raw = C.CDLL(os.path.join(ROOT, "nfai_amd", "csrc", "libnfai_hip.so"))
    cs = open(os.path.join(ROOT, "csharp", "NFAI.HIP", "NativeMethods.g.cs")).read()
    for name, nparams in BATCH_FUNCTIONS.items():
        assert hasattr(raw, name), f"{name} is not exported"
        assert header.get(name) == nparams, (name, header.get(name))
        assert len(_lib.SIGNATURES[name]) == nparams, name
        m = re.search(r"\b" + name + r"\(([^)]*)\)", cs)
        assert m, f"{name} is missing from NativeMethods.g.cs"
        assert m.group(1).count(",") + 1 == nparams, (name, m.group(1))
    assert "typedef uint64_t nfai_batch_t;" in open(os.path.join(ROOT, "include", "nfai_hip.h")).read()


def test_generated_csharp_is_current():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_csharp_bindings.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_host_has_the_batch_class():
    from nfai_amd.llama_model import LlamaBatch
    for method in ("Step", "Greedy", "BytesPerToken", "Dispose"):
        assert callable(getattr(LlamaBatch, method))
    src = open(os.path.join(ROOT, "csharp", "NFAI.HIP", "HipLlamaBatch.cs")).read()
    for name in BATCH_FUNCTIONS:
        assert name in src, f"HipLlamaBatch does not call {name}"


def _err(lib):
    return lib.nfai_hip_last_error().decode("utf-8", "replace")


def test_bad_arguments_are_errors_not_crashes(lib):
    """The pattern of test_abi.py::test_invalid_handles_are_errors_not_crashes: an error code and a non-empty message."""
    from nfai_amd import _lib
    h = _lib.H()
    dead = (_lib.H * 8)(*([987654321] * 8))
    for models, n, what in ((dead, 1, "dead handle"), (dead, 0, "n = 0"), (dead, 9, "n = 9"), (None, 2, "NULL list")):
        rc = lib.nfai_hip_llama_batch_create(models, n, C.byref(h))
        assert rc == _lib.ERR_INVALID, (what, rc)
        assert "invalid" in _err(lib) or "null" in _err(lib), (what, _err(lib))
        assert _err(lib), what
    rc = lib.nfai_hip_llama_batch_create(dead, 1, None)
    assert rc == _lib.ERR_INVALID and _err(lib)
    toks = (C.c_uint32 * 8)()
    am = (C.c_uint32 * 8)()
    total = C.c_uint64()
    for name, args in (("nfai_hip_llama_batch_step", (123456789, toks, None, am)),
                       ("nfai_hip_llama_batch_destroy", (123456789,)),
                       ("nfai_hip_llama_batch_destroy", (0,)),
                       ("nfai_hip_llama_batch_greedy", (123456789, toks, 4, am)),
                       ("nfai_hip_llama_batch_bytes_per_token", (123456789, C.byref(total)))):
        with pytest.raises(_lib.NfaiHipError, match="invalid"):
            _lib.call(name, *args)
    # a live handle of another kind (a context would need a GPU; the registry is shared, so a dead one of each kind is the CPU-side check)
    with pytest.raises(_lib.NfaiHipError, match="invalid"):
        _lib.call("nfai_hip_llama_batch_step", 0, toks, None, am)
