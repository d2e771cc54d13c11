"""CPU-side checks of nfai_hip_llama_batch_create_ex (the batch that also admits Q4_K / Q6_K members): exported, declared with 4
parameters, bound in ctypes and in the C# P/Invoke surface with matching counts; bad arguments are error codes with a message,
never a crash.  No GPU needed: every call here is refused before it touches the device.  The pattern of tests/test_batch_decode.py."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "nfai_hip_llama_batch_create_ex"


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


def _err(lib):
    return lib.nfai_hip_last_error().decode("utf-8", "replace")


def test_symbol_exported_declared_and_bound(lib):
    from nfai_amd import _lib
    raw = C.CDLL(os.path.join(ROOT, "nfai_amd", "csrc", "libnfai_hip.so"))
    assert hasattr(raw, NAME), f"{NAME} is not exported"
    assert _header_params().get(NAME) == 4
    assert len(_lib.SIGNATURES[NAME]) == 4
    cs = open(os.path.join(ROOT, "csharp", "NFAI.HIP", "NativeMethods.g.cs")).read()
    m = re.search(r"\b" + NAME + r"\(([^)]*)\)", cs)
    assert m, f"{NAME} is missing from NativeMethods.g.cs"
    assert m.group(1).count(",") + 1 == 4, m.group(1)
    header = open(os.path.join(ROOT, "include", "nfai_hip.h")).read()
    assert re.search(r"NFAI_BATCH_QUANT\s*=\s*1u\s*<<\s*0", header)
    assert _lib.BATCH_QUANT == 1


def test_generated_csharp_is_current():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_csharp_bindings.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_hosts_take_the_quantized_argument():
    import inspect
    from nfai_amd.llama_model import LlamaBatch
    p = inspect.signature(LlamaBatch.__init__).parameters
    assert "quantized" in p and p["quantized"].default is False
    src = open(os.path.join(ROOT, "csharp", "NFAI.HIP", "HipLlamaBatch.cs")).read()
    assert NAME in src and "bool quantized = false" in src
    assert "nfai_hip_llama_batch_create(" in src   # the default path is unchanged


@pytest.mark.parametrize("flags", [0, 1])
def test_bad_arguments_are_errors_not_crashes(lib, flags):
    from nfai_amd import _lib
    h = _lib.H()
    dead = (_lib.H * 8)(*([987654321] * 8))
    for models, n, what in ((dead, 1, "dead handle"), (dead, 0, "n = 0"), (dead, 9, "n = 9"), (None, 2, "NULL list")):
        rc = lib.nfai_hip_llama_batch_create_ex(models, n, flags, C.byref(h))
        assert rc == _lib.ERR_INVALID, (what, rc)
        assert "invalid" in _err(lib) or "null" in _err(lib), (what, _err(lib))
        assert "batch_create_ex" in _err(lib), (what, _err(lib))
    rc = lib.nfai_hip_llama_batch_create_ex(dead, 1, flags, None)
    assert rc == _lib.ERR_INVALID and "null" in _err(lib)


@pytest.mark.parametrize("flags", [2, 3, 0x80000000, 0xFFFFFFFE])
def test_unknown_flag_bits_are_invalid(lib, flags):
    from nfai_amd import _lib
    h = _lib.H()
    dead = (_lib.H * 8)(*([987654321] * 8))
    rc = lib.nfai_hip_llama_batch_create_ex(dead, 1, flags, C.byref(h))
    assert rc == _lib.ERR_INVALID, rc
    assert "flags" in _err(lib), _err(lib)
    with pytest.raises(_lib.NfaiHipError, match="invalid flags"):
        _lib.call(NAME, dead, 1, flags, C.byref(h))
