"""CPU-side checks of NFAI_BATCH_QUANT_ANY (the flag that, with NFAI_BATCH_QUANT, lets a batch or a window take Q5_K and Q8_0
matrices too): declared, bound in ctypes and in both C# hosts, and the flag rules are error codes with a message.  No GPU needed:
every call here is refused before it touches the device.  The pattern of tests/test_batch_quant.py."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEAD = 987654321


@pytest.fixture(scope="module")
def lib():
    from nfai_amd import build as hb, _lib
    hb.build()
    return _lib.load()


def _err(lib):
    return lib.nfai_hip_last_error().decode("utf-8", "replace")


def _create(lib, which, flags):
    """(status, message) of a creation over a dead model handle."""
    from nfai_amd import _lib
    h = _lib.H()
    if which == "batch":
        dead = (_lib.H * 8)(*([DEAD] * 8))
        rc = lib.nfai_hip_llama_batch_create_ex(dead, 1, flags, C.byref(h))
    else:
        rc = lib.nfai_hip_llama_window_create(_lib.H(DEAD), 4, flags, C.byref(h))
    return rc, _err(lib)


def test_flag_is_declared_and_bound():
    from nfai_amd import _lib
    header = open(os.path.join(ROOT, "include", "nfai_hip.h")).read()
    assert re.search(r"NFAI_BATCH_QUANT_ANY\s*=\s*1u\s*<<\s*2", header)
    assert re.search(r"NFAI_BATCH_QUANT\s*=\s*1u\s*<<\s*0", header)
    assert "reserved" in header[header.index("enum nfai_batch_flags"):header.index("nfai_hip_llama_batch_create_ex(")]
    assert _lib.BATCH_QUANT_ANY == 4 and _lib.BATCH_QUANT == 1
    assert len(_lib.SIGNATURES["nfai_hip_llama_batch_create_ex"]) == 4 and len(_lib.SIGNATURES["nfai_hip_llama_window_create"]) == 4


@pytest.mark.parametrize("which", ["batch", "window"])
def test_both_flags_reach_the_handle_check(lib, which):
    from nfai_amd import _lib
    rc, msg = _create(lib, which, 5)
    assert rc == _lib.ERR_INVALID, rc
    assert "invalid model handle" in msg and "flags" not in msg, msg


@pytest.mark.parametrize("which", ["batch", "window"])
def test_any_without_quant_is_invalid_and_names_the_rule(lib, which):
    from nfai_amd import _lib
    rc, msg = _create(lib, which, 4)
    assert rc == _lib.ERR_INVALID, rc
    assert "NFAI_BATCH_QUANT_ANY" in msg and re.search(r"NFAI_BATCH_QUANT\b(?!_)", msg), msg
    assert "handle" not in msg, msg


@pytest.mark.parametrize("flags", [6, 7, 8, 0x80000005])
@pytest.mark.parametrize("which", ["batch", "window"])
def test_unknown_bits_beside_the_new_flag_are_invalid(lib, which, flags):
    from nfai_amd import _lib
    rc, msg = _create(lib, which, flags)
    assert rc == _lib.ERR_INVALID, rc
    assert "invalid flags" in msg, msg


def test_hosts_take_the_any_quant_argument():
    from nfai_amd.llama_model import LlamaBatch, LlamaWindow
    for cls in (LlamaBatch, LlamaWindow):
        p = inspect.signature(cls.__init__).parameters
        assert "any_quant" in p and p["any_quant"].default is False
        assert list(p).index("any_quant") > list(p).index("quantized")
    for name in ("HipLlamaBatch.cs", "HipLlamaWindow.cs"):
        src = open(os.path.join(ROOT, "csharp", "NFAI.HIP", name)).read()
        assert re.search(r"bool quantized = false,\s*bool anyQuant = false", src), name


def test_any_quant_needs_quantized_before_any_device_call():
    """The models are objects without a handle: the ValueError comes before anything reads one."""
    from nfai_amd.llama_model import LlamaBatch, LlamaWindow
    with pytest.raises(ValueError, match="quantized"):
        LlamaBatch([object()], quantized=False, any_quant=True)
    with pytest.raises(ValueError, match="quantized"):
        LlamaWindow(object(), 4, quantized=False, any_quant=True)


def test_generated_csharp_is_current():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_csharp_bindings.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
