"""CPU tier of the batched frame calls (snapmi_frame_compress_batch /
snapmi_frame_decompress_batch): the ABI - exported by both libraries, bound by
_lib with the header's parameter count, argument errors without a GPU."""
import ctypes as C
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("snapmi_frame_compress_batch", "snapmi_frame_decompress_batch")
SNAPMI_E_ARGUMENT = 101


def header_params(name):
    text = (ROOT / "include" / "snapmi.h").read_text()
    m = re.search(r"SNAPMI_API\s+int\s+" + name + r"\s*\(([^;]*?)\)\s*;",
                  text, re.S)
    assert m, f"{name} is not declared in include/snapmi.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)],
                         capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if " T " in ln}


def test_both_libraries_export_the_batch_frame_calls(built):
    pkg = ROOT / "rust-snappy_amd"
    for lib in ("libsnapmi.so", "libsnapmi_test.so"):
        syms = exported(pkg / lib)
        for name in NAMES:
            assert name in syms, f"{lib} does not export {name}"
    # the product library stays within its export budget
    assert len(exported(pkg / "libsnapmi.so")) <= 60


def test_lib_binds_the_header_parameter_count(built):
    from rust_snappy_amd import _lib
    table = {name: args for name, _, args in _lib.SYMBOLS}
    L = _lib.load()
    for name in NAMES:
        params = header_params(name)
        assert len(table[name]) == len(params), (name, params)
        assert len(getattr(L, name).argtypes) == len(params)
    # the shape of the raw batch calls: the context first, n last, the
    # compress call with the host copy of the lengths
    for name in NAMES:
        assert header_params(name)[0] == "snapmi_ctx *ctx"
        assert header_params(name)[-1] == "size_t n"
    assert header_params(NAMES[0])[3] == "const uint64_t *h_in_lens"


def test_null_context_is_an_argument_error(built):
    from rust_snappy_amd import _lib
    for L in (_lib.load(), _lib.load_product()):
        dummy = (C.c_void_p * 1)()
        lens = (C.c_uint64 * 1)(5)
        assert L.snapmi_frame_compress_batch(
            None, dummy, dummy, lens, dummy, None, dummy, None, 1) == \
            SNAPMI_E_ARGUMENT
        assert L.snapmi_frame_decompress_batch(
            None, dummy, dummy, dummy, dummy, dummy, None, 1) == \
            SNAPMI_E_ARGUMENT
        # n == 0 does not make a missing context acceptable
        assert L.snapmi_frame_compress_batch(
            None, None, None, None, None, None, None, None, 0) == \
            SNAPMI_E_ARGUMENT
        assert L.snapmi_frame_decompress_batch(
            None, None, None, None, None, None, None, 0) == SNAPMI_E_ARGUMENT
