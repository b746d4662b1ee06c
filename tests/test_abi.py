"""The C-ABI library loads (no GPU needed) and exports every symbol include/sfx.h declares; the header, the
definitions under csrc/ and the ctypes signatures (parsed from the header) name the same entry points."""
import ctypes
import glob
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "sfx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sfx_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_entry_points():
    syms = declared_symbols()
    assert "sfx_rasterize_fwd" in syms and "sfx_sort_pairs_u64" in syms
    assert len(syms) >= 15


def test_library_exports_all_declared_symbols():
    from splatformer_amd import _lib
    lib = _lib.load()
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, f"libsfx.so lacks: {missing}"
    assert lib.sfx_abi_version() == 17


def test_python_signatures_cover_header():
    from splatformer_amd import _lib  # alone: no op module has to be imported for the table to be complete
    missing = [s for s in declared_symbols() if s not in _lib.SIGNATURES]
    assert not missing, f"no ctypes signature for: {missing}"


def defined_symbols():
    """sfx_* functions with a body in csrc/*.hip (the extern "C" definitions; kernels return void and do not match)."""
    names = []
    for path in glob.glob(os.path.join(ROOT, "splatformer_amd", "csrc", "*.hip")):
        src = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(path).read(), flags=re.S)
        names += re.findall(r'^(?:extern "C" )?(?:int|size_t|long long|const char\s*\*)\s*\b(sfx_\w+)\s*\([^;{}]*\)\s*'
                            r'\{', src, flags=re.M)
    return names


def test_header_definitions_and_signatures_name_the_same_entry_points():
    from splatformer_amd import _lib
    defined = defined_symbols()
    assert len(defined) == len(set(defined)), "an entry point is defined twice"
    declared = set(declared_symbols())
    assert declared == set(defined), (sorted(declared - set(defined)), sorted(set(defined) - declared))
    assert declared == set(_lib.SIGNATURES)
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in declared)


def test_no_hand_redeclared_prototypes_in_csrc():
    """Every translation unit sees the prototypes through common.h -> sfx.h, so the compiler compares each
    definition with its declaration; a hand re-declaration would hide a drift from it."""
    csrc = os.path.join(ROOT, "splatformer_amd", "csrc")
    assert '#include "sfx.h"' in open(os.path.join(csrc, "common.h")).read()
    for path in glob.glob(os.path.join(csrc, "*")):
        src = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(path).read(), flags=re.S)
        assert not re.search(r'extern\s+"C"\s+[^{;]*\bsfx_\w+\s*\([^{}]*?\)\s*;', src), path
        assert not re.search(r"#\s*define\s+SFX_(OK|ERR_)", src), path


def test_signatures_do_not_depend_on_import_order():
    """A fresh interpreter that imports _lib alone has every entry point bound with its full argtypes."""
    code = ("from splatformer_amd import _lib\n"
            "lib = _lib.load()\n"
            "assert len(_lib.SIGNATURES) > 100\n"
            "for name, args in _lib.SIGNATURES.items():\n"
            "    f = _lib.fn(name)\n"
            "    assert f.argtypes is not None and len(f.argtypes) == len(args), name\n"
            "    assert getattr(lib, name).argtypes is not None, name\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_pinned_signatures():
    """Literal copies of hand-typed signatures (not produced by the parser) the parsed table must reproduce."""
    from splatformer_amd import _lib
    I, U, L, F, Z, P = (ctypes.c_int, ctypes.c_uint, ctypes.c_longlong, ctypes.c_float, ctypes.c_size_t,
                        ctypes.c_void_p)
    S = _lib.SIGNATURES
    assert S["sfx_sh_fwd"] == [I, I, I, P, P, P, P]
    assert S["sfx_scan_i32"] == [L, P, P, I, P, Z, P, P]
    assert S["sfx_drop_mask"] == [L, F, ctypes.c_ulonglong, P, P]
    assert S["sfx_render_prep_project"] == [I, I, P, L, P, L, P, L, P, L, P, L, P, L, P, F, F, F, F, I, I, I,
                                            P, P, P, P, P, P, P, P, P]
    assert S["sfx_rasterize_bwd_nd"] == [I] * 6 + [P] * 17
    assert S["sfx_linear"] == [I, I, I, P, L, P, I, P, L, P, P, P, I, I, P, L, P, P, L, P, L, I, L, L, L, L, P, P, I,
                               P, U, P, U, P, U, P, P, P]
    assert S["sfx_abi_version"] == [] and S["sfx_last_error"] == []
    lib = _lib.load()
    assert lib.sfx_last_error.restype is ctypes.c_char_p
    assert lib.sfx_sort_workspace_bytes.restype is ctypes.c_size_t
    assert lib.sfx_lookback_timeouts.restype is ctypes.c_longlong
    assert lib.sfx_sh_fwd.restype is ctypes.c_int
    for name, args in S.items():
        assert getattr(lib, name).argtypes == args, name


# (`double` is in the table: sfx_bn_finalize and sfx_bn_act_bwd_apply take a `double count`)
@pytest.mark.parametrize("text,name", [
    ("int sfx_ok(int a);\nint sfx_x(long double a);", "sfx_x"),   # a scalar type outside the table
    ("int sfx_x(short a);", "sfx_x"),
    ("float sfx_x(int a);", "sfx_x"),                              # a return type outside the table
    ("int sfx_y(struct foo a);", "sfx_y"),                         # a struct passed by value
    ("int sfx_y(int a)\nint sfx_ok(void);", "sfx_y"),              # a missing `;`
    ("int sfx_y(int (*cb)(int), void* stream);", "sfx_y"),         # a function pointer
])
def test_parser_is_strict(text, name):
    from splatformer_amd import _lib
    with pytest.raises(ValueError, match=rf"\b{name}\b"):
        _lib.parse_header(text)


def test_parser_reads_every_form_the_header_uses():
    from splatformer_amd import _lib
    sigs, rets = _lib.parse_header(
        "/* int sfx_in_comment(double); */\n#define SFX_X sfx_macro(\n// sfx_line(\n"
        "const char* sfx_a(void);\nsize_t sfx_b(long long n, const float* x,\n   unsigned tag, double d);\n"
        "long long sfx_c(void* stream, uint64_t k, const unsigned long long* p, unsigned long long s);\n")
    assert sigs == {"sfx_a": [], "sfx_b": [ctypes.c_longlong, ctypes.c_void_p, ctypes.c_uint, ctypes.c_double],
                    "sfx_c": [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_ulonglong]}
    assert rets == {"sfx_a": ctypes.c_char_p, "sfx_b": ctypes.c_size_t, "sfx_c": ctypes.c_longlong}


def test_stale_library_is_reported(monkeypatch):
    """load() names the declared symbol a library lacks and says to rebuild (here: a shared library that exports
    nothing of ours, the interpreter's own _ctypes extension)."""
    import _ctypes
    from splatformer_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(RuntimeError, match=r"sfx_\w+.*rebuild"):
        _lib.load(_ctypes.__file__)
    assert _lib._lib is None


def test_header_is_valid_c99():
    """include/sfx.h compiles on its own as C99 with the clang of the HIP compiler that builds the library."""
    from splatformer_amd import build_lib
    ver = subprocess.run([build_lib.HIPCC, "--version"], capture_output=True, text=True, check=True).stdout
    clang = os.path.join(re.search(r"InstalledDir:\s*(\S+)", ver).group(1), "clang")
    assert os.path.exists(clang), clang
    r = subprocess.run([clang, "-x", "c", "-std=c99", "-fsyntax-only", os.path.join(ROOT, "include", "sfx.h")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_invalid_args_report_errors_without_gpu():
    """Argument validation runs host-side and fails with a message (no kernel launched)."""
    from splatformer_amd import _lib
    lib = _lib.load()
    rc = lib.sfx_project_fwd(-1, None, None, 1.0, None, None, 1.0, 1.0, 0.0, 0.0, 8, 8, 16, 0.01,
                             None, None, None, None, None, None, None, None)
    assert rc == -1
    assert b"n < 0" in lib.sfx_last_error()
    rc = lib.sfx_sort_pairs_u64(10, None, None, None, None, 0, 70, None, 0, None)
    assert rc == -1
    assert b"bit range" in lib.sfx_last_error()


def test_no_cpu_fallback_on_cpu_tensors():
    import torch
    from splatformer_amd import gsplat_compat
    with pytest.raises(RuntimeError):
        gsplat_compat.spherical_harmonics(1, torch.randn(4, 3), torch.randn(4, 4, 3))
