"""ctypes binding of the libsfx C-ABI (include/sfx.h).

The product path has exactly one implementation: the HIP kernels in
`libsfx.so`.  If the library is missing, or no GPU is visible, every op raises
immediately -- there is no CPU fallback.  (The CPU restatement under
`oracle/` is test infrastructure only and is never imported from here.)
"""
from __future__ import annotations

import ctypes as C
import os
import re
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SFX_LIB", os.path.join(_HERE, "libsfx.so"))

HEADER = os.path.join(os.path.dirname(_HERE), "include", "sfx.h")

_SCALARS = {
    "int": C.c_int, "unsigned": C.c_uint, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong,
    "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "int32_t": C.c_int32, "int64_t": C.c_int64,
    "uint64_t": C.c_uint64,
}
_RETURNS = {"int": C.c_int, "size_t": C.c_size_t, "long long": C.c_longlong, "const char*": C.c_char_p}
_TYPE_WORDS = {w for t in _SCALARS for w in t.split()}
_PROTO = re.compile(r"([A-Za-z_][\w\s*]*?)\b(sfx_\w+)\s*\(([^(){};]*)\)\s*;")


def parse_header(text: str) -> tuple[dict[str, list], dict[str, type]]:
    """(name -> argtypes, name -> restype) of every `<ret> sfx_name(<params>);` prototype of a C header text.  A
    pointer parameter is a c_void_p (callers pass data_ptr() integers and None); scalar and return types come from
    the fixed tables above.  Strict: a type outside the tables, or an `sfx_name(` that is not part of a prototype
    of that form, raises and names the function -- a wrong guess would corrupt arguments silently."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    sigs, rets = {}, {}
    for ret, name, params in _PROTO.findall(text):
        ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
        if ret not in _RETURNS:
            raise ValueError(f"{name}: return type '{ret}' is not one the binding knows")
        args = []
        for prm in ([] if params.strip() == "void" else params.split(",")):
            words = re.sub(r"\bconst\b", " ", prm).split()
            ctype = " ".join(words if words and words[-1] in _TYPE_WORDS else words[:-1])  # drop the parameter's name
            if "*" not in prm and ctype not in _SCALARS:
                raise ValueError(f"{name}: parameter '{' '.join(prm.split())}' has no known scalar type")
            args.append(C.c_void_p if "*" in prm else _SCALARS[ctype])
        sigs[name], rets[name] = args, _RETURNS[ret]
    stray = re.search(r"\b(sfx_\w+)\s*\(", _PROTO.sub(" ", text))
    if stray:
        raise ValueError(f"{stray.group(1)}: not a `<ret> sfx_name(<params>);` prototype the binding can read")
    return sigs, rets


# name -> argtypes / restype of every entry point, read once from the header the library is compiled against
with open(HEADER) as _f:
    SIGNATURES, _RESTYPES = parse_header(_f.read())

_lib = None
_lock = threading.Lock()


def load(path: str | None = None):
    """Load libsfx.so (no GPU needed) and bind every entry point include/sfx.h declares; raises if the library is
    absent or lacks one."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise RuntimeError(
                f"libsfx.so not found at {p}; build it with `python -m splatformer_amd.build_lib` "
                "(the HIP extension is required: there is no CPU fallback)")
        lib = C.CDLL(p)
        for name, args in SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise RuntimeError(f"{p} does not export {name}, which include/sfx.h declares: the library is stale, "
                                   "rebuild it with `python -m splatformer_amd.build_lib`") from None
            fn.argtypes = args
            fn.restype = _RESTYPES[name]
        _lib = lib
        return lib


def lib():
    return _lib if _lib is not None else load()


def fn(name: str):
    return getattr(lib(), name)


_FNS: dict = {}  # name -> resolved ctypes function (one dict lookup per launch instead of lib() + getattr + checks)


def call(name: str, *args) -> None:
    f = _FNS.get(name)
    if f is None:
        f = _FNS[name] = fn(name)
    rc = f(*args)
    if rc != 0:
        msg = lib().sfx_last_error()
        raise RuntimeError(f"{name} failed ({rc}): {msg.decode() if msg else ''}")


class HostRead:
    """Asynchronous device -> pinned-host copy of a small tensor: `get()` waits only for the work enqueued before
    the copy, so GPU work enqueued between the two keeps the device busy while the host waits (the sizes that
    must reach the host -- pooled point counts, pair offsets, the grid depth -- cost no queue drain)."""

    def __init__(self, t: torch.Tensor):
        self._h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        self._h.copy_(t, non_blocking=True)
        self._ev = torch.cuda.Event()
        self._ev.record()
        self._v = None

    def get(self) -> list:
        if self._v is None:
            self._ev.synchronize()
            self._v = self._h.tolist()
        return self._v

    def ready(self) -> bool:
        """Whether get() would return without waiting."""
        return self._v is not None or self._ev.query()


_LB_SEEN: dict = {}  # stream -> look-back timeouts already reported (one process per GPU)


def check_lookback(where: str, st=None) -> None:
    """Raise if a decoupled look-back wait (single-pass scan / radix pass, csrc/common.h lb_lookback_wave) on this
    stream reached its spin cap since the last check: that scan's prefix -- an intersection list, a pooled count --
    is wrong.  Call where results are consumed on the host (the stream is drained there anyway: the call
    synchronises it).  Each timeout is reported once; later checks only report new ones."""
    st = stream() if st is None else st
    n = int(fn("sfx_lookback_timeouts")(st))
    if n <= 0:  # 0: every wait exact; -1: nothing scanned on this stream yet
        return
    seen = _LB_SEEN.get(st, 0)
    if n > seen:
        _LB_SEEN[st] = n
        raise RuntimeError(f"{where}: {n - seen} decoupled look-back wait(s) on this stream reached the spin cap "
                           "(a scan or radix pass produced a wrong prefix; its results are invalid)")


def require_gpu(t: torch.Tensor | None = None) -> None:
    if not torch.cuda.is_available():
        raise RuntimeError("splatformer_amd requires a ROCm GPU (MI355X); no device is visible")
    if t is not None and not t.is_cuda:
        raise RuntimeError("splatformer_amd ops take device tensors; got a CPU tensor")


def ptr(t: torch.Tensor | None, dtype: torch.dtype | None = None) -> int | None:
    """Device pointer of a contiguous tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("expected a device tensor")
    if not t.is_contiguous():
        raise RuntimeError("expected a contiguous tensor")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"expected dtype {dtype}, got {t.dtype}")
    return t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_get_device = torch._C._cuda_getDevice
_cuda_ready = [False]


def stream() -> int:
    """The current HIP stream of the current device (torch's), as a pointer.  Called once per launch: the raw
    accessor costs ~0.3 us against ~8 us for torch.cuda.current_stream()'s Python wrapper (tools/host_profile.py)."""
    if _raw_stream is not None:
        if _cuda_ready[0] or torch.cuda.is_initialized():
            _cuda_ready[0] = True
            return _raw_stream(_get_device())
    return torch.cuda.current_stream().cuda_stream


def workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
