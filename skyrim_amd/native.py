"""The one binding policy of the C-ABI libraries (include/skyrim_{pangu,sfno,graphcast,fcn,dlwp,fuxi,fengwu,io,ens,score,noise,track,derive,thermo,vert,point,gram,breed,stoch,spec,object,clim,pack,nbr,regrid,agg,event}.h, built into skyrim_amd/lib/).

Each binding module declares a ``Spec`` -- file stem, override variable, symbol prefix, ABI version, signature table -- and its
``load_library()`` calls ``load(SPEC)`` once: the path (the override variable names a variant build), the ctypes signatures and the ABI
check live here.  ``check`` turns a non-zero return code into a RuntimeError, ``stream`` is torch's current stream as the ``void* stream`` of
every launch, ``tensor_ptr`` is the address of a tensor a launch may be handed (contiguous, of the dtype, on the device), and
``HiLoWeight`` is the fp16 hi/lo upload of a constant matrix that SFNO, GraphCast and FourCastNet v1 share.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from pathlib import Path

import torch

LIB_DIR = Path(__file__).resolve().parent / "lib"
BUILD = "python -c 'import __graft_entry__ as g; g.build()'"
# the codes of the libraries without an error-string entry point (include/skyrim_{sfno,graphcast,io}.h: *_E_ARG, *_E_HIP)
_GENERIC = {-1: "invalid argument", -2: "HIP runtime error"}


@dataclass
class Spec:
    stem: str            # lib<stem>.so
    env: str             # override variable: the path of another build of the library
    prefix: str          # <prefix>_abi_version, <prefix>_error_string (when exported)
    abi: int             # the header's <PREFIX>_ABI_VERSION this package binds
    symbols: dict        # {symbol: (restype, argtypes)}: every entry point the header declares
    hint: str = ""       # appended to the "not found" message

    @property
    def exports(self) -> list[str]:
        return list(self.symbols)


def load(spec: Spec) -> ctypes.CDLL:
    """The library of ``spec``: resolved, typed and version-checked.  Each binding module keeps the handle in its ``_lib`` and calls this
    only while that is None, so a launch pays one global lookup; tests set ``_lib`` to None to load again."""
    path = os.environ.get(spec.env, str(LIB_DIR / f"lib{spec.stem}.so"))
    if not os.path.exists(path):
        raise RuntimeError(f"HIP library {path} not found; build it with `{BUILD}`{spec.hint}")
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in spec.symbols.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    err = f"{spec.prefix}_error_string"
    lib.error_string = getattr(lib, err) if err in spec.symbols else None
    # a stale build, or an override from other sources, would read this package's descriptors and prepared layouts as something else
    got = getattr(lib, f"{spec.prefix}_abi_version")()
    if got != spec.abi:
        raise RuntimeError(f"{path}: {spec.prefix} ABI {got}, this package binds ABI {spec.abi} (include/{spec.stem}.h); "
                           f"rebuild the library (`{BUILD}`)")
    return lib


def check(code: int, what: str, lib: ctypes.CDLL | None = None) -> None:
    """RuntimeError for a non-zero return code of ``what``; the text from ``lib``'s error-string entry point when it has one."""
    if code != 0:
        strerror = getattr(lib, "error_string", None) if lib is not None else None
        msg = strerror(code).decode() if strerror is not None else _GENERIC.get(code, "unknown error")
        raise RuntimeError(f"{what} failed: {msg} (code {code})")


def stream(device: torch.device) -> ctypes.c_void_p:
    """torch's current stream on ``device`` as the ``void* stream`` argument of a launch."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def tensor_ptr(t, what: str, dtype, dev=None) -> int:
    """``t.data_ptr()`` of a contiguous ``dtype`` tensor on the GPU (on ``dev`` when given); anything else is a ValueError named ``what``."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or not t.is_cuda or (dev is not None and t.device != dev):
        raise ValueError(f"{what}: expected a contiguous {str(dtype).split('.')[-1]} tensor on {dev or 'the GPU'}")
    return t.data_ptr()


class HiLoWeight:
    """A constant matrix [batch][N][K] (2-D: batch 1) as fp16 hi/lo planes on ``device``: ``buf`` holds the hi planes of every batch
    entry ([batch][N][ldw], ldw = K rounded up to 8), then the lo planes ``plane`` elements further; ``w_sb`` is the batch stride.
    ``prepare``: the library's split entry point (``sk*_prepare_weight``, one signature; ``engine.Engine._weight`` names it per engine)."""

    def __init__(self, device: torch.device, prepare, w: torch.Tensor):
        w = w.float().contiguous()
        if w.dim() == 2:
            w = w[None]
        self.batch, self.N, self.K = w.shape
        self.ldw = (self.K + 7) // 8 * 8
        per = self.N * self.ldw
        self.plane = self.batch * per
        self.w_sb = per
        self.buf = torch.empty(2 * self.plane, dtype=torch.float16, device=device)
        chunk = max(1, (256 << 20) // (self.N * self.K * 4))          # upload at most ~256 MB of fp32 at a time
        for b0 in range(0, self.batch, chunk):
            src = w[b0:b0 + chunk].to(device)
            for j in range(src.shape[0]):
                dst = self.buf.data_ptr() + 2 * (b0 + j) * per
                check(prepare(src[j].data_ptr(), self.K, 1, self.N, self.K, dst, self.plane, self.ldw, stream(device)), prepare.__name__)
            torch.cuda.current_stream(device).synchronize()
