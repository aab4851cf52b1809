"""DLWP call on one MI355X: the host owns buffers, prepared weights and call order; every FLOP runs in the HIP kernels of
include/skyrim_dlwp.h (libskyrim_dlwp.so, loaded through ctypes; PyTorch is device memory + streams).  There is no CPU fallback.

One call = ingest, the 11 convs of ``spec.convs`` (pooling, upsampling and the skip concatenation inside their loaders), egress:
13 launches on the current stream, no host synchronisation.  Layouts (fp32):

    states        [C][n_lat][n_lon]                the raw lat-lon fields, as the TimeLoop holds them
    activations   [face][y][x][channels]           one buffer per conv (the encoder outputs are the decoder's skips)
    conv weights  [2][cout][tap][cin] as fp16 hi/lo planes, equatorial then polar (k = tap cin + c)
"""
from __future__ import annotations

import ctypes
import datetime

import numpy as np
import torch

from .. import native
from ..engine import Engine
from .spec import MAP_SLOTS, SKIP_OF, DlwpConfig, convs, days_since_j2000, pad_table_i32, param_spec, to_csr

_P = ctypes.c_void_p
_LL = ctypes.c_longlong
_I = ctypes.c_int
_F = ctypes.c_float
_D = ctypes.c_double

IN_LD = 24          # ingest row: 18 channels padded to a multiple of 8 (the loader reads 8 channels at a time)
OUT_LD = 16         # output conv row: 14 channels padded to a multiple of 4 (egress reads float4)


class IngestDesc(ctypes.Structure):
    _fields_ = [("x0", _P), ("x1", _P), ("center", _P), ("inv_scale", _P), ("row_ptr", _P), ("col", _P), ("S", _P), ("lat", _P), ("lon", _P),
                ("statics", _P), ("days0", _D), ("days1", _D), ("out", _P), ("channels", _I), ("cells", _I), ("points", _I), ("ld_out", _I)]


class ConvDesc(ctypes.Structure):
    _fields_ = [("src0", _P), ("src1", _P), ("pad", _P), ("w", _P), ("w_plane", _LL), ("w_polar", _LL), ("ldw", _I), ("bias", _P), ("out", _P),
                ("n", _I), ("c0", _I), ("c1", _I), ("mode0", _I), ("taps", _I), ("cout", _I), ("ld_out", _I), ("act", _I), ("flip_face", _I),
                ("slope", _F), ("clamp_max", _F)]


class EgressDesc(ctypes.Structure):
    _fields_ = [("y", _P), ("row_ptr", _P), ("col", _P), ("S", _P), ("center", _P), ("scale", _P), ("out6", _P), ("out12", _P),
                ("channels", _I), ("cells", _I), ("points", _I), ("ld_y", _I)]


SPEC = native.Spec("skyrim_dlwp", "SKYRIM_DLWP_LIB", "skdlwp", 1, {          # include/skyrim_dlwp.h SKDLWP_ABI_VERSION
    "skdlwp_abi_version": (_I, []),
    "skdlwp_error_string": (ctypes.c_char_p, [_I]),
    "skdlwp_prepare_weight": (_I, [_P, _LL, _LL, _I, _I, _P, _LL, _I, _P]),
    "skdlwp_ingest": (_I, [ctypes.POINTER(IngestDesc), _P]),
    "skdlwp_conv": (_I, [ctypes.POINTER(ConvDesc), _P]),
    "skdlwp_egress": (_I, [ctypes.POINTER(EgressDesc), _P]),
})
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi

_lib = None


def load_library() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


MODES = {"x": 0, "prev": 0, "pool": 1, "up+skip": 2}


def conv_matrix(w: torch.Tensor, cin_pad: int) -> torch.Tensor:
    """[cout][cin][k][k] -> [cout][k k cin_pad] rows (k = tap cin_pad + c, channels beyond cin zero)."""
    cout, cin, kh, kw = w.shape
    out = torch.zeros(cout, kh * kw, cin_pad, dtype=w.dtype)
    out[:, :, :cin] = w.permute(0, 2, 3, 1).reshape(cout, kh * kw, cin)
    return out.reshape(cout, kh * kw * cin_pad)


class _Map:
    """A sparse map as int32 CSR on the device; indices checked on the host (the kernels trust them)."""

    def __init__(self, rows, cols, S, n_rows: int, n_cols: int, device, what: str):
        rows, cols = np.asarray(rows, np.int64).ravel(), np.asarray(cols, np.int64).ravel()
        S = np.asarray(S, np.float64).ravel()
        if not (rows.shape == cols.shape == S.shape):
            raise ValueError(f"{what}: row / col / S have different lengths")
        if rows.size and (rows.min() < 0 or rows.max() >= n_rows or cols.min() < 0 or cols.max() >= n_cols):
            raise ValueError(f"{what}: indices outside the {n_rows} x {n_cols} map")
        if not np.isfinite(S).all():
            raise ValueError(f"{what}: non-finite weights")
        ptr, col, s = to_csr(rows, cols, S, n_rows)
        if ptr[-1] >= 2 ** 31:
            raise ValueError(f"{what}: too many non-zeros")
        self.ptr = torch.from_numpy(ptr.astype(np.int32)).to(device)
        self.col = torch.from_numpy(col.astype(np.int32)).to(device)
        self.S = torch.from_numpy(s.astype(np.float32)).to(device)


class DlwpEngine(Engine):
    keep = ("convs",)
    prepare_symbol = "skdlwp_prepare_weight"

    def __init__(self, cfg: DlwpConfig | None = None, device: str | torch.device = "cuda:0"):
        self.cfg = c = cfg or DlwpConfig()
        if c.face % 4 or c.channels > 8 or c.n_history != 2 or c.in_ch > IN_LD or c.out_ch > OUT_LD or not -1 <= c.polar_flip_face <= 5:
            raise ValueError(f"compiled for face sizes that are multiples of 4, at most 8 channels and 2 history levels; got face {c.face}, "
                             f"{c.channels} channels, {c.n_history} levels")
        self.convs = convs(c)
        self._bind(load_library(), device, (c.channels, c.n_lat, c.n_lon))

    def load_params(self, params: dict):
        c = self.cfg
        for name, shape in param_spec(c):
            if name not in params or tuple(params[name].shape) != tuple(shape):
                raise ValueError(f"parameter {name}: expected shape {shape}, got {tuple(params[name].shape) if name in params else None}")
        for m in MAP_SLOTS:
            for part in ("row", "col", "S"):
                if f"{m}.{part}" not in params:
                    raise ValueError(f"parameter {m}.{part} missing (sparse map as row / col / S)")
        dev = self.device
        f32 = lambda t: torch.as_tensor(t).float().contiguous().to(dev)          # noqa: E731
        with torch.cuda.device(dev):
            scale = params["scale"].double()
            if not bool((scale != 0).all()):
                raise ValueError("scale has zero entries")
            self.center, self.scale, self.inv_scale = f32(params["center"]), f32(scale), f32(1.0 / scale)
            topo = (params["topography"].double() - c.topo_center) / c.topo_scale
            self.statics = f32(torch.stack([params["lsm"].double().reshape(-1), topo.reshape(-1)], 1))
            self.lat = params["cube_lat"].double().reshape(-1).contiguous().to(dev)
            self.lon = params["cube_lon"].double().reshape(-1).contiguous().to(dev)
            p = lambda k: params[k].numpy() if torch.is_tensor(params[k]) else params[k]     # noqa: E731
            self.ll_to_cs = _Map(p("ll_to_cs.row"), p("ll_to_cs.col"), p("ll_to_cs.S"), c.cells, c.points, dev, "ll_to_cs")
            self.cs_to_ll = _Map(p("cs_to_ll.row"), p("cs_to_ll.col"), p("cs_to_ll.S"), c.points, c.cells, dev, "cs_to_ll")
            self.pad = pad_table_i32().to(dev)
            self.layers = []
            bufs = {}
            for name, lvl, cin, cout, k, src in self.convs:
                n = c.face >> lvl
                cells = 6 * n * n
                cin_pad = IN_LD if src == "x" else cin
                ws = [params[f"{kind}_{name}.weight"].double() for kind in ("equatorial", "polar")]
                w = self._weight(torch.stack([conv_matrix(x, cin_pad) for x in ws]))
                bias = f32(torch.stack([params[f"{kind}_{name}.bias"].double() for kind in ("equatorial", "polar")]))
                ld = OUT_LD if name == "last" else cout
                out = torch.zeros(cells * ld, dtype=torch.float32, device=dev)
                skip = SKIP_OF.get(name)
                self.layers.append(dict(name=name, n=n, cout=cout, ld=ld, taps=k * k, mode0=MODES[src], w=w, bias=bias, out=out,
                                        skip=bufs[skip] if skip else None, skip_c=self.convs[[q[0] for q in self.convs].index(skip)][3] if skip else 0,
                                        act=0 if name == "last" else 1))
                bufs[name] = out
            self.x = torch.zeros(c.cells * IN_LD, dtype=torch.float32, device=dev)
        self.prepared = True

    # ---- stages (also the units the GPU tests check) ---- #
    def ingest(self, x0: torch.Tensor, x1: torch.Tensor, days0: float, days1: float, out: torch.Tensor | None = None):
        c, m = self.cfg, self.ll_to_cs
        out = self.x if out is None else out
        d = IngestDesc(x0.data_ptr(), x1.data_ptr(), self.center.data_ptr(), self.inv_scale.data_ptr(), m.ptr.data_ptr(), m.col.data_ptr(),
                       m.S.data_ptr(), self.lat.data_ptr(), self.lon.data_ptr(), self.statics.data_ptr(), days0, days1, out.data_ptr(),
                       c.channels, c.cells, c.points, IN_LD)
        native.check(self.lib.skdlwp_ingest(ctypes.byref(d), native.stream(self.device)), "skdlwp_ingest", self.lib)

    def conv(self, i: int, src: torch.Tensor | None = None, skip: torch.Tensor | None = None, out: torch.Tensor | None = None):
        """Conv i of ``spec.convs`` reading the previous stage's buffer (or ``src`` / ``skip``), writing its own (or ``out``)."""
        c, L = self.cfg, self.layers[i]
        if src is None:
            src = self.x if i == 0 else self.layers[i - 1]["out"]
        skip = L["skip"] if skip is None else skip
        out = L["out"] if out is None else out
        cin = self.convs[i][2] if i else IN_LD
        c0 = cin - L["skip_c"]
        w = L["w"]
        d = ConvDesc(src.data_ptr(), skip.data_ptr() if skip is not None else None, self.pad.data_ptr(), w.buf.data_ptr(), w.plane, w.w_sb, w.ldw,
                     L["bias"].data_ptr(), out.data_ptr(), L["n"], c0, L["skip_c"], L["mode0"], L["taps"], L["cout"], L["ld"], L["act"],
                     c.polar_flip_face, c.leaky_slope, c.clamp_max)
        native.check(self.lib.skdlwp_conv(ctypes.byref(d), native.stream(self.device)), "skdlwp_conv", self.lib)

    def egress(self, y6: torch.Tensor, y12: torch.Tensor, y: torch.Tensor | None = None):
        c, m = self.cfg, self.cs_to_ll
        y = self.layers[-1]["out"] if y is None else y
        d = EgressDesc(y.data_ptr(), m.ptr.data_ptr(), m.col.data_ptr(), m.S.data_ptr(), self.center.data_ptr(), self.scale.data_ptr(),
                       y6.data_ptr(), y12.data_ptr(), c.channels, c.cells, c.points, OUT_LD)
        native.check(self.lib.skdlwp_egress(ctypes.byref(d), native.stream(self.device)), "skdlwp_egress", self.lib)

    def tisr_days(self, time: datetime.datetime) -> tuple[float, float]:
        """The TISR times of the two input levels of a call whose newest level is at ``time`` (days since J2000.0)."""
        return tuple(days_since_j2000(time + datetime.timedelta(hours=h)) for h in self.cfg.tisr_offsets_h)

    def call(self, x0: torch.Tensor, x1: torch.Tensor, time: datetime.datetime):
        """One network call: states at time - 6 h (x0) and time (x1) -> new tensors (t + 6 h, t + 12 h)."""
        self.require_prepared("call")
        self.check_state(x0, "x0")
        self.check_state(x1, "x1")
        with torch.cuda.device(self.device):
            y6 = torch.empty(self.state_shape, dtype=torch.float32, device=self.device)
            y12 = torch.empty_like(y6)
            self.ingest(x0, x1, *self.tisr_days(time))
            for i in range(len(self.layers)):
                self.conv(i)
            self.egress(y6, y12)
        return y6, y12
