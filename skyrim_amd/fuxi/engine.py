"""FuXi call on one MI355X: the host owns buffers, prepared weights and call order; every FLOP runs in the HIP kernels of
include/skyrim_fuxi.h (libskyrim_fuxi.so, loaded through ctypes; PyTorch is device memory + streams).  There is no CPU fallback.

One call of one cascade stage (levels t - 6 h, t -> t + 6 h) is a fixed launch sequence on the current stream, no host synchronisation:
embed, LayerNorm, down block (stride-2 conv, residual block), ``depth`` Swin V2 blocks (QKV, window attention, proj, residual LayerNorm,
fc1 + GELU, fc2, residual LayerNorm), up block (transposed conv over the concatenation, residual block), head, resample.  The engine holds
the prepared weights of all three stages and ONE workspace; which stage runs is a choice of pointers.  Layouts (fp32):

    states        [C][n_lat][n_lon]              the raw lat-lon fields, as the TimeLoop holds them
    activations   [lat][lon][channels]           channels-last token grids (180 x 360 around the down / up blocks, 90 x 180 in between)
    head output   [C][4 h0][4 w0]                normalised, before the 720 -> 721 row resample
    weights       fp16 hi/lo planes [N][K]: Linear [out][in]; conv [out][ky][kx][in]; transposed conv [(dy dx) out][in]
"""
from __future__ import annotations

import ctypes
import datetime

import torch

from .. import native
from ..engine import CheckedParams, Engine
from .spec import STAGES, FuxiConfig, check_config, cpb_table, full_param_spec, param_spec, shift, time_encoding

_P = ctypes.c_void_p
_LL = ctypes.c_longlong
_I = ctypes.c_int
_F = ctypes.c_float


class EmbedDesc(ctypes.Structure):
    _fields_ = [("x0", _P), ("x1", _P), ("mean", _P), ("inv_std", _P), ("w", _P), ("w_plane", _LL), ("ldw", _I), ("bias", _P), ("tw", _P),
                ("tb", _P), ("temb", _F * 12), ("tvec", _P), ("out", _P), ("channels", _I), ("n_lat", _I), ("n_lon", _I), ("C", _I)]


class ConvDesc(ctypes.Structure):
    _fields_ = [("src0", _P), ("src1", _P), ("gn_stats", _P), ("gn_gamma", _P), ("gn_beta", _P), ("w", _P), ("w_plane", _LL), ("ldw", _I),
                ("bias", _P), ("out", _P), ("h_in", _I), ("w_in", _I), ("h_out", _I), ("w_out", _I), ("c0", _I), ("c1", _I), ("taps", _I),
                ("stride", _I), ("groups", _I), ("cout", _I), ("shuffle", _I)]


class LinearDesc(ctypes.Structure):
    _fields_ = [("a", _P), ("w", _P), ("w_plane", _LL), ("ldw", _I), ("bias", _P), ("out", _P), ("M", _I), ("N", _I), ("K", _I), ("act", _I),
                ("mode", _I), ("w_tok", _I), ("patch", _I)]


class AttnDesc(ctypes.Structure):
    _fields_ = [("qkv", _P), ("out", _P), ("cpb", _P), ("logit_scale", _P), ("H", _I), ("W", _I), ("C", _I), ("heads", _I), ("wh", _I),
                ("ww", _I), ("sh", _I), ("sw", _I), ("mask_lon", _I), ("mask_value", _F), ("logit_max", _F), ("norm_eps", _F)]


class ResampleDesc(ctypes.Structure):
    _fields_ = [("src", _P), ("mean", _P), ("std", _P), ("out", _P), ("channels", _I), ("h_src", _I), ("w_src", _I), ("h_out", _I),
                ("w_out", _I), ("align_corners", _I)]


SPEC = native.Spec("skyrim_fuxi", "SKYRIM_FUXI_LIB", "skfuxi", 1, {          # include/skyrim_fuxi.h SKFUXI_ABI_VERSION
    "skfuxi_abi_version": (_I, []),
    "skfuxi_error_string": (ctypes.c_char_p, [_I]),
    "skfuxi_prepare_weight": (_I, [_P, _LL, _LL, _I, _I, _P, _LL, _I, _P]),
    "skfuxi_embed": (_I, [ctypes.POINTER(EmbedDesc), _P]),
    "skfuxi_layer_norm": (_I, [_P, _P, _P, _P, _P, _LL, _I, _F, _P]),
    "skfuxi_conv": (_I, [ctypes.POINTER(ConvDesc), _P]),
    "skfuxi_gn_stats": (_I, [_P, _LL, _I, _I, _F, _P, _P]),
    "skfuxi_gn_residual": (_I, [_P, _P, _P, _P, _P, _P, _LL, _I, _I, _P]),
    "skfuxi_linear": (_I, [ctypes.POINTER(LinearDesc), _P]),
    "skfuxi_window_attention": (_I, [ctypes.POINTER(AttnDesc), _P]),
    "skfuxi_resample": (_I, [ctypes.POINTER(ResampleDesc), _P]),
})
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi

_lib = None


def load_library() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


def conv_matrix(w: torch.Tensor) -> torch.Tensor:
    """Conv2d [out][in][ky][kx] -> [out][(ky kx) in] rows (k = tap in + c)."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def tconv_matrix(w: torch.Tensor) -> torch.Tensor:
    """ConvTranspose2d [in][out][2][2] -> [(2 dy + dx) out + co][in] rows."""
    return w.permute(2, 3, 1, 0).reshape(4 * w.shape[1], w.shape[0])


class FuxiEngine(Engine):
    prepare_symbol = "skfuxi_prepare_weight"

    def __init__(self, cfg: FuxiConfig | None = None, device: str | torch.device = "cuda:0"):
        self.cfg = c = cfg or FuxiConfig()
        check_config(c)
        self._bind(load_library(), device, (c.channels, c.n_lat, c.n_lon))

    # ---- loading ---- #
    def _prepare_stage(self, p) -> dict:
        c, dev = self.cfg, self.device
        f32 = lambda t: torch.as_tensor(t).float().contiguous().to(dev)          # noqa: E731

        def res(prefix):
            return [dict(w=self._weight(conv_matrix(p[f"{prefix}.res.{j}.conv.weight"])), b=f32(p[f"{prefix}.res.{j}.conv.bias"]),
                         g=f32(p[f"{prefix}.res.{j}.norm.weight"]), beta=f32(p[f"{prefix}.res.{j}.norm.bias"])) for j in range(2)]

        s = dict(embed=self._weight(p["embed.weight"].reshape(c.embed, -1)), embed_b=f32(p["embed.bias"]), tw=f32(p["time_embed.weight"]),
                 tb=f32(p["time_embed.bias"]), en_g=f32(p["embed_norm.weight"]), en_b=f32(p["embed_norm.bias"]),
                 down=self._weight(conv_matrix(p["down.conv.weight"])), down_b=f32(p["down.conv.bias"]), down_res=res("down"), blocks=[])
        for i in range(c.depth):
            b = lambda n: p[f"blocks.{i}.{n}"]                                   # noqa: E731
            zero = torch.zeros(c.embed, dtype=torch.float32, device=b("attn.q_bias").device)
            cpb = cpb_table(c.window, b("attn.cpb_mlp.0.weight").cpu(), b("attn.cpb_mlp.0.bias").cpu(), b("attn.cpb_mlp.2.weight").cpu())
            s["blocks"].append(dict(
                qkv=self._weight(b("attn.qkv.weight")), qkv_b=f32(torch.cat([b("attn.q_bias").float(), zero, b("attn.v_bias").float()])),
                scale=f32(b("attn.logit_scale").reshape(-1)), cpb=f32(cpb), proj=self._weight(b("attn.proj.weight")), proj_b=f32(b("attn.proj.bias")),
                n1_g=f32(b("norm1.weight")), n1_b=f32(b("norm1.bias")), fc1=self._weight(b("mlp.fc1.weight")), fc1_b=f32(b("mlp.fc1.bias")),
                fc2=self._weight(b("mlp.fc2.weight")), fc2_b=f32(b("mlp.fc2.bias")), n2_g=f32(b("norm2.weight")), n2_b=f32(b("norm2.bias"))))
        s.update(up=self._weight(tconv_matrix(p["up.conv.weight"])), up_b=f32(p["up.conv.bias"]), up_res=res("up"), head=self._weight(p["head.weight"]),
                 head_b=f32(p["head.bias"]))
        return s

    def load_params(self, params):
        """``params``: a mapping keyed by ``spec.full_param_spec`` (``norm.mean``, ``norm.std``, then ``<stage>.<name>``) -- read one key
        at a time, so a lazy mapping (spec.SyntheticParams, a checkpoint reader) never holds a whole stage in memory."""
        c, dev = self.cfg, self.device
        for name, shape in full_param_spec(c):
            if name not in params:
                raise ValueError(f"parameter {name} missing (expected shape {shape})")
        with torch.cuda.device(dev):
            self.upload_affine(params["norm.mean"], params["norm.std"], c.channels)
            shapes = dict(param_spec(c))
            self.stages = {st: self._prepare_stage(CheckedParams(params, shapes, prefix=f"{st}.")) for st in STAGES}
            C, (h0, w0), (h1, w1) = c.embed, c.grid0, c.grid1
            t0, t1 = h0 * w0, h1 * w1
            z = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)         # noqa: E731
            self.buf = dict(emb=z(t0 * C), h0=z(t0 * C), ra0=z(t0 * C), rb0=z(t0 * C), u0=z(t0 * C), u=z(t0 * C), d0=z(t1 * C), ra1=z(t1 * C),
                            rb1=z(t1 * C), d=z(t1 * C), x=z(t1 * C), y=z(t1 * C), att=z(t1 * C), qkv=z(t1 * 3 * C), hid=z(t1 * c.hidden),
                            head=z(c.channels * 4 * h0 * 4 * w0), tvec=z(C), stats=z(2 * c.groups))
        self.prepared = True

    # ---- launches (also the units the GPU tests check) ---- #
    def _s(self):
        return native.stream(self.device)

    def embed(self, x0, x1, temb, st: str, out=None):
        """Cube embedding + bias + time vector -> ``emb`` (before its LayerNorm)."""
        c, S = self.cfg, self.stages[st]
        out = self.buf["emb"] if out is None else out
        d = EmbedDesc(x0.data_ptr(), x1.data_ptr(), self.mean.data_ptr(), self.inv_std.data_ptr(), S["embed"].buf.data_ptr(), S["embed"].plane,
                      S["embed"].ldw, S["embed_b"].data_ptr(), S["tw"].data_ptr(), S["tb"].data_ptr(), (_F * 12)(*[float(v) for v in temb]),
                      self.buf["tvec"].data_ptr(), out.data_ptr(), c.channels, c.n_lat, c.n_lon, c.embed)
        native.check(self.lib.skfuxi_embed(ctypes.byref(d), self._s()), "skfuxi_embed", self.lib)

    def layer_norm(self, x, gamma, beta, out, rows: int, res=None):
        native.check(self.lib.skfuxi_layer_norm(x.data_ptr(), res.data_ptr() if res is not None else None, gamma.data_ptr(), beta.data_ptr(),
                                                out.data_ptr(), rows, self.cfg.embed, self.cfg.ln_eps, self._s()), "skfuxi_layer_norm", self.lib)

    def conv(self, src0, W, bias, out, grid_in, grid_out, taps=9, stride=1, src1=None, gn=None, shuffle=0):
        """gn = (stats, gamma, beta): src0 read GroupNorm-applied + SiLU."""
        C = self.cfg.embed
        c1 = C if src1 is not None else 0
        st, g, b = gn if gn is not None else (None, None, None)
        d = ConvDesc(src0.data_ptr(), src1.data_ptr() if src1 is not None else None, st.data_ptr() if st is not None else None,
                     g.data_ptr() if g is not None else None, b.data_ptr() if b is not None else None, W.buf.data_ptr(), W.plane, W.ldw,
                     bias.data_ptr(), out.data_ptr(), grid_in[0], grid_in[1], grid_out[0], grid_out[1], C, c1, taps, stride, self.cfg.groups, C, shuffle)
        native.check(self.lib.skfuxi_conv(ctypes.byref(d), self._s()), "skfuxi_conv", self.lib)

    def gn_stats(self, x, rows: int, stats=None):
        stats = self.buf["stats"] if stats is None else stats
        c = self.cfg
        native.check(self.lib.skfuxi_gn_stats(x.data_ptr(), rows, c.embed, c.groups, c.gn_eps, stats.data_ptr(), self._s()), "skfuxi_gn_stats", self.lib)
        return stats

    def gn_residual(self, x, a, stats, gamma, beta, out, rows: int):
        c = self.cfg
        native.check(self.lib.skfuxi_gn_residual(x.data_ptr(), a.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(),
                                                 rows, c.embed, c.groups, self._s()), "skfuxi_gn_residual", self.lib)

    def linear(self, a, W, bias, out, M: int, act=0, head=False):
        c = self.cfg
        d = LinearDesc(a.data_ptr(), W.buf.data_ptr(), W.plane, W.ldw, bias.data_ptr(), out.data_ptr(), M, W.N, W.K, act, 1 if head else 0,
                       c.grid0[1], c.patch[1])
        native.check(self.lib.skfuxi_linear(ctypes.byref(d), self._s()), "skfuxi_linear", self.lib)

    def attention(self, qkv, out, cpb, scale, grid, sh: int, sw: int, window=None):
        c = self.cfg
        wh, ww = window or c.window
        d = AttnDesc(qkv.data_ptr(), out.data_ptr(), cpb.data_ptr(), scale.data_ptr(), grid[0], grid[1], c.embed, c.heads, wh, ww, sh, sw,
                     int(c.shift_mask_lon), c.mask_value, c.logit_max, c.norm_eps)
        native.check(self.lib.skfuxi_window_attention(ctypes.byref(d), self._s()), "skfuxi_window_attention", self.lib)

    def resample(self, src, out):
        c = self.cfg
        h0, w0 = c.grid0
        d = ResampleDesc(src.data_ptr(), self.mean.data_ptr(), self.std.data_ptr(), out.data_ptr(), c.channels, 4 * h0, 4 * w0, c.n_lat, c.n_lon,
                         int(c.align_corners))
        native.check(self.lib.skfuxi_resample(ctypes.byref(d), self._s()), "skfuxi_resample", self.lib)

    # ---- blocks ---- #
    def res_block(self, x, R, out, grid, ra, rb):
        """out = x + SiLU(GN(conv(SiLU(GN(conv(x))))))."""
        rows = grid[0] * grid[1]
        st = self.buf["stats"]
        self.conv(x, R[0]["w"], R[0]["b"], ra, grid, grid)
        self.gn_stats(ra, rows, st)
        self.conv(ra, R[1]["w"], R[1]["b"], rb, grid, grid, gn=(st, R[0]["g"], R[0]["beta"]))
        self.gn_stats(rb, rows, st)
        self.gn_residual(x, rb, st, R[1]["g"], R[1]["beta"], out, rows)

    def swin_block(self, i: int, st: str, x=None):
        """x <- x + LN(attn(x)); x <- x + LN(MLP(x)) on the 90 x 180 grid (``x``: the residual stream, default the engine's own)."""
        c, B, b = self.cfg, self.stages[st]["blocks"][i], self.buf
        x = b["x"] if x is None else x
        g1 = c.grid1
        rows = g1[0] * g1[1]
        self.linear(x, B["qkv"], B["qkv_b"], b["qkv"], rows)
        self.attention(b["qkv"], b["att"], B["cpb"], B["scale"], g1, *shift(c, i))
        self.linear(b["att"], B["proj"], B["proj_b"], b["y"], rows)
        self.layer_norm(b["y"], B["n1_g"], B["n1_b"], x, rows, res=x)
        self.linear(x, B["fc1"], B["fc1_b"], b["hid"], rows, act=1)
        self.linear(b["hid"], B["fc2"], B["fc2_b"], b["y"], rows)
        self.layer_norm(b["y"], B["n2_g"], B["n2_b"], x, rows, res=x)

    def call(self, x0: torch.Tensor, x1: torch.Tensor, time: datetime.datetime, stage: str = "short"):
        """One network call of ``stage``: states at time - 6 h (x0) and time (x1) -> a new tensor, the state at time + 6 h."""
        self.require_prepared("call")
        if stage not in STAGES:
            raise ValueError(f"stage {stage!r} not one of {STAGES}")
        self.check_state(x0, "x0")
        self.check_state(x1, "x1")
        c, S, b = self.cfg, self.stages[stage], self.buf
        g0, g1 = c.grid0, c.grid1
        t0 = g0[0] * g0[1]
        with torch.cuda.device(self.device):
            y = torch.empty(self.state_shape, dtype=torch.float32, device=self.device)
            self.embed(x0, x1, time_encoding(time), stage)
            self.layer_norm(b["emb"], S["en_g"], S["en_b"], b["h0"], t0)
            self.conv(b["h0"], S["down"], S["down_b"], b["d0"], g0, g1, stride=2)
            self.res_block(b["d0"], S["down_res"], b["d"], g1, b["ra1"], b["rb1"])
            b["x"].copy_(b["d"])
            for i in range(c.depth):
                self.swin_block(i, stage)
            self.conv(b["d"], S["up"], S["up_b"], b["u0"], g1, g1, taps=1, src1=b["x"], shuffle=1)
            self.res_block(b["u0"], S["up_res"], b["u"], g0, b["ra0"], b["rb0"])
            self.linear(b["u"], S["head"], S["head_b"], b["head"], t0, head=True)
            self.resample(b["head"], y)
        return y
