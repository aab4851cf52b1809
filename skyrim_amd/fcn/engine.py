"""FourCastNet v1 (AFNO) 6-h step on one MI355X: the host owns buffers, prepared matrices and call order; every FLOP runs in the HIP
kernels of include/skyrim_fcn.h (libskyrim_fcn.so, loaded through ctypes; PyTorch is device memory + streams).  There is no CPU fallback.

One step = patch embedding, ``depth`` x (spectral filter + token MLP), head.  Layouts (fp32):

    tokens      [h][w][C]                  (h, w) = the 8 x 8 patch grid, C = embed; ping-pong between two buffers
    spectra     [2 freq + re/im][km][C]    latitude index (or frequency) and re / im interleaved so that both the longitude and
                                           the latitude DFT are plain strided GEMMs against constant matrices

The input normalisation is a per-k affine in the patch loader (before the fp16 split), the output de-normalisation is folded into the
head matrix and its bias.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from .. import native
from ..engine import Engine
from .spec import FcnConfig, param_spec

SPECTRAL_BLOCK = 96            # block size the spectral MLP kernel is compiled for
TOKEN_WIDTHS = (192, 768)      # embed widths the token MLP kernel is compiled for

_P = ctypes.c_void_p
_LL = ctypes.c_longlong
_I = ctypes.c_int
_F = ctypes.c_float


class PatchEmbedDesc(ctypes.Structure):
    _fields_ = [("x", _P), ("kscale", _P), ("kshift", _P), ("w", _P), ("w_plane", _LL), ("ldw", _I), ("bias", _P), ("pos", _P), ("out", _P),
                ("cin", _I), ("himg", _I), ("wimg", _I), ("patch", _I), ("embed", _I)]


class SpectralMlpDesc(ctypes.Structure):
    _fields_ = [("z", _P), ("rows", _LL), ("sm", _LL), ("sm2", _LL), ("im_off", _LL), ("m1", _I), ("nblocks", _I),
                ("w1f", _P), ("w2f", _P), ("b1e", _P), ("b2e", _P), ("lam", _F)]


class SpectralDesc(ctypes.Structure):
    _fields_ = [("t", _P), ("u", _P), ("s0", _P), ("s1", _P), ("gamma", _P), ("beta", _P), ("eps", _F),
                ("fw", _P), ("fl", _P), ("il", _P), ("iw", _P), ("fw_plane", _LL), ("fl_plane", _LL), ("il_plane", _LL), ("iw_plane", _LL),
                ("fw_ld", _I), ("fl_ld", _I), ("il_ld", _I), ("iw_ld", _I), ("h", _I), ("w", _I), ("C", _I), ("km", _I), ("nblocks", _I),
                ("w1f", _P), ("w2f", _P), ("b1e", _P), ("b2e", _P), ("lam", _F)]


class MlpDesc(ctypes.Structure):
    _fields_ = [("x", _P), ("out", _P), ("rows", _LL), ("C", _I), ("hidden", _I), ("gamma", _P), ("beta", _P), ("eps", _F),
                ("w1f", _P), ("w2f", _P), ("b1", _P), ("b2", _P)]


class HeadDesc(ctypes.Structure):
    _fields_ = [("t", _P), ("w", _P), ("w_plane", _LL), ("ldw", _I), ("bias", _P), ("out", _P),
                ("cout", _I), ("himg", _I), ("wimg", _I), ("patch", _I), ("embed", _I)]


SPEC = native.Spec("skyrim_fcn", "SKYRIM_FCN_LIB", "skfcn", 1, {             # include/skyrim_fcn.h SKFCN_ABI_VERSION
    "skfcn_abi_version": (_I, []),
    "skfcn_error_string": (ctypes.c_char_p, [_I]),
    "skfcn_prepare_weight": (_I, [_P, _LL, _LL, _I, _I, _P, _LL, _I, _P]),
    "skfcn_prepare_mlp_weights": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "skfcn_patch_embed": (_I, [ctypes.POINTER(PatchEmbedDesc), _P]),
    "skfcn_layer_norm": (_I, [_P, _P, _P, _P, _LL, _I, _F, _P]),
    "skfcn_spectral_mlp": (_I, [ctypes.POINTER(SpectralMlpDesc), _P]),
    "skfcn_spectral_run": (_I, [ctypes.POINTER(SpectralDesc), _P]),
    "skfcn_mlp_run": (_I, [ctypes.POINTER(MlpDesc), _P]),
    "skfcn_head_run": (_I, [ctypes.POINTER(HeadDesc), _P]),
})
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi


_lib = None


def load_library() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


# ---- constant matrices ------------------------------------------------------------------------------------------------------------ #
def dft_matrices(h: int, w: int, km: int) -> dict:
    """The four DFT matrices of the filter (float64), in the spectrum layout of include/skyrim_fcn.h:
    fw [2 km][w]: longitude R2C, row ri km + m;   fl [2 h][2 h]: latitude forward, (2 kk + ri') x (2 h + ri);
    il [2 h][2 h]: latitude inverse;              iw [w][2 km]: longitude C2R (Hermitian weight 2 for 0 < m < w/2, Im of m = 0 and of
    the Nyquist column dropped).  Ortho normalisation: 1/sqrt(w) along longitude, 1/sqrt(h) along latitude, each direction."""
    m = np.arange(km)[:, None].astype(np.float64)
    x = np.arange(w)[None, :].astype(np.float64)
    ang = 2.0 * np.pi * m * x / w
    fw = np.concatenate([np.cos(ang), -np.sin(ang)], 0) / math.sqrt(w)
    coef = np.where((m[:, 0] == 0) | (2 * m[:, 0] == w), 1.0, 2.0)[:, None]
    keep_im = np.where((m[:, 0] == 0) | (2 * m[:, 0] == w), 0.0, 1.0)[:, None]
    iw = np.concatenate([coef * np.cos(ang), -coef * keep_im * np.sin(ang)], 0).T / math.sqrt(w)
    k = np.arange(h)[:, None].astype(np.float64)
    y = np.arange(h)[None, :].astype(np.float64)
    th = 2.0 * np.pi * k * y / h                        # [kk][h]
    c, s = np.cos(th) / math.sqrt(h), np.sin(th) / math.sqrt(h)
    fl = np.zeros((2 * h, 2 * h))
    fl[0::2, 0::2], fl[0::2, 1::2], fl[1::2, 0::2], fl[1::2, 1::2] = c, s, -s, c          # Z = sum_h Y e^{-i th}
    il = np.zeros((2 * h, 2 * h))
    il[0::2, 0::2], il[0::2, 1::2], il[1::2, 0::2], il[1::2, 1::2] = c.T, -s.T, s.T, c.T  # X = sum_kk S e^{+i th}
    return {"fw": fw, "fl": fl, "il": il, "iw": iw}


def complex_block_matrices(w: torch.Tensor, b: torch.Tensor):
    """AFNO weights w [2][nb][bs in][bs out] (x @ W), b [2][nb][bs] -> the real forms [nb][2 bs out][2 bs in] (rows: re outputs, then im;
    columns: re inputs, then im) and biases [nb][2 bs]."""
    wr, wi = w[0].transpose(1, 2), w[1].transpose(1, 2)          # [nb][out][in]
    top = torch.cat([wr, -wi], 2)
    bot = torch.cat([wi, wr], 2)
    return torch.cat([top, bot], 1).contiguous(), torch.cat([b[0], b[1]], 1).contiguous()


class _Pairs:
    """``batch`` expand / contract pairs w1 [batch][H][K], w2 [batch][N][H] as fragment-order fp16 hi/lo planes."""

    def __init__(self, eng, w1: torch.Tensor, w2: torch.Tensor):
        if w1.dim() == 2:
            w1, w2 = w1[None], w2[None]
        batch, H, K = w1.shape
        N = w2.shape[1]
        a, b = w1.float().contiguous().to(eng.device), w2.float().contiguous().to(eng.device)
        self.w1f = torch.empty(2 * batch * H * K, dtype=torch.float16, device=eng.device)
        self.w2f = torch.empty(2 * batch * N * H, dtype=torch.float16, device=eng.device)
        native.check(eng.lib.skfcn_prepare_mlp_weights(a.data_ptr(), b.data_ptr(), K, H, N, batch, self.w1f.data_ptr(), self.w2f.data_ptr(),
                                                       native.stream(eng.device)), "skfcn_prepare_mlp_weights", eng.lib)
        torch.cuda.current_stream(eng.device).synchronize()


class FcnEngine(Engine):
    prepare_symbol = "skfcn_prepare_weight"

    def __init__(self, cfg: FcnConfig | None = None, device: str | torch.device = "cuda:0"):
        self.cfg = c = cfg or FcnConfig()
        if c.n_lat % c.patch or c.n_lon % c.patch:
            raise ValueError(f"grid {c.n_lat} x {c.n_lon} is not a multiple of the patch {c.patch}")
        if c.block_size != SPECTRAL_BLOCK or c.embed_dim not in TOKEN_WIDTHS or c.hidden % 32:
            raise ValueError(f"compiled for spectral blocks of {SPECTRAL_BLOCK}, embed widths {TOKEN_WIDTHS} and hidden widths that are "
                             f"multiples of 32; got embed {c.embed_dim}, {c.num_blocks} blocks, hidden {c.hidden}")
        if not 0 < c.km <= c.w // 2 + 1:
            raise ValueError(f"kept_lon_modes {c.km} outside (0, {c.w // 2 + 1}]")
        self._bind(load_library(), device, (c.in_chans, c.n_lat, c.n_lon))

    def load_params(self, params: dict):
        c = self.cfg
        for name, shape in param_spec(c):
            if name not in params or tuple(params[name].shape) != tuple(shape):
                raise ValueError(f"parameter {name}: expected shape {shape}, got {tuple(params[name].shape) if name in params else None}")
        p = {k: v.double() for k, v in params.items()}
        dev, e, P = self.device, c.embed_dim, c.patch
        f32 = lambda t: t.float().contiguous().to(dev)          # noqa: E731
        with torch.cuda.device(dev):
            mean, std = p["norm.mean"], p["norm.std"]
            self.kscale = f32((1.0 / std).repeat_interleave(P * P))
            self.kshift = f32((-mean / std).repeat_interleave(P * P))
            self.embed_w = self._weight(p["patch_embed.proj.weight"].reshape(e, -1))
            self.embed_b = f32(p["patch_embed.proj.bias"])
            self.pos = f32(p["pos_embed"].reshape(c.tokens, e))
            # head: rows n = (p1 P + p2) cout + c scaled by std_c, bias mean_c
            cidx = torch.arange(c.out_chans * P * P) % c.out_chans
            self.head_w = self._weight(p["head.weight"] * std[cidx][:, None])
            self.head_b = f32(mean[cidx])
            mats = dft_matrices(c.h, c.w, c.km)
            self.dft = {k: self._weight(torch.from_numpy(v)) for k, v in mats.items()}
            self.blocks = []
            for i in range(c.depth):
                b = f"blocks.{i}."
                w1e, b1e = complex_block_matrices(p[b + "filter.w1"], p[b + "filter.b1"])
                w2e, b2e = complex_block_matrices(p[b + "filter.w2"], p[b + "filter.b2"])
                self.blocks.append({
                    "g1": f32(p[b + "norm1.weight"]), "be1": f32(p[b + "norm1.bias"]),
                    "spec": _Pairs(self, w1e, w2e), "b1e": f32(b1e), "b2e": f32(b2e),
                    "g2": f32(p[b + "norm2.weight"]), "be2": f32(p[b + "norm2.bias"]),
                    "mlp": _Pairs(self, p[b + "mlp.fc1.weight"], p[b + "mlp.fc2.weight"]),
                    "fb1": f32(p[b + "mlp.fc1.bias"]), "fb2": f32(p[b + "mlp.fc2.bias"])})
            spec_n = 2 * c.h * c.km * e
            self.t = [torch.empty(c.tokens * e, dtype=torch.float32, device=dev) for _ in range(2)]
            self.u = torch.empty(c.tokens * e, dtype=torch.float32, device=dev)
            self.s = [torch.empty(spec_n, dtype=torch.float32, device=dev) for _ in range(2)]
        self.prepared = True

    # ---- stages (also the units the GPU tests check) ---- #
    def patch_embed(self, x: torch.Tensor, out: torch.Tensor):
        c = self.cfg
        d = PatchEmbedDesc(x.data_ptr(), self.kscale.data_ptr(), self.kshift.data_ptr(), self.embed_w.buf.data_ptr(), self.embed_w.plane,
                           self.embed_w.ldw, self.embed_b.data_ptr(), self.pos.data_ptr(), out.data_ptr(), c.in_chans, c.n_lat, c.n_lon,
                           c.patch, c.embed_dim)
        native.check(self.lib.skfcn_patch_embed(ctypes.byref(d), native.stream(self.device)), "skfcn_patch_embed", self.lib)

    def spectral(self, i: int, t: torch.Tensor):
        c, blk, D = self.cfg, self.blocks[i], self.dft
        d = SpectralDesc(t.data_ptr(), self.u.data_ptr(), self.s[0].data_ptr(), self.s[1].data_ptr(), blk["g1"].data_ptr(), blk["be1"].data_ptr(),
                         c.eps, D["fw"].buf.data_ptr(), D["fl"].buf.data_ptr(), D["il"].buf.data_ptr(), D["iw"].buf.data_ptr(),
                         D["fw"].plane, D["fl"].plane, D["il"].plane, D["iw"].plane, D["fw"].ldw, D["fl"].ldw, D["il"].ldw, D["iw"].ldw,
                         c.h, c.w, c.embed_dim, c.km, c.num_blocks, blk["spec"].w1f.data_ptr(), blk["spec"].w2f.data_ptr(),
                         blk["b1e"].data_ptr(), blk["b2e"].data_ptr(), c.sparsity_threshold)
        native.check(self.lib.skfcn_spectral_run(ctypes.byref(d), native.stream(self.device)), "skfcn_spectral_run", self.lib)

    def token_mlp(self, i: int, x: torch.Tensor, out: torch.Tensor):
        c, blk = self.cfg, self.blocks[i]
        d = MlpDesc(x.data_ptr(), out.data_ptr(), c.tokens, c.embed_dim, c.hidden, blk["g2"].data_ptr(), blk["be2"].data_ptr(), c.eps,
                    blk["mlp"].w1f.data_ptr(), blk["mlp"].w2f.data_ptr(), blk["fb1"].data_ptr(), blk["fb2"].data_ptr())
        native.check(self.lib.skfcn_mlp_run(ctypes.byref(d), native.stream(self.device)), "skfcn_mlp_run", self.lib)

    def head(self, t: torch.Tensor, y: torch.Tensor):
        c = self.cfg
        d = HeadDesc(t.data_ptr(), self.head_w.buf.data_ptr(), self.head_w.plane, self.head_w.ldw, self.head_b.data_ptr(), y.data_ptr(),
                     c.out_chans, c.n_lat, c.n_lon, c.patch, c.embed_dim)
        native.check(self.lib.skfcn_head_run(ctypes.byref(d), native.stream(self.device)), "skfcn_head_run", self.lib)

    def step(self, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """One 6-h step: fp32 (in_chans, n_lat, n_lon) on the engine device -> (out_chans, n_lat, n_lon)."""
        self.require_prepared("step")
        c = self.cfg
        self.check_state(x)
        with torch.cuda.device(self.device):
            y = out if out is not None else torch.empty((c.out_chans, c.n_lat, c.n_lon), dtype=torch.float32, device=self.device)
            if y.device != self.device or y.dtype != torch.float32 or tuple(y.shape) != (c.out_chans, c.n_lat, c.n_lon) or not y.is_contiguous():
                raise ValueError("bad output tensor")
            a, b = self.t
            self.patch_embed(x, a)
            for i in range(c.depth):
                self.spectral(i, a)                  # in place: a <- filter(norm1(a)) + norm1(a) + a
                self.token_mlp(i, a, b)              # b <- a + mlp(norm2(a))
                a, b = b, a
            self.head(a, y)
        return y
