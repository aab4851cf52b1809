"""FengWu call on one MI355X: the host owns buffers, prepared weights, bias tables and call order; every FLOP runs in the HIP kernels of
include/skyrim_fengwu.h (libskyrim_fengwu.so, loaded through ctypes; PyTorch is device memory + streams).  There is no CPU fallback.

One call (levels t - 6 h, t -> t + 6 h) is a fixed launch sequence on the current stream, no host synchronisation (spec.n_launches):
embed (all modalities), its LayerNorm, the encoders' 181 x 360 blocks, merge, the encoders' 91 x 180 blocks, the fuser's 3-D blocks, the
decoders' 91 x 180 blocks, expand, skip linear, the decoders' 181 x 360 blocks, recovery.  Everything per modality runs as one launch
with the modality as grid z.  Layouts (fp32):

    states        [channels][n_lat][n_lon]           the raw lat-lon fields, as the TimeLoop holds them
    activations   [mods][lat][lon][C]                modality-major, channels-last (the fuser reads the same memory as a 3-D grid)
    weights       fp16 hi/lo planes [mods][N][K]: Linear [out][in]; embedding [C][(p 4 + dh) 4 + dw] with p = l c_m + c, zero-padded to
                  K = 32 c_max; recovery [(c 4 + p1) 4 + p2][C], zero-padded to 16 c_max rows
    bias tables   [mods][types][heads][N][N]         spec.bias_table: position bias + shift mask, float32
"""
from __future__ import annotations

import ctypes
import math

import torch

from .. import native
from ..engine import CheckedParams, Engine
from .spec import (FengwuConfig, bias_table, block_geometry, block_shift, check_config, full_param_spec, pad_to, shape_source,
                   window_types)

_P = ctypes.c_void_p
_LL = ctypes.c_longlong
_I = ctypes.c_int
_F = ctypes.c_float
_MODS = 8                                           # SKFW_MAX_MODS


class EmbedDesc(ctypes.Structure):
    _fields_ = [("x0", _P), ("x1", _P), ("mean", _P), ("inv_std", _P), ("w", _P), ("w_plane", _LL), ("w_sb", _LL), ("ldw", _I), ("bias", _P),
                ("out", _P), ("mods", _I), ("n_lat", _I), ("n_lon", _I), ("lat_front", _I), ("h_tok", _I), ("C", _I), ("K", _I),
                ("ch_off", _I * _MODS), ("ch_cnt", _I * _MODS)]


class LnDesc(ctypes.Structure):
    _fields_ = [("x", _P), ("gamma", _P), ("beta", _P), ("out", _P), ("rows", _LL), ("batch", _I), ("C", _I), ("merge", _I), ("h_src", _I),
                ("w_src", _I), ("front", _I), ("eps", _F)]


class LinearDesc(ctypes.Structure):
    _fields_ = [("a", _P), ("a2", _P), ("w", _P), ("w_plane", _LL), ("w_sb", _LL), ("ldw", _I), ("bias", _P), ("res", _P), ("out", _P),
                ("a_sb", _LL), ("a2_sb", _LL), ("o_sb", _LL), ("b_sb", _LL), ("batch", _I), ("M", _I), ("N", _I), ("K", _I), ("lda", _I),
                ("lda2", _I), ("k_split", _I), ("act", _I), ("mode", _I), ("w_tok", _I), ("h_out", _I), ("front", _I)]


class AttnDesc(ctypes.Structure):
    _fields_ = [("qkv", _P), ("qkv_bias", _P), ("table", _P), ("out", _P), ("table_sb", _LL)] + \
               [(n, _I) for n in ("batch", "Z", "H", "W", "Zp", "Hp", "Wp", "fz", "fh", "fw", "wz", "wh", "ww", "sz", "sh", "sw", "types_z",
                                  "types_y", "C", "heads")] + [("scale", _F)]


class RecoverDesc(ctypes.Structure):
    _fields_ = [("a", _P), ("w", _P), ("w_plane", _LL), ("w_sb", _LL), ("ldw", _I), ("bias", _P), ("mean", _P), ("std", _P), ("out", _P),
                ("mods", _I), ("h_tok", _I), ("w_tok", _I), ("C", _I), ("c_max", _I), ("n_lat", _I), ("lat_front", _I),
                ("ch_off", _I * _MODS), ("ch_cnt", _I * _MODS)]


SPEC = native.Spec("skyrim_fengwu", "SKYRIM_FENGWU_LIB", "skfw", 1, {          # include/skyrim_fengwu.h SKFW_ABI_VERSION
    "skfw_abi_version": (_I, []),
    "skfw_error_string": (ctypes.c_char_p, [_I]),
    "skfw_prepare_weight": (_I, [_P, _LL, _LL, _I, _I, _P, _LL, _I, _P]),
    "skfw_embed": (_I, [ctypes.POINTER(EmbedDesc), _P]),
    "skfw_layer_norm": (_I, [ctypes.POINTER(LnDesc), _P]),
    "skfw_linear": (_I, [ctypes.POINTER(LinearDesc), _P]),
    "skfw_window_attention": (_I, [ctypes.POINTER(AttnDesc), _P]),
    "skfw_recover": (_I, [ctypes.POINTER(RecoverDesc), _P]),
})
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi

_lib = None


def load_library() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


def _ptr(t, off: int = 0):
    return None if t is None else t.data_ptr() + 4 * off


class FengwuEngine(Engine):
    prepare_symbol = "skfw_prepare_weight"

    def __init__(self, cfg: FengwuConfig | None = None, device: str | torch.device = "cuda:0"):
        self.cfg = c = cfg or FengwuConfig()
        check_config(c)
        self._bind(load_library(), device, (c.channels, c.n_lat, c.n_lon))

    # ---- loading ---- #
    def _f32(self, ts) -> torch.Tensor:
        return torch.stack([torch.as_tensor(t).float().cpu() for t in ts]).contiguous().to(self.device)

    def _blocks(self, p, prefixes: list, where: str, n: int) -> list:
        """n Swin blocks, each stacked over ``prefixes`` (the modalities, or the fuser alone)."""
        c = self.cfg
        grid, win, D, heads = block_geometry(c, where)
        out = []
        for i in range(n):
            g = lambda name: [p[f"{pre}.{i}.{name}"] for pre in prefixes]           # noqa: E731
            sh = block_shift(win, i)
            tabs = [bias_table(c, t, grid, win, sh) for t in g("attn.bias_table")]
            out.append(dict(n1_g=self._f32(g("norm1.weight")), n1_b=self._f32(g("norm1.bias")), qkv=self._weight(self._f32(g("attn.qkv.weight"))),
                            qkv_b=self._f32(g("attn.qkv.bias")), table=self._f32(tabs), proj=self._weight(self._f32(g("attn.proj.weight"))),
                            proj_b=self._f32(g("attn.proj.bias")), n2_g=self._f32(g("norm2.weight")), n2_b=self._f32(g("norm2.bias")),
                            fc1=self._weight(self._f32(g("mlp.fc1.weight"))), fc1_b=self._f32(g("mlp.fc1.bias")),
                            fc2=self._weight(self._f32(g("mlp.fc2.weight"))), fc2_b=self._f32(g("mlp.fc2.bias")), shift=sh,
                            types=window_types(c, grid, win, sh)))
        return out

    def load_params(self, params):
        """``params``: a mapping keyed by ``spec.full_param_spec`` (``norm.mean``, ``norm.std``, then the network), shape-checked."""
        c, dev = self.cfg, self.device
        shapes = dict(full_param_spec(c))
        for name, shape in shapes.items():
            if name not in params:
                raise ValueError(f"parameter {name} missing (expected shape {shape})")
        p = CheckedParams(params, shapes, source=lambda name: f"FengwuConfig.{shape_source(name)}")
        for name in shapes:                      # every shape before any upload: a mismatched graph is refused as a whole
            p[name]
        D1, D2 = c.dims
        names = [n for n, _ in c.modalities]
        enc, dec = [f"enc.{n}" for n in names], [f"dec.{n}" for n in names]
        with torch.cuda.device(dev):
            self.upload_affine(p["norm.mean"], p["norm.std"], c.channels)
            emb = torch.zeros(c.n_mod, D1, c.k_embed)
            rec = torch.zeros(c.n_mod, c.n_recover, D1)
            for z, (n, cm) in enumerate(c.modalities):
                emb[z, :, :32 * cm] = p[f"enc.{n}.embed.weight"].float().reshape(D1, -1)
                rec[z, :16 * cm] = p[f"dec.{n}.recovery.weight"].float().permute(1, 2, 3, 0).reshape(16 * cm, D1)
            rec_b = torch.zeros(c.n_mod, c.c_max)
            for z, (n, cm) in enumerate(c.modalities):
                rec_b[z, :cm] = p[f"dec.{n}.recovery.bias"].float()
            self.w = dict(
                embed=self._weight(emb), embed_b=self._f32([p[f"{e}.embed.bias"] for e in enc]),
                en_g=self._f32([p[f"{e}.embed_norm.weight"] for e in enc]), en_b=self._f32([p[f"{e}.embed_norm.bias"] for e in enc]),
                enc0=self._blocks(p, [f"{e}.s0" for e in enc], "s0", c.enc_depths[0]),
                mg_g=self._f32([p[f"{e}.merge.norm.weight"] for e in enc]), mg_b=self._f32([p[f"{e}.merge.norm.bias"] for e in enc]),
                merge=self._weight(self._f32([p[f"{e}.merge.reduction.weight"] for e in enc])),
                enc1=self._blocks(p, [f"{e}.s1" for e in enc], "s1", c.enc_depths[1]),
                fuser=self._blocks(p, ["fuser"], "fuser", c.fuser_depth),
                dec1=self._blocks(p, [f"{d}.s1" for d in dec], "s1", c.dec_depths[0]),
                expand=self._weight(self._f32([p[f"{d}.expand.weight"] for d in dec])),
                skip=self._weight(self._f32([p[f"{d}.skip.weight"] for d in dec])), skip_b=self._f32([p[f"{d}.skip.bias"] for d in dec]),
                dec0=self._blocks(p, [f"{d}.s0" for d in dec], "s0", c.dec_depths[1]),
                recover=self._weight(rec), recover_b=rec_b.contiguous().to(dev))
            (h1, w1), (h2, w2) = c.grid1, c.grid2
            M, t1, t2 = c.n_mod, h1 * w1, h2 * w2
            big = M * max(t1 * D1, t2 * D2, t2 * 4 * D1)
            z = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)         # noqa: E731
            self.buf = dict(emb=z(M * t1 * D1), xe=z(M * t1 * D1), xd=z(M * t1 * D1), up=z(M * t1 * D1), x2=z(M * t2 * D2), h=z(big),
                            att=z(M * max(t1 * D1, t2 * D2)), qkv=z(3 * M * max(t1 * D1, t2 * D2)),
                            hid=z(c.mlp_ratio * M * max(t1 * D1, t2 * D2)))
        self.prepared = True

    # ---- launches (also the units the GPU tests check) ---- #
    def _s(self):
        return native.stream(self.device)

    def _mods(self, arr_type=_I * _MODS):
        c = self.cfg
        return arr_type(*[o for o in c.offsets]), arr_type(*[n for _, n in c.modalities])

    def embed(self, x0, x1, out=None):
        """Every modality's patch embedding + bias -> ``emb`` [mods][h1 w1][D1] (before its LayerNorm)."""
        c, W = self.cfg, self.w["embed"]
        out = self.buf["emb"] if out is None else out
        off, cnt = self._mods()
        d = EmbedDesc(x0.data_ptr(), x1.data_ptr(), self.mean.data_ptr(), self.inv_std.data_ptr(), W.buf.data_ptr(), W.plane, W.w_sb, W.ldw,
                      self.w["embed_b"].data_ptr(), out.data_ptr(), c.n_mod, c.n_lat, c.n_lon, c.lat_pad[1], c.grid1[0], c.dims[0], c.k_embed,
                      off, cnt)
        native.check(self.lib.skfw_embed(ctypes.byref(d), self._s()), "skfw_embed", self.lib)

    def layer_norm(self, x, gamma, beta, out, rows: int, batch: int, C: int, merge=None):
        """merge = (h_src, w_src, front): the 2 x 2 patch-merge gather of [batch][h_src][w_src][C / 4] first."""
        h, w, f = merge or (0, 0, 0)
        d = LnDesc(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), rows, batch, C, 1 if merge else 0, h, w, f, self.cfg.ln_eps)
        native.check(self.lib.skfw_layer_norm(ctypes.byref(d), self._s()), "skfw_layer_norm", self.lib)

    def linear(self, a, W, bias, out, M: int, act=0, res=None, a2=None, k_split=0, expand=None, mod=None):
        """Batched over W.batch (the modalities); ``mod``: only that entry of W and of the bias, as batch 1 (the caller passes that
        entry's a / out).  expand = (w_tok, h_out, front): the patch expand's shuffle + crop."""
        batch, z = (W.batch, 0) if mod is None else (1, mod)
        N, K = W.N, W.K
        lda = k_split if a2 is not None else K
        w_tok, h_out, front = expand or (0, 0, 0)
        o_sb = (h_out * 2 * w_tok * (N // 4)) if expand else M * N
        d = LinearDesc(a.data_ptr(), _ptr(a2), W.buf.data_ptr() + 2 * z * W.w_sb, W.plane, W.w_sb, W.ldw, _ptr(bias, z * N), _ptr(res),
                       out.data_ptr(), M * lda, M * (K - k_split), o_sb, N, batch, M, N, K, lda, K - k_split, k_split, act,
                       1 if expand else 0, w_tok, h_out, front)
        native.check(self.lib.skfw_linear(ctypes.byref(d), self._s()), "skfw_linear", self.lib)

    def attention(self, qkv, qkv_b, table, out, where: str, shift, types, mod=None):
        c = self.cfg
        grid, win, D, heads = block_geometry(c, where)
        if where == "fuser":
            Z, (H, W), batch = c.n_mod, c.grid2, 1
        else:
            Z, (H, W), batch = 1, (c.grid1 if where == "s0" else c.grid2), c.n_mod
        z = 0
        if mod is not None:
            batch, z = 1, mod
        fh = pad_to(H, win[1], c.pad)[1]
        N = win[0] * win[1] * win[2]
        tsb = types[0] * types[1] * heads * N * N
        d = AttnDesc(qkv.data_ptr(), _ptr(qkv_b, z * 3 * D), _ptr(table, z * tsb), out.data_ptr(), tsb, batch, Z, H, W, grid[0], grid[1],
                     grid[2], 0, fh, 0, *win, *shift, types[0], types[1], D, heads, 1.0 / math.sqrt(D // heads))
        native.check(self.lib.skfw_window_attention(ctypes.byref(d), self._s()), "skfw_window_attention", self.lib)

    def recover(self, a, out):
        c, W = self.cfg, self.w["recover"]
        off, cnt = self._mods()
        d = RecoverDesc(a.data_ptr(), W.buf.data_ptr(), W.plane, W.w_sb, W.ldw, self.w["recover_b"].data_ptr(), self.mean.data_ptr(),
                        self.std.data_ptr(), out.data_ptr(), c.n_mod, c.grid1[0], c.grid1[1], c.dims[0], c.c_max, c.n_lat, c.lat_pad[1], off, cnt)
        native.check(self.lib.skfw_recover(ctypes.byref(d), self._s()), "skfw_recover", self.lib)

    # ---- blocks and stages ---- #
    def swin_block(self, B: dict, x, where: str):
        """x <- x + proj(attn(LN1(x))); x <- x + fc2(GELU(fc1(LN2(x)))) on the grid of ``where``, every batch entry at once."""
        c, b = self.cfg, self.buf
        _, _, D, _ = block_geometry(c, where)
        batch = B["qkv"].batch
        rows = (c.grid1[0] * c.grid1[1]) if where == "s0" else (c.grid2[0] * c.grid2[1]) * (c.n_mod if where == "fuser" else 1)
        self.layer_norm(x, B["n1_g"], B["n1_b"], b["h"], rows, batch, D)
        self.linear(b["h"], B["qkv"], B["qkv_b"], b["qkv"], rows)
        self.attention(b["qkv"], B["qkv_b"], B["table"], b["att"], where, B["shift"], B["types"])
        self.linear(b["att"], B["proj"], B["proj_b"], x, rows, res=x)
        self.layer_norm(x, B["n2_g"], B["n2_b"], b["h"], rows, batch, D)
        self.linear(b["h"], B["fc1"], B["fc1_b"], b["hid"], rows, act=1)
        self.linear(b["hid"], B["fc2"], B["fc2_b"], x, rows, res=x)

    def embed_stage(self, x0, x1):
        c, b = self.cfg, self.buf
        self.embed(x0, x1)
        self.layer_norm(b["emb"], self.w["en_g"], self.w["en_b"], b["xe"], c.grid1[0] * c.grid1[1], c.n_mod, c.dims[0])

    def encoders(self):
        c, b, W = self.cfg, self.buf, self.w
        for B in W["enc0"]:
            self.swin_block(B, b["xe"], "s0")
        self.merge(b["xe"], b["x2"])
        for B in W["enc1"]:
            self.swin_block(B, b["x2"], "s1")

    def merge(self, x, out):
        c, b = self.cfg, self.buf
        (h1, w1), (h2, w2) = c.grid1, c.grid2
        self.layer_norm(x, self.w["mg_g"], self.w["mg_b"], b["h"], h2 * w2, c.n_mod, 4 * c.dims[0], merge=(h1, w1, c.merge_pad[1]))
        self.linear(b["h"], self.w["merge"], None, out, h2 * w2)

    def fuser(self):
        for B in self.w["fuser"]:
            self.swin_block(B, self.buf["x2"], "fuser")

    def expand_skip(self, x2, skip, out):
        c, b = self.cfg, self.buf
        (h1, w1), (h2, w2) = c.grid1, c.grid2
        self.linear(x2, self.w["expand"], None, b["up"], h2 * w2, expand=(w2, h1, c.merge_pad[1]))
        self.linear(b["up"], self.w["skip"], self.w["skip_b"], out, h1 * w1, a2=skip, k_split=c.dims[0])

    def decoders(self, y):
        b, W = self.buf, self.w
        for B in W["dec1"]:
            self.swin_block(B, b["x2"], "s1")
        self.expand_skip(b["x2"], b["xe"], b["xd"])
        for B in W["dec0"]:
            self.swin_block(B, b["xd"], "s0")
        self.recover(b["xd"], y)

    def call(self, x0: torch.Tensor, x1: torch.Tensor) -> torch.Tensor:
        """One network call: states at t - 6 h (x0) and t (x1) -> a new tensor, the state at t + 6 h."""
        self.require_prepared("call")
        self.check_state(x0, "x0")
        self.check_state(x1, "x1")
        with torch.cuda.device(self.device):
            y = torch.empty(self.state_shape, dtype=torch.float32, device=self.device)
            self.embed_stage(x0, x1)
            self.encoders()
            self.fuser()
            self.decoders(y)
        return y
