"""FourCastNet v1 (AFNO) in plain PyTorch-CPU: the contract of the HIP engine restated with torch.fft (rfft2 / irfft2), not with the
engine's DFT GEMMs.  Self-contained on purpose (no skyrim_amd import): parameters are the slot dict of skyrim_amd.fcn.spec.param_spec,
``cfg`` anything with the FcnConfig fields."""
from __future__ import annotations

import torch
import torch.nn.functional as F


def kept_lon_modes(cfg) -> int:
    if getattr(cfg, "kept_lon_modes", None) is not None:
        return cfg.kept_lon_modes
    return int(((cfg.n_lat // cfg.patch) // 2 + 1) * cfg.hard_thresholding_fraction)


def spectral_mlp(U: torch.Tensor, w1, b1, w2, b2, lam: float) -> torch.Tensor:
    """Block-diagonal complex MLP on a spectrum U (..., nb, bs) complex: ReLU after the first layer, softshrink after the second."""
    ur, ui = U.real, U.imag
    o1r = F.relu(torch.einsum("...bi,bio->...bo", ur, w1[0]) - torch.einsum("...bi,bio->...bo", ui, w1[1]) + b1[0])
    o1i = F.relu(torch.einsum("...bi,bio->...bo", ui, w1[0]) + torch.einsum("...bi,bio->...bo", ur, w1[1]) + b1[1])
    o2r = torch.einsum("...bi,bio->...bo", o1r, w2[0]) - torch.einsum("...bi,bio->...bo", o1i, w2[1]) + b2[0]
    o2i = torch.einsum("...bi,bio->...bo", o1i, w2[0]) + torch.einsum("...bi,bio->...bo", o1r, w2[1]) + b2[1]
    return torch.complex(F.softshrink(o2r, lam), F.softshrink(o2i, lam))


def afno_filter(u: torch.Tensor, w1, b1, w2, b2, cfg) -> torch.Tensor:
    """u (h, w, C) real -> irfft2(softshrink(MLP(rfft2(u)))) with the longitude modes m >= kept zeroed (no "+ u")."""
    h, w, C = u.shape
    nb = w1.shape[1]
    km = kept_lon_modes(cfg)
    U = torch.fft.rfft2(u, dim=(0, 1), norm="ortho")                    # (h, w//2+1, C)
    U = U.reshape(h, w // 2 + 1, nb, C // nb)
    S = torch.zeros_like(U)
    S[:, :km] = spectral_mlp(U[:, :km], w1, b1, w2, b2, cfg.sparsity_threshold)
    return torch.fft.irfft2(S.reshape(h, w // 2 + 1, C), s=(h, w), dim=(0, 1), norm="ortho")


def forward(p: dict, x: torch.Tensor, cfg, dtype=torch.float64) -> torch.Tensor:
    """One step: raw state x (cin, H, W) -> (cout, H, W) in physical units."""
    P, e = cfg.patch, cfg.embed_dim
    h, w = cfg.n_lat // P, cfg.n_lon // P
    q = {k: v.to(dtype) for k, v in p.items()}
    mean, std = q["norm.mean"], q["norm.std"]
    xn = (x.to(dtype) - mean[:, None, None]) / std[:, None, None]
    t = F.conv2d(xn[None], q["patch_embed.proj.weight"], q["patch_embed.proj.bias"], stride=P)[0]    # (e, h, w)
    t = t.permute(1, 2, 0) + q["pos_embed"].reshape(h, w, e)
    for i in range(cfg.depth):
        b = f"blocks.{i}."
        r = t
        u = F.layer_norm(t, (e,), q[b + "norm1.weight"], q[b + "norm1.bias"], cfg.eps)
        f = afno_filter(u, q[b + "filter.w1"], q[b + "filter.b1"], q[b + "filter.w2"], q[b + "filter.b2"], cfg)
        t = f + u + r
        v = F.layer_norm(t, (e,), q[b + "norm2.weight"], q[b + "norm2.bias"], cfg.eps)
        v = F.linear(F.gelu(F.linear(v, q[b + "mlp.fc1.weight"], q[b + "mlp.fc1.bias"])), q[b + "mlp.fc2.weight"], q[b + "mlp.fc2.bias"])
        t = t + v
    y = F.linear(t, q["head.weight"])                                   # (h, w, P P cout)
    co = cfg.out_chans
    y = y.reshape(h, w, P, P, co).permute(4, 0, 2, 1, 3).reshape(co, h * P, w * P)
    return (y * std[:co, None, None] + mean[:co, None, None]).to(x.dtype if x.is_floating_point() else dtype)


def per_channel_rel_err(y: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    d = (y.double() - ref.double()).abs().flatten(1).amax(1)
    return d / ref.double().abs().flatten(1).amax(1).clamp_min(1e-30)
