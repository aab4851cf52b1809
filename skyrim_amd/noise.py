"""Spatially correlated (spherical) initial-condition perturbations (include/skyrim_noise.h).

Per member and per (history level, channel) an isotropic Gaussian random field on the sphere with unit pointwise variance and a
prescribed spectrum: random spherical-harmonic coefficients from the ensemble's Philox generator (``noise_coeffs``), synthesised on the
device by two calls of the SFNO engine's three-term GEMM (Legendre synthesis per order, inverse DFT per field) against matrices built
once per (grid, lmax), and put on the initial condition by ``noise_apply``.  Layers:

* the binding of libskyrim_noise.so (``SPEC``, ``load_library``, ``coeffs``, ``apply``); the same calls are
  ``torch.ops.skyrim_hip.noise_coeffs / noise_apply`` (skyrim_amd/ops.py);
* the host-side definitions in float64: ``spectrum``, ``scale_exponent`` (the power of two that keeps the GEMM's fp16 planes normal),
  ``full_grid`` (which grids qualify), ``plan`` (every refusal of a request, before the device is touched);
* ``Synthesis`` (cached per device, grid and lmax) and ``Perturber``, what ``ensemble.run`` calls once per member.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import native

KINDS = ("white", "spherical")
EARTH_RADIUS_KM = 6371.0
DEFAULT_LMAX = 256
MAX_LMAX = 4096                                           # include/skyrim_noise.h SKNOISE_MAX_LMAX
_P, _I, _U = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32

SPEC = native.Spec("skyrim_noise", "SKYRIM_NOISE_LIB", "sknoise", 1, {       # include/skyrim_noise.h SKNOISE_ABI_VERSION
    "sknoise_abi_version": (_I, []),
    "sknoise_coeffs": (_I, [_P, _P, _I, _I, _U, _U, _U, _I, _P]),
    "sknoise_apply": (_I, [_P, _P, _P, _P, ctypes.c_size_t, ctypes.c_size_t, _I, _P]),
}, " -- spherical perturbations have no torch fallback")
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi

_lib = None


def load_library() -> ctypes.CDLL:
    """libskyrim_noise.so (built in-tree by ``__graft_entry__.build()`` / ``make -C skyrim_amd/csrc``)."""
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


# ---- host-side definitions (float64) ------------------------------------------------------------------------------------------------- #
def default_lmax(n_lat_full: int, n_lon: int) -> int:
    return min(DEFAULT_LMAX, int(n_lat_full), int(n_lon) // 2)


def spectrum(lmax: int, length_scale_km: float = 500.0, alpha: float = 2.0) -> np.ndarray:
    """sigma_l for l < lmax in float64: s_l = (kappa^2 + l (l + 1))^(-alpha / 2) for l >= 1, kappa = a / length_scale, normalised so that
    sum (2 l + 1) sigma_l^2 / 4 pi = 1 (unit variance at every point); sigma_0 = 0."""
    if not (isinstance(lmax, (int, np.integer)) and 2 <= lmax <= MAX_LMAX):
        raise ValueError(f"lmax = {lmax}: 2 to {MAX_LMAX} (degree 0 carries no variance)")
    if not (math.isfinite(length_scale_km) and length_scale_km > 0):
        raise ValueError(f"length_scale_km = {length_scale_km}: must be positive")
    if not math.isfinite(alpha):
        raise ValueError(f"alpha = {alpha}: must be finite")
    l = np.arange(lmax, dtype=np.float64)
    kappa = EARTH_RADIUS_KM / float(length_scale_km)
    s = (kappa * kappa + l * (l + 1.0)) ** (-0.5 * float(alpha))
    s[0] = 0.0
    norm = math.sqrt(float(np.sum((2.0 * l + 1.0) * s * s)) / (4.0 * math.pi))
    if not (math.isfinite(norm) and norm > 0):
        raise ValueError(f"the spectrum of length_scale_km = {length_scale_km}, alpha = {alpha} has no finite variance at lmax = {lmax}")
    return s / norm


def scale_exponent(sigma: np.ndarray) -> int:
    """The power of two e of include/skyrim_noise.h: the smallest integer with sigma_min 2^e >= 2^-2; ValueError unless
    6.5 sigma_max 2^e <= 2^14 (the spectrum's dynamic range does not fit the fp16 planes of the synthesis GEMM)."""
    nz = np.asarray(sigma, np.float64)
    nz = nz[nz > 0]
    if nz.size == 0 or not np.all(np.isfinite(nz)):
        raise ValueError("the spectrum has no finite non-zero degree")
    e = -2 - int(math.floor(math.log2(float(nz.min()))))
    while float(nz.min()) * 2.0 ** e < 0.25:              # (log2 of a value just under a power of two)
        e += 1
    while float(nz.min()) * 2.0 ** (e - 1) >= 0.25:
        e -= 1
    if 6.5 * float(nz.max()) * 2.0 ** e > 2.0 ** 14:
        raise ValueError(f"the spectrum's dynamic range sigma_max / sigma_min = {float(nz.max() / nz.min()):.4g} does not fit the fp16 planes of "
                         "the synthesis (include/skyrim_noise.h: 6.5 sigma_max 2^e <= 2^14 with sigma_min 2^e >= 2^-2); lower lmax or alpha, "
                         "or choose a shorter length scale")
    return e


def full_grid(lat, lon) -> int:
    """n_lat_full of the pole-to-pole equiangular grid whose FIRST rows ``lat`` are (721 rows; FourCastNet's 720 rows are rows 0..719 of
    721); ValueError naming the grid for anything else."""
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    what = f"{lat.size} x {lon.size} grid (lat {lat[0]:g} .. {lat[-1]:g})" if lat.size and lon.size else "empty grid"
    if lat.size < 2 or lon.size < 2 or lon.size % 2:
        raise ValueError(f"spherical perturbations need an equiangular latitude-longitude grid with an even number of longitudes; got a {what}")
    d = lat[0] - lat[1]
    n_full = int(round(180.0 / d)) + 1 if d > 0 else 0
    ok = n_full >= lat.size and abs(lat[0] - 90.0) < 1e-9 and abs((n_full - 1) * d - 180.0) < 1e-6 \
        and np.allclose(lat, 90.0 - d * np.arange(lat.size), rtol=0, atol=1e-6) \
        and np.allclose(np.diff(lon), 360.0 / lon.size, rtol=0, atol=1e-6)
    if not ok:
        raise ValueError(f"spherical perturbations need the first rows of a pole-to-pole equiangular grid (north pole first, uniform "
                         f"longitudes); got a {what}")
    return n_full


@dataclass
class Plan:
    """A validated request: everything ``Perturber`` needs that the host can decide."""
    kind: str
    n_lat: int = 0
    n_lat_full: int = 0
    n_lon: int = 0
    lmax: int = 0
    length_scale_km: float = 500.0
    alpha: float = 2.0
    sigma: np.ndarray | None = None       # float64 [lmax]
    e: int = 0
    channel_mask: np.ndarray | None = None      # bool [C] or None = every channel


def plan(model, perturbation: str = "white", length_scale_km: float = 500.0, alpha: float = 2.0, lmax: int | None = None,
         perturb_channels=None) -> Plan:
    """Every refusal of the perturbation keywords of ``ensemble_forecast``, on the host: an unknown kind, a length scale <= 0, lmax outside
    2 .. min(n_lat_full, n_lon / 2), a grid that is not equiangular, unknown channels, a spectrum whose dynamic range does not fit."""
    if perturbation not in KINDS:
        raise ValueError(f"perturbation = {perturbation!r}: choose from {KINDS}")
    mask = None
    if perturb_channels is not None:
        names = list(model.in_channel_names)
        unknown = [c for c in perturb_channels if c not in names]
        if unknown:
            raise ValueError(f"perturb_channels {unknown} are not input channels of this model")
        mask = np.array([n in set(perturb_channels) for n in names], bool)
    if not (isinstance(length_scale_km, (int, float)) and math.isfinite(length_scale_km) and length_scale_km > 0):
        raise ValueError(f"length_scale_km = {length_scale_km}: must be positive")
    if perturbation == "white":
        return Plan("white", channel_mask=mask)
    lat, lon = model.grid.lat, model.grid.lon
    n_full = full_grid(lat, lon)
    top = min(n_full, len(lon) // 2)
    if lmax is None:
        lmax = default_lmax(n_full, len(lon))
    if not (isinstance(lmax, (int, np.integer)) and not isinstance(lmax, bool) and 2 <= lmax <= top):
        raise ValueError(f"lmax = {lmax}: 2 to {top} on this grid (min(n_lat_full, n_lon / 2); every order m < lmax must be resolved)")
    sigma = spectrum(int(lmax), float(length_scale_km), float(alpha))
    return Plan("spherical", len(lat), n_full, len(lon), int(lmax), float(length_scale_km), float(alpha), sigma, scale_exponent(sigma), mask)


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------- #
def coeffs(out: torch.Tensor, sigma: torch.Tensor, F: int, f_first: int, seed: int, member_first: int) -> None:
    """``out`` ([members][lmax][lmax][2][F] floats: members ``member_first ..``) from the device table ``sigma`` (lmax floats, sigma_l 2^e)
    for the fields ``f_first .. f_first + F - 1``.  Queued on torch's current stream."""
    dev = out.device
    po, ps = native.tensor_ptr(out, "noise_coeffs: out", torch.float32), native.tensor_ptr(sigma, "noise_coeffs: sigma", torch.float32, dev)
    lmax = sigma.numel()
    per = lmax * lmax * 2 * F
    if F < 1 or lmax < 1 or out.numel() == 0 or out.numel() % per:
        raise ValueError(f"noise_coeffs: out holds {out.numel()} elements, not a multiple of lmax * lmax * 2 * F = {per}")
    if not (0 <= seed < 2 ** 32 and 0 <= member_first < 2 ** 32 and 0 <= f_first and f_first + F <= 2 ** 32):
        raise ValueError("noise_coeffs: seed, member and field index are 32-bit (the generator's key and counter)")
    lib = load_library()
    with torch.cuda.device(dev):
        native.check(lib.sknoise_coeffs(po, ps, lmax, F, f_first, seed, member_first, out.numel() // per, native.stream(dev)),
                     "sknoise_coeffs", lib)


def apply(x0: torch.Tensor, y: torch.Tensor, g: torch.Tensor, out: torch.Tensor, chan_stride: int) -> None:
    """``out = fma(g[c], y, x0)`` over the flat (L, C, H, W) state; ``g``: C amplitudes, ``chan_stride`` = H * W."""
    dev = x0.device
    px = native.tensor_ptr(x0, "noise_apply: x0", torch.float32)
    py, pg, po = (native.tensor_ptr(t, f"noise_apply: {w}", torch.float32, dev) for t, w in ((y, "y"), (g, "g"), (out, "out")))
    n = x0.numel()
    if n == 0 or y.numel() != n or out.numel() != n:
        raise ValueError(f"noise_apply: x0, y and out must hold the same {n} elements")
    lib = load_library()
    with torch.cuda.device(dev):
        native.check(lib.sknoise_apply(px, py, pg, po, n, chan_stride, g.numel(), native.stream(dev)), "sknoise_apply", lib)


# ---- synthesis ------------------------------------------------------------------------------------------------------------------------- #
class Synthesis:
    """Coefficients [l][m][re/im][F] -> fields [F][n_lat][n_lon] on ``device``: the Legendre GEMM per order (ragged: order m contracts
    l >= floor32(m)) into the longitude spectrum t [m][re/im][F][ldl], then the inverse-DFT GEMM per field -- ``SfnoEngine._synthesis`` with
    mmax = lmax and C = F, against the first ``n_lat`` rows of the matrices of the ``n_lat_full``-row equiangular grid."""

    def __init__(self, device, n_lat: int, n_lat_full: int, n_lon: int, lmax: int):
        from .sfno import engine
        from .sfno.sht import ShtMatrices
        self.device = torch.device(device)
        self.n_lat, self.n_lat_full, self.n_lon, self.lmax = n_lat, n_lat_full, n_lon, lmax
        self.ldl = (n_lat + 3) // 4 * 4
        lib = engine.load_library()
        m = ShtMatrices(n_lat_full, n_lon, lmax, lmax, "equiangular")
        with torch.cuda.device(self.device):
            self.syn = native.HiLoWeight(self.device, lib.sksfno_prepare_weight, torch.from_numpy(np.ascontiguousarray(m.synthesis[:, :n_lat, :])))
            self.idft = native.HiLoWeight(self.device, lib.sksfno_prepare_weight, torch.from_numpy(m.idft))

    def sizes(self, F: int) -> tuple[int, int, int]:
        """Elements of (coefficients, longitude spectrum, fields) for F fields."""
        return self.lmax * self.lmax * 2 * F, 2 * self.lmax * F * self.ldl, F * self.n_lat * self.n_lon

    def run(self, coef: torch.Tensor, t: torch.Tensor, y: torch.Tensor, F: int) -> None:
        from . import ops
        nc, nt, ny = self.sizes(F)
        if coef.numel() < nc or t.numel() < nt or y.numel() < ny:
            raise ValueError(f"noise synthesis: buffers of {coef.numel()}, {t.numel()}, {y.numel()} elements; {nc}, {nt}, {ny} are needed")
        H, W, L, ldl, big = self.n_lat, self.n_lon, self.lmax, self.ldl, 1 << 30
        s, d = self.syn, self.idft
        # geom: ops.SFNO_GEMM_GEOM.  Legendre: batch = order, rows (re/im, field), k = degree
        ops.hip.sfno_gemm(coef, s.buf, t, None, None, None, None, None, None,
                          [0, 2 * F, big, 1, 0, L * 2 * F, s.w_sb, s.plane, s.ldw, 0, 2 * F * ldl, big, ldl, 0, 1, 2 * F, H, L, L, 0, 1, 0, 0, 0, 0, 3])
        # inverse DFT: batch = field, rows = latitudes, k = (order, re/im)
        ops.hip.sfno_gemm(t, d.buf, y, None, None, None, None, None, None,
                          [0, ldl, big, 1, 0, F * ldl, 0, d.plane, d.ldw, 0, H * W, big, W, 0, 1, H, W, 2 * L, F, 0, 0, 0, 0, 0, 0, 3])


_synth: dict = {}


def synthesis(device, n_lat: int, n_lat_full: int, n_lon: int, lmax: int) -> Synthesis:
    """The cached ``Synthesis`` of (device, grid, lmax): its matrices are built and uploaded once."""
    key = (str(torch.device(device)), n_lat, n_lat_full, n_lon, lmax)
    if key not in _synth:
        _synth[key] = Synthesis(device, n_lat, n_lat_full, n_lon, lmax)
    return _synth[key]


def release() -> None:
    """Drop the cached matrices (189 MB for 721 x 1440 at lmax 256)."""
    _synth.clear()


def amplitudes(std: torch.Tensor, perturb_scale: float, e: int, mask=None) -> torch.Tensor:
    """g[c] = fl32(perturb_scale * std[c] * 2^-e) in float64, rounded once; 0 where ``mask`` is False."""
    g = std.detach().double().cpu().numpy() * float(perturb_scale) * 2.0 ** -e
    if mask is not None:
        g = np.where(mask, g, 0.0)
    return torch.from_numpy(g.astype(np.float32)).to(std.device)


class Perturber:
    """The members of one ``ensemble_forecast`` with spherical noise: ``member(m, out)`` writes x0 (m = 0, a bit copy) or
    fma(g[c], y_m, x0).  Work buffers for ONE member are held here (coefficients, longitude spectrum, fields) and dropped with it."""

    def __init__(self, p: Plan, x0: torch.Tensor, std: torch.Tensor, perturb_scale: float, seed: int):
        self.plan, self.x0, self.seed = p, x0, int(seed)
        dev = x0.device
        L, C = x0.shape[1], x0.shape[2]
        if tuple(x0.shape[-2:]) != (p.n_lat, p.n_lon):
            raise ValueError(f"the state's grid {tuple(x0.shape[-2:])} is not the model's {p.n_lat} x {p.n_lon}")
        self.F = L * C
        self.synth = synthesis(dev, p.n_lat, p.n_lat_full, p.n_lon, p.lmax)
        self.sigma = torch.from_numpy((p.sigma * 2.0 ** p.e).astype(np.float32)).to(dev)
        self.g = amplitudes(std, perturb_scale, p.e, p.channel_mask)
        nc, nt, ny = self.synth.sizes(self.F)
        self.coef = torch.empty(nc, dtype=torch.float32, device=dev)
        self.t = torch.empty(nt, dtype=torch.float32, device=dev)
        self.y = torch.empty(ny, dtype=torch.float32, device=dev)

    def member(self, m: int, out: torch.Tensor) -> None:
        if m == 0:
            out.copy_(self.x0)
            return
        coeffs(self.coef, self.sigma, self.F, 0, self.seed, m)
        self.synth.run(self.coef, self.t, self.y, self.F)
        apply(self.x0, self.y, self.g, out, self.plan.n_lat * self.plan.n_lon)
