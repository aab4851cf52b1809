"""Per-step stochastic perturbations of the perturbed-IC ensembles: SPPT and additive noise (include/skyrim_stoch.h).

The initial perturbations (white, spherical, bred) disturb the analysis once; after that every member runs deterministically, and a network
trained on a mean-square loss damps the small-scale differences.  Here the MODEL is perturbed as it runs, by a random pattern that is
correlated in space (the spectrum of skyrim_amd/noise.py) and in time (a first-order autoregressive process per spherical-harmonic
coefficient): SPPT multiplies each step's tendency x_{k} - x_{k-1} by 1 + w with ONE clipped pattern w for all channels, additive noise puts
one field per channel on the state.  Layers:

* the binding of libskyrim_stoch.so (``SPEC``, ``load_library``, ``coeffs``, ``evolve``, ``apply``); the same calls are
  ``torch.ops.skyrim_hip.stoch_coeffs / stoch_evolve / stoch_apply`` (skyrim_amd/ops.py);
* ``plan`` -- every refusal of ``ensemble_forecast(stochastic=...)`` that needs no device, and the factors phi and psi in float64;
* ``Stepper``, the coefficient states of all members and what ``ensemble.run`` calls after each member's model step.

The defaults (amplitude 0.3, decorrelation time 6 h, length scale 500 km, clip 0.9) are those of the first of the three scales of ECMWF's
SPPT.  Nobody has measured whether they give a calibrated spread with real weights of any of the models here: ``verify --stochastic`` is
where that is tuned.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import native, noise

KINDS = ("sppt", "additive", "both")
KEYS = ("kind", "amplitude", "clip", "additive_scale", "tau_h", "length_scale_km", "alpha", "lmax", "channels")
MAX_DRAW = 2 ** 32 - 2                                    # include/skyrim_stoch.h SKSTOCH_MAX_DRAW
_P, _I, _U, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_float

SPEC = native.Spec("skyrim_stoch", "SKYRIM_STOCH_LIB", "skstoch", 1, {       # include/skyrim_stoch.h SKSTOCH_ABI_VERSION
    "skstoch_abi_version": (_I, []),
    "skstoch_coeffs": (_I, [_P, _P, _I, _I, _U, _U, _U, _I, _U, _P]),
    "skstoch_evolve": (_I, [_P, _P, _I, _I, _U, _U, _U, _I, _U, _F, _F, _P]),
    "skstoch_apply": (_I, [_P, _P, _P, _P, _P, _P, _F, _P, ctypes.c_size_t, ctypes.c_size_t, _I, _P]),
}, " -- stochastic perturbations have no torch fallback")
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi

_lib = None


def load_library() -> ctypes.CDLL:
    """libskyrim_stoch.so (built in-tree by ``__graft_entry__.build()`` / ``make -C skyrim_amd/csrc``)."""
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------- #
def _coeff_args(out, sigma, F, f_first, seed, member_first, draw, what):
    dev = out.device
    po, ps = native.tensor_ptr(out, f"{what}: out", torch.float32), native.tensor_ptr(sigma, f"{what}: sigma", torch.float32, dev)
    lmax = sigma.numel()
    per = lmax * lmax * 2 * F
    if F < 1 or lmax < 1 or out.numel() == 0 or out.numel() % per:
        raise ValueError(f"{what}: the state holds {out.numel()} elements, not a multiple of lmax * lmax * 2 * F = {per}")
    if not (0 <= seed < 2 ** 32 and 0 <= member_first < 2 ** 32 and 0 <= f_first and f_first + F <= 2 ** 32):
        raise ValueError(f"{what}: seed, member and field index are 32-bit (the generator's key and counter)")
    if not 0 <= draw <= MAX_DRAW:
        raise ValueError(f"{what}: draw = {draw}: 0 to 2^32 - 2 (the generator's fourth counter word is 1 + draw)")
    return dev, po, ps, lmax, out.numel() // per


def coeffs(out: torch.Tensor, sigma: torch.Tensor, F: int, f_first: int, seed: int, member_first: int, draw: int) -> None:
    """``noise.coeffs`` with the Philox counter word 1 + ``draw``: ``draw = 0`` gives its bits.  Queued on torch's current stream."""
    dev, po, ps, lmax, n = _coeff_args(out, sigma, F, f_first, seed, member_first, draw, "stoch_coeffs")
    lib = load_library()
    with torch.cuda.device(dev):
        native.check(lib.skstoch_coeffs(po, ps, lmax, F, f_first, seed, member_first, n, draw, native.stream(dev)), "skstoch_coeffs", lib)


def evolve(p: torch.Tensor, sigma: torch.Tensor, F: int, f_first: int, seed: int, member_first: int, draw: int, phi: float, psi: float) -> None:
    """One autoregressive step of the coefficient state ``p`` in place: ``p = fma(phi, p, fl32(psi * fresh))`` with ``fresh`` what
    ``coeffs`` writes for ``draw``.  ``phi``, ``psi``: fp32 values (``plan`` makes them)."""
    dev, pp, ps, lmax, n = _coeff_args(p, sigma, F, f_first, seed, member_first, draw, "stoch_evolve")
    if not (math.isfinite(phi) and math.isfinite(psi)):
        raise ValueError(f"stoch_evolve: phi = {phi}, psi = {psi}: must be finite")
    lib = load_library()
    with torch.cuda.device(dev):
        native.check(lib.skstoch_evolve(pp, ps, lmax, F, f_first, seed, member_first, n, draw, phi, psi, native.stream(dev)), "skstoch_evolve", lib)


def apply(xp, xn: torch.Tensor, r, y, gs, ga, lim: float, out: torch.Tensor, chan_stride: int) -> None:
    """``skstoch_apply`` over the flat (L, C, H, W) step ``xp`` -> ``xn``: the SPPT term with the plane ``r`` (``chan_stride`` floats) and
    the C amplitudes ``gs``, the additive term with the fields ``y`` and the C amplitudes ``ga``; either pair may be None.  ``out`` may
    be ``xn``."""
    dev = xn.device
    n = xn.numel()
    if (r is None) != (gs is None) or (y is None) != (ga is None) or (r is None and y is None):
        raise ValueError("stoch_apply: r goes with gs, y with ga, and one of the two terms must be given")
    pn, po = native.tensor_ptr(xn, "stoch_apply: xn", torch.float32), native.tensor_ptr(out, "stoch_apply: out", torch.float32, dev)
    if n == 0 or out.numel() != n:
        raise ValueError(f"stoch_apply: xn and out must hold the same {n} elements")
    C = (gs if gs is not None else ga).numel()
    pp = pr = pgs = py = pga = None
    if r is not None:
        pp, pr, pgs = (native.tensor_ptr(t, f"stoch_apply: {w}", torch.float32, dev) for t, w in ((xp, "xp"), (r, "r"), (gs, "gs")))
        if xp.numel() != n or r.numel() != chan_stride:
            raise ValueError(f"stoch_apply: xp must hold the state's {n} elements and r one plane of {chan_stride}")
    if y is not None:
        py, pga = native.tensor_ptr(y, "stoch_apply: y", torch.float32, dev), native.tensor_ptr(ga, "stoch_apply: ga", torch.float32, dev)
        if y.numel() != n or ga.numel() != C:
            raise ValueError(f"stoch_apply: y must hold the state's {n} elements and ga as many amplitudes as gs")
    if not 0.0 < lim <= 1.0:
        raise ValueError(f"stoch_apply: lim = {lim}: in (0, 1], so that 1 + w never changes a tendency's sign")
    lib = load_library()
    with torch.cuda.device(dev):
        code = lib.skstoch_apply(pp, pn, pr, py, pgs, pga, lim, po, n, chan_stride, C, native.stream(dev))
    if code == -1:
        raise ValueError("stoch_apply: refused (SKSTOCH_E_ARG): out is xp, or the state is not L * C * chan_stride elements")
    native.check(code, "skstoch_apply", lib)


# ---- the request --------------------------------------------------------------------------------------------------------------------------- #
def ar1(dt_h: float, tau_h: float) -> tuple[float, float]:
    """(phi, psi) of include/skyrim_stoch.h as fp32 values: phi = fl32(exp(-dt / tau)), psi = fl32(sqrt(1 - exp(-2 dt / tau))), formed in
    float64 and rounded once each; tau = 0 is white in time, (0, 1)."""
    if tau_h == 0:
        return 0.0, 1.0
    x = float(dt_h) / float(tau_h)
    return float(np.float32(math.exp(-x))), float(np.float32(math.sqrt(-math.expm1(-2.0 * x))))


@dataclass
class Plan:
    """A validated ``stochastic=`` request: everything ``Stepper`` needs that the host can decide."""
    kind: str
    amplitude: float
    clip: float
    additive_scale: float | None          # None: the ensemble's perturb_scale (``plan`` without one)
    tau_h: float
    phi: float
    psi: float
    spectrum: noise.Plan                  # grid, lmax, sigma_l, the power of two e
    channels: list | None
    channel_mask: np.ndarray | None       # bool [C] or None = every channel

    @property
    def sppt(self) -> bool:
        return self.kind in ("sppt", "both")

    @property
    def additive(self) -> bool:
        return self.kind in ("additive", "both")

    def as_dict(self) -> dict:
        s = self.spectrum
        return dict(kind=self.kind, amplitude=self.amplitude, clip=self.clip, additive_scale=self.additive_scale, tau_h=self.tau_h,
                    length_scale_km=s.length_scale_km, alpha=s.alpha, lmax=s.lmax, channels=self.channels)


def _number(d: dict, key: str, default, ok, rule: str) -> float:
    v = d.get(key, default)
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or not ok(v):
        raise ValueError(f"stochastic: {key} = {v!r}: {rule}")
    return float(v)


def plan(model, stochastic, perturb_scale: float | None = None) -> Plan | None:
    """Every refusal of ``ensemble_forecast(stochastic=...)`` that needs no device.  ``stochastic``: None, or a dict with
      ``kind``             "sppt", "additive" or "both"
      ``amplitude``        SPPT: the standard deviation of the multiplier's pattern before clipping, default 0.3
      ``clip``             the multiplier stays within 1 -+ clip, in (0, 1], default 0.9
      ``additive_scale``   additive: the standard deviation in units of each channel's ``channel_std``, default ``perturb_scale``
      ``tau_h``            decorrelation time in hours, default 6; 0: a fresh pattern every step
      ``length_scale_km``, ``alpha``, ``lmax``    the pattern's spectrum, as for ``perturbation="spherical"`` (same grid rule, same rule
                           for the power of two e: skyrim_amd/noise.py ``plan``)
      ``channels``         the input channels either term touches (default: all); the others get amplitude exactly 0
    The defaults are the first scale of ECMWF's SPPT; whether they give a calibrated spread with real weights is not measured.
    Refused: models that breeding refuses, for its reasons (each stochastic step is taken as a breeding step is: one history level, the
    same channels in and out); a Pangu loaded with its 24-h network (each step is the 6-h network from the perturbed state; the 24-h one
    would step from a state four perturbations old)."""
    if stochastic is None:
        return None
    if not isinstance(stochastic, dict):
        raise ValueError(f"stochastic = {stochastic!r}: None or a dict with the keys {KEYS}")
    unknown = [k for k in stochastic if k not in KEYS]
    if unknown:
        raise ValueError(f"stochastic: unknown keys {unknown}; choose from {KEYS}")
    kind = stochastic.get("kind")
    if kind not in KINDS:
        raise ValueError(f"stochastic: kind = {kind!r}: choose from {KINDS}")
    amplitude = _number(stochastic, "amplitude", 0.3, lambda v: v > 0, "must be positive (the standard deviation of the SPPT pattern)")
    clip = _number(stochastic, "clip", 0.9, lambda v: 0 < v <= 1, "in (0, 1]: the multiplier 1 + w must not change a tendency's sign")
    scale = None if perturb_scale is None else float(perturb_scale)
    if "additive_scale" in stochastic:
        scale = _number(stochastic, "additive_scale", None, lambda v: v > 0, "must be positive (units of channel_std)")
    elif kind != "sppt" and scale is not None and not (math.isfinite(scale) and scale > 0):
        raise ValueError(f"stochastic: additive_scale defaults to perturb_scale = {scale}, which must then be positive")
    tau = _number(stochastic, "tau_h", 6.0, lambda v: v >= 0, "hours, 0 or more (0: white in time)")
    from . import breeding
    try:
        breeding.plan(model, dict(cycles=1))               # one history level, the same channels in and out, at most 256 of them
    except ValueError as e:
        raise ValueError("stochastic: every step is taken from the perturbed state as a breeding step is, and " + str(e)) from e
    if getattr(model, "engine24", None) is not None:
        raise ValueError("stochastic: this Pangu model is loaded with its 24-h network, whose every fourth step starts from the state 24 h "
                         "earlier; a stochastic step is the 6-h network from the perturbed state -- load the model without the 24-h weights")
    names, channels, mask = list(model.in_channel_names), stochastic.get("channels"), None
    if channels is not None:
        channels = list(channels)
        missing = [c for c in channels if c not in names]
        if missing or not channels:
            raise ValueError(f"stochastic: channels {missing or channels} are not input channels of this model")
        mask = np.array([n in set(channels) for n in names], bool)
    spec = noise.plan(model, "spherical", stochastic.get("length_scale_km", 500.0), stochastic.get("alpha", 2.0), stochastic.get("lmax"))
    dt_h = model.time_step.total_seconds() / 3600.0
    phi, psi = ar1(dt_h, tau)
    return Plan(kind, amplitude, clip, scale, tau, phi, psi, spec, channels, mask)


# ---- the rollout's side ------------------------------------------------------------------------------------------------------------------ #
class Stepper:
    """The stochastic patterns of one ``ensemble_forecast``: per member m >= 1 the coefficient state of the SPPT pattern (F = 1, field
    index C) and of the additive fields (F = C, field indices 0 .. C - 1), n_members * lmax^2 * 2 * F floats together, plus the work
    buffers of ONE member's synthesis.  ``advance(k, m, xp, xn)`` perturbs member m's step k >= 1 from ``xp`` to ``xn`` in place on
    ``xn``: a fresh draw at k = 1, one autoregressive step after it, the synthesis, ``stoch_apply``.  Member 0 is never touched.  A
    member's bits depend on (seed, member, request) only."""

    def __init__(self, p: Plan, device, shape, std: torch.Tensor, n_members: int, seed: int, perturb_scale: float):
        self.plan, self.seed, self.M = p, int(seed), int(n_members)
        s = p.spectrum
        self.C, H, W = (int(v) for v in shape)
        if (H, W) != (s.n_lat, s.n_lon):
            raise ValueError(f"the state's grid {H} x {W} is not the model's {s.n_lat} x {s.n_lon}")
        dev = torch.device(device)
        self.hw = H * W
        scale = p.additive_scale if p.additive_scale is not None else float(perturb_scale)
        if p.additive and not (math.isfinite(scale) and scale > 0):
            raise ValueError(f"stochastic: additive_scale defaults to perturb_scale = {scale}, which must then be positive")
        self.terms = ([("sppt", 1, self.C)] if p.sppt else []) + ([("additive", self.C, 0)] if p.additive else [])      # (name, F, f_first)
        self.synth = noise.synthesis(dev, s.n_lat, s.n_lat_full, s.n_lon, s.lmax)
        self._check_memory(dev)
        self.sigma = torch.from_numpy((s.sigma * 2.0 ** s.e).astype(np.float32)).to(dev)
        self.gs = self.ga = None
        if p.sppt:
            self.gs = noise.amplitudes(torch.ones(self.C, dtype=torch.float32, device=dev), p.amplitude, s.e, p.channel_mask)
        if p.additive:
            self.ga = noise.amplitudes(std, scale, s.e, p.channel_mask)
        self.state, self.t, self.field = {}, {}, {}
        for name, F, _ in self.terms:
            nc, nt, ny = self.synth.sizes(F)
            self.state[name] = torch.zeros((max(self.M - 1, 1), nc), dtype=torch.float32, device=dev)
            self.t[name] = torch.empty(nt, dtype=torch.float32, device=dev)
            self.field[name] = torch.empty(ny, dtype=torch.float32, device=dev)

    def bytes_needed(self) -> int:
        """The coefficient states of members 1 .. M - 1 and one member's synthesis buffers."""
        total = 0
        for _, F, _ in self.terms:
            nc, nt, ny = self.synth.sizes(F)
            total += 4 * (max(self.M - 1, 1) * nc + nt + ny)
        return total

    def _check_memory(self, dev) -> None:
        need = self.bytes_needed()
        free, _ = torch.cuda.mem_get_info(dev)
        free += torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
        if need > free:
            s = self.plan.spectrum
            raise RuntimeError(f"stochastic perturbations of {self.M} members at lmax {s.lmax} need {need / 2 ** 30:.1f} GiB of device memory "
                               f"for the coefficient states of {sum(F for _, F, _ in self.terms)} fields per member; {free / 2 ** 30:.1f} GiB "
                               "are free: fewer members, a smaller lmax, or kind='sppt' (one field per member)")

    def advance(self, k: int, m: int, xp: torch.Tensor, xn: torch.Tensor) -> None:
        if m == 0:
            return
        if not (1 <= k <= MAX_DRAW and 1 <= m < self.M):
            raise ValueError(f"stochastic: step {k} of member {m}: steps count from 1, members 1 .. {self.M - 1}")
        p = self.plan
        for name, F, f_first in self.terms:
            coef = self.state[name][m - 1]
            if k == 1:
                coeffs(coef, self.sigma, F, f_first, self.seed, m, 1)
            else:
                evolve(coef, self.sigma, F, f_first, self.seed, m, k, p.phi, p.psi)
            self.synth.run(coef, self.t[name], self.field[name], F)
        apply(xp if p.sppt else None, xn, self.field.get("sppt"), self.field.get("additive"), self.gs, self.ga, p.clip, xn, self.hw)
