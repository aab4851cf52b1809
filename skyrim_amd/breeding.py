"""Bred-vector initial perturbations of the perturbed-IC ensembles (include/skyrim_breed.h).

Breeding runs the model on the perturbed and on the unperturbed analysis, keeps the difference, scales it back to the wanted amplitude,
puts it on the analysis again and repeats: what survives is the part of a perturbation the model itself grows, with the balance between
variables the model gives it.  Layers:

* the binding of libskyrim_breed.so (``SPEC``, ``load_library``, ``workspace_bytes``, ``norms``, ``apply``, ``bound_k``); the same calls are
  ``torch.ops.skyrim_hip.breed_norms / breed_apply`` (skyrim_amd/ops.py);
* ``plan`` -- every refusal of ``ensemble_forecast(breeding=...)`` that needs no device -- and ``factors``, the rescaling factors from the
  norms, in float64 on whatever device the norms lie on;
* ``Breeder``, the cycle itself: what ``ensemble.run`` calls to fill its members when ``breeding`` is given.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import native
from .members import member_count, member_set

MAX_MEMBERS, MAX_CHANNELS, TILE, MAX_GROUPS = 64, 256, 256, 256       # include/skyrim_breed.h SKBREED_*
MAX_CYCLES = 50
NORMS = ("total", "channel")
KEYS = ("cycles", "norm", "paired")
_P, _I = ctypes.c_void_p, ctypes.c_int


class NormsDesc(ctypes.Structure):
    """skbreed_norms_desc."""
    _fields_ = [("y0", _P), ("members", _P), ("members_host", _P), ("M", _I), ("C", _I), ("H", _I), ("W", _I), ("lat_weight", _P), ("S", _P),
                ("workspace", _P), ("workspace_bytes", ctypes.c_size_t)]


class ApplyDesc(ctypes.Structure):
    """skbreed_apply_desc."""
    _fields_ = [("x0", _P), ("y0", _P), ("members", _P), ("members_host", _P), ("out", _P), ("out_host", _P), ("M", _I), ("C", _I), ("H", _I),
                ("W", _I), ("f", _P)]


SPEC = native.Spec("skyrim_breed", "SKYRIM_BREED_LIB", "skbreed", 1, {            # include/skyrim_breed.h SKBREED_ABI_VERSION
    "skbreed_abi_version": (_I, []),
    "skbreed_groups": (_I, [_I, _I, _I]),
    "skbreed_workspace_bytes": (ctypes.c_size_t, [_I, _I, _I, _I]),
    "skbreed_norms": (_I, [ctypes.POINTER(NormsDesc), _P]),
    "skbreed_apply": (_I, [ctypes.POINTER(ApplyDesc), _P]),
}, " -- the breeding cycle has no torch fallback")
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi

_lib = None


def load_library() -> ctypes.CDLL:
    """libskyrim_breed.so (built in-tree by ``__graft_entry__.build()`` / ``make -C skyrim_amd/csrc``)."""
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


# ---- the binding ------------------------------------------------------------------------------------------------------------------------- #
def workspace_bytes(M: int, C: int, H: int, W: int) -> int:
    """``skbreed_workspace_bytes``: 0 for arguments ``skbreed_norms`` would refuse."""
    return int(load_library().skbreed_workspace_bytes(int(M), int(C), int(H), int(W)))


def groups(C: int, H: int, W: int) -> int:
    """Workgroups (= partials) per channel of ``skbreed_norms``, restated from the header: the library's ``skbreed_groups``."""
    tiles = H * ((W + TILE - 1) // TILE)
    return min(tiles, max(1, min(MAX_GROUPS, (4096 + C - 1) // C)))


def bound_k(C: int, H: int, W: int) -> int:
    """k of the header's bound |S - exact| <= k 2^-53 sum_j |w_j| sum_i d^2."""
    tiles, G = H * ((W + TILE - 1) // TILE), groups(C, H, W)
    return min(3 + 1 + (tiles + G - 1) // G + 63 + (G - 1) + 1, H * W + H + 2)


def _states(y0, members, table, what: str):
    member_count(members, what, MAX_MEMBERS)
    if y0.dim() != 3:
        raise ValueError(f"{what}: states are (C, H, W)")
    native.tensor_ptr(y0, f"{what}: the control", torch.float32, None)
    M, dev, _ = member_set(members, table, what, MAX_MEMBERS, ndim=None, dev=y0.device)
    if members[0].shape != y0.shape:
        raise ValueError(f"{what}: a member differs from the control in shape")
    return M, dev, (ctypes.c_void_p * M)(*[t.data_ptr() for t in members])


def norms(y0, members, table, lat_weight, S, workspace) -> None:
    """One ``skbreed_norms``: ``S`` (M, C) float64, S[m][c] = sum_j w_j sum_i fl32(y_m - y_0)^2 over the M ``members`` (equal-shaped
    contiguous float32 (C, H, W) device tensors; ``table`` = ``ensemble.member_table(members)``) with the H float64 weights ``lat_weight``.
    ``workspace``: a device tensor of at least ``workspace_bytes(M, C, H, W)`` bytes.  Queued on torch's current stream."""
    M, dev, host = _states(y0, members, table, "breed_norms")
    C, H, W = y0.shape
    if C > MAX_CHANNELS:
        raise ValueError(f"breed_norms: {C} channels; 1 to {MAX_CHANNELS} are supported")
    d = NormsDesc()
    d.y0, d.members, d.members_host, d.M, d.C, d.H, d.W = y0.data_ptr(), table.data_ptr(), ctypes.addressof(host), M, C, H, W
    d.lat_weight = native.tensor_ptr(lat_weight, "breed_norms: lat_weight", torch.float64, dev)
    if lat_weight.numel() != H:
        raise ValueError(f"breed_norms: {lat_weight.numel()} weights for {H} rows")
    d.S = native.tensor_ptr(S, "breed_norms: S", torch.float64, dev)
    if tuple(S.shape) != (M, C):
        raise ValueError(f"breed_norms: S must be ({M}, {C})")
    if not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError("breed_norms: workspace must be a contiguous device tensor")
    d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    lib = load_library()
    with torch.cuda.device(dev):
        native.check(lib.skbreed_norms(ctypes.byref(d), native.stream(dev)), "skbreed_norms", lib)


def apply(x0, y0, members, table, f, out, out_table) -> None:
    """One ``skbreed_apply``: ``out[m] = x0 + f[m][c] * (members[m] - y0)`` in fp32, a bit copy of ``x0`` where ``f`` is 0.  ``f``: float32
    (M, C) on the device; ``out``: M tensors, none of them ``x0``, ``y0`` or the ``members`` entry of ANOTHER member (``out[m]`` may be
    ``members[m]``: in place); ``out_table`` = ``ensemble.member_table(out)``.  Queued on torch's current stream."""
    M, dev, host = _states(y0, members, table, "breed_apply")
    C, H, W = y0.shape
    if C > MAX_CHANNELS:
        raise ValueError(f"breed_apply: {C} channels; 1 to {MAX_CHANNELS} are supported")
    if len(out) != M:
        raise ValueError(f"breed_apply: {len(out)} outputs for {M} members")
    _, _, out_host = _states(y0, out, out_table, "breed_apply: out")
    d = ApplyDesc()
    d.x0, d.y0 = native.tensor_ptr(x0, "breed_apply: x0", torch.float32, dev), y0.data_ptr()
    if x0.shape != y0.shape:
        raise ValueError("breed_apply: x0 differs from the control forecast in shape")
    d.members, d.members_host, d.out, d.out_host = table.data_ptr(), ctypes.addressof(host), out_table.data_ptr(), ctypes.addressof(out_host)
    d.M, d.C, d.H, d.W = M, C, H, W
    d.f = native.tensor_ptr(f, "breed_apply: f", torch.float32, dev)
    if tuple(f.shape) != (M, C):
        raise ValueError(f"breed_apply: f must be ({M}, {C})")
    lib = load_library()
    with torch.cuda.device(dev):
        code = lib.skbreed_apply(ctypes.byref(d), native.stream(dev))
    if code == -1:
        raise ValueError("breed_apply: refused (SKBREED_E_ARG): an output overlaps x0, y0, another member's state or another output")
    native.check(code, "skbreed_apply", lib)


# ---- the request --------------------------------------------------------------------------------------------------------------------------- #
@dataclass
class Plan:
    """A validated ``breeding=`` request."""
    cycles: int
    norm: str = "total"
    paired: bool = False

    def as_dict(self) -> dict:
        return dict(cycles=self.cycles, norm=self.norm, paired=self.paired)


def plan(model, breeding) -> Plan | None:
    """Every refusal of ``ensemble_forecast(breeding=...)`` that needs no device.  ``breeding``: None, or a dict with ``cycles`` (int,
    1 .. 50), ``norm`` ("total", the default: one factor per member over the perturbed channels; or "channel": every channel to its own
    amplitude) and ``paired`` (False; True: members 2j - 1 and 2j are +- one bred vector).  The model must have one history level and
    the same channels in and out, in order: the difference of two forecasts is put back on the analysis channel by channel."""
    if breeding is None:
        return None
    if not isinstance(breeding, dict):
        raise ValueError(f"breeding = {breeding!r}: None or a dict with the keys {KEYS}")
    unknown = [k for k in breeding if k not in KEYS]
    if unknown:
        raise ValueError(f"breeding: unknown keys {unknown}; choose from {KEYS}")
    cycles = breeding.get("cycles")
    if isinstance(cycles, bool) or not isinstance(cycles, (int, np.integer)) or not 1 <= cycles <= MAX_CYCLES:
        raise ValueError(f"breeding: cycles = {cycles!r}: an integer from 1 to {MAX_CYCLES}")
    norm = breeding.get("norm", "total")
    if norm not in NORMS:
        raise ValueError(f"breeding: norm = {norm!r}: choose from {NORMS}")
    paired = breeding.get("paired", False)
    if not isinstance(paired, (bool, np.bool_)):
        raise ValueError(f"breeding: paired = {paired!r}: True or False")
    levels = int(getattr(model, "n_history_levels", 1))
    if levels != 1:
        raise ValueError(f"breeding: {type(model).__name__} steps from {levels} history levels; a bred vector is the difference of two "
                         "forecasts put back on ONE analysis state, so only models with one history level are bred (DESIGN.md 27)")
    if list(model.in_channel_names) != list(model.out_channel_names):
        raise ValueError(f"breeding: the input channels of {type(model).__name__} are not its output channels (forcing or static channels "
                         "that the model does not forecast): the forecast difference cannot be put back on the analysis (DESIGN.md 27)")
    if len(model.in_channel_names) > MAX_CHANNELS:
        raise ValueError(f"breeding: {len(model.in_channel_names)} channels; at most {MAX_CHANNELS} (SKBREED_MAX_CHANNELS)")
    return Plan(int(cycles), norm, bool(paired))


def factors(S, std, perturb_scale: float, norm: str, mask, weight_sum: float, n_lon: int) -> torch.Tensor:
    """The fp32 table f (M, C) of ``breed_apply`` from the norms ``S`` (M, C) float64, on the device of ``S`` and without a host
    synchronisation.  A[m][c] = S[m][c] / (weight_sum n_lon) is the area-mean square of the difference (``weight_sum``: the sum of the
    latitude weights).  ``std``: the C per-channel sigmas; ``mask``: bool (C,), the perturbed channels, or None = all.
      "channel":  f = perturb_scale std_c / sqrt(A[m][c])
      "total":    f = perturb_scale / sqrt(mean over the perturbed channels of A[m][c] / std_c^2), one factor per member
    f is exactly 0 for channels that are not perturbed (a channel with sigma 0 counts as not perturbed) and wherever the divisor is 0; it
    is formed in float64 and rounded to fp32 once."""
    if norm not in NORMS:
        raise ValueError(f"norm = {norm!r}: choose from {NORMS}")
    S = S.to(torch.float64)
    std = std.to(S.device, torch.float64).reshape(1, -1)
    on = std > 0
    if mask is not None:
        on = on & torch.as_tensor(mask, dtype=torch.bool, device=S.device).reshape(1, -1)
    A = S / (float(weight_sum) * float(n_lon))
    zero = torch.zeros((), dtype=torch.float64, device=S.device)
    if norm == "channel":
        div = torch.sqrt(A)
        f = float(perturb_scale) * std / div
        f = torch.where(on & (div != 0), f, zero)
    else:
        one = torch.ones((), dtype=torch.float64, device=S.device)
        rel = torch.where(on, A / torch.where(on, std * std, one), zero)
        count = on.sum().to(torch.float64)
        div = torch.sqrt(rel.sum(dim=1, keepdim=True) / torch.where(count > 0, count, one))
        f = float(perturb_scale) / div
        f = torch.where(on & (div != 0), f.expand_as(A), zero)
    return f.to(torch.float32).contiguous()


# ---- the cycle ------------------------------------------------------------------------------------------------------------------------------ #
def step_once(model, time, x: torch.Tensor, who: str) -> torch.Tensor:
    """Lead 1 of the model's own generator from ``x`` (1, 1, C, H, W) at ``time``, as (C, H, W); the generator is closed and its pending
    non-finite check taken.  What a breeding cycle and a stochastic step (skyrim_amd/stochastic.py) advance a member with."""
    loop = model(time, x)
    try:
        next(loop)
        _, out, _ = next(loop)
    except FloatingPointError as e:
        raise FloatingPointError(f"{who}: {e}") from e
    try:
        loop.close()
    except FloatingPointError as e:
        raise FloatingPointError(f"{who}: {e}") from e
    return (out[0] if out.dim() == 4 else out).contiguous()


class Breeder:
    """The breeding cycle of one ``ensemble_forecast``.

    ``model``: the TimeLoop; ``plan``: ``plan(model, breeding)``; ``x0``: the analysis (1, 1, C, H, W) on the GPU; ``std``: the C sigmas;
    ``seeder(m, out)`` writes the seed perturbation of member m >= 1 into ``out`` -- exactly the call ``perturbation="white"`` /
    ``"spherical"`` makes without breeding; ``mask``: the perturbed channels (bool (C,)) or None.

    The control forecast y_0 is the state the model's own generator yields at lead 1 from ``x0``; it is made once.  A cycle is, for a
    batch of members: each member one step, ONE ``breed_norms`` launch, ``factors``, ONE ``breed_apply`` launch that writes the next x_m
    over the previous one.  ``member(m)`` returns the final x_m; member 0 is a bit copy of ``x0``.  With ``paired`` the members 2j - 1 and 2j share the vector
    bred as member 2j - 1, with factors +f and -f: half the model steps.  A member's bits depend on (seed, member, request) only: every
    member is normalised on its own, so neither the ensemble size nor the batch size enters.

    Memory: beside ``x0`` and ``y0`` the final states of all members stay alive (they are what the ensemble starts from), and during a
    cycle one more state per member of the batch (its forecast) plus two transient ones inside a model step: ``(n_members + batch + 4)``
    states.  That is checked against the free device memory before the first step.

    After ``run()``: ``growth`` (cycles, n_members, C) float64 on the host, sqrt(S_k / S_{k-1}) with S_0 the seed's own norm
    (``breed_norms`` of (x_m, x0)) and NaN where S_{k-1} is 0 -- the control's row, and an even member of a pair repeats its partner's;
    ``S`` (cycles + 1, n_members, C) likewise; ``factors_used`` (cycles, n_members, C) float32, the tables ``breed_apply`` got (an even
    member of a pair: the negated row of its partner)."""

    def __init__(self, model, plan: Plan, x0: torch.Tensor, std: torch.Tensor, perturb_scale: float, seed: int, start_time, seeder,
                 mask=None, batch: int = 16, trace: bool = False):
        from .verify import area_weights
        if x0.dim() != 5 or x0.shape[0] != 1 or x0.shape[1] != 1:
            raise ValueError(f"breeding needs a state of one history level (1, 1, C, H, W), got {tuple(x0.shape)}")
        if x0.device.type != "cuda":
            raise RuntimeError("breeding runs its cycle with HIP kernels: the state must be on a GPU")
        self.model, self.plan, self.x0, self.seed, self.start_time, self.seeder = model, plan, x0, int(seed), start_time, seeder
        self.perturb_scale, self.std, self.mask = float(perturb_scale), std, mask
        self.batch = max(1, min(int(batch), MAX_MEMBERS))
        self.C, self.H, self.W = (int(v) for v in x0.shape[2:])
        w = area_weights(np.asarray(model.grid.lat, np.float64))
        self.weight_sum = float(w.sum())
        self.weights = torch.from_numpy(w).to(x0.device)
        self.trace = [] if trace else None                 # per (cycle, member): (y_m, x_m) on the host, for the tests
        self.y0 = None
        self.growth = self.S = self.factors_used = None
        self._x = {}

    def _step(self, x: torch.Tensor, who: str) -> torch.Tensor:
        """Lead 1 of the model's own generator from ``x``; the generator is closed and its pending non-finite check taken."""
        return step_once(self.model, self.start_time, x, f"breeding, {who}")

    def _check_memory(self, n_members: int, batch: int) -> None:
        state = self.x0.numel() * 4
        need = (n_members + batch + 4) * state
        free, _ = torch.cuda.mem_get_info(self.x0.device)
        free += torch.cuda.memory_reserved(self.x0.device) - torch.cuda.memory_allocated(self.x0.device)
        if need > free:
            raise RuntimeError(f"breeding {n_members} members in batches of {batch} needs {need / 2 ** 30:.1f} GiB of device memory for its "
                               f"states ({n_members} + {batch} + 4 states of {state / 2 ** 20:.0f} MiB); {free / 2 ** 30:.1f} GiB are free: "
                               "fewer members or a smaller batch")

    def run(self, n_members: int) -> None:
        from .ensemble import member_table
        M, p, dev = int(n_members), self.plan, self.x0.device
        C, H, W, K = self.C, self.H, self.W, self.plan.cycles
        bred = [m for m in range(1, M) if not p.paired or m % 2 == 1]
        batch = max(1, min(self.batch, len(bred) or 1))
        self._check_memory(M, batch)
        S = torch.zeros((K + 1, M, C), dtype=torch.float64, device=dev)
        F = torch.zeros((K, M, C), dtype=torch.float32, device=dev)
        x0 = self.x0[0, 0]
        self._x = {}
        if bred:
            self.y0 = self._step(self.x0, "the control forecast")
            work = torch.empty(max(workspace_bytes(batch, C, H, W), 8) // 8, dtype=torch.float64, device=dev)
        for b0 in range(0, len(bred), batch):
            ids = bred[b0:b0 + batch]
            idx = torch.tensor(ids, dtype=torch.int64, device=dev)
            xs = []
            for m in ids:
                xm = torch.empty_like(self.x0)
                self.seeder(m, xm)
                xs.append(xm)
            xv = [x[0, 0] for x in xs]
            x_table = member_table(xv)
            Sb = torch.empty((len(ids), C), dtype=torch.float64, device=dev)
            norms(x0, xv, x_table, self.weights, Sb, work)              # the seed's own norm
            S[0].index_copy_(0, idx, Sb)
            for k in range(1, K + 1):
                ys = [self._step(x, f"member {m}, cycle {k}") for m, x in zip(ids, xs)]
                y_table = member_table(ys)
                norms(self.y0, ys, y_table, self.weights, Sb, work)
                S[k].index_copy_(0, idx, Sb)
                f = factors(Sb, self.std, self.perturb_scale, p.norm, self.mask, self.weight_sum, W)
                F[k - 1].index_copy_(0, idx, f)
                apply(x0, self.y0, ys, y_table, f, xv, x_table)
                if p.paired:                                             # the mirrored members: the same vector, -f
                    twins = [m + 1 for m in ids if m + 1 < M]
                    if twins:
                        F[k - 1].index_copy_(0, torch.tensor(twins, dtype=torch.int64, device=dev), -f[:len(twins)])
                    if k == K and twins:
                        tv = [torch.empty_like(self.x0) for _ in twins]
                        tw = [t[0, 0] for t in tv]
                        apply(x0, self.y0, ys[:len(twins)], member_table(ys[:len(twins)]), (-f[:len(twins)]).contiguous(), tw, member_table(tw))
                        for m, t in zip(twins, tv):
                            self._x[m] = t
                if self.trace is not None:
                    self.trace.append(dict(cycle=k, members=list(ids), y=[y.cpu().numpy() for y in ys], x=[x.cpu().numpy() for x in xv]))
                del ys, y_table
            for m, x in zip(ids, xs):
                self._x[m] = x
        if p.paired:                                                     # an even member repeats the record of its partner
            for m in range(2, M, 2):
                S[:, m] = S[:, m - 1]
        ratio = S[1:] / S[:-1]
        growth = torch.where(S[:-1] == 0, torch.full_like(ratio, float("nan")), torch.sqrt(ratio))
        self.growth, self.S, self.factors_used = growth.cpu().numpy(), S.cpu().numpy(), F.cpu().numpy()       # one copy, at the end

    def member(self, m: int) -> torch.Tensor:
        """The initial state of member m (1, 1, C, H, W) after ``run``; member 0: a bit copy of ``x0``."""
        if m == 0:
            return self.x0.clone()
        return self._x.pop(m)
