"""Ensemble scenarios on the device (include/skyrim_gram.h): how the members of an ensemble relate to each other as
patterns -- clusters (scenarios) with their probabilities, mean fields and representative members, the EOFs of the spread and the energy
score.  All of them are functions of one small object, the M x M Gram matrix of area-weighted inner products of the members' anomalies
over a region, which one HIP pass makes where the members lie in HBM; the rest is float64 algebra on the host.

Layers:

* the binding of libskyrim_gram.so (``SPEC``, ``load_library``, ``workspace_bytes``, ``gram``, ``combine``); the same calls are
  ``torch.ops.skyrim_hip.gram / member_combine``.  Neither has a CPU fallback;
* the host algebra, float64 numpy: ``centre``, ``combine_channels``, ``distances``, ``eofs``, ``ward``, ``summarise``, ``energy_score``;
* the drivers: ``LeadScenarios`` (what ``ensemble.run`` calls at every saved lead time with ``scenarios=...``) and ``from_members`` for
  member tensors that are already on the device, e.g. a forecast read back from disk;
* ``Scenarios``: the result.

This version takes raw channels on the model's own grid only: derived fields, regridded and aggregated channels are refused.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import native
from .members import fill_channels, member_set

# include/skyrim_gram.h SKGRAM_*
MAX_MEMBERS, MAX_CHANNELS, MAX_OUT, TILE, CHAIN, GROUPS = 64, 32, 8, 256, 64, 512
NORMALISE = ("spread", "std", "none")
_P = ctypes.c_void_p


class GramDesc(ctypes.Structure):
    """skgram_desc."""
    _fields_ = [("members", _P), ("M", ctypes.c_int), ("truth", _P), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("nc", ctypes.c_int), ("channels", ctypes.c_int32 * MAX_CHANNELS), ("j0", ctypes.c_int), ("nj", ctypes.c_int),
                ("i0", ctypes.c_int), ("ni", ctypes.c_int), ("lat_weight", _P), ("out", _P), ("out_stride", ctypes.c_size_t), ("workspace", _P),
                ("workspace_bytes", ctypes.c_size_t)]


class CombineDesc(ctypes.Structure):
    """skgram_combine_desc."""
    _fields_ = [("members", _P), ("M", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("nc", ctypes.c_int),
                ("channels", ctypes.c_int32 * MAX_CHANNELS), ("coef", _P), ("b", _P), ("K", ctypes.c_int), ("out", _P)]


SPEC = native.Spec("skyrim_gram", "SKYRIM_GRAM_LIB", "skgram", 1, {              # include/skyrim_gram.h SKGRAM_ABI_VERSION
    "skgram_abi_version": (ctypes.c_int, []),
    "skgram_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "skgram_run": (ctypes.c_int, [ctypes.POINTER(GramDesc), _P]),
    "skgram_combine": (ctypes.c_int, [ctypes.POINTER(CombineDesc), _P]),
}, " -- the member Gram matrix has no torch fallback")
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi

_lib = None


def load_library() -> ctypes.CDLL:
    """libskyrim_gram.so (built in-tree by ``__graft_entry__.build()`` / ``make -C skyrim_amd/csrc``)."""
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


def bound_factor() -> float:
    """The factor of the header's bound: |Gd - exact| <= bound_factor() * sum_j |w_j| sum_i |d_m| |d_n|."""
    return (CHAIN + 3) * 2.0 ** -24 + 2.0 ** -40


# ---- the binding ------------------------------------------------------------------------------------------------------------------------- #
def workspace_bytes(Mp: int, nc: int, nj: int, ni: int) -> int:
    """``skgram_workspace_bytes``: 0 for arguments ``skgram_run`` would refuse."""
    return int(load_library().skgram_workspace_bytes(int(Mp), int(nc), int(nj), int(ni)))


def describe(M, C, H, W, channels, region) -> GramDesc:
    """The descriptor of a ``skgram_run`` call without a truth, its pointers still NULL.  ``region``: (j0, nj, i0, ni)."""
    d = GramDesc()
    d.M, d.C, d.H, d.W, d.out_stride = M, C, H, W, M * M
    d.j0, d.nj, d.i0, d.ni = (int(v) for v in region)
    fill_channels(d, channels, MAX_CHANNELS)
    return d


def describe_combine(M, C, H, W, channels, K) -> CombineDesc:
    """The descriptor of a ``skgram_combine`` call, its pointers still NULL."""
    d = CombineDesc()
    d.M, d.C, d.H, d.W, d.K = M, C, H, W, K
    fill_channels(d, channels, MAX_CHANNELS)
    return d


def gram(members, table, truth, channels, region, lat_weight, out, workspace) -> None:
    """One ``skgram_run``: the matrices Gd of the channels ``channels`` of the M ``members`` (equal-shaped contiguous float32 (C, H, W)
    device tensors; ``table`` = ``ensemble.member_table(members)``) and, when ``truth`` (C, H, W) is given, of the truth as column M, over
    ``region`` = (j0, nj, i0, ni) with the H float64 weights ``lat_weight``, into ``out``, float64 (nc, M', M'), or (nc, stride) with stride >= M'^2 of which each channel's first M'^2 elements are written.  ``workspace``: a float64
    (or uint8) device tensor of at least ``workspace_bytes(M', nc, nj, ni)`` bytes.  Queued on torch's current stream."""
    import torch
    M, dev, _ = member_set(members, table, "gram", MAX_MEMBERS, lo=2)
    C, H, W = members[0].shape
    channels = [int(c) for c in channels]
    if not 1 <= len(channels) <= MAX_CHANNELS:
        raise ValueError(f"gram: {len(channels)} channels; 1 to {MAX_CHANNELS} are supported")
    Mp = M + (truth is not None)
    if Mp > MAX_MEMBERS:
        raise ValueError(f"gram: {M} members and a truth; the truth needs a column of the {MAX_MEMBERS}")
    d = describe(M, C, H, W, channels, region)
    if truth is not None:
        d.truth = native.tensor_ptr(truth, "gram: truth", torch.float32, dev)
        if truth.shape != members[0].shape:
            raise ValueError("gram: the truth differs from the members in shape")
    d.members, d.lat_weight = table.data_ptr(), native.tensor_ptr(lat_weight, "gram: lat_weight", torch.float64, dev)
    if lat_weight.numel() != H:
        raise ValueError(f"gram: {lat_weight.numel()} weights for {H} rows")
    d.out = native.tensor_ptr(out, "gram: out", torch.float64, dev)
    if out.dim() == 3 and tuple(out.shape) == (len(channels), Mp, Mp):
        d.out_stride = Mp * Mp
    elif out.dim() == 2 and out.shape[0] == len(channels) and out.shape[1] >= Mp * Mp:
        d.out_stride = int(out.shape[1])
    else:
        raise ValueError(f"gram: out must be ({len(channels)}, {Mp}, {Mp}) or ({len(channels)}, stride >= {Mp * Mp})")
    if not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError("gram: workspace must be a contiguous device tensor")
    d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    lib = load_library()
    with torch.cuda.device(dev):
        native.check(lib.skgram_run(ctypes.byref(d), native.stream(dev)), "skgram_run", lib)


def combine(members, table, channels, coef, b, out) -> None:
    """One ``skgram_combine``: ``out`` (K, nc, H, W) float32, out[k] = b[k] x_0 + sum_{m >= 1} coef[k, m] (x_m - x_0) in the header's
    fp32 operation order, for the channels ``channels``.  ``coef``: float32 (K, M), ``b``: float32 (K,), both on the device."""
    import torch
    M, dev, _ = member_set(members, table, "member_combine", MAX_MEMBERS, lo=2)
    C, H, W = members[0].shape
    channels = [int(c) for c in channels]
    if not 1 <= len(channels) <= MAX_CHANNELS:
        raise ValueError(f"member_combine: {len(channels)} channels; 1 to {MAX_CHANNELS} are supported")
    pc, pb, po = (native.tensor_ptr(t, f"member_combine: {w}", torch.float32, dev) for t, w in ((coef, "coef"), (b, "b"), (out, "out")))
    if coef.dim() != 2 or coef.shape[1] != M or not 1 <= coef.shape[0] <= MAX_OUT or tuple(b.shape) != (coef.shape[0],):
        raise ValueError(f"member_combine: coef is (K, {M}) with 1 <= K <= {MAX_OUT}, b is (K,)")
    K = int(coef.shape[0])
    if tuple(out.shape) != (K, len(channels), H, W):
        raise ValueError(f"member_combine: out must be ({K}, {len(channels)}, {H}, {W})")
    d = describe_combine(M, C, H, W, channels, K)
    d.members, d.coef, d.b, d.out = table.data_ptr(), pc, pb, po
    lib = load_library()
    with torch.cuda.device(dev):
        native.check(lib.skgram_combine(ctypes.byref(d), native.stream(dev)), "skgram_combine", lib)


# ---- the region -------------------------------------------------------------------------------------------------------------------------- #
def region_index(lat, lon, region) -> tuple:
    """(j0, nj, i0, ni) of ``region`` = (lat_s, lat_n, lon_w, lon_e) in degrees on the grid (lat, lon); None is the globe.  Rows: those with
    lat_s <= lat <= lat_n; columns: from lon_w eastward to lon_e, across the date line or Greenwich where the box does (lon_e - lon_w >= 360:
    every column; lon_e < lon_w: eastward around, so (300, 40) is (-60, 40)).  An empty box and bounds outside [-90, 90] are ValueError."""
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    if region is None:
        return 0, lat.size, 0, lon.size
    if not hasattr(region, "__len__") or len(region) != 4:
        raise ValueError("scenarios: region is (lat_s, lat_n, lon_w, lon_e) or None")
    lat_s, lat_n, lon_w, lon_e = (float(v) for v in region)
    if not all(np.isfinite([lat_s, lat_n, lon_w, lon_e])) or lat_s < -90 or lat_n > 90:
        raise ValueError(f"scenarios: region {tuple(region)} lies outside the grid: latitudes are in [-90, 90]")
    if lat_s > lat_n:
        raise ValueError(f"scenarios: region {tuple(region)} is empty: lat_s > lat_n")
    rows = np.nonzero((lat >= lat_s) & (lat <= lat_n))[0]
    if rows.size == 0:
        raise ValueError(f"scenarios: region {tuple(region)} holds no row of the grid (it lies outside the grid's latitudes or between two rows)")
    if lon_e - lon_w >= 360.0:
        return int(rows[0]), int(rows.size), 0, lon.size
    width = lon_e - lon_w if lon_e >= lon_w else np.mod(lon_e - lon_w, 360.0)      # (300, 40) is the same box as (-60, 40)
    east = np.mod(lon - lon_w, 360.0)                       # degrees east of the western edge
    inside = east <= width
    if not inside.any():
        raise ValueError(f"scenarios: region {tuple(region)} holds no column of the grid")
    return int(rows[0]), int(rows.size), int(np.argmin(np.where(inside, east, np.inf))), int(inside.sum())


# ---- the host algebra (float64) ---------------------------------------------------------------------------------------------------------- #
def centre(Gd, M: int) -> np.ndarray:
    """Double-centring about the mean of the M members: the (M', M') Gram matrix of a_m = d_m - mean_n d_n (m < M) and, with a truth column,
    a_y = d_y - mean_n d_n, from the Gram matrix ``Gd`` of the d.  G = J' Gd J with J = I - (1/M) [1_M; 0] 1': exact M x M algebra."""
    Gd = np.asarray(Gd, np.float64)
    Mp = Gd.shape[-1]
    J = np.eye(Mp)
    J[:M, :] -= 1.0 / M
    return J.T @ Gd @ J


def combine_channels(Gc, M: int, normalise: str = "spread", std=None) -> tuple:
    """(G, scale): the channels' centred matrices ``Gc`` (nc, M', M') added up as sum_c Gc[c] / scale[c].  ``"spread"``: scale = the
    channel's trace over the members / (M - 1), its mean member variance, so that channels weigh equally (a channel without spread: 1);
    ``"std"``: scale = std[c]^2; ``"none"``: 1."""
    Gc = np.asarray(Gc, np.float64)
    if normalise == "spread":
        scale = np.array([np.trace(g[:M, :M]) / (M - 1) for g in Gc])
        scale = np.where(scale > 0, scale, 1.0)
    elif normalise == "std":
        scale = np.asarray(std, np.float64) ** 2
        if scale.shape != (Gc.shape[0],) or not np.all(scale > 0):
            raise ValueError("scenarios: normalise='std' needs one positive sigma per channel")
    elif normalise == "none":
        scale = np.ones(Gc.shape[0])
    else:
        raise ValueError(f"scenarios: unknown normalise {normalise!r}; choose from {NORMALISE}")
    return np.einsum("cmn,c->mn", Gc, 1.0 / scale), scale


def distances(G) -> np.ndarray:
    """D2[m, n] = G[m, m] + G[n, n] - 2 G[m, n], clipped at 0, the diagonal exactly 0."""
    G = np.asarray(G, np.float64)
    g = np.diag(G)
    D2 = np.maximum(g[:, None] + g[None, :] - 2.0 * G, 0.0)
    np.fill_diagonal(D2, 0.0)
    return D2


def eofs(G, n: int) -> dict:
    """The leading ``n`` EOFs of the M x M centred Gram matrix ``G``: ``eigh`` of G / (M - 1).  ``variance_fraction`` (n,): eigenvalue over
    the sum of all (an eigenvalue below 1e-12 of the largest counts as 0); ``pcs`` (M, n): column k is v_k sqrt((M - 1) lambda_k), the
    members' coordinates along pattern k, its sign fixed so that its largest-magnitude entry (the first of equals) is positive; ``coef``
    (n, M): v_k / sqrt((M - 1) lambda_k), the weights of the members in pattern k (rows sum to 0; a zero eigenvalue: zeros), so that
    anomaly_m = sum_k pcs[m, k] pattern_k over all non-zero eigenvalues; ``eigenvalues`` (n,)."""
    G = np.asarray(G, np.float64)
    M = G.shape[0]
    lam, V = np.linalg.eigh((G + G.T) / (2.0 * (M - 1)))
    lam, V = lam[::-1], V[:, ::-1]
    lam = np.where(lam > 1e-12 * max(lam[0], 0.0), lam, 0.0)
    total = lam.sum()
    n = int(n)
    pcs, coef = np.zeros((M, n)), np.zeros((n, M))
    for k in range(n):
        v = V[:, k]
        if lam[k] <= 0:
            continue
        v = v if v[int(np.argmax(np.abs(v)))] > 0 else -v
        s = np.sqrt((M - 1) * lam[k])
        pcs[:, k], coef[k] = v * s, v / s
    return dict(variance_fraction=lam[:n] / total if total > 0 else np.zeros(n), pcs=pcs, coef=coef, eigenvalues=lam[:n].copy())


def ward(D2, n_clusters: int) -> np.ndarray:
    """Ward's agglomeration by the Lance-Williams update on the squared distances ``D2``, down to ``n_clusters`` clusters: deterministic,
    no random start.  Of equal merge costs the pair with the lowest (first, second) lowest-member indices is merged.  Returns the labels
    (M,), the clusters numbered by size descending, then by lowest member."""
    D = np.array(D2, np.float64)
    M = D.shape[0]
    if not 1 <= int(n_clusters) <= M:
        raise ValueError(f"scenarios: n_clusters = {n_clusters} is outside [1, {M}]")
    alive = list(range(M))                                   # a cluster is named by its lowest member
    size = np.ones(M)
    group = {m: [m] for m in range(M)}
    while len(alive) > n_clusters:
        best, bi, bj = np.inf, -1, -1
        for x, i in enumerate(alive):                        # ascending (i, j): the first minimum wins a tie
            for j in alive[x + 1:]:
                if D[i, j] < best:
                    best, bi, bj = D[i, j], i, j
        for k in alive:
            if k != bi and k != bj:
                t = size[bi] + size[bj] + size[k]
                D[bi, k] = D[k, bi] = ((size[bi] + size[k]) * D[bi, k] + (size[bj] + size[k]) * D[bj, k] - size[k] * D[bi, bj]) / t
        size[bi] += size[bj]
        group[bi] += group.pop(bj)
        alive.remove(bj)
    order = sorted(alive, key=lambda i: (-len(group[i]), i))
    labels = np.empty(M, np.int64)
    for c, i in enumerate(order):
        labels[group[i]] = c
    return labels


def summarise(G, labels) -> dict:
    """The clusters of ``labels`` measured in the centred M x M Gram matrix ``G``: ``sizes``, ``probability`` (size / M), ``within`` (the sum
    over the clusters of the members' squared distances to their centroid), ``total`` (trace G) and ``explained`` (total - within), and the
    ``representative`` of each cluster: the member closest to its centroid.  Of equals the lowest index: the two members of a pair are
    equally far from their centroid whatever G holds, so distances within 1e-12 of trace G of the smallest count as equal."""
    G, labels = np.asarray(G, np.float64), np.asarray(labels)
    M, n = G.shape[0], int(labels.max()) + 1
    sizes, reps, within = [], [], 0.0
    tie = 1e-12 * abs(float(np.trace(G)))
    for c in range(n):
        idx = np.nonzero(labels == c)[0]
        sub = G[np.ix_(idx, idx)]
        d2 = np.diag(sub) - 2.0 * sub.mean(axis=1) + sub.mean()          # |a_m - centroid|^2
        sizes.append(idx.size)
        reps.append(int(idx[int(np.nonzero(d2 <= d2.min() + tie)[0][0])]))
        within += float(np.maximum(d2, 0.0).sum())
    total = float(np.trace(G))
    return dict(labels=labels.astype(np.int64), sizes=np.asarray(sizes), probability=np.asarray(sizes) / float(M), within=within, total=total,
                explained=total - within, representative=np.asarray(reps))


def energy_score(Gf, M: int, labels=None) -> dict:
    """The fair energy score from the (M + 1, M + 1) centred Gram matrix with the truth as last column:
    mean_m |x_m - y| - sum_{m != n} |x_m - x_n| / (2 M (M - 1)), the norms from ``distances``; with ``labels`` also ``nearest_cluster``,
    the cluster whose centroid is nearest the truth (the lowest index of equals)."""
    Gf = np.asarray(Gf, np.float64)
    D = np.sqrt(distances(Gf))
    out = dict(energy_score=float(D[:M, M].mean() - D[:M, :M].sum() / (2.0 * M * (M - 1))))
    if labels is not None:
        labels = np.asarray(labels)
        d2 = []
        for c in range(int(labels.max()) + 1):
            idx = np.nonzero(labels == c)[0]
            d2.append(Gf[M, M] - 2.0 * Gf[M, idx].mean() + Gf[np.ix_(idx, idx)].mean())
        out["nearest_cluster"] = int(np.argmin(d2))
    return out


def analyse(Gd, M: int, area: float, n_clusters: int, n_eofs: int, normalise: str = "spread", std=None) -> dict:
    """Everything the host makes of one lead time's device result ``Gd`` (nc, M', M'): ``gram`` (nc, M', M'), centred and divided by
    ``area`` = sum_j w_j * ni so that entries are area means; ``combined`` (M', M') and ``scale`` from ``combine_channels``; the clusters
    (``summarise`` of ``ward``), the EOFs and, with a truth column, the energy score."""
    Gd = np.asarray(Gd, np.float64)
    Gc = np.stack([centre(g, M) for g in Gd]) / float(area)
    Gf, scale = combine_channels(Gc, M, normalise, std)
    G = Gf[:M, :M]
    clusters = summarise(G, ward(distances(G), n_clusters))
    out = dict(gram=Gc, combined=Gf, scale=scale, clusters=clusters, **eofs(G, n_eofs))
    if Gf.shape[0] > M:
        out.update(energy_score(Gf, M, clusters["labels"]))
    return out


# ---- the request ------------------------------------------------------------------------------------------------------------------------- #
def check_request(names, lat, lon, n_members: int, spec, scores: bool = False, other=()) -> dict:
    """Every refusal that needs no device; returns the request normalised: ``channels``, ``index``, ``region`` (j0, nj, i0, ni),
    ``n_clusters``, ``n_eofs``, ``normalise``.  ``other``: names of derived, regridded or aggregated channels of the same forecast, which
    this version refuses by name."""
    if not isinstance(spec, dict):
        raise ValueError("scenarios: a dict with channels, region, n_clusters, n_eofs, normalise")
    unknown = [k for k in spec if k not in ("channels", "region", "n_clusters", "n_eofs", "normalise")]
    if unknown:
        raise ValueError(f"scenarios: unknown keys {unknown}")
    names, M = list(names), int(n_members)
    channels = list(spec.get("channels") or [])
    if not 1 <= len(channels) <= MAX_CHANNELS:
        raise ValueError(f"scenarios: {len(channels)} channels; name 1 to {MAX_CHANNELS} (SKGRAM_MAX_CHANNELS)")
    for c in channels:
        if c in other and c not in names:
            raise ValueError(f"scenarios: {c!r} is a derived, regridded or aggregated channel; this version takes raw channels on the model's "
                             "own grid only")
        if c not in names:
            raise ValueError(f"scenarios: channel {c!r} is not an output channel of this model")
    if len(set(channels)) != len(channels):
        raise ValueError("scenarios: a channel is named twice")
    if M < 2:
        raise ValueError(f"scenarios: n_members = {M}; scenarios relate members to each other and need at least 2")
    if M > MAX_MEMBERS or (M == MAX_MEMBERS and scores):
        raise ValueError(f"scenarios: n_members = {M}" + (" with scores=True: the truth needs a column of its own" if M == MAX_MEMBERS else "")
                         + f"; at most {MAX_MEMBERS} columns (SKGRAM_MAX_MEMBERS)")
    n_clusters, n_eofs = int(spec.get("n_clusters", 3)), int(spec.get("n_eofs", 3))
    if not 1 <= n_clusters <= M:
        raise ValueError(f"scenarios: n_clusters = {n_clusters} is outside [1, {M}]")
    top = min(M - 1, MAX_OUT)
    if not 0 <= n_eofs <= top:
        raise ValueError(f"scenarios: n_eofs = {n_eofs} is outside [0, {top}] (min(M - 1, SKGRAM_MAX_OUT))")
    normalise = spec.get("normalise", "spread")
    if normalise not in NORMALISE:
        raise ValueError(f"scenarios: unknown normalise {normalise!r}; choose from {NORMALISE}")
    if len(names) * len(lat) * len(lon) > 2 ** 30:
        raise ValueError("scenarios: a state holds at most 2^30 elements")
    region = region_index(lat, lon, spec.get("region"))
    if region[1] * -(-region[3] // TILE) > 2 ** 21:
        raise ValueError("scenarios: the region holds more than 2^21 tiles of 256 points")
    return dict(channels=channels, index=[names.index(c) for c in channels], region=region, n_clusters=n_clusters, n_eofs=n_eofs,
                normalise=normalise)


def check_scored(channels, scored) -> None:
    """With ``scores=True`` the truth is one more column of the Gram matrix: every scenario channel must be among the channels the
    scorer holds a truth for."""
    unscored = [c for c in channels if c not in list(scored)]
    if unscored:
        raise ValueError(f"scenarios: the channels {unscored} are not among the scored channels (the truth must hold them for the energy score)")


# ---- the result -------------------------------------------------------------------------------------------------------------------------- #
@dataclass
class Scenarios:
    """What ``LeadScenarios.result`` returns.  ``gram`` (time, channel, member, member): the centred area-mean Gram matrices per channel,
    float64; ``combined`` (time, member, member): their channel combination, the matrix the clusters and EOFs are made from; ``scale``
    (time, channel); ``clusters_at``: per time the dict of ``summarise`` (labels, sizes, probability, within, total, explained,
    representative); ``cluster_mean``: DataArray(time, cluster, channel, lat, lon) float32; ``eof_pattern``: DataArray(time, eof,
    channel, lat, lon) float32 or None with n_eofs = 0; ``variance_fraction`` (time, eof); ``pcs`` (time, member, eof);
    ``energy_score`` (time,) and ``nearest_cluster`` (time,) with a truth, else None."""
    channels: list
    times: list
    region: tuple
    normalise: str
    n_members: int
    gram: np.ndarray
    combined: np.ndarray
    scale: np.ndarray
    clusters_at: list
    cluster_mean: object = None
    eof_pattern: object = None
    variance_fraction: np.ndarray = None
    pcs: np.ndarray = None
    energy_score: np.ndarray = None
    nearest_cluster: np.ndarray = None
    model_name: str = ""
    forecast_id: str = ""

    def clusters(self, n: int, times=None) -> dict:
        """Trajectory scenarios: the members re-clustered into ``n`` clusters on the SUM of the combined Gram matrices of the lead times
        ``times`` (indices or entries of ``self.times``; None: all).  Host only; ``summarise``'s dict."""
        pick = range(len(self.times)) if times is None else [t if isinstance(t, (int, np.integer)) else self.times.index(t) for t in times]
        pick = list(pick)
        if not pick:
            raise ValueError("scenarios: clusters() needs at least one lead time")
        G = np.sum([self.combined[t][:self.n_members, :self.n_members] for t in pick], axis=0)
        return summarise(G, ward(distances(G), n))


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------- #
class LeadScenarios:
    """The scenarios of one lead time after the other.  ``names``: the channels of the (C, H, W) states in their order; ``spec``: the dict of
    ``ensemble_forecast(scenarios=...)``.  ``add`` makes ONE ``gram`` call, copies its (nc, M', M') doubles to the host (20 KB per channel for 50
    members), clusters and decomposes them there, takes ``ensemble.stats`` means over the member sub-table of each cluster and makes the
    EOF patterns with one ``member_combine``.  ``truth=True``: ``add`` is given the truth state of the valid time as one more column."""

    def __init__(self, names, lat, lon, n_members, spec, device="cuda:0", truth: bool = False, std=None):
        self.req = check_request(names, lat, lon, n_members, spec, scores=truth)
        self.names, self.M, self.device, self.truth = list(names), int(n_members), device, bool(truth)
        self.lat, self.lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
        from .verify import area_weights
        self.weights = area_weights(self.lat)
        j0, nj, _, ni = self.req["region"]
        self.area = float(self.weights[j0:j0 + nj].sum() * ni)
        self.std = None
        if self.req["normalise"] == "std":
            if std is None:
                raise ValueError("scenarios: normalise='std' needs the model's channel_std")
            self.std = np.asarray(std, np.float64).reshape(-1)[self.req["index"]]
        self.times, self.parts, self.cmean, self.patterns = [], [], [], []
        self._dev = None

    def _buffers(self):
        if self._dev is None:
            import torch
            dev = torch.device(self.device)
            nc, Mp, H, W = len(self.req["index"]), self.M + self.truth, self.lat.size, self.lon.size
            j0, nj, i0, ni = self.req["region"]
            K = self.req["n_eofs"]
            self._dev = dict(w=torch.from_numpy(self.weights).to(dev), out=torch.empty((nc, Mp, Mp), dtype=torch.float64, device=dev),
                             ws=torch.empty(max(workspace_bytes(Mp, nc, nj, ni) // 8, 1), dtype=torch.float64, device=dev),
                             mean=torch.empty((self.req["n_clusters"], nc, H, W), dtype=torch.float32, device=dev),
                             pat=torch.empty((K, nc, H, W), dtype=torch.float32, device=dev) if K else None,
                             b=torch.zeros(K, dtype=torch.float32, device=dev) if K else None)
        return self._dev

    def add(self, time, states, table=None, truth=None) -> None:
        import torch
        from . import ensemble as E
        if len(states) != self.M:
            raise ValueError(f"{len(states)} states for scenarios of {self.M} members")
        if self.truth != (truth is not None):
            raise ValueError("scenarios: the truth state is given exactly when truth=True")
        b, r = self._buffers(), self.req
        table = E.member_table(states) if table is None else table
        gram(states, table, truth, r["index"], r["region"], b["w"], b["out"], b["ws"])
        a = analyse(b["out"].cpu().numpy(), self.M, self.area, r["n_clusters"], r["n_eofs"], r["normalise"], self.std)
        hw = self.lat.size * self.lon.size
        labels = a["clusters"]["labels"]
        for c in range(r["n_clusters"]):                      # the mean field of a cluster: ens_stats over its members' sub-table
            sub = [states[m] for m in np.nonzero(labels == c)[0]]
            tab = E.member_table(sub)
            for cc, ch in enumerate(r["index"]):
                E.stats(sub, tab, ch * hw, hw, mean=b["mean"][c, cc].reshape(-1))
        self.cmean.append(b["mean"].cpu().numpy())
        if r["n_eofs"]:
            coef = torch.from_numpy(a["coef"].astype(np.float32)).to(b["out"].device)
            combine(states, table, r["index"], coef, b["b"], b["pat"])
            self.patterns.append(b["pat"].cpu().numpy())
        self.times.append(time)
        self.parts.append(a)

    def result(self, model_name: str = "", forecast_id: str = "") -> Scenarios:
        from .labeled import DataArray
        r, M = self.req, self.M
        grid = dict(lat=self.lat, lon=self.lon)
        stack = lambda k: np.stack([p[k] for p in self.parts]) if self.parts else np.zeros((0,))      # noqa: E731
        s = Scenarios(list(r["channels"]), list(self.times), tuple(r["region"]), r["normalise"], M, stack("gram"), stack("combined"), stack("scale"),
                      [p["clusters"] for p in self.parts], model_name=model_name, forecast_id=forecast_id)
        if self.parts:
            s.cluster_mean = DataArray(np.stack(self.cmean), ["time", "cluster", "channel", "lat", "lon"],
                                       dict(time=self.times, cluster=np.arange(r["n_clusters"]), channel=list(r["channels"]), **grid))
            s.variance_fraction, s.pcs = stack("variance_fraction"), stack("pcs")
            if r["n_eofs"]:
                s.eof_pattern = DataArray(np.stack(self.patterns), ["time", "eof", "channel", "lat", "lon"],
                                          dict(time=self.times, eof=np.arange(r["n_eofs"]), channel=list(r["channels"]), **grid))
            if self.truth:
                s.energy_score, s.nearest_cluster = stack("energy_score"), stack("nearest_cluster")
        return s


def from_members(members, lat, lon, names=None, channels=None, region=None, n_clusters: int = 3, n_eofs: int = 3, normalise: str = "spread",
                 truth=None, times=None, std=None) -> Scenarios:
    """The scenarios of member tensors that are already on the device -- the public function for forecasts read back from disk.
    ``members``: M float32 device tensors, each (C, H, W) for one valid time or (T, C, H, W) for T of them; ``names``: their C channel
    names (default "0", "1", ...); ``channels``: the names the Gram matrix is made of (default: all); ``truth``: a tensor of a member's
    shape, for the energy score; ``times``: the T labels.  The other arguments are those of ``ensemble_forecast(scenarios=...)``."""
    import torch
    members = list(members)
    if not members or not all(isinstance(t, torch.Tensor) for t in members) or members[0].dim() not in (3, 4):
        raise ValueError("from_members: members are (C, H, W) or (T, C, H, W) tensors")
    single = members[0].dim() == 3
    if single:
        members = [t[None] for t in members]
        truth = None if truth is None else truth[None]
    T, C = members[0].shape[0], members[0].shape[1]
    names = [str(k) for k in range(C)] if names is None else list(names)
    if len(names) != C:
        raise ValueError(f"from_members: {len(names)} names for {C} channels")
    spec = dict(channels=list(channels) if channels is not None else names, region=region, n_clusters=n_clusters, n_eofs=n_eofs, normalise=normalise)
    ls = LeadScenarios(names, lat, lon, len(members), spec, device=members[0].device, truth=truth is not None, std=std)
    if not members[0].is_cuda:
        raise RuntimeError("from_members makes the Gram matrix with HIP kernels: the members must be on a GPU")
    times = list(range(T)) if times is None else list(times)
    for t in range(T):
        ls.add(times[t], [m[t].contiguous() for m in members], None, None if truth is None else truth[t].contiguous())
    return ls.result()
