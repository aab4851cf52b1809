"""NumPy restatement of include/skyrim_spec.h, written from the header's text: float64 ``np.fft.rfft`` of the same fp32 differences the
kernel forms, all six slots straight from their definitions (member powers, NOT the kernel's origin trick), and the header's bound
evaluated with the exact coefficients.  Also the inputs the GPU tests share."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
KINDS = ("member", "mean", "spread", "truth", "error_mean", "error_member")
RHO = {2: 1.0, 4: 2.0, 3: 5.25, 5: 7.25}


def factor(W: int) -> list:
    """The radices in the kernel's order: 4s, a 2, 3s, 5s."""
    out = []
    while W % 4 == 0:
        out.append(4)
        W //= 4
    if W % 2 == 0:
        out.append(2)
        W //= 2
    for r in (3, 5):
        while W % r == 0:
            out.append(r)
            W //= r
    assert W == 1
    return out


def c_w(W: int) -> float:
    return 1.02 * sum(3.25 + np.sqrt(r) * RHO[r] for r in factor(W))


def c_k(W: int) -> np.ndarray:
    c = np.full(W // 2 + 1, 2.0)
    c[0] = 1.0
    if W % 2 == 0:
        c[-1] = 1.0
    return c


def coeffs(rows) -> np.ndarray:
    """F_k = (1/W) sum_n d_n e^(-2 pi i k n / W) of float64 rows (..., W) -> (..., K)."""
    rows = np.asarray(rows, np.float64)
    return np.fft.rfft(rows, axis=-1) / rows.shape[-1]


def rms(rows) -> np.ndarray:
    return np.sqrt((np.asarray(rows, np.float64) ** 2).mean(axis=-1))


def differences(members, truth, ch: int):
    """The kernel's fp32 differences of channel ``ch``: first (H, 1), f0 (H, W), d (M, H, W) with d[0] = 0, dy (H, W) or None."""
    x0 = np.asarray(members[0], np.float32)[ch]
    first = x0[:, :1].copy()
    f0 = x0 - first
    d = np.stack([np.asarray(m, np.float32)[ch] - x0 for m in members])
    dy = None if truth is None else np.asarray(truth, np.float32)[ch] - x0
    assert f0.dtype == d.dtype == np.float32
    return first.astype(np.float64), f0, d, dy


def row_spectra(members, truth, ch: int):
    """Per row: (value, bound), each (slots, H, K), before the band mean.  ``value`` holds c_k |G|^2 from the definitions; ``bound`` the
    header's c_k (2 |G| eps_G + eps_G^2) + 2^-40 c_k A."""
    first, f0, d, dy = differences(members, truth, ch)
    M, H, W = d.shape
    ck = c_k(W)
    cw = c_w(W) * U
    x = first[None] + f0.astype(np.float64)[None] + d.astype(np.float64)           # the members, exactly as the differences define them
    Fx = coeffs(x)                                                                 # (M, H, K)
    xbar = x.mean(axis=0)
    Fbar = coeffs(xbar)
    Fa = coeffs(x - xbar[None])
    P = lambda F: np.abs(F) ** 2                                                   # noqa: E731
    vals = [P(Fx).mean(axis=0), P(Fbar), P(Fa).sum(axis=0) / (M - 1) if M > 1 else np.zeros_like(P(Fbar))]
    # the transforms' eps: f0 and dy alone; d_1, d_2 | d_3, d_4 | ... in pairs that share sqrt(rms_a^2 + rms_b^2); d_0 is not transformed
    e0 = cw * rms(f0)[:, None]                                                     # (H, 1)
    r = rms(d)                                                                     # (M, H)
    em = np.zeros((M, H))
    for m in range(1, M, 2):
        pair = np.sqrt(r[m] ** 2 + (r[m + 1] ** 2 if m + 1 < M else 0.0))
        em[m] = cw * pair
        if m + 1 < M:
            em[m + 1] = cw * pair
    em = em[:, :, None]                                                            # (M, H, 1)
    esum = em.sum(axis=0) / M
    quad = lambda G, e: 2.0 * np.abs(G) * e + e ** 2                               # noqa: E731
    F0 = coeffs(first + f0.astype(np.float64))
    D = coeffs(d.astype(np.float64))
    aF0, aD = np.abs(F0), np.abs(D)
    lims = [quad(Fx, e0[None] + em).mean(axis=0), quad(Fbar, e0 + esum),
            quad(Fa, em + esum[None]).sum(axis=0) / (M - 1) if M > 1 else np.zeros_like(aF0)]
    A = [((aF0[None] + aD) ** 2).mean(axis=0), (aF0 + aD.sum(axis=0) / M) ** 2, 2.0 * (aD ** 2).sum(axis=0) / (M - 1) if M > 1 else np.zeros_like(aF0)]
    if dy is not None:
        y = first + f0.astype(np.float64) + dy.astype(np.float64)
        Fy = coeffs(y)
        ey = cw * rms(dy)[:, None]
        aDy = np.abs(coeffs(dy.astype(np.float64)))
        vals += [P(Fy), P(coeffs(xbar - y)), P(coeffs(x - y[None])).mean(axis=0)]
        lims += [quad(Fy, e0 + ey), quad(coeffs(xbar - y), esum + ey), quad(coeffs(x - y[None]), em + ey[None]).mean(axis=0)]
        A += [(aF0 + aDy) ** 2, (aD.sum(axis=0) / M + aDy) ** 2, ((aD + aDy[None]) ** 2).mean(axis=0)]
    value = np.stack(vals) * ck
    bound = (np.stack(lims) + 2.0 ** -40 * np.stack(A)) * ck
    return value, bound


def spectra(members, truth, channels, bands, w):
    """(out, bound), each (nc, nb, slots, K): the band values sum_j w_j P_jk / sum_j w_j and the bound carried through with |w_j|."""
    w = np.asarray(w, np.float64)
    outs, lims = [], []
    cache = {}
    for ch in channels:
        if ch not in cache:
            cache[ch] = row_spectra(members, truth, ch)
        value, bound = cache[ch]
        ob, lb = [], []
        for j0, j1 in bands:
            ws = w[j0:j1]
            ob.append(np.einsum("j,sjk->sk", ws, value[:, j0:j1]) / ws.sum())
            lb.append(np.einsum("j,sjk->sk", np.abs(ws), bound[:, j0:j1]) / abs(ws.sum()))
        outs.append(np.stack(ob))
        lims.append(np.stack(lb))
    return np.stack(outs), np.stack(lims)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------ #
def red_rows(rng, shape, W: int, amplitude: float = 1.0, phase_span: float = np.pi) -> np.ndarray:
    """Rows sum_k k^-3 cos(k lambda + phi_k), k = 1 .. W // 2, phases uniform in [-phase_span, phase_span]: float64 (*shape, W)."""
    k = np.arange(1, W // 2 + 1)
    lam = 2.0 * np.pi * np.arange(W) / W
    phi = rng.uniform(-phase_span, phase_span, size=tuple(shape) + (k.size,))
    return amplitude * np.einsum("k,...kn->...n", k ** -3.0, np.cos(k[:, None] * lam[None, :] + phi[..., None]))


def case(W: int, H: int, M: int, truth: bool, C: int = 3, seed: int = 0, white: bool = False):
    """(members, truth): float32 (C, H, W) states.  k^-3 rows of amplitude 1e3 on a 5.5e4 offset; the members differ from member 0 by red
    (``white``: white) fields of relative size 1e-3, the truth by one of 2e-3."""
    rng = np.random.default_rng(1000 * W + 10 * M + seed)
    base = 5.5e4 + red_rows(rng, (C, H), W, 1e3)
    pert = (lambda: rng.standard_normal((C, H, W))) if white else (lambda: red_rows(rng, (C, H), W))
    members = [(base + (1.0 * pert() if m else 0.0)).astype(np.float32) for m in range(M)]
    y = (base + 2.0 * pert()).astype(np.float32) if truth else None
    return members, y
