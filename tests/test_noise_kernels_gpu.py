"""The spherical-perturbation kernels on the MI355X against tests/_noise_reference.py: ``noise_coeffs`` element by element (bound of
include/skyrim_noise.h, exact zeros, bits independent of batching), the two-GEMM synthesis against a float64 synthesis of the coefficients
read back from the device (bound u (k S + Q) of the header), ``noise_apply`` bit for bit, and the statistics of 512 fields per point."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import _noise_reference as NR
from skyrim_amd import noise as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _table(lmax: int):
    """(float32 table sigma_l 2^e as the device holds it, e) of the default spectrum; lmax 1 has degree 0 alone."""
    if lmax < 2:
        return np.zeros(1, np.float32), 0
    s = N.spectrum(lmax)
    e = N.scale_exponent(s)
    return (s * 2.0 ** e).astype(np.float32), e


def _coeffs(table, F, seed, member_first, n, f_first=0):
    from skyrim_amd import ops
    lmax = len(table)
    out = torch.full((n * lmax * lmax * 2 * F,), float("nan"), dtype=torch.float32, device=DEV)      # the kernel writes its zeros itself
    ops.hip.noise_coeffs(out, torch.from_numpy(table).to(DEV), F, f_first, seed, member_first)
    return out.cpu().numpy().reshape(n, lmax, lmax, 2, F)


# ---- sknoise_coeffs ----------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("F,lmax", [(1, 1), (1, 2), (3, 5), (7, 9), (70, 8), (5, 33), (138, 32)])
def test_coeffs_against_the_restatement(F, lmax):
    table, _ = _table(lmax)
    got = _coeffs(table, F, 9, 1, 2)
    worst = 0.0
    for j, member in enumerate((1, 2)):
        ref, bound = NR.coefficients(9, member, np.arange(F), lmax, table)
        dead = bound == 0
        assert np.all(got[j].view(np.uint32)[dead] == 0)                       # l = 0, m > l, Im a_l0: +0, bit for bit
        err = np.abs(got[j].astype(np.float64) - ref)
        assert np.all(err[~dead] <= bound[~dead])
        if (~dead).any():
            worst = max(worst, float((err[~dead] / bound[~dead]).max()))
            assert np.all(got[j][~dead] != 0)
    print(f"coeffs F={F} lmax={lmax}: max err / bound {worst:.3f}")


def test_coeff_bits_do_not_depend_on_batching():
    table, _ = _table(32)
    F = 7
    six = _coeffs(table, F, 4, 1, 6)
    parts = np.concatenate([_coeffs(table, F, 4, 1, 1), _coeffs(table, F, 4, 2, 2), _coeffs(table, F, 4, 4, 3)])
    assert np.array_equal(six.view(np.uint32), parts.view(np.uint32))
    fields = np.concatenate([_coeffs(table, 3, 4, 1, 6), _coeffs(table, 4, 4, 1, 6, f_first=3)], axis=-1)
    assert np.array_equal(six.view(np.uint32), fields.view(np.uint32))
    small = _coeffs(table[:9].copy(), F, 4, 1, 6)                               # a caller with a smaller lmax: the common coefficients
    assert np.array_equal(small.view(np.uint32), six[:, :9, :9].view(np.uint32))
    assert not np.array_equal(_coeffs(table, F, 5, 1, 1), six[:1]) and not np.array_equal(six[0], six[1])


# ---- synthesis ---------------------------------------------------------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=2)
def _legendre(lmax, n_full, n_lat):
    return NR.legendre(lmax, n_full, n_lat)


def _synthesis_case(n_lat, n_full, n_lon, lmax, F, seed=7, member=1):
    """Runs one member's synthesis; returns (device field, float64 field, bound) in the scaled units of the device, [F][lat][lon]."""
    table, _ = _table(lmax)
    synth = N.synthesis(DEV, n_lat, n_full, n_lon, lmax)
    nc, nt, ny = synth.sizes(F)
    coef = torch.empty(nc, dtype=torch.float32, device=DEV)
    t = torch.zeros(nt, dtype=torch.float32, device=DEV)
    y = torch.full((ny,), float("nan"), dtype=torch.float32, device=DEV)
    N.coeffs(coef, torch.from_numpy(table).to(DEV), F, 0, seed, member)
    synth.run(coef, t, y, F)
    a = coef.cpu().numpy().astype(np.float64).reshape(lmax, lmax, 2, F)         # what the device holds: the synthesis' input
    assert float(t.abs().max()) < 65504 / 4                                     # the longitude spectrum keeps its room in fp16 (header)
    ref, S, Q = NR.synthesize(a, _legendre(lmax, n_full, n_lat), n_lon)
    return y.cpu().numpy().reshape(F, n_lat, n_lon), ref, NR.U * (NR.k_bound(lmax) * S + Q), S, Q


def _hold(got, ref, bound, S, Q, lmax, n_full, what):
    err = np.abs(got.astype(np.float64) - ref)
    assert np.isfinite(got).all()
    print(f"{what}: max err / bound {np.max(err / bound):.4f}; against k u S alone {np.max(err / (NR.U * NR.k_bound(lmax) * S)):.4f}; "
          f"max Q / (k S) {np.max(Q / (NR.k_bound(lmax) * S)):.2e}; field rms {ref.std():.3g}, max err {err.max():.3g}")
    assert np.all(err <= bound)
    rows = [0] + ([got.shape[1] - 1] if got.shape[1] == n_full else [])         # the pole rows hold m = 0 alone: constant along longitude
    for r in rows:
        assert np.all(np.abs(got[:, r, :].astype(np.float64) - got[:, r, :1]) <= bound[:, r, :] + bound[:, r, :1])


@pytest.mark.parametrize("F", [1, 3, 70])
@pytest.mark.parametrize("n_lat,n_full,n_lon,lmax", [(33, 33, 64, 32), (49, 49, 192, 49), (49, 49, 192, 7), (32, 33, 64, 32)])
def test_synthesis_against_float64(n_lat, n_full, n_lon, lmax, F):
    got, ref, bound, S, Q = _synthesis_case(n_lat, n_full, n_lon, lmax, F)
    _hold(got, ref, bound, S, Q, lmax, n_full, f"synthesis {n_lat}({n_full}) x {n_lon} lmax {lmax} F {F}")
    if n_lat < n_full:                                                          # the crop is the first rows of the full grid's field
        full = _synthesis_case(n_full, n_full, n_lon, lmax, F)
        assert np.all(np.abs(got.astype(np.float64) - full[0][:, :n_lat]) <= bound + full[2][:, :n_lat])


def test_synthesis_full_size():
    """721 x 1440, lmax 256, three fields of one member: every element to the same bound."""
    got, ref, bound, S, Q = _synthesis_case(721, 721, 1440, 256, 3)
    _hold(got, ref, bound, S, Q, 256, 721, "synthesis 721 x 1440 lmax 256 F 3")
    _, e = _table(256)
    v = (ref * 2.0 ** -e) ** 2
    assert abs(v.mean() - 1) < 0.5                                              # (unit variance: three fields, a sanity check only)
    N.release()


# ---- sknoise_apply ------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("L,C,hw", NR.APPLY_SHAPES)
def test_apply_is_one_fma(L, C, hw, offset):
    from skyrim_amd import ops
    x0, y, g = NR.apply_inputs(L, C, hw)
    n = x0.size
    gg = np.repeat(np.tile(g, L), hw)
    assert NR.fma32_is_exact(gg, y, x0)
    dev = lambda a: torch.cat([torch.zeros(offset, dtype=torch.float32), torch.from_numpy(a)]).to(DEV)[offset:]      # noqa: E731
    dx, dy = dev(x0), dev(y)
    out = torch.full((offset + n + 4,), float("nan"), dtype=torch.float32, device=DEV)
    ops.hip.noise_apply(dx, dy, torch.from_numpy(g).to(DEV), out[offset:offset + n], hw)
    got = out.cpu().numpy()
    want = NR.fma32(gg, y, x0)
    assert np.array_equal(got[offset:offset + n].view(np.uint32), want.view(np.uint32))
    assert np.isnan(got[:offset]).all() and np.isnan(got[offset + n:]).all()    # nothing outside the range is written
    off = gg == 0
    assert np.array_equal(got[offset:offset + n][off].view(np.uint32), x0[off].view(np.uint32))      # g = 0: a bit copy
    assert C == 1 or off.any()


# ---- statistics --------------------------------------------------------------------------------------------------------------------------- #
def test_field_statistics():
    """64 members x 8 fields at 33 x 64 (seed fixed: deterministic): the bars of ``_noise_reference.statistics_check``, which the float64
    restatement with the same seed passes on the CPU (tests/test_noise_cpu.py; seed 2024 was the first one tried)."""
    s = NR.STAT
    table, e = _table(s["lmax"])
    synth = N.synthesis(DEV, s["n_lat"], s["n_lat"], s["n_lon"], s["lmax"])
    nc, nt, ny = synth.sizes(s["F"])
    coef = torch.empty(s["members"] * nc, dtype=torch.float32, device=DEV)
    N.coeffs(coef, torch.from_numpy(table).to(DEV), s["F"], 0, s["seed"], 1)
    t = torch.empty(nt, dtype=torch.float32, device=DEV)
    y = torch.empty((s["members"], ny), dtype=torch.float32, device=DEV)
    for m in range(s["members"]):
        synth.run(coef[m * nc:(m + 1) * nc], t, y[m], s["F"])
    fields = y.cpu().numpy().astype(np.float64).reshape(-1, s["n_lat"], s["n_lon"]) * 2.0 ** -e
    worst = NR.statistics_check(fields)
    print("device: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    ref = NR.statistics_fields_float64()
    assert np.abs(fields - ref).max() < 1e-3                                    # the same fields as the restatement (sigma units)
