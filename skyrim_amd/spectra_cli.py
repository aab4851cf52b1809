"""``spectra`` command line: the options of ``forecast`` (skyrim_amd/forecast.py: same names, short flags and defaults) plus the channels
whose zonal power spectra are made (``--channel z500``, repeatable), the latitude bands (``--band NAME=LAT_S,LAT_N``, repeatable;
``NAME=globe`` is every row; default: nh_mid, tropics, sh_mid, globe) and, with ``--members`` above 1, the size of a perturbed ensemble.
At every lead time the spectra are made where the states lie on the device (``Skyrim.spectrum_forecast`` or
``Skyrim.ensemble_forecast(spectra=...)``); per lead time, channel and band the power in a few wavenumber ranges is printed, ``--truth``
adds the effective resolution against the model's own kind of data source, ``--output`` writes everything as ``.json``."""
from __future__ import annotations

from pathlib import Path

import click
import numpy as np

from .common import AVAILABLE_MODELS
from .forecast import start_time_of, steps_for, yesterday


def parse_band(text: str):
    """(name, (lat_s, lat_n) or None) from ``NAME=LAT_S,LAT_N`` or ``NAME=globe``."""
    name, sep, rest = text.partition("=")
    if not sep or not name:
        raise ValueError(f"--band {text!r} is not NAME=LAT_S,LAT_N or NAME=globe (for example nh_mid=30,60)")
    if rest == "globe":
        return name, None
    parts = rest.split(",")
    try:
        if len(parts) != 2:
            raise ValueError
        return name, tuple(float(p) for p in parts)
    except ValueError:
        raise ValueError(f"--band {text!r} is not NAME=LAT_S,LAT_N or NAME=globe (for example nh_mid=30,60)") from None


def request(channels, bands, members, output, n_steps=None) -> dict:
    """The ``spectra=`` dict of the options; every refusal is a ValueError before a model is built."""
    from .spectra import MAX_BANDS, MAX_CHANNELS, MAX_MEMBERS
    if not channels:
        raise ValueError("name the channels whose spectra are made with --channel (repeatable), for example --channel z500")
    if len(channels) > MAX_CHANNELS:
        raise ValueError(f"{len(channels)} channels: at most {MAX_CHANNELS}")
    if not 1 <= members <= MAX_MEMBERS:
        raise ValueError(f"--members {members}: 1 to {MAX_MEMBERS} members")
    if output and Path(output).suffix.lower() != ".json":
        raise ValueError(f"--output {output!r}: a .json path")
    if n_steps is not None and n_steps < 0:
        raise ValueError("--n_steps >= 0")
    spec = dict(channels=list(channels))
    if bands:
        parsed = [parse_band(b) for b in bands]
        if len({n for n, _ in parsed}) != len(parsed):
            raise ValueError("--band: a band is named twice")
        if len(parsed) > MAX_BANDS:
            raise ValueError(f"{len(parsed)} bands: at most {MAX_BANDS}")
        spec["bands"] = dict(parsed)
    return spec


def run_spectra(model_name: str, date: str, time: str, lead_time: int, list_models: bool, initial_conditions: str, spec: dict, n_steps=None,
                members: int = 1, perturb_scale: float = 1e-3, seed: int = 0, perturbation: str = "white", truth: bool = False):
    """Returns the ``spectra.Spectra``; None with ``list_models``."""
    from .core import Skyrim
    if list_models:
        print("Available models:", Skyrim.list_available_models())
        return None
    model = Skyrim(model_name, ic_source=initial_conditions)
    start_time = start_time_of(date, time)
    if n_steps is None:
        n_steps = steps_for(model, lead_time)
    if members == 1:
        from .verify import default_truth
        return model.spectrum_forecast(start_time, n_steps=n_steps, spectra=spec, truth=default_truth(model.model) if truth else None)
    ens = model.ensemble_forecast(start_time, n_steps=n_steps, n_members=members, perturb_scale=perturb_scale, seed=seed, products=(),
                                  perturbation=perturbation, spectra=spec, scores=truth)
    return ens.spectra


def ranges(K: int) -> list:
    """Wavenumber ranges [k0, k1) the lines sum over: 1-3, 4-9, 10-29, 30-99, 100 and up, as far as the grid has them."""
    edges = [1, 4, 10, 30, 100, K]
    return [(a, min(b, K)) for a, b in zip(edges[:-1], edges[1:]) if a < K]


def lines(sp) -> list[str]:
    """One line per lead time, channel, band and kind: the power summed over the wavenumber ranges; with a truth one more with the
    effective resolution."""
    res = []
    K = sp.power.values.shape[-1]
    rg = ranges(K)
    head = " ".join(f"k{a}-{b - 1}" for a, b in rg)
    for ti, t in enumerate(sp.times):
        stamp = t.isoformat() if hasattr(t, "isoformat") else str(t)
        for ci, ch in enumerate(sp.channels):
            for bi, band in enumerate(sp.bands):
                for ki, kind in enumerate(sp.kinds):
                    if kind == "spread" and sp.n_members == 1:
                        continue
                    p = sp.power.values[ti, ci, bi, ki]
                    res.append(f"{stamp} {ch} {band} {kind} [{head}]: " + " ".join(f"{p[a:b].sum():.4g}" for a, b in rg))
                if "truth" in sp.kinds:
                    res.append(f"{stamp} {ch} {band} effective resolution: {sp.effective_resolution(ch, band)[ti]:.0f} km")
    return res


@click.command(name="spectra")
@click.option("--model_name", "-m", type=click.Choice(AVAILABLE_MODELS, case_sensitive=False), default="pangu", help="Select model")
@click.option("--date", "-d", type=str, default=yesterday, help="YYYYMMDD")
@click.option("--time", "-t", type=str, default="0000", help="HHMM")
@click.option("--lead_time", "-l", type=int, default=24, help="Lead time in hours, rounded up to whole 6-h steps (--n_steps overrides it)")
@click.option("--list_models", "-lm", is_flag=True, help="List all available models and exit")
@click.option("--initial_conditions", "-ic", type=click.Choice(["cds", "ifs", "gfs"], case_sensitive=False), default="gfs",
              help="Initial conditions provider.")
@click.option("--modal", "-mo", is_flag=True, help="(reference only) run on Modal -- not available in this build")
@click.option("--channel", "-c", "channels", type=str, multiple=True, help="Raw channel whose spectra are made, repeatable")
@click.option("--band", "-b", "bands", type=str, multiple=True, help="NAME=LAT_S,LAT_N or NAME=globe, repeatable (default: nh_mid, tropics, sh_mid, globe)")
@click.option("--n_steps", type=int, default=None, help="Model steps (default: from --lead_time)")
@click.option("--members", "-n", type=int, default=1, help="1: the deterministic forecast; 2-64: a perturbed-IC ensemble")
@click.option("--perturb_scale", type=float, default=1e-3, help="Perturbation amplitude in units of each channel's sigma")
@click.option("--perturbation", type=click.Choice(["white", "spherical"]), default="white", help="Kind of the initial perturbations")
@click.option("--seed", type=int, default=0, help="Seed of the perturbations (32-bit)")
@click.option("--truth", is_flag=True, help="Also the spectra of the truth (the model's own kind of data source) and of the errors")
@click.option("--output", "-o", type=str, default="", help="Write the spectra to this .json path")
def spectra(model_name, date, time, lead_time, list_models, initial_conditions, modal, channels, bands, n_steps, members, perturb_scale,
            perturbation, seed, truth, output):
    if modal:
        raise click.UsageError("--modal runs the reference on a hosted A100 service; this build runs on the local MI355X")
    spec = None
    if not list_models:
        try:
            spec = request(channels, bands, members, output, n_steps)
        except ValueError as e:
            raise click.UsageError(str(e)) from None
    sp = run_spectra(model_name, date, time, lead_time, list_models, initial_conditions, spec, n_steps, members, perturb_scale, seed,
                     perturbation, truth)
    if sp is None:
        return None
    for ln in lines(sp):
        click.echo(ln)
    if output:
        click.echo(sp.save(output))
    return sp


if __name__ == "__main__":
    spectra()
