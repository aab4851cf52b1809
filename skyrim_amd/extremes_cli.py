"""``extremes`` command line, two subcommands.

``extremes build FILES... --field t2m --out DIR``: saved forecasts or analyses (netCDF files or zarr stores) to a quantile climate, one
file per calendar slice under ``DIR`` (``climate.build_from_files``: ``--derived``, ``--half_window_days``, ``--hour`` repeatable,
``--levels N`` evenly spaced levels).

``extremes apply --climate DIR``: a forecast to its Extreme Forecast Index, Shift of Tails and tail odds against that climate -- a
forecast on disk (``FILES...``: ``extremes.extremes_prediction``) or a live one with the options of ``forecast`` (skyrim_amd/forecast.py:
same names, short flags and defaults; ``--members 1``, the default, is the deterministic forecast, more is
``Skyrim.ensemble_forecast(extremes=...)``).  ``--output DIR`` writes one netCDF file per array."""
from __future__ import annotations

import click
import numpy as np

from .common import AVAILABLE_MODELS
from .forecast import start_time_of, steps_for, yesterday


def request(climate, fields, efi, sot, above, below, floor) -> dict:
    """The ``extremes=`` dict of the options; ``floor``: ``FIELD=VALUE`` texts.  Every refusal is a ValueError before a model is built."""
    fl = {}
    for text in floor:
        name, sep, val = text.partition("=")
        try:
            fl[name.strip()] = float(val)
        except ValueError:
            sep = ""
        if not sep or not name.strip():
            raise ValueError(f"--floor {text!r} is not FIELD=VALUE (for example mucape=0)")
    if not climate:
        raise ValueError("--climate DIR: the directory `extremes build` wrote")
    return dict(climate=climate, fields=list(fields) or None, efi=bool(efi), sot=list(sot), above=list(above), below=list(below), floor=fl)


def lines(ex) -> list[str]:
    """One line per array, lead time and field: the extremes of the plane."""
    res = []
    for stem, da in ex.arrays().items():
        v = np.asarray(da.values)
        for ti, t in enumerate(np.asarray(da._coords["time"]).astype("datetime64[s]")):
            for fi, f in enumerate(ex.fields):
                with np.errstate(all="ignore"):
                    res.append(f"{t} {stem} {f}: min={np.nanmin(v[ti, fi]):.6g} max={np.nanmax(v[ti, fi]):.6g}")
    return res


@click.group(name="extremes")
def extremes():
    """Quantile climates and climate-relative extremes: build, apply."""


@extremes.command(name="build")
@click.argument("files", nargs=-1, required=True)
@click.option("--field", "-f", "fields", type=str, multiple=True, required=True, help="Field of the climate, repeatable: a channel of the files or a derived field")
@click.option("--derived", type=str, multiple=True, help="Derived field to make from the files, repeatable")
@click.option("--half_window_days", type=int, default=15, help="Valid times within this many days of a slice's day go into it")
@click.option("--hour", "hours", type=int, multiple=True, help="Hour of day to make slices for, repeatable (default: one slice per day)")
@click.option("--levels", type=int, default=101, help="Number of evenly spaced probability levels from 0 to 1")
@click.option("--out", "-o", type=str, required=True, help="Directory of the climate")
@click.option("--device", type=str, default="cuda:0")
def build(files, fields, derived, half_window_days, hours, levels, out, device):
    from . import climate
    try:
        c = climate.build_from_files(list(files), list(fields), derived=list(derived) or None, half_window_days=half_window_days,
                                     hours=list(hours) or None, levels=np.linspace(0.0, 1.0, levels), device=device)
    except (ValueError, OSError) as e:
        raise click.UsageError(str(e)) from None
    for p in c.save(out):
        click.echo(p)
    return c


@extremes.command(name="apply")
@click.argument("files", nargs=-1)
@click.option("--climate", "climate_dir", type=str, default="", help="Directory written by `extremes build`")
@click.option("--field", "-f", "fields", type=str, multiple=True, help="Field, repeatable (default: every field of the climate)")
@click.option("--derived", type=str, multiple=True, help="Derived field to make, repeatable")
@click.option("--no_efi", is_flag=True, help="Leave the Extreme Forecast Index out")
@click.option("--sot", type=float, multiple=True, help="Shift-of-Tails tail, repeatable (0.9 reads the climate's 0.9 and 0.99); members > 1")
@click.option("--above", type=float, multiple=True, help="Climate level: fraction of members above it, repeatable")
@click.option("--below", type=float, multiple=True, help="Climate level: fraction of members below it, repeatable")
@click.option("--floor", type=str, multiple=True, help="FIELD=VALUE: leave the climate at or below VALUE out of the index, repeatable")
@click.option("--model_name", "-m", type=click.Choice(AVAILABLE_MODELS, case_sensitive=False), default="pangu", help="Select model")
@click.option("--date", "-d", type=str, default=yesterday, help="YYYYMMDD")
@click.option("--time", "-t", type=str, default="0000", help="HHMM")
@click.option("--lead_time", "-l", type=int, default=24, help="Lead time in hours, rounded up to whole 6-h steps (--n_steps overrides it)")
@click.option("--initial_conditions", "-ic", type=click.Choice(["cds", "ifs", "gfs"], case_sensitive=False), default="gfs",
              help="Initial conditions provider.")
@click.option("--n_steps", type=int, default=None, help="Model steps (default: from --lead_time)")
@click.option("--members", "-n", type=int, default=1, help="Ensemble members, 1-64; 1 = the deterministic forecast")
@click.option("--perturb_scale", type=float, default=1e-3, help="Perturbation amplitude in units of each channel's sigma (members > 1)")
@click.option("--seed", type=int, default=0, help="Seed of the perturbations (32-bit)")
@click.option("--output", "-o", type=str, default="", help="Directory for one netCDF file per array")
@click.option("--device", type=str, default="cuda:0")
def apply(files, climate_dir, fields, derived, no_efi, sot, above, below, floor, model_name, date, time, lead_time, initial_conditions, n_steps,
          members, perturb_scale, seed, output, device):
    from . import extremes as extreming
    try:
        req = request(climate_dir, fields, not no_efi, sot, above, below, floor)
        if files:
            ex = extreming.extremes_prediction(list(files), req, derived=list(derived) or None, device=device)
        else:
            from . import core
            model = core.Skyrim(model_name, ic_source=initial_conditions)
            start = start_time_of(date, time)
            n = steps_for(model, lead_time) if n_steps is None else n_steps
            if members == 1:
                ex = model.extremes_forecast(start, n_steps=n, extremes=req, derived=list(derived) or None)
            else:
                ex = model.ensemble_forecast(start, n_steps=n, n_members=members, perturb_scale=perturb_scale, seed=seed, products=(),
                                             derived=list(derived) or None, extremes=req).extremes
    except (ValueError, OSError) as e:
        raise click.UsageError(str(e)) from None
    for ln in lines(ex):
        click.echo(ln)
    if output:
        for p in ex.to_netcdf(output):
            click.echo(p)
    return ex


if __name__ == "__main__":
    extremes()
