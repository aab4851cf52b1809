"""``point`` command line: the options of ``forecast`` (skyrim_amd/forecast.py: same names, short flags and defaults) plus the places to
sample (``--point NAME:LAT,LON``, repeatable, or ``--stations FILE.csv`` with the columns ``name,lat,lon``), the channels
(``--channel t2m``, repeatable), the interpolation (``--method bilinear``) and the size of the ensemble (``--members 1``, the default, is the
deterministic forecast).  Every lead time is sampled where the forecast lies on the device (``Skyrim.point_forecast`` /
``Skyrim.ensemble_forecast(points=...)``); ``--output`` writes the values as ``.json`` or long-form ``.csv``; with ``--observations`` (a
long-form CSV ``time,channel,point,value``) the station scores are printed."""
from __future__ import annotations

from pathlib import Path

import click
import numpy as np

from .common import AVAILABLE_MODELS
from .forecast import start_time_of, steps_for, yesterday


def parse_point(text: str) -> tuple:
    """(name, lat, lon) from ``NAME:LAT,LON``."""
    name, sep, rest = text.rpartition(":")
    parts = rest.split(",")
    if not sep or not name.strip() or len(parts) != 2:
        raise ValueError(f"--point {text!r} is not NAME:LAT,LON (for example Istanbul:41.01,28.98)")
    try:
        return name.strip(), float(parts[0]), float(parts[1])
    except ValueError:
        raise ValueError(f"--point {text!r}: LAT and LON are numbers") from None


def request(point, stations, output, n_steps=None):
    """The ``Points`` of the options and the checked output path; every refusal is a ValueError before a model is built."""
    from .points import Points
    if bool(point) == bool(stations):
        raise ValueError("name the places with --point NAME:LAT,LON (repeatable) or with --stations FILE.csv, not both and not neither")
    if output and Path(output).suffix.lower() not in (".json", ".csv"):
        raise ValueError(f"--output {output!r}: a .json or a .csv path")
    if n_steps is not None and n_steps < 0:
        raise ValueError("--n_steps >= 0")
    return Points(stations) if stations else Points([parse_point(p) for p in point])


def run_point(model_name: str, date: str, time: str, lead_time: int, list_models: bool, initial_conditions: str, points, channels=(),
              method: str = "bilinear", n_steps=None, members: int = 1, perturb_scale: float = 1e-3, seed: int = 0):
    """Returns the ``PointForecast`` (one member, or ``members`` of an ensemble); None with ``list_models``."""
    from .core import Skyrim
    if list_models:
        print("Available models:", Skyrim.list_available_models())
        return None
    model = Skyrim(model_name, ic_source=initial_conditions)
    start_time = start_time_of(date, time)
    if n_steps is None:
        n_steps = steps_for(model, lead_time)
    channels = list(channels) or None
    if members == 1:
        return model.point_forecast(start_time, n_steps=n_steps, points=points, channels=channels, method=method)
    ens = model.ensemble_forecast(start_time, n_steps=n_steps, n_members=members, perturb_scale=perturb_scale, seed=seed, products=(),
                                  points=points, point_channels=channels, point_method=method)
    return ens.points


def lines(pf) -> list[str]:
    """One line per lead time, channel and place: the ensemble mean and, with members, the spread."""
    mean, spread = pf.mean().values, pf.spread().values
    res = []
    for ti, t in enumerate(pf.times):
        for ci, ch in enumerate(pf.channels):
            for pi, name in enumerate(pf.names):
                tail = f" spread={spread[ti, ci, pi]:.6g}" if pf.n_members > 1 else ""
                res.append(f"{t.isoformat()} {ch} {name}: {mean[ti, ci, pi]:.6g}{tail}")
    return res


def score_lines(scores: dict) -> list[str]:
    res = []
    for ti, t in enumerate(scores["times"]):
        for ci, ch in enumerate(scores["channels"]):
            res.append(f"score {t.isoformat()} {ch}: n={int(scores['n'][ti, ci])} " + " ".join(
                f"{k}={scores[k][ti, ci]:.6g}" for k in ("bias", "mae", "rmse", "crps", "spread", "ssr") if np.isfinite(scores[k][ti, ci])))
    return res


@click.command(name="point")
@click.option("--model_name", "-m", type=click.Choice(AVAILABLE_MODELS, case_sensitive=False), default="pangu", help="Select model")
@click.option("--date", "-d", type=str, default=yesterday, help="YYYYMMDD")
@click.option("--time", "-t", type=str, default="0000", help="HHMM")
@click.option("--lead_time", "-l", type=int, default=24, help="Lead time in hours, rounded up to whole 6-h steps (--n_steps overrides it)")
@click.option("--list_models", "-lm", is_flag=True, help="List all available models and exit")
@click.option("--initial_conditions", "-ic", type=click.Choice(["cds", "ifs", "gfs"], case_sensitive=False), default="gfs",
              help="Initial conditions provider.")
@click.option("--modal", "-mo", is_flag=True, help="(reference only) run on Modal -- not available in this build")
@click.option("--point", "-p", "point", type=str, multiple=True, help="NAME:LAT,LON, repeatable (for example Istanbul:41.01,28.98)")
@click.option("--stations", "-s", type=str, default="", help="CSV file with the columns name,lat,lon")
@click.option("--channel", "-c", "channels", type=str, multiple=True, help="Channel to sample, repeatable (default: all)")
@click.option("--method", type=click.Choice(["bilinear", "nearest"]), default="bilinear", help="Interpolation")
@click.option("--n_steps", type=int, default=None, help="Model steps (default: from --lead_time)")
@click.option("--members", "-n", type=int, default=1, help="Ensemble members, 1-64; 1 = the deterministic forecast")
@click.option("--perturb_scale", type=float, default=1e-3, help="Perturbation amplitude in units of each channel's sigma (members > 1)")
@click.option("--seed", type=int, default=0, help="Seed of the perturbations (32-bit)")
@click.option("--output", "-o", type=str, default="", help="Write the values to this .json or .csv (long form) path")
@click.option("--observations", type=str, default="", help="Long-form CSV time,channel,point,value: print the station scores against it")
def point(model_name, date, time, lead_time, list_models, initial_conditions, modal, point, stations, channels, method, n_steps, members,
          perturb_scale, seed, output, observations):
    if modal:
        raise click.UsageError("--modal runs the reference on a hosted A100 service; this build runs on the local MI355X")
    pts = None
    if not list_models:
        try:
            pts = request(point, stations, output, n_steps)
        except (ValueError, OSError) as e:
            raise click.UsageError(str(e)) from None
    pf = run_point(model_name, date, time, lead_time, list_models, initial_conditions, pts, channels, method, n_steps, members, perturb_scale, seed)
    if pf is None:
        return None
    for ln in lines(pf):
        click.echo(ln)
    if observations:
        from .points import read_observations
        for ln in score_lines(pf.verify(read_observations(observations, pf.channels, pf.times, pf.names))):
            click.echo(ln)
    if output:
        if Path(output).suffix.lower() == ".csv":
            pf.to_csv(output)
        else:
            Path(output).write_text(pf.to_json())
        click.echo(output)
    return pf


if __name__ == "__main__":
    point()
