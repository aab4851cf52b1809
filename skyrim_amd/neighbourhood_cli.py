"""``neighbourhood`` command line: the options of ``forecast`` (skyrim_amd/forecast.py: same names, short flags and defaults) plus the
neighbourhood fields to make (``--neighbourhood ws10m:max:100km``, repeatable), the derived fields they may name (``--derived ws10m``) and
the size of the ensemble (``--members 1``, the default, is the deterministic forecast).  Every lead time is reduced over the discs where
the forecast lies on the device (``Skyrim.neighbourhood_forecast`` / ``Skyrim.ensemble_forecast(neighbourhood=[...])``); prints one line
per lead time and field and echoes the paths of the files."""
from __future__ import annotations

from pathlib import Path

import click
import numpy as np

from .common import AVAILABLE_MODELS
from .forecast import start_time_of, steps_for, yesterday


def run_neighbourhood(model_name: str, date: str, time: str, lead_time: int, list_models: bool, initial_conditions: str, output_dir: str,
                      requests, derived=(), members: int = 1, perturb_scale: float = 1e-3, seed: int = 0):
    """Returns (DataArray(time, channel = fields, lat, lon), paths): the fields of the deterministic forecast, or the ensemble mean of the
    fields with ``members`` > 1; (None, []) with ``list_models``."""
    from . import neighbourhood
    from .core import Skyrim
    if list_models:
        print("Available models:", Skyrim.list_available_models())
        return None, []
    for r in requests:
        neighbourhood.parse_request(r)                       # the grammar, before a model is built
    model = Skyrim(model_name, ic_source=initial_conditions)
    start_time = start_time_of(date, time)
    n_steps = steps_for(model, lead_time)
    cfg = {"output_dir": output_dir or str(Path.cwd() / "outputs")}
    derived = list(derived) or None
    if members == 1:
        out = model.neighbourhood_forecast(start_time, n_steps=n_steps, neighbourhood=list(requests), derived=derived, save=True, save_config=cfg)
        return out, [out.path]
    ens = model.ensemble_forecast(start_time, n_steps=n_steps, n_members=members, perturb_scale=perturb_scale, seed=seed,
                                  products=("mean", "spread"), derived=derived, neighbourhood=list(requests), save=True, save_config=cfg)
    return ens.neighbourhood.mean, [p for p in ens.paths if "-nbr-" in str(p)]


def lines(da) -> list[str]:
    """One line per lead time and field: the lead, the range and the mean of the field."""
    times = np.asarray(da._coords["time"]).astype("datetime64[s]")
    res = []
    for t in range(len(times)):
        lead = (times[t] - times[0]) / np.timedelta64(1, "h")
        for k, name in enumerate(da.channel.values.tolist()):
            v = np.asarray(da.values[t, k])
            res.append(f"+{lead:g}h {name}: min={v.min():.6g} mean={v.mean():.6g} max={v.max():.6g}")
    return res


@click.command(name="neighbourhood")
@click.option("--model_name", "-m", type=click.Choice(AVAILABLE_MODELS, case_sensitive=False), default="pangu", help="Select model")
@click.option("--date", "-d", type=str, default=yesterday, help="YYYYMMDD")
@click.option("--time", "-t", type=str, default="0000", help="HHMM")
@click.option("--lead_time", "-l", type=int, default=24, help="Lead time in hours, rounded up to whole 6-h steps")
@click.option("--list_models", "-lm", is_flag=True, help="List all available models and exit")
@click.option("--initial_conditions", "-ic", type=click.Choice(["cds", "ifs", "gfs"], case_sensitive=False), default="gfs",
              help="Initial conditions provider.")
@click.option("--output_dir", "-o", type=str, default="", help="Output directory (local path)")
@click.option("--modal", "-mo", is_flag=True, help="(reference only) run on Modal -- not available in this build")
@click.option("--neighbourhood", "-a", "requests", type=str, multiple=True, help="channel:stat:radius, repeatable; stat: max, min, mean, "
              "frac_above@<threshold>; radius: <N>km (for example ws10m:max:100km)")
@click.option("--derived", "-f", type=str, default="", help="Comma-separated derived fields the requests may name (ws10m, ivt, ...)")
@click.option("--members", "-n", type=int, default=1, help="Ensemble members, 1-64; 1 = the deterministic forecast")
@click.option("--perturb_scale", type=float, default=1e-3, help="Perturbation amplitude in units of each channel's sigma (members > 1)")
@click.option("--seed", type=int, default=0, help="Seed of the perturbations (32-bit)")
def neighbourhood(model_name, date, time, lead_time, list_models, initial_conditions, output_dir, modal, requests, derived, members, perturb_scale,
                  seed):
    if modal:
        raise click.UsageError("--modal runs the reference on a hosted A100 service; this build runs on the local MI355X")
    if not requests and not list_models:
        raise click.UsageError("at least one --neighbourhood channel:stat:radius")
    fields = [f.strip() for f in derived.split(",") if f.strip()]
    out, paths = run_neighbourhood(model_name, date, time, lead_time, list_models, initial_conditions, output_dir, list(requests), fields, members,
                                   perturb_scale, seed)
    if out is None:
        return None
    for ln in lines(out):
        click.echo(ln)
    for p in paths:
        click.echo(p)
    return paths


if __name__ == "__main__":
    neighbourhood()
