"""``derive`` command line: the options of ``forecast`` (skyrim_amd/forecast.py: same names, short flags and defaults) plus the derived
fields to make (``--fields ws10m,ivt,vo850``) and the size of the ensemble (``--members 1``, the default, is the deterministic forecast).
The fields are formed at every lead time where the forecast lies on the device (``Skyrim.derive_fields`` /
``Skyrim.ensemble_forecast(derived=[...])``); prints one line per lead time and field and echoes the paths of the files."""
from __future__ import annotations

from pathlib import Path

import click
import numpy as np

from .common import AVAILABLE_MODELS
from .forecast import start_time_of, steps_for, yesterday


def run_derive(model_name: str, date: str, time: str, lead_time: int, list_models: bool, initial_conditions: str, output_dir: str,
               fields, members: int = 1, perturb_scale: float = 1e-3, seed: int = 0):
    """Returns (DataArray(time, channel=fields, lat, lon), paths): the derived fields of the deterministic forecast, or the ensemble mean of
    the derived fields with ``members`` > 1; (None, []) with ``list_models``."""
    from .core import Skyrim
    if list_models:
        print("Available models:", Skyrim.list_available_models())
        return None, []
    model = Skyrim(model_name, ic_source=initial_conditions)
    start_time = start_time_of(date, time)
    n_steps = steps_for(model, lead_time)
    if n_steps < 1:
        raise ValueError(f"lead time {lead_time} h is shorter than one {model.model.time_step.total_seconds() / 3600:g}-h step of {model_name}")
    cfg = {"output_dir": output_dir or str(Path.cwd() / "outputs")}
    if members == 1:
        da = model.derive_fields(start_time, n_steps=n_steps, fields=list(fields), save=True, save_config=cfg)
        return da, [da.path]
    ens = model.ensemble_forecast(start_time, n_steps=n_steps, n_members=members, perturb_scale=perturb_scale, seed=seed,
                                  products=("mean", "spread"), derived=list(fields), save=True, save_config=cfg)
    return ens.derived.mean, [p for p in ens.paths if "derived-" in str(p)]


def lines(da) -> list[str]:
    """One line per lead time and field: the range and the mean of the field."""
    out = []
    times = list(da.time.values)
    for t, time in enumerate(times):
        lead = (np.datetime64(time, "s") - np.datetime64(times[0], "s")) / np.timedelta64(1, "h")
        for k, name in enumerate(da.channel.values.tolist()):
            v = np.asarray(da.values[t, k])
            out.append(f"+{lead:g}h {name}: min={v.min():.6g} mean={v.mean():.6g} max={v.max():.6g}")
    return out


@click.command(name="derive")
@click.option("--model_name", "-m", type=click.Choice(AVAILABLE_MODELS, case_sensitive=False), default="pangu", help="Select model")
@click.option("--date", "-d", type=str, default=yesterday, help="YYYYMMDD")
@click.option("--time", "-t", type=str, default="0000", help="HHMM")
@click.option("--lead_time", "-l", type=int, default=24, help="Lead time in hours, rounded up to whole 6-h steps; every lead time from 0 to this one is derived")
@click.option("--list_models", "-lm", is_flag=True, help="List all available models and exit")
@click.option("--initial_conditions", "-ic", type=click.Choice(["cds", "ifs", "gfs"], case_sensitive=False), default="gfs",
              help="Initial conditions provider.")
@click.option("--output_dir", "-o", type=str, default="", help="Output directory (local path)")
@click.option("--modal", "-mo", is_flag=True, help="(reference only) run on Modal -- not available in this build")
@click.option("--fields", "-f", type=str, default="ws10m", help="Comma-separated derived fields: ws10m, ws100m, ws<level>, thk<a>_<b>, "
              "vo<X>, div<X>, ivt, ivtu, ivtv, iwv")
@click.option("--members", "-n", type=int, default=1, help="Ensemble members, 1-64; 1 = the deterministic forecast")
@click.option("--perturb_scale", type=float, default=1e-3, help="Perturbation amplitude in units of each channel's sigma (members > 1)")
@click.option("--seed", type=int, default=0, help="Seed of the perturbations (32-bit)")
def derive(model_name, date, time, lead_time, list_models, initial_conditions, output_dir, modal, fields, members, perturb_scale, seed):
    if modal:
        raise click.UsageError("--modal runs the reference on a hosted A100 service; this build runs on the local MI355X")
    names = [f.strip() for f in fields.split(",") if f.strip()]
    da, paths = run_derive(model_name, date, time, lead_time, list_models, initial_conditions, output_dir, names, members, perturb_scale, seed)
    if da is None:
        return None
    for ln in lines(da):
        click.echo(ln)
    for p in paths:
        click.echo(p)
    return paths


if __name__ == "__main__":
    derive()
