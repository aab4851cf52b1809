"""``aggregate`` command line: the options of ``forecast`` (skyrim_amd/forecast.py: same names, short flags and defaults) plus the
time-window aggregates to make (``--aggregate ws10m:max:24h``, repeatable), the derived fields they may name (``--derived ws10m``) and the
size of the ensemble (``--members 1``, the default, is the deterministic forecast).  Every lead time is folded into its windows where the
forecast lies on the device (``Skyrim.aggregate_forecast`` / ``Skyrim.ensemble_forecast(aggregates=[...])``); prints one line per window and
aggregate and echoes the paths of the files."""
from __future__ import annotations

from pathlib import Path

import click
import numpy as np

from .common import AVAILABLE_MODELS
from .forecast import start_time_of, steps_for, yesterday


def run_aggregate(model_name: str, date: str, time: str, lead_time: int, list_models: bool, initial_conditions: str, output_dir: str,
                  aggregates, derived=(), members: int = 1, perturb_scale: float = 1e-3, seed: int = 0):
    """Returns ({window label: DataArray(time = window ends, channel = aggregates, lat, lon)}, paths): the aggregates of the deterministic
    forecast, or the ensemble mean of the aggregates with ``members`` > 1; (None, []) with ``list_models``."""
    from . import aggregate
    from .core import Skyrim
    if list_models:
        print("Available models:", Skyrim.list_available_models())
        return None, []
    for a in aggregates:
        aggregate.parse_request(a)                           # the grammar, before a model is built
    model = Skyrim(model_name, ic_source=initial_conditions)
    start_time = start_time_of(date, time)
    n_steps = steps_for(model, lead_time)
    if n_steps < 1:
        raise ValueError(f"lead time {lead_time} h is shorter than one {model.model.time_step.total_seconds() / 3600:g}-h step of {model_name}")
    cfg = {"output_dir": output_dir or str(Path.cwd() / "outputs")}
    derived = list(derived) or None
    if members == 1:
        out = model.aggregate_forecast(start_time, n_steps=n_steps, aggregates=list(aggregates), derived=derived, save=True, save_config=cfg)
        return out, [da.path for da in out.values()]
    ens = model.ensemble_forecast(start_time, n_steps=n_steps, n_members=members, perturb_scale=perturb_scale, seed=seed,
                                  products=("mean", "spread"), derived=derived, aggregates=list(aggregates), save=True, save_config=cfg)
    return {label: p.mean for label, p in ens.aggregated.items()}, [p for p in ens.paths if "-agg" in str(p)]


def lines(out: dict, t0=None) -> list[str]:
    """One line per window and aggregate: the window, the range and the mean of the aggregate."""
    res = []
    for label, da in out.items():
        ends = np.asarray(da._coords["time"]).astype("datetime64[s]")
        starts = np.asarray(da._coords["window_start"]).astype("datetime64[s]")
        origin = np.datetime64(t0, "s") if t0 is not None else starts[0]
        for w in range(len(ends)):
            a, b = ((t - origin) / np.timedelta64(1, "h") for t in (starts[w], ends[w]))
            for k, name in enumerate(da.channel.values.tolist()):
                v = np.asarray(da.values[w, k])
                res.append(f"({a:g}h, {b:g}h] {name}: min={v.min():.6g} mean={v.mean():.6g} max={v.max():.6g}")
    return res


@click.command(name="aggregate")
@click.option("--model_name", "-m", type=click.Choice(AVAILABLE_MODELS, case_sensitive=False), default="pangu", help="Select model")
@click.option("--date", "-d", type=str, default=yesterday, help="YYYYMMDD")
@click.option("--time", "-t", type=str, default="0000", help="HHMM")
@click.option("--lead_time", "-l", type=int, default=24, help="Lead time in hours, rounded up to whole 6-h steps; the windows cover the lead times after 0 up to this one")
@click.option("--list_models", "-lm", is_flag=True, help="List all available models and exit")
@click.option("--initial_conditions", "-ic", type=click.Choice(["cds", "ifs", "gfs"], case_sensitive=False), default="gfs",
              help="Initial conditions provider.")
@click.option("--output_dir", "-o", type=str, default="", help="Output directory (local path)")
@click.option("--modal", "-mo", is_flag=True, help="(reference only) run on Modal -- not available in this build")
@click.option("--aggregate", "-a", "aggregates", type=str, multiple=True, help="channel:stat:window, repeatable; stat: max, min, mean, sum, "
              "hours_above@<threshold>, when_max, when_min; window: <N>h or all (for example ws10m:max:24h)")
@click.option("--derived", "-f", type=str, default="", help="Comma-separated derived fields the aggregates may name (ws10m, ivt, ...)")
@click.option("--members", "-n", type=int, default=1, help="Ensemble members, 1-64; 1 = the deterministic forecast")
@click.option("--perturb_scale", type=float, default=1e-3, help="Perturbation amplitude in units of each channel's sigma (members > 1)")
@click.option("--seed", type=int, default=0, help="Seed of the perturbations (32-bit)")
def aggregate(model_name, date, time, lead_time, list_models, initial_conditions, output_dir, modal, aggregates, derived, members, perturb_scale,
              seed):
    if modal:
        raise click.UsageError("--modal runs the reference on a hosted A100 service; this build runs on the local MI355X")
    if not aggregates and not list_models:
        raise click.UsageError("at least one --aggregate channel:stat:window")
    fields = [f.strip() for f in derived.split(",") if f.strip()]
    out, paths = run_aggregate(model_name, date, time, lead_time, list_models, initial_conditions, output_dir, list(aggregates), fields, members,
                               perturb_scale, seed)
    if out is None:
        return None
    for ln in lines(out):
        click.echo(ln)
    for p in paths:
        click.echo(p)
    return paths


if __name__ == "__main__":
    aggregate()
