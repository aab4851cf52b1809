"""``ensemble`` command line: the options of ``forecast`` (skyrim_amd/forecast.py: same names, short flags and defaults) plus the size,
perturbation scale and seed of a perturbed-initial-condition ensemble (``Skyrim.ensemble_forecast``).  Writes the ensemble mean and
spread of every step and echoes the paths."""
from __future__ import annotations

from pathlib import Path

import click

from .common import AVAILABLE_MODELS
from .forecast import start_time_of, steps_for, yesterday


def run_ensemble(model_name: str, date: str, time: str, lead_time: int, list_models: bool, initial_conditions: str, output_dir: str,
                 filter_vars: str, members: int = 10, perturb_scale: float = 1e-3, seed: int = 0):
    from .core import Skyrim
    if list_models:
        print("Available models:", Skyrim.list_available_models())
        return []
    model = Skyrim(model_name, ic_source=initial_conditions)
    start_time = start_time_of(date, time)
    n_steps = steps_for(model, lead_time)
    if n_steps < 1:
        raise ValueError(f"lead time {lead_time} h is shorter than one {model.model.time_step.total_seconds() / 3600:g}-h step of {model_name}")
    ens = model.ensemble_forecast(start_time, n_steps=n_steps, n_members=members, perturb_scale=perturb_scale, seed=seed,
                                  products=("mean", "spread"), save=True,
                                  save_config={"output_dir": output_dir or str(Path.cwd() / "outputs"),
                                               "filter_vars": (filter_vars.split(",") if bool(filter_vars) else [])})
    return ens.paths


@click.command(name="ensemble")
@click.option("--model_name", "-m", type=click.Choice(AVAILABLE_MODELS, case_sensitive=False), default="pangu", help="Select model")
@click.option("--date", "-d", type=str, default=yesterday, help="YYYYMMDD")
@click.option("--time", "-t", type=str, default="0000", help="HHMM")
@click.option("--lead_time", "-l", type=int, default=6, help="Lead time in hours, int 0-24")
@click.option("--list_models", "-lm", is_flag=True, help="List all available models and exit")
@click.option("--initial_conditions", "-ic", type=click.Choice(["cds", "ifs", "gfs"], case_sensitive=False), default="gfs",
              help="Initial conditions provider.")
@click.option("--output_dir", "-o", type=str, default="", help="Output directory (local path)")
@click.option("--filter_vars", "-f", type=str, default="", help="Filter variables such as t2m (temperature) before saving forecasts.")
@click.option("--modal", "-mo", is_flag=True, help="(reference only) run on Modal -- not available in this build")
@click.option("--members", "-n", type=int, default=10, help="Ensemble members (member 0 is the unperturbed control), 1-64")
@click.option("--perturb_scale", type=float, default=1e-3, help="Perturbation amplitude in units of each channel's sigma")
@click.option("--seed", type=int, default=0, help="Seed of the perturbations (32-bit)")
def ensemble(model_name, date, time, lead_time, list_models, initial_conditions, output_dir, filter_vars, modal, members, perturb_scale, seed):
    if modal:
        raise click.UsageError("--modal runs the reference on a hosted A100 service; this build runs on the local MI355X")
    paths = run_ensemble(model_name, date, time, lead_time, list_models, initial_conditions, output_dir, filter_vars, members, perturb_scale, seed)
    for p in paths:
        click.echo(p)
    return paths


if __name__ == "__main__":
    ensemble()
