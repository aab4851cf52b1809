"""``verify`` command line: the options of ``forecast`` (skyrim_amd/forecast.py: same names, short flags and defaults) plus the size of
the ensemble to score (``--members 1``, the default, is the deterministic forecast), an optional climatology file for the ACC, and the
channels to print, and the kind of perturbation (``--perturbation spherical --length_scale_km --lmax``: this is where spread against skill is
tuned; ``--breed_cycles 3 --breed_norm total --breed_paired`` breeds those perturbations through the model, skyrim_amd/breeding.py;
``--stochastic sppt --stoch_amplitude --stoch_tau_h --stoch_length_scale_km`` perturbs every step of every member, skyrim_amd/stochastic.py;
the ``ensemble`` command keeps white noise), and the grid to score on (``--grid 1.5deg --regrid_method conservative``: forecast and
truth are regridded on the device, skyrim_amd/regrid.py; the default scores on the model's own grid), and the threshold events to verify
(``--event ws10m:15,25 --neighbourhood_km 100``, both repeatable: skyrim_amd/events.py).  Scores every lead time against the truth of the chosen source (``Skyrim.verify`` /
``Skyrim.ensemble_forecast(scores=True)``), prints one line per lead time and channel and echoes the path of the JSON file."""
from __future__ import annotations

from pathlib import Path

import click

from .common import AVAILABLE_MODELS
from .forecast import start_time_of, steps_for, yesterday
from .verify import DEFAULT_CHANNELS


def run_verify(model_name: str, date: str, time: str, lead_time: int, list_models: bool, initial_conditions: str, output_dir: str,
               filter_vars: str, members: int = 1, climatology: str | None = None, channels: str = "", perturb_scale: float = 1e-3,
               seed: int = 0, perturbation: str = "white", length_scale_km: float = 500.0, lmax: int | None = None,
               grid: str | None = None, regrid_method: str = "conservative", event=(), neighbourhood_km=(), breed_cycles: int = 0,
               breed_norm: str = "total", breed_paired: bool = False, stochastic: str | None = None, stoch_amplitude: float | None = None,
               stoch_tau_h: float | None = None, stoch_length_scale_km: float | None = None):
    """Returns the ``verify.Scores`` (None with ``list_models``); the JSON file's path is ``scores.path``."""
    from .core import Skyrim
    if list_models:
        print("Available models:", Skyrim.list_available_models())
        return None
    asked = {}
    if event:                                              # --event ws10m:15,25 (repeatable): threshold events, skyrim_amd/events.py
        from .events import parse_event
        asked = dict(events=dict(parse_event(e) for e in event), neighbourhoods_km=tuple(neighbourhood_km))
    elif neighbourhood_km:
        raise ValueError("--neighbourhood_km gives the scales of the events' fractions skill score: it needs --event")
    model = Skyrim(model_name, ic_source=initial_conditions)
    start_time = start_time_of(date, time)
    n_steps = steps_for(model, lead_time)
    if n_steps < 1:
        raise ValueError(f"lead time {lead_time} h is shorter than one {model.model.time_step.total_seconds() / 3600:g}-h step of {model_name}")
    scored = filter_vars.split(",") if bool(filter_vars) else None
    cfg = {"output_dir": output_dir or str(Path.cwd() / "outputs")}
    on_grid = {} if not grid else dict(grid=grid, regrid_method=regrid_method)
    on_grid.update(asked)
    bred = {} if not breed_cycles else dict(breeding=dict(cycles=breed_cycles, norm=breed_norm, paired=breed_paired))
    if stochastic:                                         # --stochastic sppt|additive|both: per-step perturbations, skyrim_amd/stochastic.py
        given = dict(amplitude=stoch_amplitude, tau_h=stoch_tau_h, length_scale_km=stoch_length_scale_km)
        bred["stochastic"] = dict(kind=stochastic, **{k: v for k, v in given.items() if v is not None})
    elif any(v is not None for v in (stoch_amplitude, stoch_tau_h, stoch_length_scale_km)):
        raise ValueError("--stoch_amplitude, --stoch_tau_h and --stoch_length_scale_km shape the per-step perturbations: they need --stochastic")
    if members == 1:
        scores = model.verify(start_time, n_steps=n_steps, climatology=climatology, channels=scored, save=True, save_config=cfg, **on_grid)
    else:
        ens = model.ensemble_forecast(start_time, n_steps=n_steps, n_members=members, perturb_scale=perturb_scale, seed=seed, products=(),
                                      channels=scored, climatology=climatology, scores=True, save_config=cfg, perturbation=perturbation,
                                      length_scale_km=length_scale_km, lmax=lmax, **bred, **on_grid)
        scores = ens.regridded.scores if grid else ens.scores
        scores.path = scores.save(cfg["output_dir"])
    return scores


def lines(scores, channels) -> list[str]:
    """One line per lead time and chosen channel: every metric of the table."""
    names = [c for c in channels if c in scores.channels] or scores.channels[:4]
    metrics = scores.table.metric.values.tolist()
    out = []
    for t, time in enumerate(scores.times):
        lead = (time - scores.times[0]).total_seconds() / 3600
        for c in names:
            vals = scores.table.values[:, t, scores.channels.index(c)]
            out.append(f"+{lead:g}h {c}: " + " ".join(f"{m}={v:.6g}" for m, v in zip(metrics, vals)))
    return out


def event_lines(scores) -> list[str]:
    """One line per lead time, event channel and threshold: the event scores that are single numbers."""
    ev = getattr(scores, "events", None)
    out = []
    for t, time in enumerate(ev.times if ev is not None else []):
        lead = (time - ev.times[0]).total_seconds() / 3600
        for e, c in enumerate(ev.channels):
            for k, thr in enumerate(ev.thresholds[c]):
                vals = " ".join(f"{m}={float(getattr(ev, m).values[t, e, k]):.6g}" for m in ev.names if m != "fss")
                fss = "" if ev.fss is None else " fss=" + ",".join(f"{v:.6g}" for v in ev.fss.values[t, e, k])
                out.append(f"+{lead:g}h {c}>{thr:g}: {vals}{fss}")
    return out


@click.command(name="verify")
@click.option("--model_name", "-m", type=click.Choice(AVAILABLE_MODELS, case_sensitive=False), default="pangu", help="Select model")
@click.option("--date", "-d", type=str, default=yesterday, help="YYYYMMDD")
@click.option("--time", "-t", type=str, default="0000", help="HHMM")
@click.option("--lead_time", "-l", type=int, default=6, help="Lead time in hours, rounded up to whole 6-h steps; every lead time from 0 to this one is scored")
@click.option("--list_models", "-lm", is_flag=True, help="List all available models and exit")
@click.option("--initial_conditions", "-ic", type=click.Choice(["cds", "ifs", "gfs"], case_sensitive=False), default="gfs",
              help="Initial conditions provider; the truth at the valid times comes from the same source.")
@click.option("--output_dir", "-o", type=str, default="", help="Output directory (local path)")
@click.option("--filter_vars", "-f", type=str, default="", 
              help="Variables that enter the scores and the JSON file, such as t2m,z500 (default: every one the truth holds).  In 'forecast' "
                   "the same flag chooses what is saved; nothing but the scores is saved here.  See --channels for what is printed.")
@click.option("--modal", "-mo", is_flag=True, help="(reference only) run on Modal -- not available in this build")
@click.option("--members", "-n", type=int, default=1, help="Ensemble members to score, 1-64; 1 = the deterministic forecast")
@click.option("--climatology", type=click.Path(exists=True), default=None, help="Saved (channel, lat, lon) or (time, ...) climatology for the ACC")
@click.option("--channels", "-c", type=str, default=",".join(DEFAULT_CHANNELS), 
              help="Which of the scored variables to print a line for, where the model has them; does not change the JSON file")
@click.option("--perturb_scale", type=float, default=1e-3, help="Perturbation amplitude in units of each channel's sigma (members > 1)")
@click.option("--seed", type=int, default=0, help="Seed of the perturbations (32-bit)")
@click.option("--perturbation", type=click.Choice(["white", "spherical"]), default="white",
              help="Perturbation kind (members > 1): grid-point white noise, or spatially correlated fields on the sphere")
@click.option("--length_scale_km", type=float, default=500.0, help="Correlation length of the spherical perturbations in km")
@click.option("--lmax", type=int, default=None, help="Spectral truncation of the spherical perturbations (default: min(256, n_lat, n_lon / 2))")
@click.option("--breed_cycles", type=int, default=0, help="Breed the perturbations through the model for this many cycles, 1-50 "
              "(members > 1; 0 = the seed perturbations as they are)")
@click.option("--breed_norm", type=click.Choice(["total", "channel"]), default="total",
              help="Rescaling of a bred vector: one factor per member, or every channel to its own amplitude")
@click.option("--breed_paired", is_flag=True, help="Members 2j-1 and 2j are the two signs of one bred vector")
@click.option("--stochastic", type=click.Choice(["sppt", "additive", "both"]), default=None,
              help="Perturb every step of every member (members > 1): SPPT multiplies the step's tendency by 1 + a random pattern, additive "
              "puts correlated noise on the state")
@click.option("--stoch_amplitude", type=float, default=None, help="Standard deviation of the SPPT multiplier's pattern (default 0.3)")
@click.option("--stoch_tau_h", type=float, default=None, help="Decorrelation time of the stochastic pattern in hours (default 6; 0 = white in time)")
@click.option("--stoch_length_scale_km", type=float, default=None, help="Correlation length of the stochastic pattern in km (default 500)")
@click.option("--grid", type=str, default=None, help="Score on this grid instead of the model's own: a resolution that divides 180 degrees, "
              "such as 1.5deg; forecast and truth are regridded on the device")
@click.option("--regrid_method", type=click.Choice(["conservative", "bilinear", "nearest"]), default="conservative",
              help="How --grid is reached (first-order conservative is what WeatherBench 2 uses)")
@click.option("--event", type=str, multiple=True, help="Verify the event NAME above each threshold, NAME:THRESHOLD[,THRESHOLD...] such as "
              "t2m:273.15,300 (repeatable; at most 4 thresholds each): Brier score, reliability, ROC, contingency scores in the JSON file")
@click.option("--neighbourhood_km", type=float, multiple=True, help="Radius in km of a neighbourhood of the events' fractions skill score "
              "(repeatable, at most 4; 0 = point-wise)")
def verify(model_name, date, time, lead_time, list_models, initial_conditions, output_dir, filter_vars, modal, members, climatology, channels,
           perturb_scale, seed, perturbation, length_scale_km, lmax, breed_cycles, breed_norm, breed_paired, stochastic, stoch_amplitude,
           stoch_tau_h, stoch_length_scale_km, grid, regrid_method, event, neighbourhood_km):
    if modal:
        raise click.UsageError("--modal runs the reference on a hosted A100 service; this build runs on the local MI355X")
    scores = run_verify(model_name, date, time, lead_time, list_models, initial_conditions, output_dir, filter_vars, members, climatology,
                        channels, perturb_scale, seed, perturbation, length_scale_km, lmax, grid, regrid_method, event, neighbourhood_km,
                        breed_cycles, breed_norm, breed_paired, stochastic, stoch_amplitude, stoch_tau_h, stoch_length_scale_km)
    if scores is None:
        return None
    for ln in lines(scores, [c for c in channels.split(",") if c]):
        click.echo(ln)
    for ln in event_lines(scores):
        click.echo(ln)
    click.echo(scores.path)
    return scores.path


if __name__ == "__main__":
    verify()
