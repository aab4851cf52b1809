"""``track`` command line: the options of ``forecast`` (skyrim_amd/forecast.py: same names, short flags and defaults) plus the size of
the ensemble to track (``--members 1``, the default, is the deterministic forecast) and the settings of ``tracks.TrackerConfig`` that
are tuned most.  Detects cyclone centres at every lead time where the forecast lies on the device (``Skyrim.track_cyclones`` /
``Skyrim.ensemble_forecast(tracks=True)``), prints one line per track point and echoes the path of the JSON file."""
from __future__ import annotations

from pathlib import Path

import click

from .common import AVAILABLE_MODELS
from .forecast import start_time_of, steps_for, yesterday


def run_track(model_name: str, date: str, time: str, lead_time: int, list_models: bool, initial_conditions: str, output_dir: str,
              members: int = 1, perturb_scale: float = 1e-3, seed: int = 0, config: dict | None = None):
    """Returns the ``tracks.Tracks`` (None with ``list_models``); the JSON file's path is ``tracks.path``."""
    from .core import Skyrim
    if list_models:
        print("Available models:", Skyrim.list_available_models())
        return None
    model = Skyrim(model_name, ic_source=initial_conditions)
    start_time = start_time_of(date, time)
    n_steps = steps_for(model, lead_time)
    if n_steps < 1:
        raise ValueError(f"lead time {lead_time} h is shorter than one {model.model.time_step.total_seconds() / 3600:g}-h step of {model_name}")
    cfg = {"output_dir": output_dir or str(Path.cwd() / "outputs")}
    if members == 1:
        return model.track_cyclones(start_time, n_steps=n_steps, config=config, save=True, save_config=cfg)
    ens = model.ensemble_forecast(start_time, n_steps=n_steps, n_members=members, perturb_scale=perturb_scale, seed=seed, products=(),
                                  tracks=True, track_config=config, save_config=cfg)
    ens.tracks.path = ens.tracks.save(cfg["output_dir"])
    return ens.tracks


def lines(tracks) -> list[str]:
    """One header line per track, then one line per point."""
    out = []
    for n, tr in enumerate(tracks):
        out.append(f"track {n} member {tr['member']}: {len(tr['times'])} points")
        for k, time in enumerate(tr["times"]):
            lead = (time - tracks.times[0]).total_seconds() / 3600
            out.append(f"  +{lead:g}h lat={tr['lat'][k]:.2f} lon={tr['lon'][k]:.2f} msl={tr['msl'][k]:.1f} wind={tr['wind'][k]:.2f} "
                       f"vort={tr['vort'][k]:.3g} core={tr['core'][k]:.4g}")
    return out


@click.command(name="track")
@click.option("--model_name", "-m", type=click.Choice(AVAILABLE_MODELS, case_sensitive=False), default="pangu", help="Select model")
@click.option("--date", "-d", type=str, default=yesterday, help="YYYYMMDD")
@click.option("--time", "-t", type=str, default="0000", help="HHMM")
@click.option("--lead_time", "-l", type=int, default=24, help="Lead time in hours, rounded up to whole 6-h steps; every lead time from 0 to this one is searched")
@click.option("--list_models", "-lm", is_flag=True, help="List all available models and exit")
@click.option("--initial_conditions", "-ic", type=click.Choice(["cds", "ifs", "gfs"], case_sensitive=False), default="gfs",
              help="Initial conditions provider.")
@click.option("--output_dir", "-o", type=str, default="", help="Output directory (local path)")
@click.option("--modal", "-mo", is_flag=True, help="(reference only) run on Modal -- not available in this build")
@click.option("--members", "-n", type=int, default=1, help="Ensemble members to track, 1-64; 1 = the deterministic forecast")
@click.option("--perturb_scale", type=float, default=1e-3, help="Perturbation amplitude in units of each channel's sigma (members > 1)")
@click.option("--seed", type=int, default=0, help="Seed of the perturbations (32-bit)")
@click.option("--lat_max", type=float, default=None, help="Centres are sought at |lat| <= this (default 60)")
@click.option("--thr_vort", type=float, default=None, help="Least cyclonic 850-hPa vorticity near a centre in 1/s (default 5e-5)")
@click.option("--thr_wind", type=float, default=None, help="Least 10-m wind near a centre in m/s (default 8)")
@click.option("--thr_core", type=float, default=None, help="Least warm-core excess of the thickness near a centre (default 0)")
@click.option("--min_points", type=int, default=None, help="Shortest track that is kept (default 2)")
def track(model_name, date, time, lead_time, list_models, initial_conditions, output_dir, modal, members, perturb_scale, seed, lat_max,
          thr_vort, thr_wind, thr_core, min_points):
    if modal:
        raise click.UsageError("--modal runs the reference on a hosted A100 service; this build runs on the local MI355X")
    given = dict(lat_max=lat_max, thr_vort=thr_vort, thr_wind=thr_wind, thr_core=thr_core, min_points=min_points)
    config = {k: v for k, v in given.items() if v is not None}
    tracks = run_track(model_name, date, time, lead_time, list_models, initial_conditions, output_dir, members, perturb_scale, seed, config)
    if tracks is None:
        return None
    if not tracks.criteria.get("warm_core", True):
        click.echo(tracks.criteria.get("note", ""))
    for ln in lines(tracks):
        click.echo(ln)
    click.echo(tracks.path)
    return tracks.path


if __name__ == "__main__":
    track()
