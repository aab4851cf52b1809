"""``scenario`` command line: the options of ``forecast`` (skyrim_amd/forecast.py: same names, short flags and defaults) plus the size of the
ensemble (``--members``), the channels the members are compared in (``--channel z500``, repeatable), the region
(``--region LAT_S,LAT_N,LON_W,LON_E``; default: the globe), ``--clusters``, ``--eofs`` and ``--normalise``.  At every lead time the member
Gram matrix is made where the members lie on the device (``Skyrim.ensemble_forecast(scenarios=...)``); the clusters with their
probabilities and representative members and the variance fractions of the EOFs are printed, ``--output`` writes them as ``.json``."""
from __future__ import annotations

import json
from pathlib import Path

import click
import numpy as np

from .common import AVAILABLE_MODELS
from .forecast import start_time_of, steps_for, yesterday


def parse_region(text: str):
    """(lat_s, lat_n, lon_w, lon_e) from ``LAT_S,LAT_N,LON_W,LON_E``; an empty text is the globe (None)."""
    if not text:
        return None
    parts = text.split(",")
    try:
        if len(parts) != 4:
            raise ValueError
        return tuple(float(p) for p in parts)
    except ValueError:
        raise ValueError(f"--region {text!r} is not LAT_S,LAT_N,LON_W,LON_E (for example 30,75,-80,40)") from None


def request(channels, region, clusters, eofs, normalise, members, output, n_steps=None) -> dict:
    """The ``scenarios=`` dict of the options; every refusal is a ValueError before a model is built."""
    from .scenarios import MAX_MEMBERS, MAX_OUT
    if not channels:
        raise ValueError("name the channels the members are compared in with --channel (repeatable), for example --channel z500")
    if not 2 <= members <= MAX_MEMBERS:
        raise ValueError(f"--members {members}: scenarios need 2 to {MAX_MEMBERS} members")
    if not 1 <= clusters <= members:
        raise ValueError(f"--clusters {clusters} is outside [1, {members}]")
    if not 0 <= eofs <= min(members - 1, MAX_OUT):
        raise ValueError(f"--eofs {eofs} is outside [0, {min(members - 1, MAX_OUT)}]")
    if output and Path(output).suffix.lower() != ".json":
        raise ValueError(f"--output {output!r}: a .json path")
    if n_steps is not None and n_steps < 0:
        raise ValueError("--n_steps >= 0")
    return dict(channels=list(channels), region=parse_region(region), n_clusters=clusters, n_eofs=eofs, normalise=normalise)


def run_scenario(model_name: str, date: str, time: str, lead_time: int, list_models: bool, initial_conditions: str, spec: dict, n_steps=None,
                 members: int = 10, perturb_scale: float = 1e-3, seed: int = 0):
    """Returns the ``scenarios.Scenarios``; None with ``list_models``."""
    from .core import Skyrim
    if list_models:
        print("Available models:", Skyrim.list_available_models())
        return None
    model = Skyrim(model_name, ic_source=initial_conditions)
    start_time = start_time_of(date, time)
    if n_steps is None:
        n_steps = steps_for(model, lead_time)
    ens = model.ensemble_forecast(start_time, n_steps=n_steps, n_members=members, perturb_scale=perturb_scale, seed=seed, products=(),
                                  scenarios=spec)
    return ens.scenarios


def document(sc) -> dict:
    """What ``--output`` writes: per lead time the labels, sizes, probabilities, representatives, sums of squares and variance fractions."""
    iso = lambda t: t.isoformat() if hasattr(t, "isoformat") else str(t)      # noqa: E731
    times = []
    for ti, t in enumerate(sc.times):
        c = sc.clusters_at[ti]
        times.append(dict(time=iso(t), labels=c["labels"].tolist(), sizes=c["sizes"].tolist(), probability=c["probability"].tolist(),
                          representative=c["representative"].tolist(), within=c["within"], explained=c["explained"], total=c["total"],
                          variance_fraction=np.asarray(sc.variance_fraction[ti]).tolist()))
    return dict(channels=list(sc.channels), region=list(sc.region), normalise=sc.normalise, n_members=sc.n_members, times=times)


def lines(sc) -> list[str]:
    """One line per lead time and cluster, one for the EOFs of the lead time."""
    res = []
    for ti, t in enumerate(sc.times):
        c = sc.clusters_at[ti]
        stamp = t.isoformat() if hasattr(t, "isoformat") else str(t)
        for k in range(len(c["sizes"])):
            who = ",".join(str(m) for m in np.nonzero(c["labels"] == k)[0])
            res.append(f"{stamp} cluster {k}: p={c['probability'][k]:.3f} size={int(c['sizes'][k])} representative={int(c['representative'][k])} "
                       f"members={who}")
        if np.asarray(sc.variance_fraction[ti]).size:
            res.append(f"{stamp} eof variance fractions: " + " ".join(f"{v:.4f}" for v in sc.variance_fraction[ti]))
    return res


@click.command(name="scenario")
@click.option("--model_name", "-m", type=click.Choice(AVAILABLE_MODELS, case_sensitive=False), default="pangu", help="Select model")
@click.option("--date", "-d", type=str, default=yesterday, help="YYYYMMDD")
@click.option("--time", "-t", type=str, default="0000", help="HHMM")
@click.option("--lead_time", "-l", type=int, default=24, help="Lead time in hours, rounded up to whole 6-h steps (--n_steps overrides it)")
@click.option("--list_models", "-lm", is_flag=True, help="List all available models and exit")
@click.option("--initial_conditions", "-ic", type=click.Choice(["cds", "ifs", "gfs"], case_sensitive=False), default="gfs",
              help="Initial conditions provider.")
@click.option("--modal", "-mo", is_flag=True, help="(reference only) run on Modal -- not available in this build")
@click.option("--channel", "-c", "channels", type=str, multiple=True, help="Raw channel the members are compared in, repeatable")
@click.option("--region", "-r", type=str, default="", help="LAT_S,LAT_N,LON_W,LON_E (default: the globe); a box may cross the date line")
@click.option("--clusters", "-k", type=int, default=3, help="Number of clusters (Ward's method)")
@click.option("--eofs", type=int, default=3, help="Number of EOFs, 0-8")
@click.option("--normalise", type=click.Choice(["spread", "std", "none"]), default="spread", help="How channels are weighed against each other")
@click.option("--n_steps", type=int, default=None, help="Model steps (default: from --lead_time)")
@click.option("--members", "-n", type=int, default=10, help="Ensemble members, 2-64")
@click.option("--perturb_scale", type=float, default=1e-3, help="Perturbation amplitude in units of each channel's sigma")
@click.option("--seed", type=int, default=0, help="Seed of the perturbations (32-bit)")
@click.option("--output", "-o", type=str, default="", help="Write the clusters and variance fractions to this .json path")
def scenario(model_name, date, time, lead_time, list_models, initial_conditions, modal, channels, region, clusters, eofs, normalise, n_steps,
             members, perturb_scale, seed, output):
    if modal:
        raise click.UsageError("--modal runs the reference on a hosted A100 service; this build runs on the local MI355X")
    spec = None
    if not list_models:
        try:
            spec = request(channels, region, clusters, eofs, normalise, members, output, n_steps)
        except ValueError as e:
            raise click.UsageError(str(e)) from None
    sc = run_scenario(model_name, date, time, lead_time, list_models, initial_conditions, spec, n_steps, members, perturb_scale, seed)
    if sc is None:
        return None
    for ln in lines(sc):
        click.echo(ln)
    if output:
        Path(output).write_text(json.dumps(document(sc)))
        click.echo(output)
    return sc


if __name__ == "__main__":
    scenario()
