"""``objects`` command line: the options of ``forecast`` (skyrim_amd/forecast.py: same names, short flags and defaults) plus the size of
the ensemble (``--members 1``, the default, is the deterministic forecast), the planes ``--object channel:above|below:thr[,thr...]``
(repeatable) and the host's filters.  Finds the contiguous regions beyond each threshold at every lead time where the forecast lies on
the device (``Skyrim.object_forecast`` / ``Skyrim.ensemble_forecast(objects=...)``), prints one line per kept object and echoes the path
of the JSON file."""
from __future__ import annotations

from pathlib import Path

import click

from .common import AVAILABLE_MODELS
from .forecast import start_time_of, steps_for, yesterday


def parse_objects(specs, connectivity=None, min_pixels=None, capacity=None, **filters) -> dict:
    """The ``objects=`` dict of ``--object channel:above|below:thr[,thr...]`` entries; the filters apply to every channel."""
    req: dict = {}
    for spec in specs:
        parts = spec.split(":")
        if len(parts) != 3 or parts[1] not in ("above", "below"):
            raise click.UsageError(f"--object {spec!r}: expected channel:above:thr[,thr...] or channel:below:thr[,thr...]")
        try:
            values = [float(v) for v in parts[2].split(",")]
        except ValueError:
            raise click.UsageError(f"--object {spec!r}: the thresholds are numbers separated by commas") from None
        entry = req.setdefault(parts[0], {k: v for k, v in filters.items() if v is not None})
        entry.setdefault(parts[1], []).extend(values)
    if not req:
        raise click.UsageError("give at least one --object channel:above|below:thr")
    for k, v in (("connectivity", connectivity), ("min_pixels", min_pixels), ("capacity", capacity)):
        if v is not None:
            req[k] = v
    return req


def run_objects(model_name: str, date: str, time: str, lead_time: int, list_models: bool, initial_conditions: str, output_dir: str,
                objects: dict, members: int = 1, perturb_scale: float = 1e-3, seed: int = 0, derived=None):
    """Returns the ``objects.Objects`` (None with ``list_models``); the JSON file's path is its ``path``."""
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
        return model.object_forecast(start_time, n_steps=n_steps, objects=objects, derived=derived, save=True, save_config=cfg)
    ens = model.ensemble_forecast(start_time, n_steps=n_steps, n_members=members, perturb_scale=perturb_scale, seed=seed, products=(),
                                  objects=objects, derived=derived, save_config=cfg)
    ens.objects.path = ens.objects.save(cfg["output_dir"])
    return ens.objects


def lines(objs) -> list[str]:
    """One header line per (lead time, plane), then one line per kept object."""
    out = []
    for t, time in enumerate(objs.times):
        lead = (time - objs.times[0]).total_seconds() / 3600
        for p, label in enumerate(objs.planes):
            kept = int(objs.count(p)[t].sum())
            out.append(f"+{lead:g}h {label}: {kept} objects in {objs.n_members} member(s)")
            for m in range(objs.n_members):
                for o in objs.objects[t][m][p]:
                    if o["keep"]:
                        out.append(f"  member {m} id {o['id']} lat={o['lat']:.2f} lon={o['lon']:.2f} area={o['area_km2']:.4g}km2 "
                                   f"length={o['length_km']:.0f}km width={o['width_km']:.0f}km mean={o['mean']:.5g} extreme={o['extreme']:.5g}")
    return out


@click.command(name="objects")
@click.option("--model_name", "-m", type=click.Choice(AVAILABLE_MODELS, case_sensitive=False), default="pangu", help="Select model")
@click.option("--date", "-d", type=str, default=yesterday, help="YYYYMMDD")
@click.option("--time", "-t", type=str, default="0000", help="HHMM")
@click.option("--lead_time", "-l", type=int, default=24, help="Lead time in hours, rounded up to whole 6-h steps; every lead time from 0 to this one is searched")
@click.option("--list_models", "-lm", is_flag=True, help="List all available models and exit")
@click.option("--initial_conditions", "-ic", type=click.Choice(["cds", "ifs", "gfs"], case_sensitive=False), default="gfs",
              help="Initial conditions provider.")
@click.option("--output_dir", "-o", type=str, default="", help="Output directory (local path)")
@click.option("--modal", "-mo", is_flag=True, help="(reference only) run on Modal -- not available in this build")
@click.option("--members", "-n", type=int, default=1, help="Ensemble members, 1-64; 1 = the deterministic forecast")
@click.option("--perturb_scale", type=float, default=1e-3, help="Perturbation amplitude in units of each channel's sigma (members > 1)")
@click.option("--seed", type=int, default=0, help="Seed of the perturbations (32-bit)")
@click.option("--object", "object_", type=str, multiple=True, help="channel:above|below:thr[,thr...], e.g. ivt:above:250,500 (repeatable)")
@click.option("--derived", type=str, multiple=True, help="A derived field the objects may name, e.g. ivt or ws10m (repeatable)")
@click.option("--min_area_km2", type=float, default=None, help="Smallest area of a kept object")
@click.option("--min_length_km", type=float, default=None, help="Shortest major axis of a kept object")
@click.option("--min_elongation", type=float, default=None, help="Least length / width of a kept object")
@click.option("--connectivity", type=click.Choice(["4", "8"]), default=None, help="Neighbourhood of the labelling (default 8)")
@click.option("--min_pixels", type=int, default=None, help="Smallest component that is numbered (default 1)")
@click.option("--capacity", type=int, default=None, help="Objects kept per member and plane (default 1024)")
def objects(model_name, date, time, lead_time, list_models, initial_conditions, output_dir, modal, members, perturb_scale, seed, object_, derived,
            min_area_km2, min_length_km, min_elongation, connectivity, min_pixels, capacity):
    if modal:
        raise click.UsageError("--modal runs the reference on a hosted A100 service; this build runs on the local MI355X")
    request = None
    if not list_models:
        request = parse_objects(object_, None if connectivity is None else int(connectivity), min_pixels, capacity, min_area_km2=min_area_km2,
                                min_length_km=min_length_km, min_elongation=min_elongation)
    objs = run_objects(model_name, date, time, lead_time, list_models, initial_conditions, output_dir, request, members, perturb_scale, seed,
                       list(derived) or None)
    if objs is None:
        return None
    for ln in lines(objs):
        click.echo(ln)
    click.echo(objs.path)
    return objs.path


if __name__ == "__main__":
    objects()
