"""``regrid`` command line: saved forecasts in, the same forecasts on another latitude-longitude grid out.  Every input file (netCDF or
zarr store, dims time, channel, lat, lon) is uploaded one time entry after the other, regridded on the device (``regrid.regrid_prediction``,
skyrim_amd/regrid.py) and written next to ``--output_dir`` under its own name with ``-regrid`` added to the model field; prints one line
per file and echoes the paths."""
from __future__ import annotations

from pathlib import Path

import click


def parse_grid(grid: str, region: str | None, res: str | None):
    """The ``grid`` of ``regrid.target_grid`` from the command's options: ``--region lat_s,lat_n,lon_w,lon_e`` (with an optional ``--res``) or a
    resolution such as ``1.5deg``."""
    if region:
        box = [float(v) for v in region.split(",")]
        if len(box) != 4:
            raise ValueError("--region takes lat_s,lat_n,lon_w,lon_e")
        return dict(region=tuple(box), res=res or None)
    return grid


def output_name(path: Path) -> str:
    """``{model}-regrid__{source}__{start}__{end}.nc`` of an input named ``{model}__{source}__{start}__{end}.*``; otherwise ``{stem}-regrid.nc``."""
    parts = path.name.split(".")[0].split("__")
    if len(parts) == 4:
        return "__".join([parts[0] + "-regrid"] + parts[1:]) + ".nc"
    return path.name.split(".")[0] + "-regrid.nc"


def run_regrid(files, grid, method: str = "conservative", output_dir: str = "", channels: str = "", device: str = "cuda:0") -> list:
    """Returns the paths written, one per input file."""
    from . import regrid
    picked = [c for c in channels.split(",") if c] or None
    out_dir = Path(output_dir or Path.cwd() / "outputs")
    out_dir.mkdir(parents=True, exist_ok=True)
    paths = []
    for f in files:
        da = regrid.regrid_prediction(str(f), grid, method, device=device, channels=picked)
        path = out_dir / output_name(Path(f))
        da.to_netcdf(path)
        paths.append(str(path))
    return paths


@click.command(name="regrid")
@click.argument("files", nargs=-1, required=True, type=click.Path(exists=True))
@click.option("--grid", "-g", type=str, default="1.5deg", help="Target resolution; 180 / res must be an integer")
@click.option("--region", "-r", type=str, default=None, help="lat_s,lat_n,lon_w,lon_e: a box instead of the globe; lon_w > lon_e crosses the date line")
@click.option("--res", type=str, default=None, help="Resolution inside --region (default: the source's own points)")
@click.option("--method", "-m", type=click.Choice(["conservative", "bilinear", "nearest"]), default="conservative", help="Regridding method")
@click.option("--channels", "-c", type=str, default="", help="Comma-separated channels to keep (default: all)")
@click.option("--output_dir", "-o", type=str, default="", help="Output directory (local path)")
def regrid(files, grid, region, res, method, channels, output_dir):
    paths = run_regrid(files, parse_grid(grid, region, res), method, output_dir, channels)
    for src, dst in zip(files, paths):
        click.echo(f"{src} -> {dst}")
    return paths


if __name__ == "__main__":
    regrid()
