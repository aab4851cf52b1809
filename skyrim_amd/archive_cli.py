"""``archive`` command line: ``archive info DIR`` prints what a member archive (``ensemble_forecast(archive=...)``, skyrim_amd/archive.py)
holds; ``archive replay DIR`` makes ensemble products from its files, without a model: the product options of the ``ensemble`` command's
forecast (mean and spread by default) plus exceedance thresholds, quantiles and derived fields, written under ``--output_dir``."""
from __future__ import annotations

import json
from pathlib import Path

import click


def parse_table(items, what: str) -> dict:
    """``{channel: [values]}`` of repeated ``CHANNEL=V1,V2`` options; a ValueError that names the option otherwise."""
    out = {}
    for item in items:
        ch, sep, vals = str(item).partition("=")
        try:
            out.setdefault(ch.strip(), []).extend(float(v) for v in vals.split(",") if v.strip())
        except ValueError:
            sep = ""
        if not sep or not ch.strip() or not out.get(ch.strip()):
            raise ValueError(f"--{what} {item!r}: expected CHANNEL=VALUE[,VALUE...]")
    return out


def run_info(directory) -> dict:
    from . import archive
    return archive.open(directory).info()


def run_replay(directory, products=("mean", "spread"), exceed=(), quantiles=(), derived=(), channels="", output_dir="", device="cuda:0"):
    """The replayed ``EnsembleForecast``; with ``output_dir`` its files are written there (``save=True``)."""
    from . import archive
    request = dict(products=tuple(products), exceed=parse_table(exceed, "exceed") or None, quantiles=parse_table(quantiles, "quantile") or None,
                   channels=[c for c in channels.split(",") if c] or None)
    if derived:
        request["derived"] = list(derived)
    if output_dir:
        request.update(save=True, save_config={"output_dir": output_dir})
    return archive.open(directory).replay(device=device, **request)


@click.group(name="archive")
def archive():
    """Member archives: what they hold, and products replayed from them."""


@archive.command(name="info")
@click.argument("directory", type=click.Path(exists=True, file_okay=False))
def info(directory):
    click.echo(json.dumps(run_info(directory), indent=1))


@archive.command(name="replay")
@click.argument("directory", type=click.Path(exists=True, file_okay=False))
@click.option("--product", "-p", "products", multiple=True, type=click.Choice(["mean", "spread", "min", "max"]), help="Products (default: mean, spread)")
@click.option("--exceed", "-x", multiple=True, help="CHANNEL=THRESHOLD[,THRESHOLD...]: fraction of members above")
@click.option("--quantile", "-q", "quantiles", multiple=True, help="CHANNEL=LEVEL[,LEVEL...]: quantiles of the members")
@click.option("--derived", multiple=True, help="Derived fields made on replay (ws10m, ivt ...)")
@click.option("--channels", "-f", type=str, default="", help="Channels of the products, comma separated (default: all the archive holds)")
@click.option("--output_dir", "-o", type=str, default="", help="Output directory (local path); default ./outputs")
@click.option("--device", type=str, default="cuda:0")
def replay(directory, products, exceed, quantiles, derived, channels, output_dir, device):
    try:
        ens = run_replay(directory, products or ("mean", "spread"), exceed, quantiles, derived, channels,
                         output_dir or str(Path.cwd() / "outputs"), device)
    except ValueError as e:
        raise click.UsageError(str(e))
    for p in ens.paths:
        click.echo(p)
    return ens.paths


if __name__ == "__main__":
    archive()
