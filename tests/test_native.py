"""The binding policy of the twenty-one C-ABI libraries, engines and products alike (skyrim_amd/native.py), without a GPU: each header's
declared entry points are the binding's EXPORTS and are exported by the built library, the library reports the header's ABI version,
and a missing file or another ABI version is refused at load."""
import re
from pathlib import Path

import pytest

from skyrim_amd import (aggregate, breeding, deliver, derived, ensemble, events, native, noise, points, regrid, scenarios, spectra, stochastic,
                        tracks, verify)
from skyrim_amd.dlwp import engine as dlwp
from skyrim_amd.fcn import engine as fcn
from skyrim_amd.fengwu import engine as fengwu
from skyrim_amd.fuxi import engine as fuxi
from skyrim_amd.graphcast import engine as graphcast
from skyrim_amd.pangu import engine as pangu
from skyrim_amd.sfno import engine as sfno

INCLUDE = Path(__file__).resolve().parent.parent / "include"
BINDINGS = {"pangu": pangu, "sfno": sfno, "graphcast": graphcast, "fcn": fcn, "dlwp": dlwp, "fuxi": fuxi, "fengwu": fengwu, "io": deliver,
            "ens": ensemble, "score": verify, "noise": noise, "track": tracks, "derive": derived, "regrid": regrid, "event": events,
            "agg": aggregate, "point": points, "gram": scenarios, "breed": breeding, "stoch": stochastic, "spec": spectra}


@pytest.fixture(params=list(BINDINGS))
def binding(request):
    return request.param, BINDINGS[request.param]


@pytest.fixture
def fresh(binding, monkeypatch):
    """The binding's handle cache emptied for the test and restored after it: the next ``load_library`` resolves and checks again."""
    monkeypatch.setattr(binding[1], "_lib", None)


def header(spec: native.Spec) -> str:
    return re.sub(r"/\*.*?\*/", "", (INCLUDE / f"{spec.stem}.h").read_text(), flags=re.S)


def test_header_symbols_equal_exports(binding):
    name, mod = binding
    spec = mod.SPEC
    assert spec.env == f"SKYRIM_{name.upper()}_LIB"                # the override variables bench.py and the tools set
    declared = set(re.findall(rf"\b({spec.prefix}_[a-z0-9_]+)\s*\(", header(spec)))
    assert declared == set(mod.EXPORTS) and len(declared) >= 2
    lib = mod.load_library()
    for s in sorted(declared):
        assert hasattr(lib, s), f"{s} declared in {spec.stem}.h but not exported"


def test_abi_version_is_the_headers(binding):
    _, mod = binding
    spec = mod.SPEC
    define = int(re.search(rf"#define {spec.prefix.upper()}_ABI_VERSION (\d+)", header(spec)).group(1))
    assert getattr(mod.load_library(), f"{spec.prefix}_abi_version")() == define == mod.ABI_VERSION


def test_missing_library_is_not_found(binding, fresh, monkeypatch, tmp_path):
    _, mod = binding
    monkeypatch.setenv(mod.SPEC.env, str(tmp_path / "missing.so"))
    with pytest.raises(RuntimeError, match="not found"):
        mod.load_library()


def test_abi_mismatch_is_refused(binding, fresh, monkeypatch):
    _, mod = binding
    monkeypatch.setattr(mod.SPEC, "abi", mod.SPEC.abi + 1)
    with pytest.raises(RuntimeError, match=rf"ABI {mod.ABI_VERSION}, this package binds ABI {mod.ABI_VERSION + 1}.*rebuild"):
        mod.load_library()


def test_error_codes_become_one_message():
    native.check(0, "anything", pangu.load_library())
    with pytest.raises(RuntimeError, match=r"^skpangu_step failed: bad argument or unsupported geometry \(code -1\)$"):
        native.check(-1, "skpangu_step", pangu.load_library())
    with pytest.raises(RuntimeError, match=r"^skfcn_mlp_run failed: HIP runtime error \(code -2\)$"):
        native.check(-2, "skfcn_mlp_run", fcn.load_library())
    with pytest.raises(RuntimeError, match=r"^sksfno_gemm_run failed: invalid argument \(code -1\)$"):     # no error-string entry point
        native.check(-1, "sksfno_gemm_run", sfno.load_library())
