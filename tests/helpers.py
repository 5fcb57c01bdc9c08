"""Shared builders for the tests: wells, digests, oracle columns."""
from functools import lru_cache
from pathlib import Path

import numpy as np

from hydromodel_amd.digest import ColumnTables, ForcingDigest
from hydromodel_amd.synthetic import default_parameters, synthetic_forcing_frame, synthetic_well

GOLDEN = Path(__file__).resolve().parent / "golden"

# well 1 of the reference's site_information.json (D = 101), the two synthetic wells and the reference's deepest well (D = 581)
WELLS = {1: {"soil": 0.0, "saprolite": 50.0, "weathered": 200.0, "max_depth": 500.0, "sat_depth": 100.0},
         200: synthetic_well(200), 300: synthetic_well(300),
         401: {"soil": 0.0, "saprolite": 50.0, "weathered": 200.0, "max_depth": 2000.0, "sat_depth": 125.0},   # well 10, the
         # one the reference's input_parameters.json selects
         581: synthetic_well(581)}      # = well 14 of the reference's site_information.json (max_depth 2 900 cm), its deepest


@lru_cache(maxsize=None)
def forcing_frame(n_years=1):
    return synthetic_forcing_frame(n_years)


@lru_cache(maxsize=None)
def digest(well, model="vrettas_fung", n_years=1):
    params = default_parameters()
    params["Hydrological_Model"]["Name"] = model
    cols = ColumnTables(params, WELLS[well])
    forcing = ForcingDigest(params, forcing_frame(n_years), cols)
    return params, cols, forcing


def forcing_with_row(forcing, row, precip, atm, daylight, wtd_obs, wet=None):
    """A copy of the digest whose row `row` carries the given arguments (the golden states were evaluated with
    explicit (hour, precip, atm, wtd) rather than a row of the synthetic forcing); never a refresh row.
    `wet`: the row's wet-season flag (None: as the forcing has it)."""
    import copy
    f = copy.copy(forcing)
    for name in ("precip", "atm", "daylight", "wtd_obs", "refresh", "wet_season"):
        setattr(f, name, np.array(getattr(forcing, name)))
    f.precip[row], f.atm[row], f.daylight[row], f.wtd_obs[row], f.refresh[row] = precip, atm, int(daylight), wtd_obs, 0
    if wet is not None:
        f.wet_season[row] = int(wet)
    return f


@lru_cache(maxsize=None)
def points():
    """Non-default parameter points of tests/golden/points.json (fixtures g1p/g2p/g34p, synthetic well D=200)."""
    import json
    with open(GOLDEN / "points.json") as fh:
        return json.load(fh)


@lru_cache(maxsize=None)
def digest_point(tag, model="vrettas_fung", well=200):
    params = default_parameters()
    params["Hydrological_Model"]["Name"] = model
    for section, values in points()[tag].items():
        params[section].update(values)
    cols = ColumnTables(params, WELLS[well])
    forcing = ForcingDigest(params, forcing_frame(1), cols)
    return params, cols, forcing


@lru_cache(maxsize=None)
def golden(name):
    return dict(np.load(GOLDEN / name))


def rel_err(a, b, floor=1.0):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b) / np.maximum(floor, np.abs(b)))) if a.size else 0.0


def cli_params(tmp_path):
    """The CLI's parameter dict on the synthetic well (D = 200) and one year of synthetic forcing, files under tmp_path."""
    from hydromodel_amd.synthetic import write_forcing_csv, write_site_information
    params = default_parameters()
    params["Site_Information"] = str(write_site_information(tmp_path / "site.json", {10: WELLS[200]}))
    params["Data_Filename"] = str(write_forcing_csv(tmp_path / "forcing.csv", 1))
    return params


def run_cli_ranks(tmp_path, name, params, gpus):
    """berkeley_hydro_main.py on `params` in tmp_path/name with `gpus` ranks sharing card 0 over gloo; returns the
    datasets of <name>_ensemble.h5 and the printed output."""
    import json
    import os
    import subprocess
    import sys
    from hydromodel_amd.simulation import loadResults
    d = tmp_path / name
    d.mkdir()
    (d / "p.json").write_text(json.dumps(dict(params, Output_Name=name)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    env.update(HYDROCOL_DIST_BACKEND="gloo", HYDROCOL_SHARE_DEVICE="1")
    cmd = [sys.executable, str(GOLDEN.parent.parent / "berkeley_hydro_main.py"), "--params", str(d / "p.json")]
    if gpus > 1:
        cmd += ["--gpus", str(gpus)]
    r = subprocess.run(cmd, cwd=d, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return loadResults(d / f"{name}_ensemble.h5"), r.stdout
