"""Correlated noise fields without a GPU or the library: the tables, the NumPy restatement of the recursion, and the
refusals of the tables' builder, of the EnsembleSimulation keyword (before any handle is made) and of the CLI block."""
import numpy as np
import pytest

from helpers import digest
from hydromodel_amd.stepper import (noise_correlate, noise_correlation_breaks, noise_correlation_settings,
                                    noise_correlation_tables)


def test_tables_of_well_1():
    _, cols, _ = digest(1)
    z = cols.z
    assert cols.dim_d == 101 and cols.dz == 5.0
    a, b = noise_correlation_tables(z, 50.0)
    rho = np.exp(-5.0 / 50.0)
    assert a[0] == 0.0 and b[0] == 1.0
    assert np.all(a[1:] == rho) and np.all(b[1:] == np.sqrt(1.0 - rho * rho))
    assert np.all(np.abs(a[1:] ** 2 + b[1:] ** 2 - 1.0) <= 1e-15)
    # breaks: the first node at or below 50 and 200 cm, and nowhere else
    breaks = noise_correlation_breaks(cols.layers, z)
    assert breaks == (50.0, 200.0)                     # the soil's top is 0: no break of its own
    ab, bb = noise_correlation_tables(z, 50.0, breaks)
    at = [int(np.flatnonzero(z >= lv)[0]) for lv in breaks]
    assert np.flatnonzero(ab == 0.0).tolist() == [0] + at
    assert np.all(bb[ab == 0.0] == 1.0)
    keep = np.ones(101, dtype=bool)
    keep[at] = False
    assert np.array_equal(ab[keep], a[keep]) and np.array_equal(bb[keep], b[keep])
    # a depth between two nodes breaks at the node below it; one outside the column at none
    assert np.flatnonzero(noise_correlation_tables(z, 50.0, (z[0] + 52.0,))[0] == 0.0).tolist() == [0, 11]
    assert np.flatnonzero(noise_correlation_tables(z, 50.0, (z[0], z[-1] + 1.0, -3.0))[0] == 0.0).tolist() == [0]


def test_layers_of_a_well_with_soil_break_at_its_top():
    z = np.arange(101) * 5.0
    assert noise_correlation_breaks((20.0, 50.0, 200.0, 500.0), z) == (20.0, 50.0, 200.0)
    assert noise_correlation_breaks((0.0, 50.0, 2000.0, 500.0), z) == (50.0,)      # an interface below the column: none


def test_restatement_is_the_cholesky_factor_of_the_exponential_covariance():
    _, cols, _ = digest(1)
    z, D, ell = cols.z, cols.dim_d, 50.0
    for breaks in ((), (50.0, 200.0)):
        a, b = noise_correlation_tables(z, ell, breaks)
        T = noise_correlate(np.eye(D), a, b).T          # column j: the field of the unit vector e_j
        assert np.all(np.triu(T, 1) == 0.0)
        block = np.cumsum(a == 0.0)                     # nodes between two breaks share a block
        want = np.where(block[:, None] == block[None, :], np.exp(-np.abs(z[:, None] - z[None, :]) / ell), 0.0)
        assert np.max(np.abs(T @ T.T - want)) <= 1e-12
        assert np.all(np.abs(np.diag(T @ T.T) - 1.0) <= 1e-12)


def test_all_break_table_returns_xi_to_the_bit():
    xi = np.random.default_rng(3).standard_normal((5, 37))
    xi[0, 3], xi[1, 4] = -0.0, 5e-324
    z = noise_correlate(xi, np.zeros(37), np.ones(37))
    assert z.tobytes() == xi.tobytes()
    # ... and a table is applied in the stated order: one product, one product, one sum, down the last axis
    a, b = noise_correlation_tables(np.arange(37) * 5.0, 20.0, (60.0,))
    got = noise_correlate(xi, a, b)
    for m in range(5):
        zp = xi[m, 0]
        for i in range(1, 37):
            zp = xi[m, i] if a[i] == 0.0 else (a[i] * zp) + (b[i] * xi[m, i])
            assert got[m, i] == zp


@pytest.mark.parametrize("length", [0.0, -5.0, float("nan"), float("inf"), True, "50", None])
def test_tables_refuse_a_bad_length(length):
    with pytest.raises(ValueError, match="length_cm"):
        noise_correlation_tables(np.arange(10) * 5.0, length)


def test_tables_refuse_a_bad_grid_or_break():
    with pytest.raises(ValueError, match="strictly increasing"):
        noise_correlation_tables([0.0, 5.0, 5.0], 50.0)
    with pytest.raises(ValueError, match="not finite"):
        noise_correlation_tables(np.arange(10) * 5.0, 50.0, (float("nan"),))
    with pytest.raises(ValueError, match="too long"):
        noise_correlation_tables(np.arange(10) * 5.0, 1e18)


def test_settings_of_the_keyword():
    assert noise_correlation_settings(None) is None
    assert noise_correlation_settings({"length_cm": 50}) == (50.0, False)
    assert noise_correlation_settings({"length_cm": 25.0, "layers": True}) == (25.0, True)
    for bad, msg in ((50.0, "must be a dict"), ({"length_cm": 50.0, "Layers": True}, "unknown key"),
                     ({"layers": True}, "needs 'length_cm'"), ({"length_cm": 50.0, "layers": 1}, "must be true or false"),
                     ({"length_cm": True}, "length_cm"), ({"length_cm": 0.0}, "length_cm")):
        with pytest.raises(ValueError, match=msg):
            noise_correlation_settings(bad)


def test_ensemble_keyword_refusals_come_before_any_handle(monkeypatch):
    from hydromodel_amd import ensemble
    from hydromodel_amd.ensemble import EnsembleSimulation, SweepSimulation

    def no_handle(*a, **k):
        raise AssertionError("a handle was made")

    monkeypatch.setattr(ensemble, "EnsembleStepper", no_handle)
    _, cols, forcing = digest(1)
    psi0 = np.zeros(cols.dim_d)
    corr = {"length_cm": 50.0, "layers": True}
    with pytest.raises(ValueError, match="noise_correlation serves the Philox noise source"):
        EnsembleSimulation(cols, forcing, 8, psi0=psi0, noise="numpy", noise_correlation=corr)
    with pytest.raises(ValueError, match="noise_correlation and filter_rejuvenation exclude each other"):
        EnsembleSimulation(cols, forcing, 8, psi0=psi0, filter_stride=48, filter_sigma_cm=10.0, filter_rejuvenation=0.95,
                           noise_correlation=corr)
    with pytest.raises(ValueError, match="length_cm"):
        EnsembleSimulation(cols, forcing, 8, psi0=psi0, noise_correlation={"length_cm": -1.0})
    with pytest.raises(ValueError, match="unknown key"):
        EnsembleSimulation(cols, forcing, 8, psi0=psi0, noise_correlation={"length_cm": 50.0, "breaks": [1.0]})
    with pytest.raises(ValueError, match="noise_correlation and filter_rejuvenation exclude each other"):
        SweepSimulation([cols, cols], forcing, 8, psi0=np.zeros((2, cols.dim_d)), filter_stride=48, filter_sigma_cm=10.0,
                        filter_rejuvenation=0.95, noise_correlation=corr)


def test_cli_block():
    from hydromodel_amd.cli import noise_correlation_settings as block
    assert block({"Members": 8}) is None
    assert block({"Noise_Correlation": {"Length_cm": 50}}) == {"length_cm": 50.0, "layers": False}
    assert block({"Noise_Correlation": {"Length_cm": 25.5, "Layers": True}, "Noise": "philox",
                  "Filter": {"Stride": 48, "Sigma_cm": 10.0}}) == {"length_cm": 25.5, "layers": True}
    for ens, msg in (({"Noise_Correlation": 50.0}, "Noise_Correlation = 50.0 must be an object"),
                     ({"Noise_Correlation": {"Length_cm": 50.0, "Breaks": []}}, r"unknown keys \['Breaks'\]"),
                     ({"Noise_Correlation": {"Length_cm": True}}, "Length_cm = True must be a finite number > 0"),
                     ({"Noise_Correlation": {"Length_cm": 0}}, "Length_cm = 0 must be a finite number > 0"),
                     ({"Noise_Correlation": {"Length_cm": -2.5}}, "Length_cm = -2.5 must be a finite number > 0"),
                     ({"Noise_Correlation": {"Layers": True}}, "Length_cm = None must be a finite number > 0"),
                     ({"Noise_Correlation": {"Length_cm": 50.0, "Layers": 1}}, "Layers = 1 must be true or false"),
                     ({"Noise_Correlation": {"Length_cm": 50.0}, "Noise": "numpy"}, "Noise_Correlation with \"Noise\": 'numpy'"),
                     ({"Noise_Correlation": {"Length_cm": 50.0}, "Filter": {"Stride": 48, "Sigma_cm": 10.0, "Rejuvenation": 0.95}},
                      "Noise_Correlation and Filter.Rejuvenation exclude each other")):
        with pytest.raises(ValueError, match=msg):
            block(ens)


def test_cli_refuses_a_bad_block_with_exit_status_1(tmp_path, capsys):
    import json
    from helpers import cli_params
    from hydromodel_amd import cli
    params = cli_params(tmp_path)
    params["Output_Name"] = "Bad"
    params["Ensemble"] = {"Members": 8, "Days": 1, "Noise_Correlation": {"Length_cm": 50.0}, "Noise": "numpy"}
    (tmp_path / "bad.json").write_text(json.dumps(params))
    with pytest.raises(SystemExit) as status:
        cli.run_cli(["berkeley_hydro_main.py", "--params", str(tmp_path / "bad.json")])
    assert status.value.code == 1
    assert "Noise_Correlation with \"Noise\": 'numpy'" in capsys.readouterr().out
    assert not list(tmp_path.glob("Bad_ensemble.*"))
