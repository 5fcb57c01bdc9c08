"""The covariance of theta(z) and the water table on the host (include/hydrocol.h hc_set_theta_cov): the NumPy restatement
of the table against a brute-force loop over Python ints, the finished covariances against the exact rational, the
worst-case row, the packed index, the CLI's "Covariance" block with its refusals, the binding's names and
``layer_std_cm`` against the direct sigma of dz sum theta.  No GPU."""
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from hydromodel_amd.stepper import (THETA_COV_MAX_MEMBERS, THETA_COV_MAX_WORDS, THETA_COV_SCALE, theta_cov_finish,
                                    theta_cov_index, theta_cov_of, theta_cov_shape, theta_sensor_gain)

REPO = Path(__file__).resolve().parents[1]
N, D = 37, 10


def _members(seed=4):
    """37 members x 10 nodes: member 3 holds a NaN at node 4 (a multiple of no stride but 1), member 5 a theta of 1.0 at
    node 0, member 7 a NaN at node 0 (selected by every stride)."""
    rng = np.random.default_rng(seed)
    theta = rng.uniform(0.05, 0.55, size=(N, D))
    theta[3, 4] = np.nan
    theta[5, 0] = 1.0
    theta[7, 0] = np.nan
    wtd = rng.integers(0, D, size=N)
    return theta, wtd


def _brute(theta, wtd, s):
    """The table's definition, member by member, in Python ints."""
    nodes = list(range(0, theta.shape[1], s))
    E = len(nodes) + 1
    count, outside, S1, S2 = 0, 0, [0] * E, {}
    for m in range(theta.shape[0]):
        sel = [float(theta[m, i]) for i in nodes]
        if not all(0.0 <= t <= 1.0 for t in sel):
            outside += 1
            continue
        q = [int(np.rint(t * 2.0 ** 20)) for t in sel] + [int(wtd[m])]
        count += 1
        for a in range(E):
            S1[a] += q[a]
            for b in range(a, E):
                S2[a, b] = S2.get((a, b), 0) + q[a] * q[b]
    return count, outside, S1, S2, E


@pytest.mark.parametrize("s", [1, 3, 10])
def test_the_restatement_equals_a_brute_force_loop_over_python_ints(s):
    theta, wtd = _members()
    words, outside = theta_cov_of(theta, wtd, s)
    count, out, S1, S2, E = _brute(theta, wtd, s)
    n, E_, W = theta_cov_shape(D, s)
    assert (n, E_) == (-(-D // s), E) and words.shape == (W,) and words.dtype == np.int64
    assert W == 1 + E + E * (E + 1) // 2
    assert outside == out == (2 if s == 1 else 1) and int(words[0]) == count == N - out
    assert [int(v) for v in words[1:1 + E]] == S1
    for (a, b), v in S2.items():
        assert int(words[1 + E + theta_cov_index(a, b, E)]) == v, (a, b)
    assert int(words[1 + theta_cov_index(0, 0, E) + E]) >= 1 << 40          # member 5's theta = 1.0: q = 2^20 exactly


@pytest.mark.parametrize("E", [1, 2, 5, 68, 201])
def test_the_packed_index_is_a_bijection_onto_the_triangle(E):
    idx = [theta_cov_index(a, b, E) for a in range(E) for b in range(a, E)]
    assert idx == list(range(E * (E + 1) // 2))                             # row-major, dense, each once


def _ulps(got, want):
    """|got - want| in units of want's last place."""
    return abs(Fraction(got) - Fraction(want)) / Fraction(np.spacing(abs(want)) if want else np.spacing(0.0))


def test_finish_is_within_two_ulp_of_the_correctly_rounded_exact_rational():
    """theta_cov_finish rounds twice on a theta-theta entry (the exact integer numerator to a double, the division by
    c^2; the 2^-40 is exact) where the correctly rounded value rounds once: 2 ulp.  dz is a power of two here, so that
    the entries with the water table are scaled exactly too and the same bound holds for them."""
    theta, wtd = _members(seed=11)
    dz = 0.5
    for s in (1, 3):
        words, _ = theta_cov_of(theta, wtd, s)
        fin = theta_cov_finish(words, dz, s, D)
        count, _, S1, S2, E = _brute(theta, wtd, s)
        n = E - 1
        scale = [Fraction(1, 1 << 20)] * n + [Fraction(dz)]
        for a in range(E):
            for b in range(a, E):
                exact = Fraction(count * S2[a, b] - S1[a] * S1[b], count * count) * scale[a] * scale[b]
                want = float(exact)                                         # Fraction -> float rounds correctly
                got = (fin["theta_cov"][a, b] if b < n else fin["wtd_theta_cov_cm"][a] if a < n else fin["wtd_var_cm2"])
                assert _ulps(float(got), want) <= 2, (s, a, b, float(got), want)
                if b < n:
                    assert fin["theta_cov"][b, a] == fin["theta_cov"][a, b]
        assert int(fin["count"]) == count
        # population moments, like the profile statistics' sigma
        ok = np.all((theta[:, ::s] >= 0) & (theta[:, ::s] <= 1), axis=1)
        q = np.rint(theta[ok][:, ::s] * 2.0 ** 20) / 2.0 ** 20
        assert np.allclose(fin["theta_cov"], np.cov(q.T, bias=True).reshape(n, n), rtol=1e-9, atol=1e-18)
        assert np.allclose(fin["wtd_var_cm2"], np.var(wtd[ok] * dz), rtol=1e-12)


def test_a_large_count_keeps_the_numerator_exact():
    """c = 2^22 - 3 members on two columns whose c S2 - S1 S1 needs more than 64 bits: the split-word route still gives the
    correctly rounded covariance within 2 ulp."""
    c = (1 << 22) - 3
    n, E, W = theta_cov_shape(1, 1)
    k = c // 3                                                              # k members at q = 2^20, the rest at 1
    hi, lo = 1 << 20, 1
    S1 = [k * hi + (c - k) * lo, k * 5 + (c - k) * 0]
    S2 = {(0, 0): k * hi * hi + (c - k), (0, 1): k * hi * 5, (1, 1): k * 25}
    words = np.array([c, *S1, S2[0, 0], S2[0, 1], S2[1, 1]], dtype=np.int64)
    assert abs(c * S2[0, 0] - S1[0] * S1[0]) > 1 << 64
    fin = theta_cov_finish(words, 1.0, 1, 1)
    got = [fin["theta_cov"][0, 0], fin["wtd_theta_cov_cm"][0], fin["wtd_var_cm2"]]
    scale = [Fraction(1, 1 << 40), Fraction(1, 1 << 20), Fraction(1)]
    for g, (a, b), sc in zip(got, [(0, 0), (0, 1), (1, 1)], scale):
        want = float(Fraction(c * S2[a, b] - S1[a] * S1[b], c * c) * sc)
        assert _ulps(float(g), want) <= 2, (a, b, float(g), want)


def test_the_worst_case_row_does_not_overflow():
    """Every q = 2^20 on 2^22 members: S2 = 2^62 fits an int64, and the covariance of a constant is exactly 0."""
    n, E, W = theta_cov_shape(6, 1)
    c, q = THETA_COV_MAX_MEMBERS, 1 << THETA_COV_SCALE
    assert c == 1 << 22 and c * q * q == 1 << 62 < np.iinfo(np.int64).max
    words = np.zeros(W, dtype=np.int64)
    words[0], words[1:1 + E], words[1 + E:] = c, c * q, c * q * q
    fin = theta_cov_finish(words, 2.5, 1, 6)
    assert np.all(fin["theta_cov"] == 0.0) and np.all(fin["wtd_theta_cov_cm"] == 0.0) and fin["wtd_var_cm2"] == 0.0
    assert np.all(fin["theta_mean"] == 1.0) and np.isnan(fin["theta_wtd_corr"]).all() and np.isnan(fin["theta_corr"]).all()
    # half the members at 0: the largest variance a column can have, 2^38 in units of q^2
    words[1:1 + E], words[1 + E:] = c // 2 * q, c // 2 * q * q
    fin = theta_cov_finish(words, 2.5, 1, 6)
    assert np.all(fin["theta_cov"] == 0.25) and np.all(fin["theta_corr"] == 1.0)
    # the restatement refuses what the library refuses
    with pytest.raises(ValueError, match="exceed 2\\^22"):
        theta_cov_of(np.zeros((c + 1, 1)), np.zeros(c + 1, dtype=np.int64), 1)


def test_an_empty_row_is_nan_and_a_constant_column_has_no_correlation():
    theta = np.full((5, 4), 0.25)
    theta[:, 1] = [0.1, 0.2, 0.3, 0.4, 0.5]
    wtd = np.array([1, 2, 3, 3, 2])
    words, _ = theta_cov_of(theta, wtd, 1)
    table = np.stack([words, np.zeros_like(words)])
    fin = theta_cov_finish(table, 2.0, 1, 4)
    assert fin["theta_cov"].shape == (2, 4, 4) and fin["count"].tolist() == [5, 0]
    assert np.isnan(fin["theta_cov"][1]).all() and np.isnan(fin["wtd_var_cm2"][1]) and np.isnan(fin["theta_mean"][1]).all()
    assert fin["theta_cov"][0, 0, 0] == 0.0 and np.isnan(fin["theta_wtd_corr"][0, 0]) and np.isfinite(fin["theta_wtd_corr"][0, 1])
    assert np.isnan(fin["theta_corr"][0, 0, 1]) and fin["theta_corr"][0, 1, 1] == 1.0
    gain = theta_sensor_gain(fin, 0.02)
    assert gain.shape == (2, 4) and gain[0, 0] == 0.0 and 0.0 < gain[0, 1] < 1.0 and np.isnan(gain[1]).all()
    const = theta_cov_finish(theta_cov_of(theta, np.full(5, 3), 1)[0], 2.0, 1, 4)
    assert np.isnan(theta_sensor_gain(const, 0.02)).all()                   # var wtd = 0


def test_layer_std_matches_the_direct_sigma_of_the_layers_storage():
    """At node stride 1 dz sqrt(1' C 1) over a layer's nodes is the population sigma of dz sum theta on the same quantised
    theta: both are formed from 20-bit integers, so they agree to rounding."""
    from hydromodel_amd.ensemble import _Run
    rng = np.random.default_rng(2)
    Dn, dz = 40, 2.5
    front = rng.integers(5, 35, size=200)
    theta = np.where(np.arange(Dn)[None, :] < front[:, None], 0.2, 0.45) + rng.uniform(0, 0.01, size=(200, Dn))
    words, _ = theta_cov_of(theta, front, 1)

    class Cols:
        z, dim_d = 10.0 + dz * np.arange(Dn), Dn
    Cols.dz = dz
    run = _Run.__new__(_Run)
    run.cols, run.theta_cov_stride, run.profile_stride = Cols, 1, 48
    layers = [(10.0, 60.0), (10.0, 110.0), (35.0, 37.5)]
    got = run.layer_std_cm(layers, table=words[None])
    q = np.rint(theta * 2.0 ** 20) / 2.0 ** 20
    for l, (top, bottom) in enumerate(layers):
        i0, i1 = int(round((top - 10.0) / dz)), int(round((bottom - 10.0) / dz))
        want = np.std(dz * q[:, i0:i1].sum(axis=1))
        assert got.shape == (1, 3) and abs(got[0, l] - want) <= 1e-9 * want, (l, got[0, l], want)
    # the nodes covary: the root of the summed variances misses the first two layers' spread
    var = np.einsum("ii->i", run.theta_covariance(words[None])["theta_cov"][0])
    assert got[0, 1] > 2.0 * dz * np.sqrt(var[:40].sum())
    run.theta_cov_stride = 2
    with pytest.raises(ValueError, match="theta_cov_stride = 1"):
        run.layer_std_cm(layers, table=words[None])


# ---- the CLI's block -----------------------------------------------------------------------------------------------------
def test_the_cli_key_parses():
    from hydromodel_amd.cli import RunSettings, covariance_check, covariance_settings
    assert covariance_settings({"Members": 8}) is None and "theta_cov_stride" not in RunSettings(cov=None).kwargs()
    assert covariance_settings({"Profiles": 48, "Covariance": {"Node_Stride": 4, "Sensor_Sigma": 0.02}}) == (4, 0.02)
    assert covariance_settings({"Profiles": 1, "Covariance": {}}) == (1, None)
    assert RunSettings(cov=(4, 0.02)).kwargs()["theta_cov_stride"] == 4
    assert covariance_check((4, 0.02), 200, 17521, 48) == 50 and covariance_check(None, 200, 17521, 48) is None
    assert covariance_check((200, None), 200, 17521, 1) == 1


@pytest.mark.parametrize("ens, message", [
    ({"Profiles": 48, "Covariance": 4}, "Covariance = 4 must be an object"),
    ({"Profiles": 48, "Covariance": [4]}, "must be an object"),
    ({"Profiles": 48, "Covariance": {"Stride": 4}}, r"unknown keys \['Stride'\]"),
    ({"Profiles": 48, "Covariance": {"Node_Stride": True}}, "Node_Stride = True must be a whole number"),
    ({"Profiles": 48, "Covariance": {"Node_Stride": 0}}, "Node_Stride = 0 must be a whole number"),
    ({"Profiles": 48, "Covariance": {"Node_Stride": 2.5}}, "Node_Stride = 2.5 must be a whole number"),
    ({"Profiles": 48, "Covariance": {"Sensor_Sigma": True}}, "Sensor_Sigma = True must be a number > 0"),
    ({"Profiles": 48, "Covariance": {"Sensor_Sigma": 0}}, "Sensor_Sigma = 0 must be a number > 0"),
    ({"Profiles": 48, "Covariance": {"Sensor_Sigma": "0.02"}}, "must be a number > 0"),
    ({"Covariance": {"Node_Stride": 4}}, "Covariance needs the profile rows: Profiles = 0"),
    ({"Profiles": True, "Covariance": {}}, "Covariance needs the profile rows: Profiles = True"),
])
def test_the_cli_refusals_fire_with_their_messages(ens, message):
    from hydromodel_amd.cli import covariance_settings
    with pytest.raises(ValueError, match=message):
        covariance_settings(ens)


def test_the_cli_refuses_a_dataset_above_two_gib_with_the_librarys_advice():
    from hydromodel_amd.cli import covariance_check
    advice = "take a larger node stride or a larger profile stride"
    with pytest.raises(ValueError, match=f"17521 rows of 300 x 300 float64.*at most 2 GiB.*{advice}"):
        covariance_check((1, None), 300, 17521, 1)
    assert covariance_check((1, None), 300, 17521, 48) == 300               # 366 rows x 300 x 300 x 8 = 0.26 GB
    with pytest.raises(ValueError, match=advice):                           # a sweep's leading [P] axis counts
        covariance_check((1, None), 300, 17521, 48, P=9)
    with pytest.raises(ValueError, match="Node_Stride = 301 exceeds the column's 300 nodes"):
        covariance_check((301, None), 300, 17521, 48)
    # the library's message gives the same advice
    hip = (REPO / "hydromodel_amd" / "csrc" / "hydrocol.hip").read_text()
    assert re.search(r"HC_THETA_COV_MAX_WORDS \(take a larger node stride or a \"\s*\"larger profile stride\)", hip)
    assert THETA_COV_MAX_WORDS == 1 << 30


def test_the_new_names_are_in_the_binding_and_in_the_header():
    from hydromodel_amd import _lib
    header = (REPO / "include" / "hydrocol.h").read_text()
    names = ["hc_set_theta_cov", "hc_get_theta_cov_layout", "hc_get_theta_cov_words", "hc_get_theta_cov",
             "hc_set_theta_cov_tables", "hc_export_theta_cov", "hc_reset_theta_cov", "hc_get_theta_cov_outside"]
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "hc_set_theta_hist" in v)
    for name in names:
        assert name in table, name
        assert re.search(rf"^int {name}\(hc_handle \*h", header, re.M), name
    assert "#define HC_THETA_COV_MAX_WORDS (1LL << 30)" in header and "#define HC_THETA_COV_MAX_MEMBERS (1LL << 22)" in header
    assert "HYDROCOL_COV_CHUNK_MEMBERS" in header
    from hydromodel_amd.stepper import EnsembleStepper
    for method in ("set_theta_cov", "theta_cov_table", "set_theta_cov_table", "reset_theta_cov", "theta_cov_outside"):
        assert callable(getattr(EnsembleStepper, method))
