"""The fixed-lag smoother of the water table by ancestry, host side (include/hydrocol.h hc_set_filter_smoother): the NumPy
restatement on a genealogy written out by hand; K = 0; the identity ancestry; the monotone-id argument the emit kernel's
neighbour count rests on; skipped rows; the flush; a ring that wraps; the CLI's "Smoother" block and its refusals; the
exported names.  No GPU."""
import numpy as np
import pytest

from hydromodel_amd import _lib, cli
from hydromodel_amd.stepper import (filter_smoother_config, filter_smoother_of, filter_smoother_settings,
                                    filter_smoother_summary)

NAMES = ("hc_set_filter_smoother", "hc_get_filter_smoother_layout", "hc_get_filter_smoother_hist",
         "hc_set_filter_smoother_hist_table", "hc_get_filter_smoother_paths", "hc_set_filter_smoother_paths",
         "hc_get_filter_smoother_ring", "hc_set_filter_smoother_ring", "hc_filter_smoother_flush",
         "hc_reset_filter_smoother")


def _systematic(rng, n):
    """a non-decreasing ancestry of n slots, as systematic resampling gives: the slots of random positive weights"""
    w = rng.random(n) ** 4 + 1e-9
    edges = np.cumsum(w) / w.sum()
    return np.minimum(np.searchsorted(edges, (rng.random() + np.arange(n)) / n), n - 1).astype(np.int64)


# ---- the genealogy written out by hand: 8 members, D = 6, stride 1, K = 2, resamplings on rows 2, 3 and 4 ----------------
W = {1: [0, 1, 2, 3, 4, 5, 0, 1], 2: [1, 1, 2, 2, 3, 3, 4, 4], 3: [5, 4, 3, 2, 1, 0, 5, 4], 4: [0, 0, 1, 1, 2, 2, 3, 3],
     5: [2, 2, 2, 2, 3, 3, 3, 3]}
ANC = {2: [0, 0, 1, 1, 2, 5, 5, 7], 3: [1, 1, 1, 3, 3, 3, 6, 6], 4: [0, 0, 0, 0, 4, 4, 4, 7]}


def test_hand_written_genealogy():
    got = filter_smoother_of(W, ANC, 1, 2, 8, 6, np.zeros(6, dtype=np.int32), 5)
    hist = np.zeros((1, 6, 6), dtype=np.int32)
    hist[0, 1] = [3, 3, 0, 0, 0, 2]          # row 1 through the ancestries of rows 2 and 3: members 0, 0, 0, 1, 1, 1, 5, 5
    hist[0, 2] = [0, 7, 0, 1, 0, 0]          # row 2 through those of rows 2, 3 and 4
    hist[0, 3] = [0, 0, 3, 0, 4, 1]          # row 3 through those of rows 3 and 4; nothing is resampled on row 5
    paths = np.array([[[0, -1], [3, 3], [3, 4], [3, 5], [0, -1], [0, -1]]], dtype=np.int64)
    assert got["hist"].dtype == np.int32 and got["paths"].dtype == np.int64
    assert np.array_equal(got["hist"], hist) and np.array_equal(got["paths"], paths)
    assert got["ring_rows"].tolist() == [-1, 4, 5]
    assert got["ring_w"].tolist() == [[0] * 8, [0, 0, 0, 0, 2, 2, 2, 3], W[5]]
    assert got["ring_id"].tolist() == [[0] * 8, [0, 0, 0, 0, 4, 4, 4, 7], list(range(8))]
    hist[0, 4] = [4, 0, 3, 1, 0, 0]          # the flush: row 4 as the ancestry of row 4 left it, row 5 as it was solved
    hist[0, 5] = [0, 0, 4, 4, 0, 0]
    paths[0, 4], paths[0, 5] = (3, 5), (8, 5)
    assert np.array_equal(got["hist_flushed"], hist) and np.array_equal(got["paths_flushed"], paths)


def test_lag_zero_is_the_bincount_through_the_ancestors():
    rng = np.random.default_rng(1)
    T, N, D = 25, 30, 9
    w = rng.integers(0, D + 2, size=(T, N))                       # some indices >= D: they go to no bin
    anc = {r: _systematic(rng, N) for r in (6, 12, 18, 24)}
    got = filter_smoother_of(w, anc, 3, 0, N, D, np.zeros(T, dtype=np.int32), 24)
    for j in range(1, 9):
        r = 3 * j
        v = w[r][anc[r]] if r in anc else w[r]
        assert np.array_equal(got["hist"][0, j], np.bincount(v[v < D], minlength=D)), r
        assert got["paths"][0, j].tolist() == [np.unique(anc[r]).size if r in anc else N, r]
    assert (got["ring_rows"] == -1).all() and np.array_equal(got["hist"], got["hist_flushed"])


def test_identity_ancestry_is_the_forecast_with_every_path():
    rng = np.random.default_rng(2)
    T, Np, P, D = 31, 7, 3, 5
    w = rng.integers(0, D, size=(T, P * Np))
    anc = {r: np.arange(P * Np) for r in (10, 20, 30)}
    got = filter_smoother_of(w, anc, 5, 2, Np, D, np.zeros(T, dtype=np.int32), 30)
    for j in range(1, 7):
        for p in range(P):
            assert np.array_equal(got["hist_flushed"][p, j], np.bincount(w[5 * j, p * Np:(p + 1) * Np], minlength=D))
            assert got["paths_flushed"][p, j].tolist() == [Np, min(5 * j + 10, 30)]


def test_composed_ancestries_keep_the_ids_sorted_and_neighbours_count_them():
    rng = np.random.default_rng(3)
    Np, P = 97, 3
    ids = np.tile(np.arange(Np), P)
    for _ in range(12):
        anc = np.concatenate([p * Np + _systematic(rng, Np) for p in range(P)])
        ids = ids[anc]
        for p in range(P):
            v = ids[p * Np:(p + 1) * Np]
            assert (np.diff(v) >= 0).all()
            assert 1 + int((v[1:] != v[:-1]).sum()) == np.unique(v).size
    # ... and the restatement's ring shows the same after three resamplings
    T, D = 40, 11
    w = rng.integers(0, D, size=(T, P * Np))
    anc = {r: np.concatenate([p * Np + _systematic(rng, Np) for p in range(P)]) for r in (12, 24, 36)}
    got = filter_smoother_of(w, anc, 6, 4, Np, D, np.zeros(T, dtype=np.int32), 36)
    live = got["ring_rows"] >= 0
    assert live.sum() == 4
    assert (np.diff(got["ring_id"][live].reshape(-1, P, Np), axis=-1) >= 0).all()
    assert got["paths"][:, 2, 0].max() < Np                           # row 12 has been through three resamplings


def test_a_skipped_record_row_is_never_emitted():
    rng = np.random.default_rng(4)
    T, N, D = 31, 12, 6
    w = rng.integers(0, D, size=(T, N))
    obs = np.zeros(T, dtype=np.int32)
    obs[[10, 25]] = -1
    anc = {r: _systematic(rng, N) for r in (15, 30)}
    got = filter_smoother_of(w, anc, 5, 1, N, D, obs, 30)
    for j, r in enumerate(range(0, 31, 5)):
        empty = r in (0, 10, 25)
        assert (got["hist_flushed"][0, j].sum() == 0) == empty, r
        assert (got["paths_flushed"][0, j].tolist() == [0, -1]) == empty, r
    assert got["paths_flushed"][0, 4].tolist()[1] == 25               # row 20 was emitted on row 25, observed or not


def test_flush_conditions_every_pending_row_on_the_last_row():
    rng = np.random.default_rng(5)
    T, N, D = 50, 10, 4
    w = rng.integers(0, D, size=(T, N))
    got = filter_smoother_of(w, {12: _systematic(rng, N)}, 4, 5, N, D, np.zeros(T, dtype=np.int32), 22)
    assert (got["paths"][0, :, 1] == -1).all() and got["hist"].sum() == 0          # j - K = 0 on row 20: nothing emitted
    assert sorted(got["ring_rows"].tolist()) == [-1, 4, 8, 12, 16, 20]
    assert got["paths_flushed"][0, 1:6, 1].tolist() == [22] * 5 and (got["paths_flushed"][0, 6:, 1] == -1).all()
    summary_lag = 22 - np.arange(1, 6) * 4
    assert (got["paths_flushed"][0, 1:6, 1] - np.arange(1, 6) * 4).tolist() == summary_lag.tolist()


def test_a_ring_that_wraps():
    rng = np.random.default_rng(6)
    T, N, D, K = 41, 16, 5, 2
    w = rng.integers(0, D, size=(T, N))
    anc = {r: _systematic(rng, N) for r in range(4, 41, 4)}
    got = filter_smoother_of(w, anc, 2, K, N, D, np.zeros(T, dtype=np.int32), 40)   # 20 records through 3 planes
    for j in range(1, 19):
        v = w[2 * j]
        for r in range(2 * j, 2 * (j + K) + 1):                   # the resamplings from its own row to its conditioning row
            if r in anc:
                v = v[anc[r]]
        assert np.array_equal(got["hist"][0, j], np.bincount(v, minlength=D)), j
        assert got["paths"][0, j, 1] == 2 * (j + K)
    assert (got["paths"][0, 19:, 1] == -1).all() and sorted(got["ring_rows"].tolist()) == [-1, 38, 40]


def test_settings_of_the_setter_and_the_constructor():
    assert filter_smoother_settings(6, 4) == (6, 4) and filter_smoother_settings(0, 9) == (0, 0)
    for bad in ((-1, 0), (6, 65), (6, -1), (True, 0), (6, 1.0)):
        with pytest.raises(ValueError):
            filter_smoother_settings(*bad)
    assert filter_smoother_config(None) is None and filter_smoother_config({"stride": 0}) is None
    assert filter_smoother_config({"stride": 48, "lag_rows": 480}) == (48, 10)
    for bad in ({"stride": 48, "lag_rows": 50}, {"stride": 1, "lag_rows": 65}, {"lag_rows": 3}, {"stride": 2, "lag": 2},
                [48, 480], {"stride": True}):
        with pytest.raises(ValueError):
            filter_smoother_config(bad)


def _ens(smoother, **filt):
    return {"Members": 64, "Filter": {"Stride": 48, "Sigma_cm": 10.0, **filt, "Smoother": smoother}}


def test_cli_block_is_parsed():
    assert cli.filter_smoother_settings({"Members": 64, "Filter": {"Sigma_cm": 10.0}}) is None
    assert cli.filter_smoother_settings({"Members": 64}) is None
    assert cli.filter_smoother_settings(_ens({})) == (48, 0, (0.05, 0.5, 0.95))
    assert cli.filter_smoother_settings(_ens({"Stride": 48, "Lag_rows": 480, "Quantiles": [0.1, 0.9]})) == (48, 10, (0.1, 0.9))
    assert cli.filter_smoother_settings(_ens({"Stride": 6, "Lag_rows": 384})) == (6, 64, (0.05, 0.5, 0.95))
    pts = [{"Soil_Properties": {"n": 1.6}}]
    assert cli.filter_smoother_settings({**_ens({"Stride": 12}, Sharded=True), "Points": pts})[0] == 12   # a sweep ignores Sharded
    a = cli.Assimilation(filt=(48, 10.0, None), smoother=(6, 4, (0.5,)))
    assert a.kwargs()["filter_smoother"] == {"stride": 6, "lag_rows": 24}
    assert "filter_smoother" not in cli.Assimilation(filt=(48, 10.0, None)).kwargs()


@pytest.mark.parametrize("ens, what", [
    (_ens([48, 480]), "must be an object"),
    (_ens({"Lag": 48}), "unknown keys"),
    (_ens({"Stride": True}), "Smoother.Stride"),
    (_ens({"Stride": 0}), "Smoother.Stride"),
    (_ens({"Stride": 48, "Lag_rows": True}), "Smoother.Lag_rows"),
    (_ens({"Stride": 48, "Lag_rows": 50}), "multiple of its Stride"),
    (_ens({"Stride": 6, "Lag_rows": 390}), "at most 64"),
    (_ens({"Quantiles": [0.01 * k for k in range(17)]}), "at most 16"),
    (_ens({"Quantiles": [True]}), "Smoother.Quantiles"),
    (_ens({"Quantiles": [1.5]}), "Smoother.Quantiles"),
    (_ens({}, Stride=0), "needs an active filter"),
    (_ens({}, Sharded=True), "not available with \"Sharded\": true"),
    ({"Members": 64, "Smoother": {}, "Filter": {"Sigma_cm": 10.0}}, "belongs inside"),
])
def test_cli_block_refusals(ens, what):
    with pytest.raises(ValueError, match=what):
        cli.filter_smoother_settings(ens)


def test_exports_hold_the_new_names_and_none_is_a_stats_getter():
    for name in NAMES:
        assert name in _lib.EXPORTS, name
        assert not name.endswith("_stats"), name
        assert _lib.EXPORTS[name][1] is _lib.C.c_int
    assert {n for n in _lib.EXPORTS if "smoother" in n} == set(NAMES)


def test_summary_reports_the_lag_reached_and_the_paths(monkeypatch):
    from hydromodel_amd import stepper
    seen = {}

    def fake(hist, obs_idx, levels, dz, z, device=0, stride=1):
        seen.update(stride=stride, shape=np.asarray(hist).shape)
        return {"rows": np.arange(np.asarray(hist).shape[-2], dtype=np.int64) * stride}

    monkeypatch.setattr(stepper, "wtd_distribution", fake)
    got = filter_smoother_of(W, ANC, 1, 2, 8, 6, np.zeros(6, dtype=np.int32), 5)
    out = filter_smoother_summary(got["hist_flushed"][0], got["paths_flushed"][0], np.zeros(6), (0.5,), 5.0, np.arange(6.0), 1)
    assert seen == {"stride": 1, "shape": (6, 6)}
    assert out["lag_rows"].tolist() == [-1, 2, 2, 2, 1, 0] and out["unique_paths"].tolist() == [0, 3, 3, 3, 3, 8]
