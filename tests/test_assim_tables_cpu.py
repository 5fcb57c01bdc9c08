"""The registry of the assimilation tables (stepper.ASSIM_TABLES) without a GPU or the library: its keys against the C
entry points, the one getter / setter pair and the eighteen named methods on a stand-in library, the trailing shapes,
and the CLI's placed table, window reducer, settings bundle and collective count on stand-in ranks and handles."""
import ctypes as C

import numpy as np
import pytest

from hydromodel_amd import _lib, cli
from hydromodel_amd.stepper import ASSIM_TABLES, EnsembleStepper, assim_table_shape, stride_rows

KEYS = ("filter", "filter_sm", "filter_temper", "filter_rejuvenation", "filter_window", "enkf", "enkf_sm", "enkf_window",
        "enkf_noise")


# ---- 1. the registry and the C ABI --------------------------------------------------------------------------------------
def test_the_registry_names_every_double_table_of_the_abi_and_nothing_else():
    assert tuple(ASSIM_TABLES) == KEYS
    assert {k: ASSIM_TABLES[k][0] for k in KEYS} == {k: k.split("_")[0] for k in KEYS}       # the owner is the key's prefix
    table_args = [C.c_void_p, C.POINTER(C.c_double), C.c_int64]
    for key in KEYS:
        for name in (f"hc_get_{key}_stats", f"hc_set_{key}_stats"):
            assert name in _lib.EXPORTS, name
            assert list(_lib.EXPORTS[name][0]) == table_args and _lib.EXPORTS[name][1] is C.c_int, name
    getters = {n[len("hc_get_"):-len("_stats")] for n, (args, _) in _lib.EXPORTS.items()
               if n.startswith("hc_get_") and n.endswith("_stats") and list(args) == table_args}
    assert getters == set(KEYS)
    assert "hc_get_profile_stats" in _lib.EXPORTS and "profile" not in getters      # an int64 table: not one of them


def test_trailing_shapes():
    D, ns, nw = 5, 3, 2
    want = {"filter": (4,), "filter_sm": (3, 6), "filter_temper": (4,), "filter_rejuvenation": (4,),
            "filter_window": (2, 4), "enkf": (8,), "enkf_sm": (3, 6), "enkf_window": (2, 4), "enkf_noise": (21,)}
    assert {k: assim_table_shape(k, D, ns, nw) for k in KEYS} == want
    assert assim_table_shape("enkf_noise", 101) == (405,) and assim_table_shape("filter_sm", 101) == (0, 6)
    with pytest.raises(KeyError):
        assim_table_shape("profile", D)


# ---- 2. the stepper's one pair and its eighteen named methods -----------------------------------------------------------
class _Lib:
    """Records (C function, entries) of every table call and says 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(handle, pointer, n_entries):
            assert isinstance(pointer, C.POINTER(C.c_double))
            self.calls.append((name, int(n_entries)))
            return 0
        return call


def _stepper():
    st = object.__new__(EnsembleStepper)
    st.lib, st.h, st.P, st.T, st.D = _Lib(), None, 2, 97, 5
    st.filter_stride, st.enkf_stride = 24, 48
    st.filter_sm_nodes = st.enkf_sm_nodes = np.array([1, 2, 3], dtype=np.int32)
    st.filter_window_offsets = st.enkf_window_offsets = (6, 12)
    return st


def test_assim_table_allocates_the_registrys_shape_and_calls_the_keys_function():
    st = _stepper()
    rows = {"filter": 5, "enkf": 3}                      # stride_rows(97, 24), stride_rows(97, 48)
    assert (stride_rows(97, 24), stride_rows(97, 48)) == (5, 3)
    for key in KEYS:
        trailing = assim_table_shape(key, 5, 3, 2)
        st.lib.calls.clear()
        t = st.assim_table(key)
        assert t.dtype == np.float64 and t.shape == (2, rows[ASSIM_TABLES[key][0]]) + trailing, key
        assert st.lib.calls == [(f"hc_get_{key}_stats", 2 * rows[ASSIM_TABLES[key][0]] * int(np.prod(trailing)))]
        st.lib.calls.clear()
        st.set_assim_table(key, t)
        assert st.lib.calls == [(f"hc_set_{key}_stats", t.size)]


def test_the_eighteen_named_methods_reach_the_function_they_reached():
    st = _stepper()
    for key in KEYS:
        st.lib.calls.clear()
        t = getattr(st, key + "_table")()
        getattr(st, f"set_{key}_table")(t[::-1])         # (any layout: the setter flattens a copy)
        assert st.lib.calls == [(f"hc_get_{key}_stats", t.size), (f"hc_set_{key}_stats", t.size)], key
        assert t.shape == st.assim_table(key).shape
        assert getattr(EnsembleStepper, key + "_table").__doc__, key          # the columns stay documented there


# ---- 3. the CLI: placed table, window reducer, bundle, collectives ------------------------------------------------------
class _Ranks:
    rank, world = 0, 1

    def __init__(self):
        self.collectives = 0

    def allreduce_sum(self, x):
        self.collectives += 1
        return x


class _Sim:
    """A handle's tables by key: [n_arow] + trailing for an ensemble, [P][n_arow] + trailing for a sweep."""

    def __init__(self, tables):
        self.tables = tables

    def assim_table(self, key):
        return self.tables[key]


class _Cols:
    dim_d = 5
    z = np.array([10.0, 15.0, 20.0, 25.0, 30.0])


T, STRIDE, SLOTS = 97, 24, (1, 2, 3, 4)                   # 97 rows, stride 24: slots 0 ... 4


def _owner_table(lead, width):
    t = np.full(lead + (5, width), np.nan)
    t[..., 0] = 0.0
    t[..., SLOTS, :] = 1.0
    t[..., SLOTS, 0] = 8.0                                # count
    return t


def _window_table(lead):
    t = np.full(lead + (5, 2, 4), np.nan)
    t[..., SLOTS, :, :] = (1.0, 120.0, 100.0, 7.0)        # observed, observation, prior mean, prior std
    t[..., 2, 1, :] = (0.0, np.nan, np.nan, np.nan)       # slot 2 had no observation on its second lagged row
    return t


def _sm_table(lead):
    t = np.full(lead + (5, 3, 6), np.nan)
    t[..., SLOTS, :, :] = (1.0, 0.30, 0.25, 0.02, 0.28, 0.01)
    return t


def test_placed_table_places_the_handles_points_and_a_rank_without_points_joins():
    lead, ids, P = (2,), [2, 0], 3
    t = _window_table(lead)
    t[1, 1, 0, 1] = -0.0                                  # every bit survives: the tables travel as int64
    ranks = _Ranks()
    got = cli._placed_table(ranks, _Sim({"filter_window": t}), ids, P, T, 5, STRIDE, "filter_window", 2)
    assert got.dtype == np.float64 and got.shape == (3, 5, 2, 4) and ranks.collectives == 1
    assert got[2].tobytes() == t[0].tobytes() and got[0].tobytes() == t[1].tobytes() and not got[1].any()
    none = cli._placed_table(ranks, None, [], P, T, 5, STRIDE, "enkf_noise")
    assert none.shape == (3, 5, 21) and not none.any() and ranks.collectives == 2
    one = cli._placed_table(ranks, _Sim({"enkf": _owner_table((), 8)}), [0], 1, T, 5, STRIDE, "enkf")
    assert one.shape == (1, 5, 8)                         # an ensemble's table gains the point axis


@pytest.mark.parametrize("owner", ["filter", "enkf"])
@pytest.mark.parametrize("keep", [False, True])
def test_window_reducer_datasets_and_closing_line(owner, keep):
    lead, ids, P = ((3,), [0, 1, 2], 3) if keep else ((), [0], 1)
    ranks, slots = _Ranks(), np.array(SLOTS)
    out, line = cli._reduce_window(ranks, _Sim({owner + "_window": _window_table(lead)}), ids, P, T, 5, STRIDE, (6, 12),
                                   slots, "Ensemble x8", keep, 10.0, owner)
    assert ranks.collectives == 1
    want = {"window_offsets": (np.int64, (2,)), "window_observed": (np.int8, lead + (4, 2)),
            "window_obs_cm": (np.float64, lead + (4, 2)), "window_prior_mean_cm": (np.float64, lead + (4, 2)),
            "window_prior_std_cm": (np.float64, lead + (4, 2))}
    if owner == "enkf":
        want["window_innovation_cm"] = (np.float64, lead + (4, 2))
    assert set(out) == {f"{owner}_{k}" for k in want}
    assert "filter_window_innovation_cm" not in out
    for k, (dtype, shape) in want.items():
        assert out[f"{owner}_{k}"].dtype == dtype and out[f"{owner}_{k}"].shape == shape, k
    assert out[f"{owner}_window_offsets"].tolist() == [6, 12]
    first = out[f"{owner}_window_observed"].reshape((-1, 4, 2))[0]
    assert first.tolist() == [[1, 1], [1, 0], [1, 1], [1, 1]]
    obs, prior = out[f"{owner}_window_obs_cm"].reshape((-1, 4, 2))[0], out[f"{owner}_window_prior_mean_cm"].reshape((-1, 4, 2))[0]
    assert obs[0].tolist() == [130.0, 130.0] and prior[0].tolist() == [110.0, 110.0] and np.isnan(obs[1, 1])
    if owner == "enkf":
        assert out["enkf_window_innovation_cm"].reshape((-1, 4, 2))[0, 0].tolist() == [20.0, 20.0]
        assert line == " [Ensemble x8] EnKF window: 7 lagged observations over 4 rows (offsets [6, 12])"
    else:
        assert line == " [Ensemble x8] filter window: 7 lagged observations over 4 rows"
    # off: no collective, nothing written, no line
    assert cli._reduce_window(ranks, None, [], P, T, 5, STRIDE, None, slots, "x", keep, 10.0, owner) == ({}, None)
    assert cli._reduce_window(ranks, None, [], P, T, 5, 0, (6, 12), slots, "x", keep, 10.0, owner) == ({}, None)
    assert ranks.collectives == 1


def _record():
    return {"nodes": np.array([1, 2, 3], dtype=np.int32), "depths_cm": np.array([15.0, 20.0, 25.0]),
            "sigma": np.array([0.02, 0.02, 0.02]), "values": np.zeros((T, 3))}


def _what(line):
    """' [Ensemble x8] filter window: 7 lagged ...' -> 'filter window'"""
    return line.split("] ")[1].split(":")[0].split(" =")[0]


def test_an_owner_costs_one_collective_per_table_that_is_on():
    filt = dict(filt=(STRIDE, 5.0, None), frecord=_record(), fwindow=(6, 12))
    tables = {"filter": _owner_table((), 4), "filter_sm": _sm_table(()), "filter_window": _window_table(()),
              "filter_temper": _owner_table((), 4), "filter_rejuvenation": _owner_table((), 4)}
    for extra, n in (({}, 3), ({"ess_floor": 0.5}, 4), ({"ess_floor": 0.5, "rejuvenation": 0.98}, 5)):
        ranks = _Ranks()
        out, lines = cli._reduce_assimilation(ranks, _Sim(tables), [0], 1, T, _Cols, cli.Assimilation(**filt, **extra),
                                              "Ensemble x8", keep_points=False)
        assert ranks.collectives == n, extra
        assert out["filter_rows"].tolist() == [24, 48, 72, 96] and out["filter_sm_obs"].shape == (4, 3)
        assert out["filter_window_obs_cm"].shape == (4, 2) and len(lines) == 3 and all(lines)
        assert ("filter_beta" in out) == ("ess_floor" in extra) and ("filter_rejuvenated" in out) == ("rejuvenation" in extra)
        want = (["filter log-likelihood"] + ["filter tempering"] * ("ess_floor" in extra)
                + ["filter rejuvenation"] * ("rejuvenation" in extra) + ["soil-moisture forecast RMSE", "filter window"])
        assert [_what(s) for s in "\n".join(lines).splitlines()] == want
    # the EnKF with sensors, a window and the noise field: four tables, four collectives; lines in the run's order
    ranks = _Ranks()
    etables = {"enkf": _owner_table((2,), 8), "enkf_sm": _sm_table((2,)), "enkf_window": _window_table((2,)),
               "enkf_noise": np.ones((2, 5, 21))}
    a = cli.Assimilation(enkf=(STRIDE, 5.0, 0.0, None), record=_record(), scheme=("sqrt", 0.5), window=(6, 12),
                         noise_alpha=0.5)
    out, lines = cli._reduce_assimilation(ranks, _Sim(etables), [0, 1], 2, T, _Cols, a, "Sweep 2 points x8", keep_points=True)
    assert ranks.collectives == 4 and out["enkf_rows"].tolist() == [24, 48, 72, 96]
    assert int(out["enkf_method"]) == 1 and float(out["enkf_relaxation"]) == 0.5 and out["enkf_noise_post_std"].shape == (2, 5, 5)
    assert [_what(s) for s in lines if s] == ["EnKF log-likelihood", "soil-moisture forecast RMSE", "EnKF window",
                                               "EnKF noise field"]
    # nothing on: nothing placed
    ranks = _Ranks()
    assert cli._reduce_assimilation(ranks, None, [], 1, T, _Cols, cli.Assimilation(), "x", False) == ({}, [])
    assert ranks.collectives == 0


def test_the_bundle_gives_the_constructors_keywords():
    rec, frec = _record(), _record()
    assert cli.Assimilation().kwargs() == {}
    assert cli.Assimilation(filt=(48, 10.0, None)).kwargs() == dict(filter_stride=48, filter_sigma_cm=10.0, filter_seed=None)
    full = cli.Assimilation((24, 10.0, 7), frec, 0.5, (6, 12), 0.98).kwargs()
    assert full == dict(filter_stride=24, filter_sigma_cm=10.0, filter_seed=7, filter_soil_moisture=frec,
                        filter_ess_floor=0.5, filter_window_offsets=(6, 12), filter_rejuvenation=0.98)
    assert cli.Assimilation(enkf=(48, 10.0, 0.0, None), window=()).kwargs() == dict(
        enkf_stride=48, enkf_sigma_cm=10.0, enkf_localisation_cm=0.0, enkf_seed=None)
    full = cli.Assimilation(enkf=(24, 10.0, 50.0, 3), record=rec, scheme=("sqrt", 0.5), window=(6, 12), noise_alpha=0.0).kwargs()
    assert full == dict(enkf_stride=24, enkf_sigma_cm=10.0, enkf_localisation_cm=50.0, enkf_seed=3, enkf_soil_moisture=rec,
                        enkf_method="sqrt", enkf_relaxation=0.5, enkf_window_offsets=(6, 12),
                        enkf_noise_field={"relaxation": 0.0})
    with pytest.raises(Exception):
        cli.Assimilation().filt = (1, 1.0, None)         # immutable
