"""The registry of the diagnostic tables (stepper.DIAG_TABLES) without a GPU or the library: its entries against the C
entry points, the one split / join against the families' own layout functions, the outside count through both of its
carriers, the one get / set / export / reset path and the named methods on a stand-in library, the refusals, the
checkpoint's datasets, and the CLI's placed table on stand-in ranks and handles."""
import ctypes as C

import numpy as np
import pytest

from hydromodel_amd import _lib, cli
from hydromodel_amd.ensemble import _Run
from hydromodel_amd.multigpu import place_points
from hydromodel_amd.stepper import (DIAG_TABLES, EnsembleStepper, diag_checkpoint, diag_counts, diag_from_checkpoint,
                                    diag_layout, diag_placed, join_diag, join_profile_table, layer_storage_table_layout,
                                    pack_diag, period_totals_table_layout, profile_layout, root_uptake_table_layout,
                                    split_diag, split_layer_storage_table, split_period_hist, split_period_totals_table,
                                    split_profile_table, split_root_uptake_table, theta_cov_shape, unpack_diag)

# key -> element type, in the order a checkpoint installs the tables
DTYPES = {"profile": np.int64, "theta_hist": np.int32, "storage": np.int64, "storage_hist": np.int32,
          "theta_cov": np.int64, "period": np.int64, "period_acc": np.int64, "period_hist": np.int32, "uptake": np.int64,
          "uptake_acc": np.int64, "uptake_hist": np.int32, "wtd_hist": np.int32}
KEYS = tuple(DTYPES)
HISTS = ("theta_hist", "storage_hist", "period_hist", "uptake_hist")           # int32 with a uint64 outside count
T, STRIDE, D, BINS, LAYERS, PERIODS, THRESHOLDS, N, COV_STRIDE = 10, 3, 7, 32, 2, 2, 1, 4, 3
PROWS, K = 4, 5                                                                # rows 0, 3, 6, 9; 4 + 1 threshold


def _counts(P):
    return diag_counts(P, T, D, N, profile_stride=STRIDE, wtd_hist_stride=STRIDE, theta_bins=BINS, storage_layers=LAYERS,
                       storage_bins=BINS, cov_stride=COV_STRIDE, periods=PERIODS, thresholds=THRESHOLDS, period_bins=BINS,
                       uptake_layers=LAYERS, uptake_bins=BINS)


def _random_raw(key, P, seed=3, outside=(1 << 40) + 5):
    """A raw table of the layout's size: counts below 1000, the outside count in its carrier."""
    n = diag_layout(key, _counts(P))["words"][0]
    raw = np.random.default_rng(seed).integers(0, 1000, n).astype(DTYPES[key])
    body, had = unpack_diag(key, raw)
    return pack_diag(key, body, outside) if had is not None else raw


# ---- 1. the registry and the C ABI --------------------------------------------------------------------------------------
def test_the_registry_names_the_twelve_tables_and_their_entry_points():
    assert tuple(DIAG_TABLES) == KEYS and {k: DIAG_TABLES[k].dtype for k in KEYS} == DTYPES
    words, exports = set(), set()
    for key, e in DIAG_TABLES.items():
        pointer = C.POINTER(C.c_int64 if e.dtype == np.int64 else C.c_int32)
        for name in ("hc_get_" + e.stem, e.set):
            assert name in _lib.EXPORTS, name
            assert list(_lib.EXPORTS[name][0]) == [C.c_void_p, pointer, C.c_int64], name
        assert list(_lib.EXPORTS[e.reset][0]) == [C.c_void_p], key
        words |= {key} if f"hc_get_{e.stem}_words" in _lib.EXPORTS else set()
        exports |= {key} if "hc_export_" + e.stem in _lib.EXPORTS else set()
    assert words == {"profile", "storage", "theta_cov", "period", "uptake"}
    assert exports == words | {"period_hist", "uptake_hist"}
    assert {k: DIAG_TABLES[k].outside for k in KEYS if DIAG_TABLES[k].outside} == dict({k: "uint64" for k in HISTS},
                                                                                      theta_cov="int64")
    # summed over the ranks: every table with parts that belong to the points, so all but the members' accumulators
    assert [k for k in KEYS if not diag_placed(k)] == ["period_acc", "uptake_acc"]
    assert diag_placed("profile") == ("prof", "pcnt", "flux", "fcnt", "aerr") and diag_placed("period_hist") == ("flux", "wtd")
    for name in ("hc_get_profile_overflow", "hc_get_theta_hist_outside", "hc_get_layer_storage_outside",
                 "hc_get_layer_storage_overflow", "hc_get_theta_cov_outside", "hc_get_period_totals_outside",
                 "hc_get_period_totals_overflow", "hc_get_root_uptake_outside", "hc_get_root_uptake_overflow"):
        assert list(_lib.EXPORTS[name][0]) == [C.c_void_p, C.POINTER(C.c_uint64)]


# ---- 2. one split / join, against the families' own functions -----------------------------------------------------------
@pytest.mark.parametrize("P", [0, 1, 3])
def test_split_is_the_inverse_of_join_and_agrees_with_the_family_functions(P):
    counts = _counts(P)
    for key in KEYS:
        raw = _random_raw(key, P)
        parts = split_diag(key, raw, counts)
        assert [k for k in parts if k != "outside"] == [name for name, _ in DIAG_TABLES[key].parts], key
        back = join_diag(key, parts)
        assert back.dtype == DTYPES[key] and back.tobytes() == raw.tobytes(), key
        assert ("outside" in parts) == (DIAG_TABLES[key].outside is not None)
        if "outside" in parts:
            assert parts["outside"] == (1 << 40) + 5
        # the wide form (the sum over ranks): int64 throughout, the outside count in one word
        wide = join_diag(key, parts, wide=True)
        assert wide.dtype == np.int64 and wide.size == diag_layout(key, counts, wide=True)["words"][0], key
        again = split_diag(key, wide, counts, wide=True)
        assert all(np.array_equal(again[k], parts[k]) for k in parts), key
    legacy = {"profile": (profile_layout(P, T, D, STRIDE), split_profile_table, (P, T, D, STRIDE)),
              "storage": (layer_storage_table_layout(P, T, LAYERS, STRIDE), split_layer_storage_table, (P, T, LAYERS, STRIDE)),
              "period": (period_totals_table_layout(P, PERIODS, K), split_period_totals_table, (P, PERIODS, K)),
              "uptake": (root_uptake_table_layout(P, PERIODS, LAYERS, D), split_root_uptake_table, (P, PERIODS, LAYERS, D))}
    for key, (lay, split, args) in legacy.items():
        raw = _random_raw(key, P)
        assert lay == diag_layout(key, counts), key
        want, got = split(raw, *args), split_diag(key, raw, counts)
        assert list(want) == list(got) and all(want[k].shape == got[k].shape and np.array_equal(want[k], got[k]) for k in want)
    assert np.array_equal(join_profile_table(split_profile_table(_random_raw("profile", P), P, T, D, STRIDE)),
                          _random_raw("profile", P))
    # the shapes, written out
    shapes = {k: {name: sh for name, (_, sh) in diag_layout(k, counts).items() if name != "words"} for k in KEYS}
    assert shapes["profile"] == {"prof": (P, PROWS, D, 2, 5), "pcnt": (P, PROWS), "flux": (P, T, 2, 5), "fcnt": (P, T),
                                 "aerr": (P, T), "ovf": (1,)}
    assert shapes["theta_hist"] == {"hist": (P, PROWS, D, BINS)} and shapes["wtd_hist"] == {"hist": (P, PROWS, D)}
    assert shapes["storage"] == {"stor": (P, PROWS, LAYERS, 5), "scnt": (P, PROWS), "ovf": (1,)}
    assert shapes["storage_hist"] == {"hist": (P, PROWS, LAYERS, BINS)}
    assert shapes["theta_cov"] == {"cov": (P, PROWS, theta_cov_shape(D, COV_STRIDE)[2])} == {"cov": (P, PROWS, 15)}
    assert shapes["period"] == {"pmom": (P, PERIODS, K, 5), "pcnt": (P, PERIODS), "ovf": (1,)}
    assert shapes["period_acc"] == {"acc": (K, N)} and shapes["uptake_acc"] == {"acc": (LAYERS + 1, N)}
    assert shapes["period_hist"] == {"flux": (P, PERIODS, 2, BINS), "wtd": (P, PERIODS, 2, D)}
    assert shapes["uptake"] == {"umom": (P, PERIODS, LAYERS + 1, 5), "ucnt": (P, PERIODS), "uprof": (P, PERIODS, D - 1, 2),
                                "ovf": (1,)}
    assert shapes["uptake_hist"] == {"hist": (P, PERIODS, LAYERS, BINS)}
    raw = _random_raw("period_hist", P)
    hf, hw = split_period_hist(unpack_diag("period_hist", raw)[0], P, PERIODS, BINS, D)
    parts = split_diag("period_hist", raw, counts)
    assert np.array_equal(hf, parts["flux"]) and np.array_equal(hw, parts["wtd"]) and hf.shape == (P, PERIODS, 2, BINS)
    with pytest.raises(ValueError, match="the layout has"):
        split_diag("theta_hist", np.zeros(7, dtype=np.int32), counts)


def test_the_outside_count_round_trips_through_both_carriers():
    for key in HISTS + ("theta_cov",):
        top = (1 << 63) - 1 if key == "theta_cov" else (1 << 64) - 1
        body = np.arange(6)
        for outside in (0, 1, 1 << 32, top):
            raw = pack_diag(key, body, outside)
            assert raw.dtype == DTYPES[key] and raw.size == 6 + (1 if key == "theta_cov" else 2)
            got, back = unpack_diag(key, raw)
            assert back == outside and got.tolist() == body.tolist(), (key, outside)
            got, back = unpack_diag(key, pack_diag(key, body, outside, wide=True), wide=True)
            assert back == outside and got.tolist() == body.tolist(), (key, outside)
        for bad in (-1, top + 1):
            with pytest.raises(ValueError, match="outside count"):
                pack_diag(key, body, bad)
    low_first = pack_diag("theta_hist", [], 5 + (7 << 32))
    assert low_first.tolist() == [5, 7]                   # as the device holds it: the low half first
    assert unpack_diag("profile", np.arange(4))[1] is None and pack_diag("profile", np.arange(4)).tolist() == [0, 1, 2, 3]


# ---- 3. the stepper's one path and its named methods ----------------------------------------------------------------------
class _Lib:
    """Records (C function, elements) of every table call, answers the words and the counters, and says 0."""

    def __init__(self, words):
        self.calls, self.words = [], words

    def __getattr__(self, name):
        def call(handle, *args):
            if name.endswith("_words"):
                args[0]._obj.value = self.words[name]
            elif len(args) == 1 and not isinstance(args[0], C.c_void_p):      # a counter
                args[0]._obj.value = 11
            self.calls.append((name, int(args[-1]) if len(args) == 2 else None))
            return 0
        return call


def _stepper(P=2):
    st = object.__new__(EnsembleStepper)
    st.P, st.T, st.D, st.N, st.h = P, T, D, N, None
    st.profile_stride = st.wtd_hist_stride = STRIDE
    st.theta_hist_bins = st.storage_bins = st.period_bins = st.uptake_bins = BINS
    st.storage_ranges, st.uptake_cells = np.zeros((LAYERS, 2), dtype=np.int32), np.zeros((LAYERS, 2), dtype=np.int32)
    st.theta_cov_stride, st.period_ends = COV_STRIDE, np.array([4, 9])
    st.period_threshold_nodes = np.zeros(THRESHOLDS, dtype=np.int32)
    st.lib = _Lib({f"hc_get_{DIAG_TABLES[k].stem}_words": diag_layout(k, _counts(P))["words"][0] for k in KEYS})
    return st


def test_the_one_path_calls_the_entrys_functions_with_the_layouts_size():
    st = _stepper()
    assert st.diag_counts() == _counts(2)
    for key, e in DIAG_TABLES.items():
        n = diag_layout(key, _counts(2))["words"][0]
        has_words = f"hc_get_{e.stem}_words" in _lib.EXPORTS
        st.lib.calls.clear()
        raw = st.diag_raw(key)
        assert raw.dtype == DTYPES[key] and raw.shape == (n,) and st.diag_words(key) == n, key
        assert [c for c in st.lib.calls if not c[0].endswith("_words")] == [("hc_get_" + e.stem, n)], key
        assert any(c[0].endswith("_words") for c in st.lib.calls) == has_words, key
        st.lib.calls.clear()
        st.set_diag_raw(key, raw.reshape(1, -1)[:, ::1])
        st.set_diag_parts(key, st.diag_parts(key))
        st.reset_diag(key)
        assert [c for c in st.lib.calls if c[0] != "hc_get_" + e.stem and not c[0].endswith("_words")] == \
            [(e.set, n), (e.set, n), (e.reset, None)], key
        st.lib.calls.clear()
        if "hc_export_" + e.stem in _lib.EXPORTS:
            st.export_diag(key, 4096)
            assert st.lib.calls[-1] == ("hc_export_" + e.stem, n), key
        else:
            with pytest.raises(ValueError, match="no device-to-device export"):
                st.export_diag(key, 4096)
    with pytest.raises(KeyError):
        st.diag_raw("filter")


def test_the_named_methods_reach_the_function_they_reached():
    st = _stepper()
    getters = {"profile_table": "profile_stats", "wtd_hist_table": "wtd_hist", "theta_hist_table": "theta_hist",
               "layer_storage_table": "layer_storage", "layer_storage_hist_table": "layer_storage_hist",
               "theta_cov_table": "theta_cov", "period_totals_table": "period_totals",
               "period_totals_hist_raw": "period_totals_hist", "period_totals_hists": "period_totals_hist",
               "period_totals_acc": "period_totals_acc", "root_uptake_table": "root_uptake",
               "root_uptake_hist_raw": "root_uptake_hist", "root_uptake_hist": "root_uptake_hist",
               "root_uptake_acc": "root_uptake_acc"}
    shapes = {"wtd_hist_table": (2, PROWS, D), "theta_hist_table": (2, PROWS, D, BINS),
              "layer_storage_hist_table": (2, PROWS, LAYERS, BINS), "theta_cov_table": (2, PROWS, 15),
              "period_totals_acc": (K, N), "root_uptake_hist": (2, PERIODS, LAYERS, BINS), "root_uptake_acc": (LAYERS + 1, N)}
    for method, stem in getters.items():
        st.lib.calls.clear()
        got = getattr(st, method)()
        assert [c[0] for c in st.lib.calls if not c[0].endswith("_words")] == ["hc_get_" + stem], method
        if method in shapes:
            assert got.shape == shapes[method], method
    hf, hw = st.period_totals_hists()
    assert hf.shape == (2, PERIODS, 2, BINS) and hw.shape == (2, PERIODS, 2, D)
    setters = {"set_profile_table": ("profile", 1), "set_wtd_hist_table": ("wtd_hist", 1),
               "set_theta_hist_table": ("theta_hist", 2), "set_layer_storage_table": ("storage", 1),
               "set_layer_storage_hist_table": ("storage_hist", 2), "set_theta_cov_table": ("theta_cov", 2),
               "set_period_totals_table": ("period", 1), "set_period_totals_acc": ("period_acc", 1),
               "set_root_uptake_table": ("uptake", 1), "set_root_uptake_hist": ("uptake_hist", 2),
               "set_root_uptake_acc": ("uptake_acc", 1)}
    for method, (key, n_args) in setters.items():
        n = diag_layout(key, _counts(2))["words"][0]
        body = unpack_diag(key, st.diag_raw(key))[0]
        st.lib.calls.clear()
        getattr(st, method)(*((body[::-1],) + ((9,) if n_args == 2 else ())))     # (any layout: the setter flattens a copy)
        assert st.lib.calls == [(DIAG_TABLES[key].set, n)], method
    st.lib.calls.clear()
    st.set_period_totals_hists(hf, hw, 3)
    assert st.lib.calls == [("hc_set_period_totals_hist_table", diag_layout("period_hist", _counts(2))["words"][0])]
    for method, name in {"reset_theta_hist": "hc_reset_theta_hist", "reset_layer_storage": "hc_reset_layer_storage",
                         "reset_theta_cov": "hc_reset_theta_cov", "reset_period_totals": "hc_reset_period_totals",
                         "reset_root_uptake": "hc_reset_root_uptake", "profile_overflow": "hc_get_profile_overflow",
                         "theta_hist_outside": "hc_get_theta_hist_outside",
                         "layer_storage_outside": "hc_get_layer_storage_outside",
                         "layer_storage_overflow": "hc_get_layer_storage_overflow",
                         "theta_cov_outside": "hc_get_theta_cov_outside",
                         "period_totals_outside": "hc_get_period_totals_outside",
                         "period_totals_overflow": "hc_get_period_totals_overflow",
                         "root_uptake_outside": "hc_get_root_uptake_outside",
                         "root_uptake_overflow": "hc_get_root_uptake_overflow"}.items():
        st.lib.calls.clear()
        got = getattr(st, method)()
        assert [c[0] for c in st.lib.calls] == [name] and got == (None if method.startswith("reset") else 11), method
    for method in ("export_profile_stats", "export_layer_storage", "export_theta_cov", "export_period_totals",
                   "export_period_totals_hist", "export_root_uptake", "export_root_uptake_hist", "reset_profile_stats",
                   "reset_wtd_hist"):
        assert not hasattr(EnsembleStepper, method), method       # had no caller: export_diag / reset_diag cover them
    for method in getters:
        assert getattr(EnsembleStepper, method).__doc__, method                    # the columns stay documented there


def test_every_count_table_refuses_a_negative_count_and_an_outside_count_out_of_range():
    st = _stepper(1)
    named = {"theta_hist": st.set_theta_hist_table, "storage_hist": st.set_layer_storage_hist_table,
             "uptake_hist": st.set_root_uptake_hist}
    for key in HISTS + ("wtd_hist",):
        parts = split_diag(key, _random_raw(key, 1, outside=0), _counts(1))
        first = DIAG_TABLES[key].parts[0][0]
        for bad in (-1, 1 << 31):
            broken = dict(parts, **{first: parts[first].astype(np.int64)})
            broken[first].reshape(-1)[3] = bad
            with pytest.raises(ValueError, match=r"counts must lie in \[0, 2\^31 - 1\]"):
                st.set_diag_parts(key, broken)
            if key in named:
                with pytest.raises(ValueError, match="counts must lie in"):
                    named[key](broken[first])
        if key == "wtd_hist":
            continue
        for bad in (-1, 1 << 64):
            with pytest.raises(ValueError, match=r"outside count must lie in \[0, 2\^64\)"):
                st.set_diag_parts(key, dict(parts, outside=bad))
            if key in named:
                with pytest.raises(ValueError, match="outside count"):
                    named[key](parts[first], bad)
        raw = join_diag(key, parts)
        raw[3] = -1                                        # a raw table's counts are checked too, its tail is not a count
        with pytest.raises(ValueError, match="counts must lie in"):
            st.set_diag_raw(key, raw)
        st.set_diag_raw(key, join_diag(key, dict(parts, outside=(1 << 64) - 1)))     # (a tail of two -1 entries)
    hf, hw = np.zeros((1, PERIODS, 2, BINS), dtype=np.int64), np.zeros((1, PERIODS, 2, D), dtype=np.int64)
    hw[0, 1, 1, 2] = -1
    with pytest.raises(ValueError, match="counts must lie in"):
        st.set_period_totals_hists(hf, hw)
    with pytest.raises(ValueError, match="outside count"):
        st.set_period_totals_hists(hf, np.abs(hw), 1 << 64)
    cov = np.zeros((1, PROWS, 15), dtype=np.int64)
    with pytest.raises(ValueError, match=r"outside count must lie in \[0, 2\^63\)"):
        st.set_theta_cov_table(cov, 1 << 63)
    assert not st.lib.calls or all(c[0].startswith("hc_set_") and "hist" in c[0] for c in st.lib.calls)


# ---- 4. the checkpoint's datasets ----------------------------------------------------------------------------------------
def test_the_checkpoint_holds_the_datasets_it_held():
    counts = _counts(1)
    want = {"profile": {"profile_table": (np.int64, (4 * (D * 10 + 1) + T * 12 + 1,))},
            "theta_hist": {"theta_hist": (np.int32, (1, PROWS, D, BINS)), "theta_hist_outside": (np.uint64, ())},
            "storage": {"storage_table": (np.int64, (PROWS * (LAYERS * 5 + 1) + 1,))},
            "storage_hist": {"storage_hist": (np.int32, (1, PROWS, LAYERS, BINS)), "storage_hist_outside": (np.uint64, ())},
            "theta_cov": {"theta_cov_table": (np.int64, (1, PROWS, 15)), "theta_cov_outside": (np.uint64, ())},
            "period": {"period_table": (np.int64, (PERIODS * (K * 5 + 1) + 1,))},
            "period_acc": {"period_acc": (np.int64, (K, N))},
            "period_hist": {"period_hist": (np.int32, (PERIODS * 2 * (BINS + D),)), "period_hist_outside": (np.uint64, ())},
            "uptake": {"uptake_table": (np.int64, (PERIODS * ((LAYERS + 1) * 5 + 1 + (D - 1) * 2) + 1,))},
            "uptake_acc": {"uptake_acc": (np.int64, (LAYERS + 1, N))},
            "uptake_hist": {"uptake_hist": (np.int32, (PERIODS * LAYERS * BINS,)), "uptake_hist_outside": (np.uint64, ())},
            "wtd_hist": {"wtd_hist": (np.int32, (1, PROWS, D))}}
    for key in KEYS:
        raw = _random_raw(key, 1)
        data = diag_checkpoint(key, raw, counts)
        assert {k: (v.dtype.type, v.shape) for k, v in data.items()} == want[key], key
        assert diag_from_checkpoint(key, data).tobytes() == raw.tobytes(), key
        for name in data:
            if name.endswith("_outside"):
                assert int(data[name]) == (1 << 40) + 5
    data = diag_checkpoint("period_hist", _random_raw("period_hist", 1), counts)
    assert data["period_hist"].tobytes() == _random_raw("period_hist", 1)[:-2].tobytes()


def test_a_run_keeps_the_tables_its_settings_turn_on_in_the_registrys_order():
    from helpers import digest
    from hydromodel_amd import settings
    _, cols, _ = digest(1)
    run = object.__new__(_Run)

    def tables_on(**options):                             # (the one source: what the constructor normalises its keywords to)
        run.on = settings.normalise("EnsembleSimulation", options, [cols], 0).on
        return run.diag_tables_on()

    assert tables_on() == []
    some = dict(profile_stride=12, storage_layers_cm=[(0.0, 100.0), (100.0, 300.0)], period_ends=[48], wtd_hist_stride=12)
    assert tables_on(**some) == ["profile", "storage", "period", "period_acc", "wtd_hist"]
    assert tables_on(theta_hist_bins=32, storage_bins=32, period_bins=32, uptake_bins=32, theta_cov_stride=4,
                     uptake_layers_cm=[(0.0, 100.0), (100.0, 300.0)], **some) == list(KEYS)


# ---- 5. the CLI's placed table -------------------------------------------------------------------------------------------
class _Ranks:
    """One rank of a world of stand-ins: records what it contributes; ``total``: what the collective then returns."""
    rank, world = 0, 2

    def __init__(self, total=None):
        self.sent, self.total = [], total

    def allreduce_sum(self, x):
        self.sent.append(np.array(x))
        return x if self.total is None else self.total


class _Handle:
    def __init__(self, tables, P):
        self.tables, self.P = tables, P

    def diag_parts(self, key):
        return split_diag(key, self.tables[key], _counts(self.P))


class _Sim:
    def __init__(self, tables, P):
        self.stepper = _Handle(tables, P)


@pytest.mark.parametrize("key", [k for k in KEYS if diag_placed(k)])
def test_two_ranks_place_their_points_and_sum_the_global_words(key):
    whole = split_diag(key, _random_raw(key, 3, outside=900), _counts(3))
    ids = ([2, 0], [1])                                   # rank 0 holds points 2 and 0 (in that order), rank 1 point 1
    share = {"ovf": (np.array([4]), None), "outside": (400, None)}      # the global words: each rank's own share
    local = []
    for r, mine in enumerate(ids):
        parts = {k: (v[mine] if k in diag_placed(key) else v) for k, v in whole.items()}
        for k, (first, _) in share.items():
            if k in parts:
                parts[k] = first if r == 0 else whole[k] - first
        local.append(_Sim({key: join_diag(key, parts)}, len(mine)))
    sent = []
    for sim, mine in zip(local, ids):
        ranks = _Ranks()
        cli._placed_diag(ranks, sim, mine, 3, key, _counts(3))
        assert len(ranks.sent) == 1 and ranks.sent[0].dtype == np.int64          # one collective, int64
        sent.append(ranks.sent[0])
    idle = _Ranks()
    cli._placed_diag(idle, None, [], 3, key, _counts(3))                         # a rank without points joins with zeros
    assert len(idle.sent) == 1 and idle.sent[0].shape == sent[0].shape and not idle.sent[0].any()
    got = cli._placed_diag(_Ranks(sent[0] + sent[1] + idle.sent[0]), local[0], ids[0], 3, key, _counts(3))
    assert list(got) == list(whole)
    for k in whole:
        assert np.array_equal(got[k], whole[k]), (key, k)
    for k in diag_placed(key):                            # placed as place_points places: zeros at the others' points
        mine = split_diag(key, sent[1], _counts(3), wide=True)[k]
        assert np.array_equal(mine, place_points(whole[k][[1]], [1], 3)) and not mine[[0, 2]].any()
