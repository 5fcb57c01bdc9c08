"""Ensemble profile statistics on the host (no GPU): quantisation, 20-bit limbs, exact normalisation, the layout of the
int64 table, its sum over ranks, and the C-ABI entries (include/hydrocol.h hc_set_profile_stats)."""
import math
import os
import re
import socket
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch.multiprocessing as mp

from hydromodel_amd import multigpu
from hydromodel_amd.stepper import (PROF_Q_MAX, PROF_SCALE_FLUX, PROF_SCALE_PSI, PROF_SCALE_THETA, join_profile_table,
                                    limbs_to_mean_std, profile_layout, profile_quantise, profile_tables_to_stats,
                                    profile_words_of, split_profile_table)

REPO = Path(__file__).resolve().parent.parent
NEW_ENTRIES = ("hc_set_profile_stats", "hc_get_profile_stats_words", "hc_profile_snapshot", "hc_get_profile_stats",
               "hc_set_profile_stats_tables", "hc_export_profile_stats", "hc_reset_profile_stats", "hc_get_profile_overflow")


def _exact(q_values):
    """Mean and population sigma of integer q by Fractions: what the limbs must reproduce."""
    n = len(q_values)
    s1 = sum(int(q) for q in q_values)
    s2 = sum(int(q) * int(q) for q in q_values)
    return float(Fraction(s1, n)), math.sqrt(float(Fraction(n * s2 - s1 * s1, n * n)))


def test_limbs_recombine_exactly_where_a_naive_int64_sum_of_squares_overflows():
    rng = np.random.default_rng(3)
    cases = [np.full(8, PROF_Q_MAX, dtype=np.int64),                       # q^2 ~ 2^80 each: no int64 holds one square
             np.array([PROF_Q_MAX, -PROF_Q_MAX, 1, 0, -5], dtype=np.int64),
             rng.integers(-PROF_Q_MAX, PROF_Q_MAX, size=1000, dtype=np.int64),
             np.full(3, 1000 * 2 ** 16, dtype=np.int64) + np.array([0, 1, 0]),   # saturated deep node: psi ~ 1000 cm, sigma ~ 0
             np.full(5, -123456789012, dtype=np.int64)]                     # all equal: sigma exactly 0
    for q in cases:
        words = profile_words_of(q).sum(axis=0)
        assert words.dtype == np.int64 and np.all(words[1:] >= 0)
        assert int(words[1]) + (int(words[2]) << 20) + (int(words[3]) << 40) + (int(words[4]) << 60) == \
            sum(int(v) * int(v) for v in q)
        mean, std = limbs_to_mean_std(len(q), words, 0)
        em, es = _exact(q)
        assert float(mean) == em and float(std) == es
    assert float(limbs_to_mean_std(5, profile_words_of(cases[-1]).sum(axis=0), 0)[1]) == 0.0


def test_mean_std_follow_the_population_convention_and_the_scale():
    x = np.array([0.25, 0.5, 0.125, 0.375])
    q, bad = profile_quantise(x, PROF_SCALE_THETA)
    assert bad == 0
    mean, std = limbs_to_mean_std(4, profile_words_of(q).sum(axis=0), PROF_SCALE_THETA)
    assert float(mean) == x.mean() and float(std) == x.std(ddof=0)
    # a table of several entries, one of them empty
    words = np.stack([profile_words_of(q).sum(axis=0), np.zeros(5, dtype=np.int64)])
    mean, std = limbs_to_mean_std(np.array([4, 0]), words, PROF_SCALE_THETA)
    assert mean[0] == x.mean() and np.isnan(mean[1]) and np.isnan(std[1])


def test_quantisation_at_the_range_limits_and_the_clamp_count():
    top = 2.0 ** 24 - 2.0 ** -16                   # the largest |psi| that fits: q = 2^40 - 1
    q, bad = profile_quantise(np.array([top, -top, 0.0, 2.0 ** -17, 3 * 2.0 ** -17]), PROF_SCALE_PSI)
    assert bad == 0 and q.tolist() == [PROF_Q_MAX, -PROF_Q_MAX, 0, 0, 2]      # rint: half to even
    q, bad = profile_quantise(np.array([2.0 ** 24, -1e30, np.inf, np.nan, 1.0]), PROF_SCALE_PSI)
    assert bad == 4 and q.tolist() == [PROF_Q_MAX, -PROF_Q_MAX, PROF_Q_MAX, 0, 2 ** 16]
    q, bad = profile_quantise(np.array([1.0 - 2.0 ** -40, 1.0]), PROF_SCALE_THETA)
    assert bad == 1 and q.tolist() == [PROF_Q_MAX, PROF_Q_MAX]
    q, bad = profile_quantise(np.array([255.0, -255.0, 256.0]), PROF_SCALE_FLUX)
    assert bad == 1


def _random_table(P, T, D, stride, n_members, seed):
    """A table as the device would build it from n_members random members (rows solved where obs >= 0)."""
    rng = np.random.default_rng(seed)
    parts = {k: np.zeros(sh, dtype=np.int64) for k, (_, sh) in profile_layout(P, T, D, stride).items() if k != "words"}
    n_prow = parts["pcnt"].shape[1]
    for p in range(P):
        psi = rng.normal(-300.0, 200.0, size=(n_prow, n_members, D))
        th = rng.uniform(0.05, 0.45, size=(n_prow, n_members, D))
        fl = rng.uniform(0.0, 1e-2, size=(T, n_members, 2))
        for j in range(n_prow):
            parts["prof"][p, j, :, 0] = profile_words_of(profile_quantise(psi[j], PROF_SCALE_PSI)[0]).sum(axis=0)
            parts["prof"][p, j, :, 1] = profile_words_of(profile_quantise(th[j], PROF_SCALE_THETA)[0]).sum(axis=0)
            parts["pcnt"][p, j] = n_members
        for r in range(1, T):
            for k in range(2):
                parts["flux"][p, r, k] = profile_words_of(profile_quantise(fl[r, :, k], PROF_SCALE_FLUX)[0]).sum(axis=0)
            parts["fcnt"][p, r] = n_members
            parts["aerr"][p, r] = int(rng.integers(0, 40, size=n_members).sum())
    return join_profile_table(parts)


def test_layout_split_and_join_are_inverse_and_the_stats_have_the_stated_shapes():
    P, T, D, stride = 2, 11, 7, 3
    lay = profile_layout(P, T, D, stride)
    assert lay["words"][0] == P * 4 * (D * 10 + 1) + P * T * 12 + 1
    t = _random_table(P, T, D, stride, 5, 1)
    assert np.array_equal(join_profile_table(split_profile_table(t, P, T, D, stride)), t)
    st = profile_tables_to_stats(t, P, T, D, stride, np.full((P, D), 0.5), 2.0)
    assert st["theta_vol_mean"].shape == (P, 4, D) and st["psi_press_std"].shape == (P, 4, D)
    assert st["transpiration_mean"].shape == (P, T) and st["abs_error_mean"].shape == (P, T)
    assert st["rows"].tolist() == [0, 3, 6, 9] and st["overflow"] == 0
    assert np.array_equal(st["S_eff_mean"], st["theta_vol_mean"] / 0.5)
    assert np.all(np.isnan(st["lateral_flow_mean"][:, 0])) and np.all(np.isfinite(st["lateral_flow_mean"][:, 1:]))
    one = profile_tables_to_stats(_random_table(1, T, D, stride, 5, 1), 1, T, D, stride, np.full((1, D), 0.5), 2.0)
    assert one["theta_vol_mean"].shape == (4, D) and one["count"].shape == (4,)
    with pytest.raises(ValueError):
        split_profile_table(t[:-1], P, T, D, stride)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _sum_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), HYDROCOL_DIST_BACKEND="gloo")
    ranks = multigpu.Ranks(expect=world)
    total = ranks.allreduce_sum(_random_table(2, 9, 6, 2, 7, 100 + rank))
    np.save(os.path.join(out_dir, f"r{rank}.npy"), total)
    ranks.close()


def test_gloo_world2_sum_of_two_tables_equals_the_single_table_bit_for_bit(tmp_path):
    mp.spawn(_sum_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    single = _random_table(2, 9, 6, 2, 7, 100) + _random_table(2, 9, 6, 2, 7, 101)
    for r in range(2):
        got = np.load(tmp_path / f"r{r}.npy")
        assert got.dtype == np.int64 and np.array_equal(got, single)
    a = profile_tables_to_stats(np.load(tmp_path / "r0.npy"), 2, 9, 6, 2, np.full((2, 6), 0.4), 1.0)
    b = profile_tables_to_stats(single, 2, 9, 6, 2, np.full((2, 6), 0.4), 1.0)
    for k, v in b.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(a[k], v, equal_nan=v.dtype.kind == "f"), k


def test_header_declares_and_the_library_exports_the_profile_entries():
    text = (REPO / "include" / "hydrocol.h").read_text()
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    for macro, value in (("HC_PROF_SCALE_PSI", PROF_SCALE_PSI), ("HC_PROF_SCALE_THETA", PROF_SCALE_THETA),
                         ("HC_PROF_SCALE_FLUX", PROF_SCALE_FLUX)):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(value) + r"\b", text), macro
    from hydromodel_amd import _lib as L
    if not L.LIB_PATH.exists():
        pytest.skip("libhydrocol.so has not been built")
    lib = L.load()
    for name in NEW_ENTRIES:
        assert name in L.EXPORTS and hasattr(lib, name), name
