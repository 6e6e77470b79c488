"""The committed estimation-length gradient fixtures keep what the GPU tests rely on, by the reference alone:
tests/golden/grad/grad_long_cases.npz (make_grad_long.py), tests/golden/tvl_grad/tvl_grad_long_cases.npz
(make_tvl_grad_long.py) and tests/golden/msed_fullgrad/msed_fullgrad_long.npz (make_msed_fullgrad_long.py) — the
compared share of every case with a candidate to spare, the set of hard candidates, the stored κ₁(Z'Z), the λ
screen on the stored differences — and the cheap part of the DNS generator reproduces the file."""
from __future__ import annotations

import sys

import numpy as np

from conftest import GOLDEN, load_golden

for d in ("grad", "tvl_grad", "msed_fullgrad"):
    sys.path.insert(0, str(GOLDEN / d))
import make_grad_long as ML  # noqa: E402
import make_msed_fullgrad as MF  # noqa: E402
import make_msed_fullgrad_long as MFL  # noqa: E402
import make_tvl_grad_long as MTL  # noqa: E402

DNS_FIELDS = {"Y", "maturities", "Theta", "T_use", "g_fd", "e_fd", "h_used", "compared", "hard", "ref_err",
              "loglik_oracle", "loglik_truth"}
DNS_COMPARED = {"L": (47, 48), "L-windows": (16, 16), "L-hard": (6, 6), "L-n64": (8, 8), "L-band": (8, 8)}


def spare(compared):
    """At least 75% compared, and still so with one candidate fewer."""
    return (int(compared.sum()) - 1) / compared.size >= 0.75


def test_dns_cases_keep_their_shape_and_share():
    cases = ML.load_cases()
    assert tuple(cases) == ML.CASE_NAMES
    for name, c in cases.items():
        assert set(c) == DNS_FIELDS | ({"kappa1"} if name == "L-band" else set()), name
        P, B = c["Theta"].shape
        assert P == 20 and c["g_fd"].shape == (P, B) and c["e_fd"].shape == (B,)
        assert (int(c["compared"].sum()), B) == DNS_COMPARED[name] and spare(c["compared"]), name
        ok = c["compared"]
        assert np.all(c["e_fd"][ok] <= 1e-9 * np.abs(c["g_fd"]).max(axis=0)[ok])
        assert set(c["h_used"][ok]) <= set(ML.LADDER)
        err = np.abs(c["loglik_oracle"] - c["loglik_truth"]) / np.maximum(1.0, np.abs(c["loglik_truth"]))
        np.testing.assert_array_equal(c["hard"], np.isfinite(c["loglik_truth"]) & ~(err <= 1e-9))
        assert np.array_equal(np.isfinite(c["ref_err"]), c["hard"])
        if name != "L-hard":
            assert not c["hard"].any(), name
    assert cases["L"]["Y"].shape == (30, 600) and cases["L-n64"]["Y"].shape == (64, 200)
    assert cases["L-band"]["Y"].shape == (30, 120)


def test_dns_hard_candidates_are_the_four_named_bench_columns():
    c = ML.load_cases()["L-hard"]
    assert ML.HARD_COLUMNS == (10283, 1679, 5390, 22413, 0, 1)
    assert c["hard"].tolist() == [True, True, True, True, False, False]
    g = load_golden("dns_hard_T600")  # the same panel and candidates as the loglik fixture of the hard columns
    assert g["bench_index"].tolist() == list(ML.HARD_COLUMNS)
    np.testing.assert_array_equal(g["Y"], c["Y"])
    np.testing.assert_array_equal(g["Theta"], c["Theta"])
    # the plain FP64 reference is no closer than the differences' own error on any hard candidate
    assert np.all(c["ref_err"][c["hard"]] > c["e_fd"][c["hard"]])


def test_dns_windows_and_missing_columns():
    cases = ML.load_cases()
    w = cases["L-windows"]
    assert w["T_use"].tolist() == [200, 333, 599, 600] * 4
    nan = np.isnan(w["Y"])
    assert nan[:, 450].all() and nan[:, 598].sum() == 1 and nan[:, 599].sum() == 1 and nan.sum() == 32
    np.testing.assert_array_equal(w["Y"][~nan], cases["L"]["Y"][~nan])
    np.testing.assert_array_equal(w["Theta"], cases["L"]["Theta"][:, :16])
    # a window that ends before the missing columns is the plain panel's
    short = w["T_use"] == 200
    full = ML.TR.loglik_truth(ML.KIND_DNS, cases["L"]["Y"], w["maturities"], w["Theta"][:, short], space=0,
                              T_use=w["T_use"][short])
    np.testing.assert_array_equal(full, w["loglik_truth"][short])


def test_dns_band_stores_the_condition_numbers():
    c = ML.load_cases()["L-band"]
    assert c["Theta"][0].tolist() == list(ML.GAMMAS)
    np.testing.assert_allclose(c["kappa1"], [ML.kappa1(g, c["maturities"]) for g in ML.GAMMAS], rtol=1e-9)
    k1 = c["kappa1"]
    assert np.all(np.diff(k1) > 0) and k1[0] < 1e5 and k1[-1] > 1e7
    assert (k1 <= 5e5).sum() == 3 and ((k1 > 5e5) & (k1 < 2e6)).sum() == 3 and (k1 >= 2e6).sum() == 2
    assert ((k1 > 5e5) & (k1 < 1e6)).sum() == 2  # below the library's 1e6 threshold, above the certain band
    assert np.all(c["compared"])


def test_dns_band_regenerates():
    old = ML.load_cases()["L-band"]
    new = ML.make_case("L-band")
    for k in ("Y", "maturities", "Theta", "T_use", "compared", "hard", "h_used"):
        np.testing.assert_array_equal(new[k], old[k], err_msg=k)
    for k in ("g_fd", "loglik_truth", "loglik_oracle", "kappa1"):
        np.testing.assert_allclose(new[k], old[k], rtol=1e-12, atol=0, err_msg=k)


def test_tvl_cases_keep_their_shape_and_share():
    cases = MTL.load_cases()
    assert tuple(cases) == MTL.CASE_NAMES
    for name, c in cases.items():
        P, B = c["Theta"].shape
        assert P == 31 and B == (8 if name == "L600-windows" else 16)
        assert c["Y"].shape == (30, 200 if name == "L200" else 600)
        ok = c["compared"]
        assert int(ok.sum()) >= MTL.NEED[name] and spare(ok), (name, int(ok.sum()))
        assert np.all(c["e_fd"][ok] <= 1e-9 * np.abs(c["g_fd"]).max(axis=0)[ok])
        err = np.abs(c["loglik_oracle"] - c["loglik_truth"]) / np.maximum(1.0, np.abs(c["loglik_truth"]))
        assert np.all(err[ok] <= 1e-9)
        assert set(c["h_used"][ok]) <= set(MTL.LADDER)
    np.testing.assert_array_equal(cases["L200"]["Theta"], MTL.case_inputs("L200")[2])
    assert MTL.SEED == 20
    w = cases["L600-windows"]
    assert w["T_use"].tolist() == [200, 599, 600, 200, 599, 600, 200, 599]
    nan = np.isnan(w["Y"])
    assert nan[:, 450].all() and nan[:, 598].sum() == 1 and nan.sum() == 31
    np.testing.assert_array_equal(w["Theta"], cases["L600"]["Theta"][:, :8])
    np.testing.assert_array_equal(w["Theta"], MTL.case_inputs("L600-windows")[2])


def test_lambda_cases_keep_their_shape_and_screen():
    c = MFL.load_cases()
    assert c["Y"].shape == (30, 600) and not np.isnan(c["Y"]).any()
    for name in MFL.case_names():
        kind = int(name[1])
        K = MF.n_lead(kind)
        win = name.endswith("win")
        assert c[f"{name}_T_use"].tolist() == ([300, 600] if win else [600, 600])
        assert np.isnan(c[f"{name}_Y"]).sum() == (1 if win else 0) and bool(np.isnan(c[f"{name}_Y"][0, 450])) == win
        for space in (0, 1):
            g, e = c[f"{name}_g_fd_s{space}"], c[f"{name}_e_fd_s{space}"]
            assert g.shape == (K + 12, 2)
            for b in range(2):
                if win and b == 1:  # the window over the missing column: −Inf, no gradient
                    assert np.isnan(g[:, b]).all() and np.isneginf(c[f"{name}_loss_s{space}"][b])
                    continue
                top = np.max(np.abs(g[:, b]))
                assert np.isfinite(g[:, b]).all() and e[b] <= 1e-9 * top, (name, space, b, e[b] / top)
                assert np.all(np.abs(g[:K, b]) >= MF.SCREEN * top), (name, space, b)
