"""The committed gradient fixture (tests/golden/grad/grad_cases.npz) is what its generator makes: case E (N = 4,
T = 8, 16 candidates) is regenerated from the binary128 truth and compared; every case keeps the fields and
the comparison cap the GPU test relies on."""
from __future__ import annotations

import sys

import numpy as np

from conftest import GOLDEN

sys.path.insert(0, str(GOLDEN / "grad"))
import make_grad as MG  # noqa: E402

FIELDS = {"Y", "maturities", "Theta", "T_use", "g_fd", "e_fd", "compared", "loglik_oracle", "loglik_truth"}
COMPARED = {"A": 69, "A-windows": 66, "A-nan": 16, "B": 15, "C": 16, "D": 14, "E": 13}


def test_case_e_regenerates():
    old = MG.load_cases()["E"]
    new = MG.make_case("E")
    assert set(new) == FIELDS
    for k in ("Y", "maturities", "Theta", "T_use", "compared"):
        np.testing.assert_array_equal(new[k], old[k], err_msg=k)
    # binary128 arithmetic is deterministic; the differences' last bits may depend on the libm in use
    for k in ("g_fd", "loglik_truth", "loglik_oracle"):
        np.testing.assert_allclose(new[k], old[k], rtol=1e-12, atol=0, err_msg=k)
    np.testing.assert_allclose(new["e_fd"], old["e_fd"], rtol=1e-3, atol=1e-13 * np.abs(old["g_fd"]).max())


def test_cases_keep_their_shape_and_cap():
    cases = MG.load_cases()
    assert tuple(cases) == MG.CASE_NAMES
    for name, c in cases.items():
        assert set(c) == FIELDS, name
        P, B = c["Theta"].shape
        assert P == 20 and c["g_fd"].shape == (P, B) and c["e_fd"].shape == (B,)
        assert int(c["compared"].sum()) == COMPARED[name] and c["compared"].mean() >= 0.75, name
        ok = c["compared"]
        assert np.all(c["e_fd"][ok] <= 1e-9 * np.abs(c["g_fd"]).max(axis=0)[ok])
    w = cases["A-windows"]
    short = w["T_use"] <= 2
    assert short.sum() == 28 and np.all(w["g_fd"][:, short] == 0.0) and np.all(w["loglik_truth"][short] == 0.0)
    assert np.isnan(cases["A-nan"]["Y"]).sum() == 3 + 30 and cases["C"]["Y"].shape[0] == 33
    assert cases["D"]["Y"].shape[0] == 64 and cases["B"]["Y"].shape[0] == 10
