"""The step table of tests/test_gpu_call_sequences.py: one call of every launch path with everything it needs, and
the comparer the sequences are held to (no GPU is needed to import this module or to build a batch).

A step is a name, a panel, the environment switches and the precision it sets, `run(engine)` → {output name: array},
and the counters the call must leave behind: yfm_last_batch_flags, _deferred, _grad_unavailable and _steady.  The
numbers are constructed, not read off a run.  Every batch is a few finite candidates of a committed fixture plus

    n_nan   candidates with Φ = I exactly (unconstrained diagonal 40: initialize_filter throws, NaN),
    n_neg   candidates with σ² = e^−800 = 0 (grad_rule.bad_sigma: −Inf),
            — for TVλ both written in the constrained space, see space_of —
    n_col   candidates with λ ≈ 148 (grad_rule.collinear: DNS and GNS5 hand them to the double-double kernel),

and a family's rule says what it counts:

    flags        (n_nan, n_neg) for every family that evaluates the loglik; (n_nan, 0) for loss_array, which counts
                 its own rows again: σ² = 0 leaves the filtered states and so every mse finite (oracle/kalman_oracle.py
                 get_loss_array agrees); (0, 0) for predict of the λ and neural kinds, whose record mode evaluates no loss
    deferred     n_col
    unavailable  0 where the family defines none (loglik, filter_states, predict, forecast, loss_array);
                 n_col for the DNS tangent calls (gradient, scores); 0 for the TVλ tangent calls, which count only
                 candidates with a finite loglik; n_nan + n_neg + n_col for the smoothers and the information calls
                 (every candidate whose outputs are NaN)
    steady       0: the frozen-covariance instantiation is loglik-mode DNS with T ≥ 80 only, and the table's panels
                 are shorter (the one step at T = 80 switches it off)

The λ and neural kinds have neither initialize_filter nor σ²: their −Inf candidates are windows over a missing panel
column (the `nan6` fixtures: T_use = 5, 8, 8 with column 5 missing), flags (0, 2).  The two calls that must launch
nothing return {} and define no counters; estimate and nm_block run many launches and define none either.

The dirtier D is the one step whose steady count cannot be constructed: its expectation is None there and the fresh
context's number is used (DIRTIER_T holds the panel length it was found at).
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from functools import lru_cache
from typing import Callable

import numpy as np

from conftest import GOLDEN
from gpu_scenarios import same_bits
from grad_rule import bad_sigma, collinear
from yfm_amd import KIND_DNS, KIND_GNS, KIND_TVL, _lib
from yfm_amd import synthetic as S
from yfm_amd.params import KIND_NNS, KIND_SD_NS, n_params, param_layout, transform_params

# The dirtier's panel: the smallest T of {200, 400, 600} at which its batch leaves last_steady() > 0 (measured on an
# MI355X: T = 200 gives 760 steady wave-steps; the steady instantiation starts at T = 80).
DIRTIER_T = 200
DIRTIER_STEADY = 760

PIPE_CHUNK = 131072   # yfm_capi.hip kPipeChunk: a host-pointer DNS batch of ≥ 2 of these goes chunk by chunk
SMOOTH_CHUNK = 2334   # yfm_capi.hip smooth_chunk at M = 3, T = 600: (128 MiB) / (8 · 12 · 599)

YFM_EINVAL, YFM_EUNSUPPORTED = -1, -4
ENV_KEYS = ("YFM_DNS_SPLIT", "YFM_DNS_STEADY", "YFM_GNS5_INIT_LANES", "YFM_GNS5_STEADY", "YFM_MSED_LANES",
            "YFM_TVL_LANES", "YFM_TVL_EXP", "YFM_DNS_KTRIM", "YFM_EST_GROUPS", "YFM_SMOOTH_SWEEP")


# ---- fixtures and batches --------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _npz(rel: str) -> dict:
    with np.load(GOLDEN / f"{rel}.npz", allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def fixture_case(rel: str, name: str) -> dict:
    """The fields of case `name` of a fixture whose keys are `name/field`."""
    pre = name + "/"
    return {k[len(pre):]: v for k, v in _npz(rel).items() if k.startswith(pre)}


def flat_case(rel: str, name: str) -> dict:
    """The same for the λ and neural fixtures, whose keys are `name_field`."""
    pre = name + "_"
    return {k[len(pre):]: v for k, v in _npz(rel).items() if k.startswith(pre)}


def space_of(kind: int) -> int:
    """The parameter space a Kalman-kind step passes its batch in: the unconstrained one, except TVλ.  Under
    YFM_PREC_CERTIFIED the TVλ kernel evaluates the transform in double-double, as the binary128 truth does
    (oracle/yfm_truth.c), so an unconstrained Φ diagonal of 40 is 1 − 8.5e−18 there, I − Φ is regular and the loglik
    finite, while the FP64 reference throws.  Φ = I written in the constrained space is exact under either precision
    (tests/test_gpu_tvl_grad.py: test_patterns does the same)."""
    return 1 if kind == KIND_TVL else 0


def phi_identity(kind: int, th: np.ndarray, space: int = 0) -> np.ndarray:
    """Φ = I exactly: initialize_filter throws.  Unconstrained, the diagonal is 40 (2eˣ/(1 + eˣ) − 1 is 1.0 in FP64)."""
    lay = param_layout(kind)
    th = th.copy()
    th[lay.phi_offset:lay.phi_offset + lay.M * lay.M] = np.eye(lay.M).reshape(-1) * (40.0 if space == 0 else 1.0)
    return th


def zero_sigma(kind: int, th: np.ndarray, space: int = 0) -> np.ndarray:
    """σ² = e^−800 = 0 (−Inf): grad_rule.bad_sigma, the same row of the GNS5 layout (it has no entry in
    grad_rule.SPACE_ROWS), or the 0.0 itself in the constrained space."""
    if space == 0 and kind in (KIND_DNS, KIND_TVL):
        return bad_sigma(kind, th)
    th = th.copy()
    th[param_layout(kind).base_offset] = -800.0 if space == 0 else 0.0
    return th


def raise_counters(kind: int, good: np.ndarray, n_nan: int = 1, n_neg: int = 2, n_col: int = 0,
                   space: int = 0) -> np.ndarray:
    """Θ[P, G + n_nan + n_neg + n_col]: the finite candidates `good` (unconstrained; transformed for space 1) with the
    counter-raising ones after the first of them, each made from another good column so that no two candidates of the
    batch are equal."""
    good = np.asarray(good, dtype=np.float64)
    if space == 1:
        good = transform_params(kind, good)
    cols = [np.array(good[:, j]) for j in range(good.shape[1])]
    G = len(cols)
    extra = [phi_identity(kind, cols[i % G], space) for i in range(n_nan)]
    extra += [zero_sigma(kind, cols[(i + 1) % G], space) for i in range(n_neg)]
    extra += [collinear(cols[(i + 2) % G]) for i in range(n_col)]
    return np.asfortranarray(np.stack([cols[0], *extra, *cols[1:]], axis=1))


# ---- the step ----------------------------------------------------------------------------------------------------------
@dataclass
class Step:
    name: str
    panel: Callable[[], tuple]            # () → (Y, maturities)
    run: Callable[[object], dict]         # engine → {output name: array}
    env: dict = field(default_factory=dict)
    precision: int | None = None
    flags: tuple | None = (0, 0)          # None: the call defines no counters (nothing is compared after it)
    deferred: int = 0
    unavailable: int = 0
    steady: int | None = 0                # None: not constructible, the fresh context's number is used
    value: str | None = None              # the output whose NaN / −Inf counts are the flags
    kind: int | None = None
    space: int = 0
    batch: Callable[[], np.ndarray] | None = None  # () → Θ of a Kalman-kind step (the CPU oracle can evaluate it)

    def expected(self) -> dict | None:
        if self.flags is None:
            return None
        return {"flags": tuple(self.flags), "deferred": self.deferred, "unavailable": self.unavailable,
                "steady": self.steady}


def read_counters(engine) -> dict:
    return {"flags": tuple(engine.last_flags()), "deferred": engine.last_deferred(),
            "unavailable": engine.last_grad_unavailable(), "steady": engine.last_steady()}


def execute(engine, step: Step):
    """The step on `engine`: its switches, precision and panel, the call, the counters read after it (None where the
    step defines none).  The environment and the precision are put back whatever happens."""
    old_env = {k: os.environ.get(k) for k in ENV_KEYS}
    old_prec = engine.precision
    try:
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(step.env)
        if step.precision is not None:
            engine.precision = step.precision
        engine.set_panel(*step.panel())
        out = {k: np.array(v) for k, v in step.run(engine).items() if v is not None}
        return out, (read_counters(engine) if step.flags is not None else None)
    finally:
        engine.precision = old_prec
        for k, v in old_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_fresh: dict = {}


def fresh_result(step: Step, device: int = 0):
    """The step on a context that has run only set_panel and the step: computed once, the context closed at once."""
    if step.name not in _fresh:
        from yfm_amd.engine import Engine
        eng = Engine(device)
        try:
            _fresh[step.name] = execute(eng, step)
        finally:
            eng.close()
    return _fresh[step.name]


# ---- the comparer ------------------------------------------------------------------------------------------------------
def assert_same_result(got, want, what: str = ""):
    """(outputs, counters) of two runs of a step: the same output names, every output the same bits (NaN payloads
    included) and every counter equal."""
    (g_out, g_cnt), (w_out, w_cnt) = got, want
    assert set(g_out) == set(w_out), (what, sorted(g_out), sorted(w_out))
    for k in sorted(w_out):
        assert same_bits(g_out[k], w_out[k]), (what, k)
    assert g_cnt == w_cnt, (what, g_cnt, w_cnt)


def assert_constructed(step: Step, got, what: str = ""):
    """The counters of a run against the table's constructed numbers (a None steady: not constructible, skipped), and
    the NaN and −Inf counts of the step's own values against the flags."""
    out, cnt = got
    want = step.expected()
    if want is None:
        assert cnt is None, (what, step.name)
        return
    if want["steady"] is None:
        want = dict(want, steady=cnt["steady"])
    assert cnt == want, (what, step.name, cnt, want)
    if step.value is not None:
        v = out[step.value]
        assert (int(np.isnan(v).sum()), int(np.isneginf(v).sum())) == tuple(step.flags), (what, step.name, v)


# ---- panels ------------------------------------------------------------------------------------------------------------
def _panel_of(case: dict):
    return lambda: (np.asfortranarray(case["Y"]), np.ascontiguousarray(case["maturities"]))


GRAD = "grad/grad_cases"
TVLG = "tvl_grad/tvl_grad_cases"
SMO = "smooth/smooth_cases"
TVLS = "tvl_smooth/tvl_smooth_cases"


@lru_cache(maxsize=None)
def _synthetic(kind: int, T: int, N: int):
    mats = S.maturities_30()[:N].copy() if N <= 30 else np.arange(1, N + 1, dtype=np.float64) * 4.0
    return S.simulate_panel(kind, T, maturities=mats), mats


def _padded(case: dict, T: int):
    """The case's panel with NaN columns up to T (tests/test_gpu_tvl_smooth.py pads T-E the same way)."""
    N, T0 = case["Y"].shape
    Y = np.full((N, T), np.nan, order="F")
    Y[:, :T0] = case["Y"]
    return Y, np.ascontiguousarray(case["maturities"])


# ---- the table ---------------------------------------------------------------------------------------------------------
def _named(names, values) -> dict:
    values = values if isinstance(values, tuple) else (values,)
    return dict(zip(names, values))


def _kalman(name, kind, panel, good, call, names, *, unavailable="none", n_nan=1, n_neg=2, n_col=None, env=None,
            precision=None, value="ll", flags=None, **kw) -> Step:
    """A step of a Kalman kind on `good` plus the counter-raising candidates; `call(engine)` is the bound method's
    name, `names` its outputs."""
    n_col = (1 if kind in (KIND_DNS, KIND_GNS) else 0) if n_col is None else n_col
    un = {"none": 0, "deferred": n_col, "all": n_nan + n_neg + n_col}[unavailable]

    space = space_of(kind)

    def batch():
        return raise_counters(kind, good, n_nan, n_neg, n_col, space)

    def run(engine):
        r = getattr(engine, call)(kind, batch(), space=space, **kw)
        return r if isinstance(r, dict) else _named(names, r)
    return Step(name, panel, run, env=env or {}, precision=precision, flags=flags or (n_nan, n_neg), deferred=n_col,
                unavailable=un, value=value, kind=kind, space=space, batch=batch)


def _window_kind(name, kind, rel, case, call, names, flags=(0, 2), **kw) -> Step:
    """A step of a λ or neural kind on its `nan6` fixture: candidate 0 on a window before the missing column, the
    other two over it (−Inf)."""
    c = flat_case(rel, case)
    assert list(c["T_use"]) == [5, 8, 8] and np.isnan(c["Y"][:, 5]).any()

    def run(engine):
        r = getattr(engine, call)(kind, c["theta"], space=0, T_use=c["T_use"], **kw)
        return r if isinstance(r, dict) else _named(names, r)
    return Step(name, _panel_of(c), run, flags=flags, value=names[0] if names[0] in ("ll", "loss") else None)


def dirtier_batch() -> np.ndarray:
    """64 candidates of θ₀ + 0.05·N(0, I) (one full wave that can freeze) and 3 Φ = I, 3 σ² = 0, 4 collinear."""
    good = S.theta_batch(KIND_DNS, 64, scale=0.05, seed=81, bad_frac=0.0)
    extra = [phi_identity(KIND_DNS, good[:, i]) for i in range(3)]
    extra += [bad_sigma(KIND_DNS, good[:, 3 + i]) for i in range(3)]
    extra += [collinear(good[:, 6 + i]) for i in range(4)]
    return np.asfortranarray(np.concatenate([good, np.stack(extra, axis=1)], axis=1))


def dirtier() -> Step:
    def run(engine):
        return _named(("ll", "grad"), engine.loglik_grad(KIND_DNS, dirtier_batch(), space=0))
    return Step("D", lambda: _synthetic(KIND_DNS, DIRTIER_T, 30), run, flags=(3, 3), deferred=4, unavailable=4,
                steady=None, value="ll", kind=KIND_DNS, batch=dirtier_batch)


def victim_inputs():
    """The panel of tests/test_gpu_workspace.py (N = 8, T = 40) and 12 finite candidates with 1 NaN, 2 −Inf and 1
    collinear one."""
    Y, mats = _synthetic(KIND_DNS, 40, 8)
    good = S.theta_batch(KIND_DNS, 12, scale=0.05, seed=82, bad_frac=0.0)
    return Y, mats, raise_counters(KIND_DNS, good, 1, 2, 1)


def victim() -> Step:
    def run(engine):
        return {"ll": engine.loglik(KIND_DNS, victim_inputs()[2])}
    return Step("V", lambda: victim_inputs()[:2], run, flags=(1, 2), deferred=1, value="ll", kind=KIND_DNS,
                batch=lambda: victim_inputs()[2])


def _pipelined() -> Step:
    """B = 2 · 131,072 + 16: three chunks, the second and third with continues = true; one NaN and one −Inf candidate
    in the first chunk and one each in the last."""
    c = fixture_case(GRAD, "E")
    B = 2 * PIPE_CHUNK + 16

    def run(engine):
        good = c["Theta"][:, :8]
        Th = np.asfortranarray(np.tile(good, (1, B // 8)))
        Th[:, 5] = phi_identity(KIND_DNS, good[:, 0])
        Th[:, 70000] = bad_sigma(KIND_DNS, good[:, 1])
        Th[:, B - 9] = phi_identity(KIND_DNS, good[:, 2])
        Th[:, B - 2] = bad_sigma(KIND_DNS, good[:, 3])
        return {"ll": engine.loglik(KIND_DNS, Th, space=0)}
    return Step("dns_loglik_pipelined", _panel_of(c), run, flags=(2, 2), value="ll")


def _smooth_two_chunks() -> Step:
    """S-E padded to T = 600 with NaN columns, B = 2,400 > 2,334: two chunks, the second with continues = true; one NaN
    and one −Inf candidate on each side of the boundary, so the counters are the sums."""
    c = fixture_case(SMO, "S-E")
    B = 2400
    assert (128 << 20) // (8 * 12 * 599) == SMOOTH_CHUNK < B

    def run(engine):
        good = c["Theta"][:, :2]
        Th = np.asfortranarray(np.tile(good, (1, B // 2)))
        Th[:, 7] = phi_identity(KIND_DNS, good[:, 0])
        Th[:, SMOOTH_CHUNK - 1] = bad_sigma(KIND_DNS, good[:, 1])
        Th[:, SMOOTH_CHUNK] = phi_identity(KIND_DNS, good[:, 1])
        Th[:, B - 1] = bad_sigma(KIND_DNS, good[:, 0])
        return _named(("beta_s", "V_s"), engine.smooth(KIND_DNS, Th, space=0, lag_one=False)[:2])
    return Step("dns_smooth_two_chunks", lambda: _padded(c, 600), run, flags=(2, 2), unavailable=4)


def _empty() -> Step:
    c = fixture_case(GRAD, "A")
    return Step("dns_loglik_empty", _panel_of(c),
                lambda engine: {"ll": engine.loglik(KIND_DNS, np.empty((n_params(KIND_DNS), 0), order="F"))},
                value="ll")


def _estimate() -> Step:
    def run(engine):
        starts = S.theta_batch(KIND_DNS, 32, seed=73, bad_frac=0.0, scale=0.05)
        r = engine.estimate(KIND_DNS, starts, space=0, iterations=3, max_group_iters=1)
        assert r["ll"].shape == (32,) and (r["status"] == 0).all()
        return dict(r, n_evals=np.array([r["n_evals"]]))
    return Step("dns_estimate_two_groups", lambda: victim_inputs()[:2], run, flags=None)


def _nm_block() -> Step:
    mats4 = np.array([3.0, 12.0, 60.0, 120.0])

    def run(engine):
        p0 = S.theta_batch(KIND_SD_NS, 3, scale=0.1, seed=15, bad_frac=0.0)
        X, f, n = engine.nm_block(KIND_SD_NS, p0, np.arange(n_params(KIND_SD_NS) - 12),
                                  T_use=np.array([40, 24, 12], dtype=np.int32), iterations=8, g_tol=1e-6)
        return {"X": X, "f": f, "n_evals": np.array([n])}
    return Step("lambda_nm_block", lambda: (S.simulate_panel(KIND_SD_NS, 40, maturities=mats4, seed=7), mats4), run,
                flags=None)


def _raises(engine, code, call):
    try:
        call()
    except _lib.YFMError as e:
        assert e.code == code, (e.code, str(e))
        return {}
    raise AssertionError("the call was accepted")


def _refused() -> Step:
    """yfm_loglik_scores_batch on GNS5: YFM_EUNSUPPORTED from the C ABI (Engine.loglik_scores would refuse in Python
    before the library saw the call)."""
    c = fixture_case(SMO, "G-E")
    return Step("gns_scores_refused", _panel_of(c),
                lambda engine: _raises(engine, YFM_EUNSUPPORTED, lambda: engine._scores_call(
                    "yfm_loglik_scores_batch", KIND_GNS, c["Theta"], 0, None)), flags=None)


def _invalid() -> Step:
    c = fixture_case(GRAD, "E")
    T = c["Y"].shape[1]
    return Step("dns_loglik_T_use_out_of_range", _panel_of(c),
                lambda engine: _raises(engine, YFM_EINVAL, lambda: engine.loglik(
                    KIND_DNS, c["Theta"][:, :3], T_use=np.array([T, T + 1, 2], dtype=np.int32))), flags=None)


def build_table() -> dict:
    gA, gD, gE = (fixture_case(GRAD, n) for n in ("A", "D", "E"))
    tC, tD = (fixture_case(TVLG, n) for n in ("C", "D"))
    sE, sN, gnsE = (fixture_case(SMO, n) for n in ("S-E", "S-nan", "G-E"))
    tE = fixture_case(TVLS, "T-E")
    k4, k16 = "msed_fullgrad/msed_fullgrad_cases", "msedn_fullgrad/msedn_fullgrad_cases"
    fin = lambda c, n: c["Theta"][:, np.flatnonzero(c["compared"])[:n]]  # noqa: E731  (candidates with a finite loglik)
    n65 = lambda: _synthetic(KIND_DNS, 12, 65)  # noqa: E731
    t80 = lambda: _synthetic(KIND_DNS, 80, 30)  # noqa: E731
    good65 = S.theta_batch(KIND_DNS, 10, scale=0.05, seed=83, bad_frac=0.0)
    traj = ("preds", "factors", "states", "factor_loadings_1", "factor_loadings_2")
    cert, fp64 = _lib.PREC_CERTIFIED, _lib.PREC_FP64
    steps = [
        # loglik, one per launch path
        _kalman("dns_loglik_n30", KIND_DNS, _panel_of(gA), fin(gA, 12), "loglik", ("ll",)),
        _kalman("dns_loglik_n65_group", KIND_DNS, n65, good65, "loglik", ("ll",)),
        _kalman("dns_loglik_split", KIND_DNS, _panel_of(gA), fin(gA, 12), "loglik", ("ll",), env={"YFM_DNS_SPLIT": "1"}),
        _kalman("dns_loglik_steady_off", KIND_DNS, t80, good65, "loglik", ("ll",), env={"YFM_DNS_STEADY": "0"}),
        _kalman("gns_loglik_n7", KIND_GNS, _panel_of(gnsE), gnsE["Theta"], "loglik", ("ll",)),
        _kalman("gns_loglik_init_lanes_1", KIND_GNS, _panel_of(gnsE), gnsE["Theta"], "loglik", ("ll",),
                env={"YFM_GNS5_INIT_LANES": "1"}),
        _kalman("tvl_loglik_certified", KIND_TVL, _panel_of(tC), fin(tC, 12), "loglik", ("ll",), precision=cert),
        _kalman("tvl_loglik_fp64", KIND_TVL, _panel_of(tD), fin(tD, 12), "loglik", ("ll",), precision=fp64),
        _window_kind("lambda_loglik_k4", KIND_SD_NS, k4, "k4_n4t8nan6", "loglik", ("ll",)),
        _window_kind("neural_loglik_k16", KIND_NNS, k16, "k16_n4t8nan6", "loglik", ("ll",)),
        _empty(),
        _pipelined(),
        # the trajectory calls
        _kalman("dns_filter_states", KIND_DNS, _panel_of(gE), fin(gE, 6), "filter_states", ("ll", "beta", "P")),
        _kalman("dns_predict_h3", KIND_DNS, _panel_of(gE), fin(gE, 6), "predict", traj, value=None, horizon=3),
        _kalman("dns_forecast_h3", KIND_DNS, _panel_of(gE), fin(gE, 6), "forecast", ("blocks",), value=None, horizon=3),
        _kalman("dns_loss_array", KIND_DNS, _panel_of(gE), fin(gE, 6), "loss_array", ("mse",), value=None,
                flags=(1, 0)),
        _kalman("tvl_filter_states", KIND_TVL, _panel_of(tC), fin(tC, 6), "filter_states", ("ll", "beta", "P")),
        _kalman("tvl_predict_h3", KIND_TVL, _panel_of(tC), fin(tC, 6), "predict", traj, value=None, horizon=3),
        _kalman("tvl_forecast_h3", KIND_TVL, _panel_of(tC), fin(tC, 6), "forecast", ("blocks",), value=None, horizon=3),
        _kalman("tvl_loss_array", KIND_TVL, _panel_of(tC), fin(tC, 6), "loss_array", ("mse",), value=None,
                flags=(1, 0)),
        _window_kind("lambda_predict_k4", KIND_SD_NS, k4, "k4_n4t8nan6", "predict", traj, flags=(0, 0), horizon=3),
        _window_kind("neural_predict_k16", KIND_NNS, k16, "k16_n4t8nan6", "predict", traj, flags=(0, 0), horizon=3),
        # gradients
        _kalman("dns_grad", KIND_DNS, _panel_of(gD), fin(gD, 8), "loglik_grad", ("ll", "grad"), unavailable="deferred"),
        _kalman("tvl_grad", KIND_TVL, _panel_of(tD), fin(tD, 8), "tvl_loglik_grad", ("ll", "grad")),
        _window_kind("lambda_grad_k4", KIND_SD_NS, k4, "k4_n4t8nan6", "lambda_loss_grad", ("loss", "grad")),
        _window_kind("lambda_full_grad_k4", KIND_SD_NS, k4, "k4_n4t8nan6", "lambda_loss_full_grad", ("loss", "grad")),
        _window_kind("neural_grad_k16", KIND_NNS, k16, "k16_n4t8nan6", "neural_loss_grad", ("loss", "grad")),
        _window_kind("neural_full_grad_k16", KIND_NNS, k16, "k16_n4t8nan6", "neural_loss_full_grad", ("loss", "grad")),
        # scores and information
        _kalman("dns_scores", KIND_DNS, _panel_of(gE), fin(gE, 6), "loglik_scores", ("ll", "scores"),
                unavailable="deferred"),
        _kalman("dns_info_opg", KIND_DNS, _panel_of(gA), fin(gA, 5), "loglik_info", (), unavailable="all",
                hessian=False),
        _kalman("dns_info_hessian", KIND_DNS, _panel_of(gA), fin(gA, 5), "loglik_info", (), unavailable="all",
                opg=False),
        _kalman("dns_info_both", KIND_DNS, _panel_of(gD), fin(gD, 5), "loglik_info", (), unavailable="all"),
        _kalman("tvl_scores", KIND_TVL, _panel_of(tC), fin(tC, 6), "tvl_loglik_scores", ("ll", "scores")),
        _kalman("tvl_info_opg", KIND_TVL, _panel_of(tE), tE["Theta"][:, :1], "tvl_loglik_info", (), unavailable="all",
                n_neg=1, hessian=False),
        _kalman("tvl_info_both", KIND_TVL, _panel_of(tE), tE["Theta"][:, 1:2], "tvl_loglik_info", (), unavailable="all",
                n_neg=1),
        # smoothers
        _kalman("dns_smooth", KIND_DNS, _panel_of(sN), sN["Theta"], "smooth", ("beta_s", "V_s", "C_s"),
                unavailable="all", value=None),
        _kalman("gns_smooth", KIND_GNS, _panel_of(gnsE), gnsE["Theta"], "smooth", ("beta_s", "V_s", "C_s"),
                unavailable="all", value=None),
        _kalman("tvl_smooth", KIND_TVL, _panel_of(tE), tE["Theta"], "tvl_smooth", ("beta_s", "V_s", "C_s"),
                unavailable="all", value=None),
        _smooth_two_chunks(),
        # the estimators, and the two calls that must launch nothing
        _estimate(),
        _nm_block(),
        _refused(),
        _invalid(),
    ]
    table = {s.name: s for s in steps}
    assert len(table) == len(steps)
    return table


# one representative per launch path for the ordered pairs: N and T differ in both directions among their panels
# (30 × 40, 65 × 12, 7 × 12, 7 × 12, 67 × 16, 64 × 12, 64 × 12, 7 × 12, 6 × 12, 4 × 8, 4 × 8, 4 × 8, 30 × 40)
PAIR_STEPS = ("dns_loglik_n30", "dns_loglik_n65_group", "gns_loglik_n7", "tvl_loglik_certified", "tvl_loglik_fp64",
              "dns_grad", "dns_info_both", "tvl_scores", "dns_smooth", "tvl_smooth", "lambda_full_grad_k4",
              "neural_full_grad_k16", "dns_loglik_empty")
