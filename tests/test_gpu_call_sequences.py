"""What one call leaves behind for the next on the same yfm_ctx (yfm_capi.hip: launch / enqueue, yfm_flags.hpp).

A launch uses the counter bank its predecessor zeroed and its own first kernel zeroes the other one; no memset is
enqueued, so every launch path has to honour `flags_next`, every restore has to hit the right bank, and the shared work
buffers (the deferral list, the scratch records, the staging arrays) have to be sized and filled by the call that reads
them.  The families' own files read the counters only after their own call, on whatever the session engine was left
with; here every step of tests/call_steps.py runs

    D, X, V     after the dirtier D (all five counters non-zero, measured at T = 200: flags (3, 3), 4 deferred, 4
                without a gradient, 760 steady wave-steps) and before the victim V (a plain DNS loglik, also held to
                the C oracle at the project's 1e-9 rule): X uses the bank D zeroed and V the bank X had to zero, which
                still holds D's numbers if X did not;
    X, Y        over the ordered pairs of one representative per launch path, on panels whose N and T grow and shrink;
    E, Y        after every `_device` entry on a torch side stream, without synchronising in between.

The reference of a step is the step on a fresh context that ran only set_panel and the step (call_steps.fresh_result:
once per step, the context closed at once); outputs are compared bit for bit, NaN payloads included, and the counters
with the fresh run's and with the table's constructed numbers.  The sequences run on an Engine of this module's own.

Slowest case on an MI355X: the two-chunk smoother, 0.33 s; the whole file 3.9 s (profiles/call_sequences/).
"""
from __future__ import annotations

import numpy as np
import pytest

import call_steps as CS
from gpu_scenarios import assert_same_bits
from test_gpu_parity import assert_parity
from yfm_amd import KIND_DNS, KIND_TVL
from yfm_amd.params import KIND_NNS, KIND_SD_NS

pytestmark = pytest.mark.gpu

TABLE = CS.build_table()
D, V = CS.dirtier(), CS.victim()


@pytest.fixture(scope="module")
def seq():
    """The sequence engine: this module's own context, closed at its end (never more than this one and the fresh
    context of a reference open at a time)."""
    import torch  # noqa: F401  (bind libyfm_hip to torch's HIP runtime when both are loaded)
    from yfm_amd.engine import Engine
    eng = Engine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def victim_oracle():
    from oracle.truth import loglik_oracle, loglik_truth
    Y, mats, Th = CS.victim_inputs()
    return loglik_oracle(KIND_DNS, Y, mats, Th), loglik_truth(KIND_DNS, Y, mats, Th)


def check(step, got, what):
    """A run of `step` in a sequence: the fresh context's bits and counters, and the table's constructed counters."""
    CS.assert_same_result(got, CS.fresh_result(step), what)
    CS.assert_constructed(step, got, what)


@pytest.mark.parametrize("name", list(TABLE))
def test_counters_and_bits_after(seq, victim_oracle, name):
    x = TABLE[name]
    d = CS.execute(seq, D)
    got_x = CS.execute(seq, x)
    got_v = CS.execute(seq, V)
    print(name, "D", d[1], "X", got_x[1], "V", got_v[1])
    check(D, d, "D")
    assert d[1]["steady"] > 0
    check(x, got_x, f"{name} after D")
    check(V, got_v, f"V after D, {name}")
    assert_parity(got_v[0]["ll"], *victim_oracle)


PAIRS = [(a, b) for a in CS.PAIR_STEPS for b in CS.PAIR_STEPS if a != b]


@pytest.mark.parametrize("first,second", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
def test_ordered_pairs(seq, first, second):
    CS.execute(seq, TABLE[first])
    check(TABLE[second], CS.execute(seq, TABLE[second]), f"{second} after {first}")


# ---- `_device` entries on a side stream -------------------------------------------------------------------------------
def device_panel():
    """N = 4, T = 8 (grad case E) with column 5 missing: every kind takes it, the Kalman kinds step over the column
    and a λ or neural window over it is −Inf."""
    c = CS.fixture_case(CS.GRAD, "E")
    Y = np.array(c["Y"], order="F")
    Y[:, 5] = np.nan
    return Y, np.ascontiguousarray(c["maturities"])


def _dns_batch():
    c = CS.fixture_case(CS.GRAD, "E")
    return CS.raise_counters(KIND_DNS, c["Theta"][:, np.flatnonzero(c["compared"])[:6]], 1, 2, 1)


def _tvl_batch():
    return CS.raise_counters(KIND_TVL, CS.fixture_case(CS.TVLS, "T-E")["Theta"], 1, 2, 0, CS.space_of(KIND_TVL))


def _window_batch(rel, case):
    c = CS.flat_case(rel, case)
    return np.asfortranarray(c["theta"]), np.array([5, 8, 8], dtype=np.int32)


K4 = ("msed_fullgrad/msed_fullgrad_cases", "k4_n4t8nan6")
K16 = ("msedn_fullgrad/msedn_fullgrad_cases", "k16_n4t8nan6")

# entry → (kind, host method, () → (Θ, T_use or None), keywords of both calls)
ENTRIES = {
    "loglik_device": (KIND_DNS, "loglik", lambda: (_dns_batch(), None), {}),
    "loglik_grad_device": (KIND_DNS, "loglik_grad", lambda: (_dns_batch(), None), {}),
    "tvl_loglik_grad_device": (KIND_TVL, "tvl_loglik_grad", lambda: (_tvl_batch(), None), {}),
    "loglik_scores_device": (KIND_DNS, "loglik_scores", lambda: (_dns_batch(), None), {}),
    "tvl_loglik_scores_device": (KIND_TVL, "tvl_loglik_scores", lambda: (_tvl_batch(), None), {}),
    "smooth_device": (KIND_DNS, "smooth", lambda: (_dns_batch(), None), {}),
    "tvl_smooth_device": (KIND_TVL, "tvl_smooth", lambda: (_tvl_batch(), None), {}),
    "lambda_loss_grad_device": (KIND_SD_NS, "lambda_loss_grad", lambda: _window_batch(*K4), {}),
    "lambda_loss_full_grad_device": (KIND_SD_NS, "lambda_loss_full_grad", lambda: _window_batch(*K4), {}),
    "neural_loss_grad_device": (KIND_NNS, "neural_loss_grad", lambda: _window_batch(*K16), {}),
    "neural_loss_full_grad_device": (KIND_NNS, "neural_loss_full_grad", lambda: _window_batch(*K16), {}),
}


def _after_steps() -> dict:
    """The three synchronous calls that follow an entry, on the entries' panel."""
    c = CS.fixture_case(CS.GRAD, "E")
    good = c["Theta"][:, np.flatnonzero(c["compared"])[:6]]
    tE = CS.fixture_case(CS.TVLS, "T-E")["Theta"]
    steps = [
        CS._kalman("tvl_loglik@device_panel", KIND_TVL, device_panel, tE, "loglik", ("ll",)),
        CS._kalman("dns_smooth@device_panel", KIND_DNS, device_panel, good, "smooth", ("beta_s", "V_s", "C_s"),
                   unavailable="all", value=None),
        CS._kalman("dns_info_opg@device_panel", KIND_DNS, device_panel, good, "loglik_info", (), unavailable="all",
                   hessian=False),
    ]
    return {s.name: s for s in steps}


AFTER = _after_steps()
GUARD = 16


class DeviceLaunch:
    """The setup of gpu_scenarios.assert_device_entry_matches without its synchronisation: the host-pointer call's
    outputs and device buffers filled with 7.0 between GUARD doubles that must stay 7.0; launch() enqueues the entry on
    a side stream (`after`: an event that stream waits for first) and returns at once; verify() once the stream is
    synchronised."""

    def __init__(self, engine, entry):
        import torch
        self.engine, self.entry = engine, entry
        self.kind, host_name, inputs, self.kw = ENTRIES[entry]
        Th, tu = inputs()
        self.P, self.B = Th.shape
        self.space = CS.space_of(self.kind)
        host = getattr(engine, host_name)(self.kind, Th, space=self.space, T_use=tu, **self.kw)
        self.host = tuple(np.array(h) for h in (host if isinstance(host, tuple) else (host,)))
        self.d_th = torch.from_numpy(np.ascontiguousarray(Th.T)).cuda()
        self.d_tu = None if tu is None else torch.from_numpy(np.ascontiguousarray(tu, dtype=np.int32)).cuda()
        self.bufs = [torch.full((h.size + 2 * GUARD,), 7.0, dtype=torch.float64, device="cuda") for h in self.host]
        self.stream = torch.cuda.Stream()

    def launch(self, after=None):
        import torch
        self.stream.wait_stream(torch.cuda.current_stream())
        if after is not None:
            self.stream.wait_event(after)
        with torch.cuda.stream(self.stream):
            getattr(self.engine, self.entry)(
                self.kind, self.d_th.data_ptr(), self.P, self.B, *(d.data_ptr() + 8 * GUARD for d in self.bufs),
                space=self.space, d_T_use=None if self.d_tu is None else self.d_tu.data_ptr(),
                stream=self.stream.cuda_stream, **self.kw)
        done = torch.cuda.Event()
        done.record(self.stream)
        return done

    def verify(self, what):
        for h, d in zip(self.host, self.bufs):
            buf = d.cpu().numpy()
            assert np.all(buf[:GUARD] == 7.0) and np.all(buf[GUARD + h.size:] == 7.0), what
            assert_same_bits(buf[GUARD:GUARD + h.size].reshape(h.shape[::-1]).T, h)


@pytest.mark.parametrize("after", list(AFTER))
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_device_entry_then_synchronous_call(seq, entry, after):
    y = AFTER[after]
    ref = CS.fresh_result(y)
    seq.set_panel(*device_panel())
    e = DeviceLaunch(seq, entry)
    e.launch()
    # no synchronisation: the synchronous call on the context's own stream must wait for the device itself
    got = CS.execute(seq, y)
    e.stream.synchronize()
    CS.assert_same_result(got, ref, f"{after} after {entry}")
    CS.assert_constructed(y, got, f"{after} after {entry}")
    e.verify(entry)


def test_device_entries_across_caller_streams(seq):
    """Three families on three streams, ordered by the caller's events (include/yfm.h): each output is its host call's
    and the counters read at the end are the last launch's — two windows over the missing column, nothing else."""
    seq.set_panel(*device_panel())
    entries = ("loglik_grad_device", "tvl_smooth_device", "lambda_loss_full_grad_device")
    launches = [DeviceLaunch(seq, entry) for entry in entries]  # the host-pointer calls first, then nothing synchronous
    ev = None
    for e in launches:
        ev = e.launch(after=ev)  # the caller orders its stream switch
    launches[-1].stream.synchronize()
    for entry, e in zip(entries, launches):
        e.verify(entry)
    assert CS.read_counters(seq) == {"flags": (0, 2), "deferred": 0, "unavailable": 0, "steady": 0}
