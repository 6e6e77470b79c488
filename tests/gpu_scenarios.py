"""The two GPU scenarios every batched call family is held to, once: the `_device` entry on a side stream writes the
host-pointer call's bits, and a candidate's outputs do not depend on the batch around it.  The test functions stay in
their files with their panels, θ batches and windows; they pass the Engine methods in."""
from __future__ import annotations

import numpy as np


def same_bits(a, b):
    """Equal shapes and equal bits as FP64: 0.0 differs from −0.0, and two NaNs are equal only with equal payloads."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_same_bits(a, b, nan_payloads=True):
    """same_bits, or with nan_payloads=False numpy's equality (any NaN equals any NaN, 0.0 equals −0.0)."""
    if nan_payloads:
        assert same_bits(a, b), (a, b)
    else:
        np.testing.assert_array_equal(a, b)


def assert_device_entry_matches(host_call, device_call, kind, Th, tu, *, guard=0, nan_payloads=True, **kw):
    """host_call(kind, Th, T_use=tu, **kw) gives one array or a tuple of them, the candidate on the last axis; the
    device entry takes the same arrays column-major.  The device buffers (filled with 7.0, each between `guard` doubles
    that must stay 7.0) are made on the current stream, the side stream waits for it, device_call runs there, and after
    the stream's synchronize each output equals the host call's.  Returns the host call's outputs."""
    import torch
    P, B = Th.shape
    host = host_call(kind, Th, T_use=tu, **kw)
    host = tuple(np.array(h) for h in (host if isinstance(host, tuple) else (host,)))
    d_th = torch.from_numpy(np.ascontiguousarray(Th.T)).cuda()
    d_tu = torch.from_numpy(np.ascontiguousarray(tu, dtype=np.int32)).cuda()
    bufs = [torch.full((h.size + 2 * guard,), 7.0, dtype=torch.float64, device="cuda") for h in host]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        device_call(kind, d_th.data_ptr(), P, B, *(d.data_ptr() + 8 * guard for d in bufs), d_T_use=d_tu.data_ptr(),
                    stream=s.cuda_stream, **kw)
    s.synchronize()
    for h, d in zip(host, bufs):
        buf = d.cpu().numpy()
        assert np.all(buf[:guard] == 7.0) and np.all(buf[guard + h.size:] == 7.0)
        assert_same_bits(buf[guard:guard + h.size].reshape(h.shape[::-1]).T, h, nan_payloads)
    return host


def assert_batch_independent(call, Th, solo, *, inside=None, nan_payloads=True):
    """call(Th) → (ll[B], g[P, B]).  The batch reversed gives the same bits per candidate, and so does each candidate of
    `solo` alone (B = 1).  inside = (Theta, idx, pos): the candidates `pos` of Th are the candidates `idx` of the larger
    batch Theta and have the same bits there.  Returns (ll, g) of Th."""
    ll, g = (np.array(x) for x in call(Th))
    llr, gr = call(np.asfortranarray(Th[:, ::-1]))
    assert_same_bits(llr[::-1], ll, nan_payloads)
    assert_same_bits(gr[:, ::-1], g, nan_payloads)
    for b in solo:
        l1, g1 = call(Th[:, b])
        assert_same_bits(l1[0], ll[b], nan_payloads)
        assert_same_bits(g1[:, 0], g[:, b], nan_payloads)
    if inside is not None:
        Theta, idx, pos = inside
        llA, gA = call(Theta)
        assert_same_bits(gA[:, idx], g[:, pos], nan_payloads)
        assert_same_bits(llA[idx], ll[pos], nan_payloads)
    return ll, g
