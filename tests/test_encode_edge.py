"""The edge path of the screened encode (csrc/glc_kernels.h EdgeLaunch): the frames whose window reaches into the
stream's zero padding - known on the host before anything is launched - get their exact coefficients and their records
on a side stream beside K1 and K2 instead of from the serial repair behind them.  The record bytes must be the
reference's whether the path is on or off, and the statistics must not tell the two apart.

CPU: the closed form of "edge frame" against the window test it stands for, the edge rows of every case, and that the
cap on edge rows is never binding.
GPU: every case with the screen forced on, through both forms of K1, with the edge path off (kind 1), forced with
either transform (kinds 2 and 3) and automatic (kind 0): records against oracle.encode_range_records and against each other, screened == M, rows_repaired
equal across kinds and within the model, the edge counters equal to the CPU model; then slot and event reuse on one
context, and a range of two chunks.

"Two or more trailing edge frames" cannot occur for any length (encode_edge_cases.py);
the lengths next to it are cases instead."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encode_edge_cases as E  # noqa: E402
import encode_screen_cases as S  # noqa: E402
from encode_screen_cases import HOP  # noqa: E402

CASES = {c.name: c for c in E.cases()}
RUNS = [(name, bound) for name, c in CASES.items() for bound in c.bounds]

_expected = {}


def expected(c):
    """Oracle records, taps and the screen's model of a case, computed once per session."""
    if c.name not in _expected:
        rec, taps = S.expected(c)
        _expected[c.name] = (rec, taps, S.model(c, taps))
    return _expected[c.name]


# ----------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ch", [1, 2, 3, 4, 8])
def test_edge_frames_equal_the_window_test(ch):
    worst = 0
    for hops in (0, 1, 2, 3, 7):
        for r in (0, 1, 511, 512, 513, 1023):
            per = hops * HOP + r
            for n_samples in {per * ch, max(per * ch - (ch - 1), 0)}:      # the last channels one sample short
                p, nf = E.plan(n_samples, ch)
                a, b = E.edge_frames(p, nf)
                assert 0 <= a <= b <= nf
                assert list(range(a)) + list(range(b, nf)) == E.brute_edge(p, nf), (n_samples, ch)
                assert nf - b <= 1, "more than one trailing edge frame"
                worst = max(worst, (a + nf - b) * ch)
    # the cap (4 frames x 8 channels) is never binding through glc_encode_range_device
    assert worst <= 2 * ch <= E.EDGE_ROWS_MAX


def test_edge_rows_of_the_cases():
    rows = {name: E.edge_rows(c) for name, c in CASES.items()}
    assert rows["mono-whole"] == [0, 139] and rows["mono-head"] == [0] and rows["mono-tail"] == [134]
    assert rows["mono-middle"] == [] and rows["mono-whole-262"] == [0, 261] == rows["mono-nan-inf"]
    assert rows["stereo-whole"] == [0, 1, 548, 549] and CASES["stereo-whole"].M % 16 == 6
    assert rows["ch1-ends-at-r300"] == [0, 138] and rows["ch1-ends-at-r512"] == [0] and rows["ch2-ends-at-r513"] == [274, 275]
    for name in ("stereo-click-frame-1", "stereo-silent-head", "stereo-noise-edges"):
        assert rows[name] == [0, 1, 278, 279]
    assert rows["ch4-whole"] == [0, 1, 2, 3, 260, 261, 262, 263]
    assert rows["ch3-whole"] == [0, 1, 2, 261, 262, 263]
    assert rows["ch8-whole"] == list(range(8)) + list(range(264, 272))
    assert all(len(r) <= E.EDGE_ROWS_MAX for r in rows.values())
    c = E.two_chunk_case()
    assert E.edge_rows(c) == [0, 1, 2 * 4395, 2 * 4395 + 1] and c.f1 - c.f0 > 4096


def test_cases_put_the_edge_rows_where_they_are_meant_to_be():
    """The click fails frame 1 (the serial repair's) beside the edge frame 0; the silent head's edge frame passes; the
    NaN and the infinity fail their edge frames; the noise makes both edge frames raw."""
    _, _, v = expected(CASES["stereo-click-frame-1"])
    assert (v[2:4] == -1).all() and (v[4:8] == 1).all()
    _, _, v = expected(CASES["stereo-silent-head"])
    assert (v[0:2] == 1).all()
    _, taps, v = expected(CASES["mono-nan-inf"])
    assert v[0] == -1 and v[261] == -1 and v[260] == -1 and v[1] == 1
    _, taps, v = expected(CASES["stereo-noise-edges"])
    assert taps.is_raw[0] and taps.is_raw[139] and (v[[0, 1, 278, 279]] == -1).all()


# ----------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU (no CPU fallback exists)"
    import glc_amd
    E.bind(glc_amd)
    enc = glc_amd.Encoder(48000)
    yield torch, glc_amd, enc
    enc.close()


def _pair(f, h):
    a, b = C.c_uint64(), C.c_uint64()
    assert f(h, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def _counters(glc_amd, enc):
    """(edge launches, edge rows, serial repair launches) of a context so far: host counters."""
    el, er = _pair(glc_amd.lib.glc_debug_encode_edge_stats, enc._h)
    return el, er, sum(_pair(glc_amd.lib.glc_debug_encode_repair_stats, enc._h))


def _set(glc_amd, enc, bound, kind):
    assert glc_amd.lib.glc_debug_set_encode_bound(enc._h, bound) == 0
    assert glc_amd.lib.glc_debug_set_encode_edge(enc._h, kind) == 0


def _run(gpu, enc, c, bound, kind, screen=2):
    torch, glc_amd, _ = gpu
    _set(glc_amd, enc, bound, kind)
    try:
        k0 = _counters(glc_amd, enc)
        rec, screened, repaired = S.records(torch, glc_amd, enc, c, screen)
        k1 = _counters(glc_amd, enc)
    finally:
        _set(glc_amd, enc, 0, 0)
    return rec, screened, repaired, tuple(y - x for x, y in zip(k0, k1))


@pytest.mark.gpu
def test_gpu_the_kinds_the_hook_takes(gpu):
    _, glc_amd, enc = gpu
    f = glc_amd.lib.glc_debug_set_encode_edge
    assert f(enc._h, 4) != 0 and f(enc._h, -1) != 0
    assert all(f(enc._h, k) == 0 for k in (1, 2, 3, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("name,bound", RUNS)
def test_gpu_records_equal_the_oracle_with_the_edge_path_off_forced_either_way_and_automatic(gpu, name, bound):
    c = CASES[name]
    exp, _, v = expected(c)
    n_edge = len(E.edge_rows(c))
    lo, hi = int((v == -1).sum()), int((v != 1).sum())
    got = {}
    for kind in (1, 2, 3, 0):
        rec, screened, repaired, (launches, rows, serial) = _run(gpu, gpu[2], c, bound, kind)
        assert np.array_equal(rec, exp), f"{name}, bound {bound}, kind {kind}: {S.explain(rec, exp, c.ch)}"
        assert screened == c.M, f"{name}: {screened} of {c.M} rows went through the screened path"
        assert lo <= repaired <= hi, f"{name}, kind {kind}: {repaired} rows repaired, the model has {lo}..{hi}"
        # the CPU model of the counters: one edge launch with the case's edge rows unless the path is off or there
        # are none; the serial repair is launched once per screened launch whatever the kind
        assert (launches, rows) == ((1, n_edge) if kind != 1 and n_edge else (0, 0)), (name, kind)
        assert serial == 1
        got[kind] = repaired
    assert got[1] == got[2] == got[3] == got[0], f"{name}: rows_repaired differs between the kinds: {got}"
    if name == "stereo-silent-head":
        assert got[1] == lo and not (v[:2] == -1).any()      # the passing edge frame counts as nothing


@pytest.mark.gpu
def test_gpu_slots_and_events_are_reused_without_waiting(gpu):
    """One context, launches alternating between ranges with and without edge frames, between channel counts and
    between kinds, queued back to back; the stream is waited for only at the end."""
    torch, glc_amd, _ = gpu
    order = [("mono-whole", 2), ("mono-middle", 2), ("stereo-whole", 0), ("mono-tail", 1), ("ch3-whole", 2),
             ("mono-head", 3), ("stereo-click-frame-1", 2), ("mono-middle", 0), ("ch8-whole", 3), ("mono-whole", 1),
             ("ch4-whole", 0), ("stereo-whole", 3)]
    enc = glc_amd.Encoder(48000)
    try:
        assert glc_amd.lib.glc_debug_set_encode_screen(enc._h, 2) == 0
        assert glc_amd.lib.glc_debug_set_encode_bound(enc._h, 2) == 0
        bufs, want_launches, want_rows = [], 0, 0
        for name, _ in order:
            c = CASES[name]
            sh, t0, tc = c.shard()
            rb = glc_amd.lib.glc_record_bytes(c.ch) * (c.f1 - c.f0)
            bufs.append((torch.from_numpy(sh.view(np.int32).copy()).cuda(), t0, tc,
                         torch.zeros(rb, dtype=torch.uint8, device="cuda")))
        torch.cuda.synchronize()
        for (name, kind), (d_pcm, t0, tc, d_rec) in zip(order, bufs):
            c = CASES[name]
            assert glc_amd.lib.glc_debug_set_encode_edge(enc._h, kind) == 0
            enc.encode_range_device(d_pcm.data_ptr(), t0, tc, c.n_samples, c.ch, c.f0, c.f1, d_rec.data_ptr())
            n_edge = len(E.edge_rows(c))
            if kind != 1 and n_edge:
                want_launches, want_rows = want_launches + 1, want_rows + n_edge
        enc.synchronize()
        for (name, kind), (_, _, _, d_rec) in zip(order, bufs):
            exp = expected(CASES[name])[0]
            got = d_rec.cpu().numpy()
            assert np.array_equal(got, exp), f"{name}, kind {kind}: {S.explain(got, exp, CASES[name].ch)}"
        assert _counters(glc_amd, enc)[:2] == (want_launches, want_rows)
        assert S.stats(glc_amd, enc)[0] == sum(CASES[name].M for name, _ in order)
    finally:
        enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bound", [1, 2])
def test_gpu_a_range_of_two_chunks_equals_the_unscreened_encode(gpu, bound):
    """4096 + 300 stereo frames: the start edge in chunk 0 on the caller's stream, the end edge in chunk 1 on the second
    one, each forking from the stream it runs on.  Against the same call with the screen off, which the other suites
    hold to the oracle (the oracle on 4396 frames is too slow for a test)."""
    c = E.two_chunk_case()
    on, screened, repaired, (launches, rows, serial) = _run(gpu, gpu[2], c, bound, 0)
    off, screened_off, repaired_off, k_off = _run(gpu, gpu[2], c, bound, 0, screen=1)
    assert (screened_off, repaired_off) == (0, 0) and k_off == (0, 0, 0)
    assert np.array_equal(on, off), S.explain(on, off, c.ch)
    assert screened == c.M and (launches, rows, serial) == (2, 4, 2)
    none, _, repaired_none, k_none = _run(gpu, gpu[2], c, bound, 1)
    assert np.array_equal(none, off) and repaired_none == repaired and k_none == (0, 0, 2)
