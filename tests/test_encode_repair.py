"""The two repairs of the screened encode (glc_kernels.h launch_encode_screened): the rows that fail the screen get
their exact columns C0.. either from k_mdct_fwd_small_cols (the row tiles that hold a failed row) or from
k_mdct_fwd_small_rows (one wave per two failed rows and 64 columns, found through the quantiser's per-wave fail
counts).  The record bytes must be the reference's whichever ran, and the host's choice between them must follow the
failed-row count the device reported last.

CPU: the new cases put exactly the intended rows in "fail", every row decided by a margin - so the GPU tests can hold
the repaired count to the row, and a repair that silently did nothing cannot pass.
GPU: every case of encode_screen_cases.cases() and the new ones with the screen forced on and the latency repair
forced, against oracle.encode_range_records and against the unscreened encode; then the automatic choice, launch by
launch, on one context."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encode_screen_cases as S  # noqa: E402
import test_encode_screen as T  # noqa: E402  (its cache of oracle records: one reference per case and session)
from encode_screen_cases import HOP, Case, _click, tones  # noqa: E402

R = 2  # failed rows of a work item of k_mdct_fwd_small_rows (glc_mdct_fwd.hpp GLC_SMALL_ROWS_R)
LOW = ([220.0, 1234.5, 3100.0, 6900.0], [0.3, 0.2, 0.1, 0.05])


def _mono(frames, f0, f1, fail_rows):
    x = tones(48000, 1, frames * HOP, *LOW)
    for r in fail_rows:
        _click(x, f0 + r)
    return x, f0, f1


def repair_cases():
    """name -> (Case, rows that must fail).  Mono: a row is a frame.  The fail counts are summed by lane l over the
    quantiser waves [4 l, 4 l + 4) at these sizes (ceil(M / 16) * 4 counts, 64 lanes, runs of a multiple of 4), i.e.
    rows [16 l, 16 l + 16): rows 15 and 16 lie on both sides of a boundary of that partition, and of two quantiser
    workgroups; rows 20 and 21 share a quantiser wave."""
    out = {}
    # R - 1 failed rows, and the failed row is row 0 of the launch
    x, f0, f1 = _mono(262, 3, 259, [0])
    out["rows-r-minus-1-row0"] = (Case("rows-r-minus-1-row0", "repair", 48000, 1, x, f0, f1), [0])
    # R failed rows, on both sides of a partition boundary, in different workgroups of the quantiser
    x, f0, f1 = _mono(310, 2, 303, [15, 16])
    out["rows-r-partition"] = (Case("rows-r-partition", "repair", 48000, 1, x, f0, f1), [15, 16])
    # R + 1 failed rows: two in one quantiser wave, and row M - 1 of M = 301 (no multiple of 16)
    x, f0, f1 = _mono(310, 2, 303, [20, 21, 300])
    out["rows-r-plus-1-last"] = (Case("rows-r-plus-1-last", "repair", 48000, 1, x, f0, f1), [20, 21, 300])
    # four channels: a frame's four rows fail together (the fused decision)
    x = tones(48000, 4, 72 * HOP, *LOW)
    _click(x, 4 + 33)
    out["ch4-one-frame"] = (Case("ch4-one-frame", "repair", 48000, 4, x, 4, 68), [132, 133, 134, 135])
    # eight channels: flags per row, decision in K3
    x = tones(48000, 8, 40 * HOP, *LOW)
    _click(x, 4 + 17)
    out["ch8-one-frame"] = (Case("ch8-one-frame", "repair", 48000, 8, x, 4, 36), list(range(136, 144)))
    return out


REPAIR = repair_cases()
ALL_NAMES = T.CASE_NAMES + list(REPAIR)


_existing = {}


def case_of(name):
    """The new case of that name, or the one of encode_screen_cases.cases() (built once)."""
    if name in REPAIR:
        return REPAIR[name][0]
    if not _existing:
        _existing.update({c.name: c for c in S.cases()})
    return _existing[name]


# ----------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(REPAIR))
def test_new_cases_fail_exactly_the_intended_rows(name):
    c, rows = REPAIR[name]
    assert 256 <= c.M <= 770
    _, _, v = T.expected(c)
    assert (v != 0).all(), f"{name}: rows {np.flatnonzero(v == 0)[:8].tolist()} are too close to the floor to call"
    assert np.flatnonzero(v == -1).tolist() == rows
    assert len(REPAIR["rows-r-minus-1-row0"][1]) == R - 1 and len(REPAIR["rows-r-partition"][1]) == R
    assert len(REPAIR["rows-r-plus-1-last"][1]) == R + 1 and REPAIR["rows-r-plus-1-last"][0].M % 16 != 0


# ----------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU (no CPU fallback exists)"
    import glc_amd
    S.bind(glc_amd)
    encoders = {}

    def encoder(sr):
        if sr not in encoders:
            encoders[sr] = glc_amd.Encoder(sr)
        return encoders[sr]
    yield torch, glc_amd, encoder
    for e in encoders.values():
        e.close()


def _repairs(glc_amd, enc):
    """(screened launches repaired by k_mdct_fwd_small_cols, by k_mdct_fwd_small_rows) of a context so far."""
    a, b = C.c_uint64(), C.c_uint64()
    assert glc_amd.lib.glc_debug_encode_repair_stats(enc._h, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL_NAMES)
def test_gpu_records_equal_the_oracle_with_the_latency_repair_forced(gpu, name):
    torch, glc_amd, encoder = gpu
    c = case_of(name)
    exp, _, v = T.expected(c)
    enc = encoder(c.sr)
    assert glc_amd.lib.glc_debug_set_encode_repair(enc._h, 2) == 0
    try:
        r0 = _repairs(glc_amd, enc)
        on, screened, repaired = S.records(torch, glc_amd, enc, c, 2)      # (sets the screen's mode: the repair's stays)
        r1 = _repairs(glc_amd, enc)
        off, screened_off, repaired_off = S.records(torch, glc_amd, enc, c, 1)
    finally:
        assert glc_amd.lib.glc_debug_set_encode_repair(enc._h, 0) == 0
    assert (r1[0] - r0[0], r1[1] - r0[1]) == (0, 1), f"{name}: the launch did not take the latency repair"
    assert (screened_off, repaired_off) == (0, 0) and _repairs(glc_amd, enc) == r1, f"{name}: mode 1 took the screened path"
    assert np.array_equal(off, exp), f"{name}, screen off: {S.explain(off, exp, c.ch)}"
    assert np.array_equal(on, exp), f"{name}, latency repair: {S.explain(on, exp, c.ch)}"
    assert np.array_equal(on, off)
    assert screened == c.M, f"{name}: {screened} of {c.M} rows went through the screened path"
    lo, hi = int((v == -1).sum()), int((v != 1).sum())
    assert lo <= repaired <= hi, f"{name}: {repaired} rows repaired, the model has {lo}..{hi}"
    if c.expect == "pass":
        assert repaired == 0 and screened > 0
    if c.expect == "fail":
        assert repaired == c.M
    if name in REPAIR:
        assert repaired == len(REPAIR[name][1])


@pytest.mark.gpu
def test_gpu_automatic_choice_follows_the_last_count(gpu):
    """One context, the screen forced on, the repair automatic, the stream waited for after every launch: a context
    that has read no count takes today's repair; the 2 failed rows of launch 1 send launch 2 to the latency repair,
    and launch 3 - noise, every row fails - still goes there on launch 2's count; its own count sends launch 4 back."""
    torch, glc_amd, _ = gpu
    mixed, noise = case_of("mixed-one-frame"), case_of("fail-noise")
    enc = glc_amd.Encoder(48000)
    try:
        assert glc_amd.lib.glc_debug_set_encode_screen(enc._h, 2) == 0
        order = []
        for c in (mixed, mixed, noise, mixed):
            exp, _, v = T.expected(c)
            r0 = _repairs(glc_amd, enc)
            got, screened, repaired = S.records(torch, glc_amd, enc, c, None)
            r1 = _repairs(glc_amd, enc)
            assert np.array_equal(got, exp), f"launch {len(order) + 1}: {S.explain(got, exp, c.ch)}"
            assert screened == c.M and repaired == int((v == -1).sum())
            order.append((r1[0] - r0[0], r1[1] - r0[1]))
        assert order == [(1, 0), (0, 1), (0, 1), (1, 0)], order
    finally:
        enc.close()
