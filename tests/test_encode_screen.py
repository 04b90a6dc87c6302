"""The screened encode path (glc_kernels.h launch_encode_screened): exact transform below C0,
a fused-multiply-add upper bound for the columns of the last band above it, today's kernels for the rows whose bound
does not stay under the noise floor.  The bytes of every record must be the reference's for every input.

CPU: the bound itself - for the rows of every case and for adversarial sign patterns, the oracle's f32 coefficient
never exceeds the bound the kernel forms from a float32 emulation of the fused sums (this guards kScreenCErr) - the
cases' design (each outcome is really reached, by a margin), and the condition on the benchmark's own input.
GPU: every case through glc_debug_set_encode_screen mode 2 (forced on) and mode 1 (off) at 256..301 rows: record
bytes against oracle.encode_range_records and against each other, and the counts of screened / repaired rows
against the model - so a path that is silently off, or one that repairs everything, does not pass."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encode_screen_cases as S  # noqa: E402
from oracle import oracle as O  # noqa: E402

F32 = np.float32


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in S.cases()}


_expected = {}


def expected(case):
    """Oracle records and taps of a case, computed once per session."""
    if case.name not in _expected:
        rec, taps = S.expected(case)
        _expected[case.name] = (rec, taps, S.model(case, taps))
    return _expected[case.name]


CASE_NAMES = [c.name for c in S.cases()]


# ----------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------

def test_shapes_of_the_shipped_rates():
    assert [S.shape(sr)[1:] for sr in (44100, 48000, 96000, 192000)] == [(384, 6), (384, 6), (192, 3), (128, 2)]
    for sr in (44100, 48000, 96000, 192000):
        L, c0, _ = S.shape(sr)
        assert c0 - 64 < L <= c0


def test_cases_reach_the_outcome_they_are_built_for(cases):
    """Every case's rows are decided by a margin (none too close to call), and the families hold what they claim."""
    count = {}
    for name, c in cases.items():
        _, taps, v = expected(c)
        assert 256 <= c.M <= 768
        if c.family != "cross":   # (a ramp through the floor has rows on it by construction)
            assert (v != 0).all(), f"{name}: rows {np.flatnonzero(v == 0)[:8].tolist()} are too close to the floor to call"
        count[name] = int((v == -1).sum())
        if c.expect == "pass":
            assert count[name] == 0, name
        if c.expect == "fail":
            assert count[name] == c.M, name
    assert expected(cases["fail-noise-raw"])[1].is_raw.all() and not expected(cases["fail-noise"])[1].is_raw.any()
    assert count["mixed-one-frame"] == 2 and count["mixed-one-channel"] == 2      # one stereo frame
    v = expected(cases["mixed-partial-tile"])[2]
    assert np.flatnonzero(v == -1).tolist() == [280, 281]
    assert count["layout-ch3"] == 1 and count["layout-m-301"] == 1                 # per row where K3 decides / mono
    for name in ("layout-halo", "layout-sr44100", "layout-sr96000", "layout-sr192000"):
        assert count[name] == 2, name
    assert count["layout-ragged-end"] <= 4                                         # at most the frames at the stream's end
    # the ramps cross once: a run of passing rows, a stretch where the line's magnitude wanders about the floor from
    # frame to frame (a few of its rows too close to call), a run of failing rows
    for name in ("cross-below-c0", "cross-above-c0"):
        v = expected(cases[name])[2]
        first, last = int(np.flatnonzero(v != 1)[0]), int(np.flatnonzero(v != -1)[-1])
        assert 32 < first < last < 224 and last - first < 100 and (v == 0).sum() < 24, (name, first, last)
    # values: zeros and 1e-40 pass, 3e38 / NaN / Inf / energy only above C0 fail
    v = expected(cases["values"])[2]
    f0 = cases["values"].f0
    assert (v[2 - f0:38 - f0] == 1).all() and (v[42 - f0:78 - f0] == 1).all()
    assert (v[81 - f0:119 - f0] == -1).all() and (v[202 - f0:256 - f0] == -1).all()
    assert v[150 - f0] == -1 and v[149 - f0] == -1 and v[170 - f0] == -1 and v[160 - f0] == 1


def test_above_c0_the_screen_fails_before_the_truth_crosses(cases):
    """cross-above-c0: every row whose true last-band magnitude exceeds the floor is a row the screen MUST fail (the
    GPU test holds the repaired count to at least the model's), and the rows it may fail early - the bound is an
    upper bound - are not a whole ramp."""
    c = cases["cross-above-c0"]
    _, taps, v = expected(c)
    L, c0, _ = S.shape(c.sr)
    a = np.abs(taps.coeffs)
    nfl = S.NOISE_FLOOR * np.maximum(a[:, :c0].max(1), F32(1e-10))
    truth = a[:, c0:].max(1) > nfl
    assert truth.any() and (v[truth] == -1).all()
    early = int(((v != 1) & ~truth).sum())        # rows the bound may already fail while the truth is under the floor
    first_truth, first_open = int(np.flatnonzero(truth)[0]), int(np.flatnonzero(v != 1)[0])
    assert early < 40 and first_open <= first_truth, (early, first_open, first_truth)


_assert_bound = S.assert_bound


def test_bound_holds_for_adversarial_sign_patterns():
    """x_i = +-sign(T_ki) puts every product of column k on one side (the largest |c_k| a row of that peak can have),
    at amplitudes from full scale down to the subnormals; with the window and without it."""
    T, w, _ = O.tables()
    rows = []
    for k in (128, 129, 384, 385, 640, 1023):
        s = np.sign(T[k]).astype(F32)
        for amp in (1.0, -1.0, 1e-3, 3e-39):
            rows.append((s * F32(amp)) * w)
        rows.append(s * F32(0.7))                     # un-windowed: A is as large as it gets for the peak
    worst = _assert_bound(np.array(rows, F32), "sign patterns")
    assert worst <= 1.0


def test_bound_holds_for_rows_of_the_cases(cases):
    """Eight rows of every case, the failing ones first."""
    for name, c in cases.items():
        _, _, v = expected(c)
        pick = np.concatenate([np.flatnonzero(v == -1)[:4], np.flatnonzero(v == 1)[:4]])
        _assert_bound(S.windowed_rows(c)[pick], name)


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2), (3, 8)])
def test_condition_on_the_flagship_input(rank, world):
    """The benchmark's chord (bench.py make_shard_pcm, 4096 stereo frames at 48 kHz per rank), for the only rank of a
    one-GPU run, the last rank of a two-GPU run and an interior rank of an eight-GPU run: only the frames
    whose window touches the stream's zero padding - the stream's first and its last - may fail the screen, so at most
    2 of a rank's 4096 frames, and none of an interior rank's."""
    import bench
    c = S.FlagshipRank(bench, rank, world)
    _, taps = S.expected(c)
    v = S.model(c, taps).reshape(-1, bench.CH)
    not_pass = set(np.flatnonzero((v != 1).any(1)).tolist())
    may = ({0} if rank == 0 else set()) | ({bench.FRAMES_PER_GPU - 1} if rank == world - 1 else set())
    assert not_pass <= may and len(not_pass) <= 2, sorted(not_pass)[:8]


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


_stats, _explain = S.stats, S.explain


def _records(gpu, enc, c, mode):
    """encode_screen_cases.records on the fixture's torch and library."""
    return S.records(gpu[0], gpu[1], enc, c, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_gpu_records_equal_the_oracle_with_the_screen_on_and_off(gpu, cases, name):
    c = cases[name]
    exp, _, v = expected(c)
    enc = gpu[2](c.sr)
    on, screened, repaired = _records(gpu, enc, c, 2)
    off, screened_off, repaired_off = _records(gpu, enc, c, 1)
    assert (screened_off, repaired_off) == (0, 0), f"{name}: mode 1 took the screened path"
    assert np.array_equal(off, exp), f"{name}, screen off: {_explain(off, exp, c.ch)}"
    assert np.array_equal(on, exp), f"{name}, screen on: {_explain(on, exp, c.ch)}"
    assert np.array_equal(on, off)
    # the path ran, and repaired the rows the model says it must - no fewer, and no more than those it cannot call
    assert screened == c.M, f"{name}: {screened} of {c.M} rows went through the screened path"
    lo, hi = int((v == -1).sum()), int((v != 1).sum())
    assert lo <= repaired <= hi, f"{name}: {repaired} rows repaired, the model has {lo}..{hi}"
    if c.expect == "pass":
        assert repaired == 0 and screened > 0
    if c.expect == "fail":
        assert repaired == c.M


@pytest.mark.gpu
def test_gpu_automatic_mode_leaves_short_launches_alone(gpu, cases):
    """Mode 0 takes the path only where the 16-wave transform kernel would run: a launch of 256 rows is today's."""
    c = cases["pass-ch2"]
    exp, _, _ = expected(c)
    got, screened, repaired = _records(gpu, gpu[2](c.sr), c, 0)
    assert np.array_equal(got, exp) and (screened, repaired) == (0, 0)


@pytest.mark.gpu
def test_gpu_guard_holds_the_path_off_after_a_launch_that_failed_everywhere_and_probes_again(gpu):
    """Automatic mode on 4098 rows of noise, a fresh context: launch 1 is screened and every row repaired; its count
    makes the guard send launches 2 .. 33 (the stated 32) down today's path; launch 34 probes again.  The records
    are the oracle's whichever path a launch took."""
    torch, glc_amd, _ = gpu
    c = S.guard_case()
    exp, _ = S.expected(c)
    enc = glc_amd.Encoder(c.sr)
    try:
        got, screened, repaired = _records(gpu, enc, c, None)
        assert np.array_equal(got, exp), f"launch 1: {_explain(got, exp, c.ch)}"
        assert (screened, repaired) == (c.M, c.M)
        got, screened, repaired = _records(gpu, enc, c, None)
        assert np.array_equal(got, exp), f"launch 2: {_explain(got, exp, c.ch)}"
        assert (screened, repaired) == (0, 0), "launch 2 was screened: the guard did not see launch 1's count"
        sh, t0, tc = c.shard()
        d_pcm = torch.from_numpy(sh.copy()).cuda()
        d_rec = torch.empty(glc_amd.lib.glc_record_bytes(c.ch) * (c.f1 - c.f0), dtype=torch.uint8, device="cuda")
        s0 = _stats(glc_amd, enc)
        for _ in range(30):                                           # launches 3 .. 32
            enc.encode_range_device(d_pcm.data_ptr(), t0, tc, c.n_samples, c.ch, c.f0, c.f1, d_rec.data_ptr())
        assert _stats(glc_amd, enc) == s0
        got, screened, repaired = _records(gpu, enc, c, None)         # launch 33: the last one held off
        assert np.array_equal(got, exp) and (screened, repaired) == (0, 0)
        got, screened, repaired = _records(gpu, enc, c, None)         # launch 34: the probe
        assert np.array_equal(got, exp), f"launch 34: {_explain(got, exp, c.ch)}"
        assert (screened, repaired) == (c.M, c.M)
    finally:
        enc.close()


@pytest.mark.gpu
def test_gpu_guard_screens_one_launch_of_a_burst_on_a_fresh_context(gpu):
    """Eight launches of the noise queued without waiting, a fresh context: the first is the context's probe, and
    whether its count is back or not when the others are decided - not back: one unjudged launch at a time; back: it
    is a bad one - none of them is screened.  The repair is paid once, and the records are the oracle's."""
    torch, glc_amd, _ = gpu
    c = S.guard_case()
    exp, _ = S.expected(c)
    enc = glc_amd.Encoder(c.sr)
    try:
        sh, t0, tc = c.shard()
        d_pcm = torch.from_numpy(sh.copy()).cuda()
        rb = glc_amd.lib.glc_record_bytes(c.ch) * (c.f1 - c.f0)
        d_rec = torch.zeros(rb, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for _ in range(8):
            enc.encode_range_device(d_pcm.data_ptr(), t0, tc, c.n_samples, c.ch, c.f0, c.f1, d_rec.data_ptr())
        assert _stats(glc_amd, enc) == (c.M, c.M)
        got = d_rec.cpu().numpy()
        assert np.array_equal(got, exp), _explain(got, exp, c.ch)
    finally:
        enc.close()
