"""The balanced wave layout of the mixed-role transform (k_mdct_mix_st): hybrid waves, the hf plane
per bound-carrying wave, the A sum split by row over four workgroups.  tests/encode_balance_cases.py restates the layout
and builds the cases.

CPU: the restated column and plane map for ne = 1 .. 11 - every column owned once, the exact columns exactly
[0, 64 ne), ne exact and 16 - ne bound pairs on every SIMD, one wave per plane - and the plane count and workspace size
the library derives (glc_debug_encode_screen_layout); every aimed row does what it was aimed to do: an exact aim's
record holds the line, a bound aim fails the numpy model WITH the aimed run's columns in the maximum and passes it with
them removed, by the model's own margins; every row of every case is decided, but for one onset frame per aimed case.
GPU: every case with the screen forced on and off - record bytes equal the oracle's, guard pages, and exactly the
model's rows repaired - at 48 kHz (2 exact pairs per hybrid wave, one exact wave per SIMD), 96 kHz and
192 kHz (2, none), 1 / 2 / 3 / 8 channels, one tile, a second tile of one row or frame, and row counts that are no
multiple of 4 (where the model leaves the one onset frame open, the count lies in the window that frame opens); rows
that only the A term fails in each quarter of the A plane; a smaller launch after a larger one on one context, per
rate.  96 kHz takes whole waves (3 pairs per hybrid wave measured no faster): its cases aim at that layout's runs."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encode_balance_cases as B  # noqa: E402
import encode_screen_edges as E  # noqa: E402
from encode_screen_cases import C_ERR, GAMMA, HOP, NOISE_FLOOR, SLACK, TINY, shape, windowed_rows  # noqa: E402
from oracle import oracle as O  # noqa: E402

CASES = {c.name: c for c in B.all_cases()}
AIMED = [n for n, c in CASES.items() if c.family == "balance"]

_expected = {}


def expected(case):
    """(oracle records, taps, decision per row) of a case, computed once per session."""
    if case.name not in _expected:
        rec, taps = E.expected(case)
        _expected[case.name] = (rec, taps, E.decide(case, taps))
    return _expected[case.name]


# ----------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------

def test_every_column_is_owned_once_and_every_simd_carries_the_same_pairs():
    for ne, hp in [(ne, B.hybrid_pairs(ne)) for ne in range(1, B.BALANCED_MAX + 1)] + [(ne, 0) for ne in range(1, 16)]:
        assert hp in (0, ne % 4)
        own = np.zeros(HOP, int)
        exact = np.zeros(HOP, bool)
        plane_waves = {}
        for j in range(8):
            pairs = np.zeros((4, 2), int)               # per SIMD: exact, bound column pairs
            for w in range(16):
                kind, plane, xr, br = B.wave_map(ne, hp, j, w)
                assert sum(n for _, n in xr + br) == 8, (ne, j, w)
                for first, n in xr + br:
                    own[first:first + n] += 1
                    assert first % 2 == 0 and n % 2 == 0
                for first, n in xr:
                    exact[first:first + n] = True
                    pairs[w % 4, 0] += n // 2
                    assert 8 * ne * j <= first and first + n <= 8 * ne * (j + 1), "an exact run outside the workgroup's exact columns"
                for first, n in br:
                    pairs[w % 4, 1] += n // 2
                    lo = 64 * ne + 8 * (16 - ne) * j
                    assert lo <= first and first + n <= lo + 8 * (16 - ne), "a bound run outside the workgroup's bound columns"
                assert (kind == "exact") == (plane is None) == (not br)
                assert (kind == "hybrid") == bool(xr and br)
                if kind == "hybrid":
                    assert xr[0][1] == 2 * hp and br[0][1] == 8 - 2 * hp and w // 4 == ne // 4
                if plane is not None:
                    plane_waves.setdefault(plane, []).append((j, w))
            if hp or ne % 4 == 0:       # balanced: every SIMD carries ne exact and 16 - ne bound pairs
                assert (pairs[:, 0] == ne).all() and (pairs[:, 1] == 16 - ne).all(), (ne, j, pairs.tolist())
            assert pairs[:, 0].sum() == 4 * ne and pairs.sum() == 64
            a = B.a_wave(ne, hp)
            assert a < 16 and B.wave_map(ne, hp, j, a)[0] == "bound", "the A sum needs a wave with bound columns only"
        assert (own == 1).all(), (ne, np.flatnonzero(own != 1)[:8].tolist())
        assert np.array_equal(np.flatnonzero(exact), np.arange(64 * ne)), ne
        n_planes = B.planes(ne, hp)
        assert sorted(plane_waves) == list(range(n_planes)) and all(len(v) == 1 for v in plane_waves.values()), ne
        assert n_planes == 8 * (16 - ne // 4 * 4 if hp else 16 - ne)
    assert B.planes(6, 2) == 96 and B.planes(3, 3) == 128 and B.planes(2, 2) == 128 and B.planes(4, 0) == 96
    assert B.planes(3, 0) == 104 and [B.shipped_pairs(ne) for ne in range(1, 16)] == [0, 2, 0, 0, 0, 2, 0, 0, 0, 2] + [0] * 5
    # above 11 no wave of a SIMD would be left with bound columns only: waves [0, ne) are exact, as for ne % 4 == 0
    for ne in (12, 13, 14, 15):
        assert B.hybrid_pairs(ne) == 0 and B.planes(ne, 0) == 8 * (16 - ne)
    # the rates: 44.1 and 48 kHz (2 exact pairs per hybrid wave, q = 1), 96 kHz (3, 0), 192 kHz (2, 0)
    assert [shape(sr)[2] for sr in (44100, 48000, 96000, 192000)] == [6, 6, 3, 2]


def test_the_library_derives_the_same_plane_count_and_sizes_the_workspace_by_it():
    import glc_amd
    f = glc_amd.lib.glc_debug_encode_screen_layout
    f.restype = C.c_int
    f.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    for ne in range(1, 16):
        for rows in (256, 257, 515, 8192):
            hp, planes, size = C.c_uint32(), C.c_uint32(), C.c_uint64()
            assert f(ne, rows, C.byref(hp), C.byref(planes), C.byref(size)) == 0
            assert hp.value == B.shipped_pairs(ne), ne
            assert planes.value == B.planes(ne, hp.value), ne
            stride = (rows + 255) // 256 * 256
            # the planes and A, the row flags, a quarter of a plane of fail counts - floats and words
            assert size.value == 4 * ((planes.value + 1) * stride + stride + stride // 4), (ne, rows)
    bad = C.c_uint32(), C.c_uint32(), C.c_uint64()
    assert f(0, 256, *map(C.byref, bad)) != 0 and f(16, 256, *map(C.byref, bad)) != 0


def _brackets(case):
    """Per row what encode_screen_cases.model() works with: |c|, the floor, A, and the width of the bracket it allows the
    fused sums around the oracle's."""
    taps = expected(case)[1]
    a = np.abs(taps.coeffs.astype(np.float64))
    _, c0, _ = shape(case.sr)
    nfl = float(NOISE_FLOOR) * np.maximum(a[:, :c0].max(1), 1e-10)
    A = np.abs(windowed_rows(case).astype(np.float64)).sum(1)
    return a, nfl, A


def test_every_aim_hits_its_run_and_nothing_else():
    """The condition the aimed rows are kept by: a bound aim fails the model with the aimed run's columns in the maximum
    and passes it with them removed; an exact aim's line is in the record."""
    _, _, norm = O.tables()
    norm = float(norm)
    seen = set()
    for name in AIMED:
        c = CASES[name]
        L, c0, ne = shape(c.sr)
        hp = B.shipped_pairs(ne)
        rec, taps, v = expected(c)
        a, nfl, A = _brackets(c)
        for row, k, side, run, what in c.aimed:
            seen.add((c.sr, what))
            if side == "exact":
                assert k < c0 and taps.dense_q[row, k] != 0, f"{name}: {what}: column {k} of row {row} is not in the record"
                continue
            first, n = run
            assert c0 <= first <= k < first + n
            in_run = a[row, first:first + n].max() / norm
            rest = np.delete(a[row, c0:], np.arange(first - c0, first - c0 + n)).max() / norm
            slack = 2.0 * GAMMA * A[row] * 1.001
            b_lo = (max(in_run - slack, 0.0) + float(C_ERR) * A[row]) * norm * float(SLACK) * (1 - 1e-4)
            b_hi = (rest + slack + float(C_ERR) * A[row]) * norm * float(SLACK) * (1 + 1e-4) + float(TINY)
            assert b_lo > nfl[row], f"{name}: {what}: row {row} does not fail through columns {first}..{first + n - 1}"
            assert b_hi <= nfl[row] and not (a[row, L:c0] > nfl[row] * (1 - 1e-5)).any(), \
                f"{name}: {what}: row {row} fails without columns {first}..{first + n - 1} as well"
            assert v[row] == -1 and (taps.dense_q[row, L:] != 0).any(), f"{name}: {what}: an unrepaired row {row} would not show"
        # the aims name what the issue asks for, per rate
        kinds = {w for _, _, _, _, w in c.aimed}
        if hp:
            assert any("hybrid" in w and "exact run" in w for w in kinds) and any("hybrid" in w and "bound run" in w for w in kinds)
        assert any("first bound-only wave" in w for w in kinds) and any("last bound run" in w for w in kinds)
        assert any(k == c0 - 1 for _, k, _, _, _ in c.aimed) and any(k == 1023 for _, k, _, _, _ in c.aimed)
        assert any(k == c0 for _, k, _, _, _ in c.aimed), "the first bound column"
        assert (hp, B.hybrid_pairs(ne), ne // 4) == {48000: (2, 2, 1), 96000: (0, 3, 0), 192000: (2, 2, 0)}[c.sr]
    assert {sr for sr, _ in seen} == set(B.RATES)


def test_every_row_of_every_case_is_decided():
    """... but for one frame per aimed case: the frame in which the line at column 1023 sets in (half a hop of it, at the
    edge of the window) lands too close to the floor for the model.  It is no aimed row; the GPU test's count of
    repaired rows has a window of exactly that frame's rows, and the record bytes are compared in full all the same."""
    for name, c in CASES.items():
        v = expected(c)[2]
        und = np.flatnonzero(v == 0)
        if c.family == "balance":
            assert und.size <= (c.ch if c.ch in (1, 2) else 1) and np.unique(und // c.ch).size <= 1, (name, und.tolist())
            assert ((und // c.ch + B.F0) % 8 == 3).all() and not set(und.tolist()) & {a[0] for a in c.aimed}, (name, und.tolist())
        else:
            assert und.size == 0, f"{name}: rows {und[:8].tolist()} are too close to the floor to call"
        assert (v == 1).sum() > c.M // 2, f"{name}: most rows are tonal rows that pass"
    assert {(c.ch, c.M) for c in CASES.values() if c.family == "balance"} == set(B.SHAPES)
    assert any(c.M == 256 for c in CASES.values()) and any(c.M == 257 for c in CASES.values())
    assert any(c.M % 4 and c.M > 512 for c in CASES.values())


def test_the_a_cases_fail_by_a_alone_in_every_quarter_of_the_a_plane():
    quarters = set()
    for c in B.a_cases():
        c = CASES[c.name]
        rec, taps, v = expected(c)
        L, c0, _ = shape(c.sr)
        got = np.flatnonzero(v == -1)
        assert got.tolist() == c.fail_rows, c.name
        a, b = E.conditions(c, taps)
        r = E.conditions(c, taps, ratio=True)[1]
        r4 = E.conditions(c, taps, 4, ratio=True)[1]          # mutation 4: A dropped from the bound
        assert not a.any() and (r[got] > 1.05).all() and (np.delete(r, got) < 0.95).all() and (r4 < 0.95).all(), c.name
        assert not (taps.dense_q[got][:, L:] != 0).any(), "nothing of these rows is over the floor: only the count shows them"
        quarters |= set((got % 4).tolist())
    assert quarters == {0, 1, 2, 3}


# ----------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU (no CPU fallback exists)"
    import glc_amd
    E.S.bind(glc_amd)
    encoders = {}

    def encoder(key):
        if key not in encoders:
            encoders[key] = glc_amd.Encoder(key)
        return encoders[key]
    yield torch, glc_amd, encoder
    for e in encoders.values():
        e.close()


def _launch_and_check(gpu, enc, c, label=""):
    """The case with the screen forced on (mode 2) and off (mode 1): bytes, guard pages (in records()), counts."""
    exp, _, v = expected(c)
    name = label + c.name
    on, screened, repaired = E.S.records(gpu[0], gpu[1], enc, c, 2)
    off, screened_off, repaired_off = E.S.records(gpu[0], gpu[1], enc, c, 1)
    print(f"{name}: M {c.M}, screened {screened}, repaired {repaired}, model {int((v == -1).sum())}..{int((v != 1).sum())}")
    assert (screened_off, repaired_off) == (0, 0), f"{name}: mode 1 took the screened path"
    assert np.array_equal(off, exp), f"{name}, screen off: {E.S.explain(off, exp, c.ch)}"
    assert np.array_equal(on, exp), f"{name}, screen on: {E.S.explain(on, exp, c.ch)}"
    assert screened == c.M, f"{name}: {screened} of {c.M} rows went through the screened path"
    lo, hi = int((v == -1).sum()), int((v != 1).sum())        # hi > lo by the one onset frame the model leaves open
    assert lo <= repaired <= hi, f"{name}: {repaired} rows repaired, the model has {lo}..{hi}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", AIMED)
def test_gpu_aimed_cases_equal_the_oracle_and_repair_exactly_the_models_rows(gpu, name):
    c = CASES[name]
    _launch_and_check(gpu, gpu[2](c.sr), c)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in B.a_cases()])
def test_gpu_rows_only_a_fails_are_repaired_in_every_quarter_of_the_a_plane(gpu, name):
    c = CASES[name]
    _launch_and_check(gpu, gpu[2](c.sr), c)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", B.reuse_pairs(), ids=lambda p: p[1])
def test_gpu_a_smaller_launch_after_a_larger_one_on_a_fresh_context(gpu, pair):
    """515 rows, then 256 on the same context: the second launch's planes lie where the first one, at a stride of 768
    rows, wrote other rows' maxima.  A stale plane that decided a row would repair it (or leave an aimed one alone)."""
    torch, glc_amd, _ = gpu
    enc = glc_amd.Encoder(CASES[pair[0]].sr)
    try:
        for i, name in enumerate(pair):
            _launch_and_check(gpu, enc, CASES[name], f"reuse[{i}] ")
    finally:
        enc.close()
