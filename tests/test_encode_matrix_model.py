"""The numerics of the matrix form of the screened transform (glc_kernels.h MatrixBound), on the
CPU: the bf16 split and its two bounds on normals, subnormals, zeros and values that overflow; the error budget from
the constants the library reports; the inequality |c_k| <= B_k with e_k emulated as three piece sums in segments and
the instruction's error model applied against the bound, on adversarial sign patterns and eight rows of every case of
encode_screen_cases; and the condition on the benchmark's own input with H widened by the whole budget."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encode_matrix_cases as X  # noqa: E402
import encode_screen_cases as S  # noqa: E402
from oracle import oracle as O  # noqa: E402

F32 = np.float32


@pytest.fixture(scope="module")
def k():
    return X.constants()


def test_split_bounds_on_normals_subnormals_zeros_and_overflow():
    rng = np.random.default_rng(7)
    bits = rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)
    a = bits.view(F32)
    a = a[np.isfinite(a) & (np.abs(a) < 3.3e38)]
    edge = np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -126, -2.0 ** -126, 2.0 ** -149, 3e-39, 1e-40, -1e-40, 1.0 + 2.0 ** -8,
                     1.0 + 2.0 ** -9, 1.0 + 3 * 2.0 ** -9, 0.999999, 3.3e38], F32)
    a = np.concatenate([a, edge])
    a1, a2, r = X.split(a)
    A, A1, A2, R = (v.astype(np.float64) for v in (a, a1, a2, r))
    assert np.array_equal(A1 + A2 + R, A), "a = a1 + a2 + r exactly"
    assert (a1.view(np.uint32) & 0xFFFF == 0).all() and (a2.view(np.uint32) & 0xFFFF == 0).all(), "the pieces are bf16"
    normal = np.abs(A) >= 2.0 ** -126
    assert (np.abs(A - A1)[normal] <= 2.0 ** -8 * np.abs(A)[normal]).all()      # half an ulp of 8 significant bits
    well = np.abs(A) >= 2.0 ** -118               # below, a - a1 may be a subnormal whose rounding is absolute: 2^-134 at most
    assert (np.abs(R)[well] <= 2.0 ** -16 * np.abs(A)[well]).all()
    assert (np.abs(R)[~well] < 2.0 ** -126).all()
    # below the normals every piece is off by less than the smallest normal: what kScreenTiny is there for
    assert (np.abs(A - A1)[~normal] < 2.0 ** -126).all() and (np.abs(R)[~normal] < 2.0 ** -126).all()
    # zeros keep their sign bit and split into zeros
    z1, z2, zr = X.split(np.array([0.0, -0.0], F32))
    assert (z1 == 0).all() and (z2 == 0).all() and (zr == 0).all()
    # a finite value that rounds past the largest bf16: a1 is infinite and a - a1 is not a number the sums survive
    o1, o2, _ = X.split(np.array([3.4e38, -3.4e38, np.finfo(F32).max], F32))
    assert np.isinf(o1).all() and not np.isfinite(o2).any()
    with np.errstate(all="ignore"):
        assert not np.isfinite(o1 * F32(0.5) + o2 * F32(0.5)).any(), "the row's totals are not finite: H must fail the row"


def test_budget_fits_in_the_half_of_c_err_that_belongs_to_the_bound_sums(k):
    assert (k["ne"], k["pieces"], k["products"], k["k_block"], k["planes"]) == (6, 2, 3, 16, 4)
    assert k["kappa"] == 17 * 2.0 ** -23 and k["split_eps"] == 3 * 2.0 ** -16
    segments = S.FRAME // (k["k_block"] * k["seg_blocks"])
    assert segments * k["k_block"] * k["seg_blocks"] == S.FRAME
    budget = k["split_eps"] + k["seg_blocks"] * k["products"] * k["kappa"] + segments * 2.0 ** -24
    assert budget == k["budget"]
    assert budget * (1 + 2.0 ** -7) <= S.GAMMA, (budget, S.GAMMA)      # (the O(2^-24) of the split: (1 + 2^-8)^2 on |p|)
    assert 2 * S.GAMMA < float(S.C_ERR)
    # subnormal pieces that flush: 3 products x 2048 terms, each off by less than 2^-126, beside what kScreenTiny
    # already covers (4096 operations of the exact sum)
    assert (k["products"] * S.FRAME + 4096) * 2.0 ** -126 < float(S.TINY)


def test_bound_holds_for_adversarial_sign_patterns(k):
    """The rows of test_encode_screen.py's test of the same name, over the columns the matrix form bounds."""
    T, w, _ = O.tables()
    rows = []
    for col in (128, 129, 384, 385, 640, 1023):
        s = np.sign(T[col]).astype(F32)
        for amp in (1.0, -1.0, 1e-3, 3e-39):
            rows.append((s * F32(amp)) * w)
        rows.append(s * F32(0.7))
    worst = X.assert_bound(np.array(rows, F32), "sign patterns", k)
    print(f"sign patterns: largest |c| / B {worst:.4f}")
    assert worst <= 1.0


def test_bound_holds_for_rows_of_the_cases(k):
    """Eight rows of every case, the failing ones first."""
    for c in S.cases():
        _, taps = S.expected(c)
        v = S.model(c, taps)
        pick = np.concatenate([np.flatnonzero(v == -1)[:4], np.flatnonzero(v == 1)[:4]])
        X.assert_bound(S.windowed_rows(c)[pick], c.name, k)


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2), (3, 8)])
def test_condition_on_the_flagship_input(k, rank, world):
    """The benchmark's chord: with H as far above the true maximum as the budget allows (k['budget'] A for e_k, gamma_2048 A
    for the exact sum the truth is an f32 of), only the stream's first and last frame may fail the screen."""
    import bench
    c = S.FlagshipRank(bench, rank, world)
    _, taps = S.expected(c)
    L, c0, _ = S.shape(c.sr)
    _, _, norm = O.tables()
    a = np.abs(taps.coeffs.astype(np.float64))
    A = np.abs(S.windowed_rows(c).astype(np.float64)).sum(1)
    nfl = float(S.NOISE_FLOOR) * np.maximum(a[:, :c0].max(1), 1e-10)
    h = a[:, c0:].max(1) / float(norm) * (1 + 2.0 ** -23) + (S.GAMMA + k["budget"] * (1 + 2.0 ** -7)) * A
    b = (h + float(S.C_ERR) * A) * float(norm) * float(S.SLACK) * (1 + 1e-4) + float(S.TINY)
    fails = (b > nfl) | (a[:, L:c0] > nfl[:, None] * (1 - 1e-5)).any(1)
    not_pass = set(np.flatnonzero(fails.reshape(-1, bench.CH).any(1)).tolist())
    may = ({0} if rank == 0 else set()) | ({bench.FRAMES_PER_GPU - 1} if rank == world - 1 else set())
    assert not_pass <= may and len(not_pass) <= 2, sorted(not_pass)[:8]
