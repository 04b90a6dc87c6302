"""The matrix form of the screened transform (k_mdct_mx_st; DESIGN.md section 2, glc_kernels.h MatrixBound) restated in
numpy: the bf16 round-to-nearest-even split by bit operations, the bound sums e_k as three piece sums cut into
segments, with the instruction's error model applied adversarially, and the constants the library reports."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encode_screen_cases as S  # noqa: E402
from encode_screen_cases import C_ERR, F32, FRAME, GAMMA, SLACK, TINY  # noqa: E402
from oracle import oracle as O  # noqa: E402

U = 2.0 ** -24


def constants():
    """The host-only query of include/glc_debug.h as a dict."""
    import glc_amd
    f = glc_amd.lib.glc_debug_encode_matrix_bound
    f.restype, f.argtypes = C.c_int, [C.POINTER(C.c_uint32)] * 6 + [C.POINTER(C.c_double)] * 3
    u = [C.c_uint32() for _ in range(6)]
    d = [C.c_double() for _ in range(3)]
    assert f(*map(C.byref, u + d)) == 0
    names = ("ne", "pieces", "products", "k_block", "seg_blocks", "planes", "kappa", "split_eps", "budget")
    return dict(zip(names, [x.value for x in u + d]))


def bf16_rn(x):
    """f32 -> the bf16 nearest (ties to even) as an f32 whose low 16 bits are zero; a value that rounds past the largest
    bf16 gives infinity, as the hardware conversion does.  Finite inputs only."""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(F32).reshape(np.shape(x))


def split(a):
    """a -> (a1, a2, r): a1 = bf16_rn(a), a2 = bf16_rn(a - a1), r = a - a1 - a2 (both subtractions exact in f32)."""
    a = np.asarray(a, F32)
    with np.errstate(all="ignore"):
        a1 = bf16_rn(a)
        d = (a - a1).astype(F32)
        a2 = np.where(np.isfinite(d), bf16_rn(np.where(np.isfinite(d), d, 0)), d).astype(F32)
        r = (d - a2).astype(F32)
    return a1, a2, r


def flush(p):
    """bf16 inputs of the matrix pipe may flush subnormals: the piece with its subnormals set to zero."""
    return np.where(np.abs(p) < np.float32(2.0 ** -126), np.float32(0.0), p).astype(F32)


def matrix_sums(xw, T, cols, k, flush_subnormals=False):
    """(e_lo, e_hi): the interval the kernel's total of every (row, column) lies in under the error model - per segment
    of k['seg_blocks'] K-blocks the three piece sums in f64, widened by (instructions per chain) * kappa * sum |p|, and
    the whole by one f32 rounding per segment on the running magnitude."""
    a1, a2, _ = split(xw)
    t1, t2, _ = split(T[cols])
    if flush_subnormals:
        a1, a2, t1, t2 = flush(a1), flush(a2), flush(t1), flush(t2)
    a1, a2, t1, t2 = (v.astype(np.float64) for v in (a1, a2, t1, t2))
    seg = k["k_block"] * k["seg_blocks"]
    n = k["seg_blocks"] * k["products"]
    lo = np.zeros((xw.shape[0], len(cols)))
    hi = np.zeros_like(lo)
    mag = np.zeros_like(lo)
    with np.errstate(all="ignore"):
        for s in range(0, FRAME, seg):
            i = slice(s, s + seg)
            p = a1[:, i] @ t1[:, i].T + a1[:, i] @ t2[:, i].T + a2[:, i] @ t1[:, i].T
            ap = np.abs(a1[:, i]) @ np.abs(t1[:, i]).T + np.abs(a1[:, i]) @ np.abs(t2[:, i]).T + np.abs(a2[:, i]) @ np.abs(t1[:, i]).T
            mag += ap
            lo += p - n * k["kappa"] * ap - U * mag
            hi += p + n * k["kappa"] * ap + U * mag
    return lo, hi


def least_magnitude(lo, hi):
    """The smallest |e| an interval allows: what an adversary would hand the bound."""
    return np.where((lo <= 0) & (hi >= 0), 0.0, np.minimum(np.abs(lo), np.abs(hi)))


def assert_bound(xw, what, k, cols=None):
    """|c| of the oracle never exceeds the kernel's bound formed from the least |e_k| the error model allows, for the rows
    `xw` over the bound columns -> the largest |c| / B seen."""
    T, _, norm = O.tables()
    cols = np.arange(64 * k["ne"], 1024) if cols is None else cols
    worst = 0.0
    for fl in (False, True):
        lo, hi = matrix_sums(xw, T, cols, k, fl)
        with np.errstate(all="ignore"):
            e = least_magnitude(lo, hi).astype(F32)
            A = np.abs(xw).astype(np.float64).sum(1).astype(F32)
            B = S.bound_per_bin(e, A)
            c = np.stack([np.abs(O.mdct_block(r))[cols] for r in xw])
            ok = (c <= B) | ~np.isfinite(B)
        assert ok.all(), f"{what} (flush {fl}): |c| exceeds the bound at (row, k) {np.argwhere(~ok)[:4].tolist()}"
        with np.errstate(all="ignore"):
            worst = max(worst, float(np.nanmax(np.where(np.isfinite(B) & (B > 0), c / B, 0.0))))
    return worst
