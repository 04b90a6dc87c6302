"""glc_plan_stream_dec_push held to the numpy restatement of the emission rule (stream_decode_cases): every stream
length 513..6000, channels 1 / 2 / 3 / 5 / 8, every chunking into pushes of 1 frame, 2 frames, everything at once and
random pushes, with the finish on the last push and as a push of its own that brings no frames.  Host only."""
import ctypes as C

import numpy as np

import stream_decode_cases as DC
from conftest import O

HOP = DC.HOP
LENGTHS = range(513, 6001)
CHANNELS = (1, 2, 3, 5, 8)
EINVAL = -1


def lib():
    import glc_amd
    return glc_amd.lib, glc_amd._lib.GlcStreamDecPlan


def plan(L, P, done, n, finish, total):
    p = P(7, 7)
    rc = L.glc_plan_stream_dec_push(done, n, 1 if finish else 0, total, C.byref(p))
    return None if rc else (p.first_sample, p.n_samples)


def test_the_model_counts_the_oracles_frames():
    for n in list(range(0, 520)) + list(LENGTHS):
        assert DC.num_frames(n) == O.num_frames(n, 1), n
    for n in LENGTHS:
        nf = DC.num_frames(n)
        assert HOP * nf - 511 <= n <= HOP * nf + 512


def test_every_chunking_tiles_the_stream():
    L, P = lib()
    rng = np.random.default_rng(11)
    for total in LENGTHS:
        nf = DC.num_frames(total)
        for sizes in DC.chunkings(nf, rng):
            for empty_finish in (False, True):
                pushes = [(k, False) for k in sizes]
                if empty_finish:
                    pushes.append((0, True))      # all frames arrive first: the finish decodes from the carry alone
                else:
                    pushes[-1] = (sizes[-1], True)
                done, at = 0, 0
                for n, fin in pushes:
                    got = plan(L, P, done, n, fin, total if fin else 0)
                    assert got == DC.model_plan(done, n, fin, total), (total, sizes, done, n, fin)
                    first, count = got
                    assert first == at                                  # the spans follow each other
                    done, at = done + n, at + count
                    if not fin:
                        assert at <= HOP * done - HOP // 2 and at < total  # nothing the trim could still remove
                assert at == total and done == nf                       # ... and tile [0, L) exactly


def test_a_span_ends_inside_the_last_hop_it_knows():
    L, P = lib()
    for ch in CHANNELS:
        for done in range(1, 8):
            first, count = plan(L, P, 0, done, False, 0)
            end = 512 + ch * (first + count)      # un-trimmed interleaved position behind the span
            assert (done - 1) * HOP * ch < end <= done * HOP * ch
            assert (end == done * HOP * ch) == (ch == 1)
            assert end == HOP * done * ch - 512 * (ch - 1)
    # the hazard the rule avoids: with two or more channels whole hops reach behind the shortest stream of nf frames
    for ch in CHANNELS[1:]:
        for nf in range(1, 6):
            shortest = HOP * nf - 511
            assert DC.num_frames(shortest) == nf and nf * HOP * ch > 512 + shortest * ch


def test_refusals():
    L, P = lib()
    for total in (513, 1536, 1537, 2048, 5000, 6000):
        nf = DC.num_frames(total)
        for done in range(nf + 1):
            assert plan(L, P, done, nf - done, True, total) is not None
            assert plan(L, P, done, nf - done, True, total + HOP) is None      # one frame more
            assert plan(L, P, done, nf - done + 1, True, total) is None
            if nf > 1:
                assert plan(L, P, done, nf - done, True, total - HOP) is None  # one frame fewer
            if nf - done >= 1:
                assert plan(L, P, done, nf - done - 1, True, total) is None
    assert plan(L, P, 0, 0, True, 0) is None and plan(L, P, 0, 0, True, 512) is None and plan(L, P, 0, 1, True, 512) is None
    assert L.glc_plan_stream_dec_push(0, 1, 0, 0, None) == EINVAL
    p = P(7, 7)
    assert L.glc_plan_stream_dec_push(2 ** 64 - 1, 2, 0, 0, C.byref(p)) == EINVAL      # the sum wraps
    assert L.glc_plan_stream_dec_push(2 ** 63, 2 ** 63, 0, 0, C.byref(p)) == EINVAL
    assert L.glc_plan_stream_dec_push(2 ** 60, 1, 0, 0, C.byref(p)) == EINVAL          # 1024 * frames wraps
    assert (p.first_sample, p.n_samples) == (0, 0)
    assert plan(L, P, 0, 0, False, 0) == (0, 0) and plan(L, P, 3, 0, False, 0) == (3 * HOP - 512, 0)
