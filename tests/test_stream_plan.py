"""glc_plan_stream_push against a frame-by-frame model (tests/stream_encode_cases.py) and the oracle's frame count, and
the argument checks of the streaming session that need no device."""
import ctypes as C

import numpy as np
import pytest

import glc_amd
import stream_encode_cases as SC
from conftest import O

lib = glc_amd.lib
EINVAL = -1


def plan(received, n_new, finish):
    p = glc_amd._lib.GlcStreamPushPlan()
    rc = lib.glc_plan_stream_push(received, n_new, 1 if finish else 0, C.byref(p))
    return rc, (p.first_frame, p.n_frames, p.carry)


def grid():
    dense = sorted({v + d for v in (512, 1536, 2560) for d in (-1, 0, 1)})
    return sorted(set(range(0, 4201, 97)) | set(dense) | {0, 1, 1023, 1024, 1025, 2047, 2048, 2049, 3583, 3584, 3585, 4200})


def test_plan_equals_the_frame_by_frame_model():
    pts = grid()
    for received in pts:
        for n_new in pts:
            for finish in (False, True):
                want = SC.model_plan(received, n_new, finish, O.num_frames)
                rc, got = plan(received, n_new, finish)
                if want is None:
                    assert rc == EINVAL and received + n_new <= 512, (received, n_new, finish)
                else:
                    assert rc == 0 and got == want, (received, n_new, finish, got, want)
                    assert got[2] <= 2047


@pytest.mark.parametrize("L", [513, 1024, 1536, 1537, 2047, 2048, 2049, 3071, 3072, 3073, 5000])
def test_random_chunkings_tile_the_stream(L):
    rng = np.random.default_rng(L)
    nf = O.num_frames(L, 1)
    assert nf > 0
    for trial in range(40):
        sizes = SC.random_chunking(rng, L, (1, 7, 600, 1100, 2100, 5000)[trial % 6])
        finish_empty = trial % 2 == 0
        if finish_empty:
            sizes = sizes + [0]
        received, next_frame = 0, 0
        for k, n in enumerate(sizes):
            fin = k == len(sizes) - 1
            rc, (f0, n_f, carry) = plan(received, n, fin)
            assert rc == 0, (L, sizes, k)
            assert f0 == next_frame and carry <= 2047
            assert carry == 0 if fin else carry == received + n - (1024 * (f0 + n_f) - 512 if f0 + n_f else 0)
            next_frame += n_f
            received += n
        assert received == L and next_frame == nf, (L, sizes)


@pytest.mark.parametrize("L", [0, 1, 511, 512])
def test_a_finish_the_reference_panics_on_is_refused(L):
    assert O.num_frames(L, 1) == 0
    for received in sorted({0, L // 2, L}):
        rc, _ = plan(received, L - received, True)
        assert rc == EINVAL
        assert b"512" in lib.glc_last_error(None)
        assert plan(received, L - received, False)[0] == 0          # without the finish the samples are only held back
    assert plan(0, 513, True) == (0, (0, 1, 0))


def test_plan_refuses_a_null_result_and_a_wrapping_sum():
    assert lib.glc_plan_stream_push(0, 1024, 0, None) == EINVAL
    assert plan(2 ** 64 - 1, 1, False)[0] == EINVAL
    assert plan(2 ** 63, 2 ** 63, True)[0] == EINVAL


def test_python_plan_stream_push():
    p = glc_amd.plan_stream_push(1000, 2000)
    assert (p.first_frame, p.n_frames, p.carry) == SC.model_plan(1000, 2000, False, O.num_frames)
    with pytest.raises(glc_amd.GlcError) as e:
        glc_amd.plan_stream_push(100, 412, finish=True)
    assert e.value.code == EINVAL
    with pytest.raises(glc_amd.GlcError):
        glc_amd.plan_stream_push(-1, 5)


def test_max_push_leaves_room_for_a_round():
    """A push of max_push samples completes at most max_push / 1024 + 1 frames; with its junk slot and the round's slot
    in front they must fit the frames of an encode round (4096, mono 8192)."""
    assert lib.glc_stream_enc_max_push(0) == 0
    for ch, budget in ((1, 8192), (2, 4096), (3, 4096), (8, 4096)):
        m = lib.glc_stream_enc_max_push(ch)
        assert m % 1024 == 0 and m > 0
        worst = max(plan(r, m, fin)[1][1] for r in (0, 511, 1535, 1536, 2047 + 1024) for fin in (False, True))
        assert worst + 2 <= budget
        assert worst == m // 1024 + 1


def test_session_calls_refuse_null_handles_without_a_device():
    vp = C.c_void_p
    out = vp()
    assert lib.glc_stream_enc_open(None, 2, 1, C.byref(out)) == EINVAL and not out.value
    n = C.c_uint64()
    one = (C.c_uint64 * 1)(0)
    ptrs = (vp * 1)(None)
    assert lib.glc_stream_enc_push(None, ptrs, SC.PF32, 32, one, None) == EINVAL
    lay = glc_amd._lib.GlcClipLayout(1, 2, 0, 0, 0, 0, None)
    seg = (glc_amd._lib.GlcStreamSeg * 1)()
    assert lib.glc_stream_enc_push_device(None, None, SC.PF32, 32, C.byref(lay), None, None, 0, None, None, seg, C.byref(n)) == EINVAL
    assert lib.glc_stream_enc_segments(None, 0, C.byref(n)) == EINVAL
    assert lib.glc_stream_enc_segment(None, 0, 0, None, None, None, None) == EINVAL
    assert lib.glc_stream_enc_frames(None, 0, C.byref(out)) == EINVAL
    assert lib.glc_stream_enc_reset(None, 0) == EINVAL
    lib.glc_stream_enc_close(None)                                   # a no-op
