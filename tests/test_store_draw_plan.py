"""glc_store_crop_slots: the hops and frames a crop of `length` samples per channel needs wherever it starts (DESIGN.md
section 3, "drawing from the store") - the fixed block of table rows, block slots and hop descriptors that a crop of
glc_decode_crops_device_store owns - held to brute force over glc_plan_crop: EVERY start of the crop in clips of 513 to
5 * 1024 + 300 samples per channel.  No start may need more than the slots, and some start must need exactly that many
(the rounds of the draw call are sized by them: a bound that is never reached would waste a slot of every crop).

  A crop begins at the un-trimmed interleaved position 512 + start * ch, which is 512 modulo ch, so the latest place in
  a hop it can have is 1024 ch - ch + 512 % ch; from there length * ch samples reach into
  floor((1024 ch - ch + 512 % ch + length ch - 1) / (1024 ch)) + 1 hops, and the frames are one more: the halo frame.

Host only: no GPU is needed."""
import ctypes as C

import pytest

from channel_axis_cases import CHANNELS

HOP = 1024
EINVAL = -1
CLIPS = (513, 1024, 1025, 1536, 2049, 3000, 4097, 5 * HOP + 300)
LENGTHS = (1, 2, 511, 512, 513, 1023, 1024, 1025, 2048, 3000)


@pytest.fixture(scope="module")
def glc_amd():
    import glc_amd as g
    assert hasattr(g.lib, "glc_store_crop_slots")
    return g


def model(length, ch):
    per_hop = HOP * ch
    hops = (per_hop - ch + 512 % ch + length * ch - 1) // per_hop + 1
    return hops, hops + 1


@pytest.mark.parametrize("ch", (1, 2, 3, 6) + CHANNELS + (1023, 1024, 1025))
@pytest.mark.parametrize("length", LENGTHS)
def test_slots_against_every_start(glc_amd, ch, length):
    g = glc_amd
    L = g._lib
    max_hops, max_frames = g.store_crop_slots(length, ch)
    assert (max_hops, max_frames) == model(length, ch)
    assert max_frames == max_hops + 1
    plan, crop = L.GlcCropPlan(), L.GlcCrop(0, length)
    f, p_crop, p_plan = g.lib.glc_plan_crop, C.byref(crop), C.byref(plan)
    most_hops = most_frames = tried = 0
    for n in CLIPS:
        if n < length:
            continue
        for start in range(n - length + 1):
            crop.start = start
            assert f(n * ch, ch, p_crop, p_plan) == 0
            assert plan.n_hops <= max_hops and plan.n_frames <= max_frames, (n, start)
            most_hops, most_frames = max(most_hops, plan.n_hops), max(most_frames, plan.n_frames)
            tried += 1
    assert tried > 3000
    assert (most_hops, most_frames) == (max_hops, max_frames)      # ... and some start reaches both


def test_slots_where_the_channel_count_matters(glc_amd):
    """One sample frame of 1 or 2 channels never straddles a hop boundary (512 is a multiple of both); one of 3 or 6
    channels can.  A crop of 1025 samples reaches a third hop only where its first position can be the last of a hop."""
    g = glc_amd
    assert [g.store_crop_slots(1, ch) for ch in (1, 2, 3, 6)] == [(1, 2), (1, 2), (2, 3), (2, 3)]
    assert [g.store_crop_slots(1025, ch) for ch in (1, 2, 3, 6)] == [(2, 3), (2, 3), (3, 4), (3, 4)]
    assert g.store_crop_slots(4095 * HOP, 2) == (4096, 4097)       # the longest crop a round of the draw call holds...
    assert g.store_crop_slots(4095 * HOP + 2, 2) == (4097, 4098)   # ... and the first it refuses


def test_refused_arguments(glc_amd):
    g = glc_amd
    hops, frames = C.c_uint64(7), C.c_uint64(7)
    f = g.lib.glc_store_crop_slots
    assert f(1000, 2, C.byref(hops), C.byref(frames)) == 0 and (hops.value, frames.value) == (2, 3)
    assert f(1000, 2, None, C.byref(frames)) == EINVAL
    assert f(1000, 2, C.byref(hops), None) == EINVAL
    assert f(1000, 0, C.byref(hops), C.byref(frames)) == EINVAL
    assert f(0, 2, C.byref(hops), C.byref(frames)) == EINVAL
    assert f(2 ** 63, 2, C.byref(hops), C.byref(frames)) == EINVAL   # length * channels wraps
    assert (hops.value, frames.value) == (2, 3)                        # a refused call writes nothing
    with pytest.raises(g.GlcError) as e:
        g.store_crop_slots(0, 2)
    assert e.value.code == EINVAL
    with pytest.raises(g.GlcError):
        g.store_crop_slots(-1, 2)
