"""glc_store_ragged_slots: the hop descriptors and frames a ragged crop of `length` samples per channel needs (DESIGN.md
section 3, "ragged crops") - held to brute force over glc_plan_crop: in clips of 513 to 3000 samples per channel EVERY
start s and EVERY wanted length that changes the valid length v = min(w, n - s), that is every v in 1 .. min(length,
n - s).  A crop needs glc_plan_crop's n_hops of {s, v} descriptors for its valid part and ceil((length - v) ch /
(1024 ch)) for its padding.  No case may need more than max_descs, and some case must need exactly that many (the
descriptor table and the overlap-add launch of every round are sized by it).

  How every pair is reached in seconds: a crop's hops run from the hop of its first kept sample to the hop of its last
  one (include/glc.h glc_plan_crop), so n_hops of {s, v} is last_hop(s + v) - first_hop(s) + 1 with first_hop(s) =
  glc_plan_crop({s, 1}).first_hop and last_hop(e) = the last hop of glc_plan_crop({0, e}).  Both come from the C function
  for every s and e; the sum over all pairs is then formed with numpy.  That this decomposition IS glc_plan_crop's answer
  is itself held to the function: for every pair of the 513-sample clip, and in the longer clips for every pair whose
  first or last sample lies within two samples of a hop boundary or of the clip's ends.

Host only: no GPU is needed."""
import ctypes as C

import numpy as np
import pytest

import crop_cases as CC
import store_draw_cases as S
import store_ragged_cases as R

HOP = 1024
EINVAL = -1
CLIPS = (513, 1024, 1025, 1536, 2049, 3000)
LENGTHS = (1, 2, 3, 512, 1024, 1025, 1026, 2048, 2049, 3000)


@pytest.fixture(scope="module")
def glc_amd():
    import glc_amd as g
    assert hasattr(g.lib, "glc_store_ragged_slots")
    return g


def hop_tables(g, n, ch):
    """first_hop[s] for s in [0, n) and last_hop[e] for e in [1, n] (index 0 unused), both from glc_plan_crop"""
    L = g._lib
    plan, crop = L.GlcCropPlan(), L.GlcCrop(0, 1)
    f, p_crop, p_plan = g.lib.glc_plan_crop, C.byref(crop), C.byref(plan)
    first, last = np.zeros(n, np.int32), np.zeros(n + 1, np.int32)
    for s in range(n):
        crop.start, crop.length = s, 1
        assert f(n * ch, ch, p_crop, p_plan) == 0
        first[s] = plan.first_hop
        crop.start, crop.length = 0, s + 1
        assert f(n * ch, ch, p_crop, p_plan) == 0
        last[s + 1] = plan.first_hop + plan.n_hops - 1
    return first, last


def hops_of_every_pair(first, last, n):
    """nh[s, v - 1] = hops of the valid part {s, v}; -30000 where s + v > n"""
    s = np.arange(n)[:, None]
    v = np.arange(1, n + 1)[None, :]
    e = np.minimum(s + v, n)
    nh = (last[e] - first[s] + 1).astype(np.int16)
    nh[s + v > n] = -30000
    return nh


def near_edges(n, ch):
    pts = {0, 1, 2, n - 3, n - 2, n - 1}
    for h in range(1, CC.hop_of(n - 1, ch - 1, ch) + 1):
        b = CC.boundary_sample(h, ch)
        pts.update(range(b - 2, b + 3))
    return sorted(p for p in pts if 0 <= p < n)


@pytest.mark.parametrize("ch", (1, 2, 3, 6))
def test_slots_against_every_start_and_every_valid_length(glc_amd, ch):
    g = glc_amd
    L = g._lib
    plan, crop = L.GlcCropPlan(), L.GlcCrop(0, 1)
    f, p_crop, p_plan = g.lib.glc_plan_crop, C.byref(crop), C.byref(plan)
    most = {length: 0 for length in LENGTHS}
    most_frames = {length: 0 for length in LENGTHS}
    tried = 0
    for n in CLIPS:
        first, last = hop_tables(g, n, ch)
        nh = hops_of_every_pair(first, last, n)
        # the decomposition against the function itself
        if n == 513:
            pairs = [(s, v) for s in range(n) for v in range(1, n - s + 1)]
        else:
            pts = near_edges(n, ch)
            pairs = {(s, e - s + 1) for s in pts for e in range(s, n, 7)} | {(s, e - s + 1) for e in pts for s in range(0, e + 1, 7)} \
                | {(s, e - s + 1) for s in pts for e in pts if e >= s}
        for s, v in pairs:
            crop.start, crop.length = s, v
            assert f(n * ch, ch, p_crop, p_plan) == 0
            assert plan.n_hops == nh[s, v - 1] and plan.first_hop == first[s], (n, s, v)
        # every start and every valid length, per output row
        for length in LENGTHS:
            max_descs, max_frames = g.store_ragged_slots(length, ch)
            assert max_frames == g.store_crop_slots(length, ch)[1] == S.slots(length, ch)[1]
            top = min(length, n)
            v = np.arange(1, top + 1)
            pads = (-(-(length - v) * ch // (HOP * ch))).astype(np.int16)
            assert all(pads[k - 1] == R.pads_of(k, length, ch) for k in {1, min(2, top), top, (top + 1) // 2})
            need = nh[:, :top] + pads[None, :]
            worst = int(need.max())
            assert worst <= max_descs, (n, length, np.unravel_index(int(need.argmax()), need.shape))
            most[length] = max(most[length], worst)
            # the frames of a valid part: its hops' frames and the halo frame, never more than the fixed draw's slot
            most_frames[length] = max(most_frames[length], int(nh[:, :top].max()) + 1)
            tried += int((need > 0).sum())
    assert tried > 20_000_000
    for length in LENGTHS:
        max_descs, max_frames = g.store_ragged_slots(length, ch)
        assert most[length] == max_descs, length                   # ... and some case needs exactly that many
        assert most_frames[length] <= max_frames
        assert S.slots(length, ch)[0] <= max_descs <= S.slots(length, ch)[0] + 1


def test_slots_where_they_differ_from_the_fixed_draw(glc_amd):
    """One descriptor more than the fixed draw's hops exactly where a short valid part can straddle a hop boundary and
    still leave a whole row of padding to describe."""
    g = glc_amd
    assert [g.store_ragged_slots(1, ch) for ch in (1, 2, 3, 6)] == [(1, 2), (1, 2), (2, 3), (2, 3)]
    more = lambda length: [g.store_ragged_slots(length, ch)[0] - g.store_crop_slots(length, ch)[0] for ch in (1, 2, 3, 6)]
    assert more(2) == [0, 0, 1, 1]          # one sample of 3 or 6 channels across a boundary, and one of padding
    assert more(1024) == [1, 1, 1, 1]
    assert more(1025) == [1, 1, 0, 0]       # two samples of 1 or 2 channels across a boundary, 1023 of padding behind them
    assert more(1026) == [0, 0, 1, 1]


def test_refused_arguments(glc_amd):
    g = glc_amd
    descs, frames = C.c_uint64(7), C.c_uint64(7)
    f = g.lib.glc_store_ragged_slots
    assert f(1000, 2, C.byref(descs), C.byref(frames)) == 0 and (descs.value, frames.value) == (3, 3)
    assert f(1000, 2, None, C.byref(frames)) == EINVAL
    assert f(1000, 2, C.byref(descs), None) == EINVAL
    assert f(1000, 0, C.byref(descs), C.byref(frames)) == EINVAL
    assert f(0, 2, C.byref(descs), C.byref(frames)) == EINVAL
    assert f(2 ** 63, 2, C.byref(descs), C.byref(frames)) == EINVAL  # length * channels wraps
    assert (descs.value, frames.value) == (3, 3)                       # a refused call writes nothing
    assert b"glc_store_ragged_slots" in g.lib.glc_last_error(None)
    with pytest.raises(g.GlcError) as e:
        g.store_ragged_slots(0, 2)
    assert e.value.code == EINVAL
    with pytest.raises(g.GlcError):
        g.store_ragged_slots(-1, 2)
