"""The model of glc_store_compact_device (tests/store_compact_cases.py) held to the invariants include/glc.h states, on every
case the GPU tests run: what tests/test_store_compact.py compares the device with must itself be what the header says."""
import numpy as np
import pytest

import store_compact_cases as M

CASES = M.all_cases()


def run(case):
    arena = M.arena_of(case)
    dst = None if case["dst_bytes"] is None else np.full(case["dst_bytes"], M.PATTERN, np.uint8)
    return arena, dst, M.compact(arena, case["arena_bytes"], case["entries"], case["lengths"], case["keep"], dst, case["dst_bytes"])


def test_case_names_are_unique():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_offsets_ascend_and_never_exceed_the_old_ones(case):
    arena, dst, got = run(case)
    n, n_out = len(case["entries"]), got["n_out"]
    kept = [i for i in range(n) if got["new_index"][i] >= 0]
    assert [got["new_index"][i] for i in kept] == list(range(n_out))
    place = 0
    for k, i in enumerate(kept):
        new, old = got["entries"][k], case["entries"][i]
        assert new[0] == place and new[0] % 64 == 0 and new[0] <= old[0]
        assert new[1] == old[1] and new[2] == old[2] and new[3] & 0xFFFFFFFF == old[3] & 0xFFFFFFFF
        assert got["lengths"][k] == case["lengths"][i]
        place += new[1]
    assert got["cursor"] == place <= case["arena_bytes"]
    assert all(e == [0, 0, 0, 0] for e in got["entries"][n_out:]) and not any(got["lengths"][n_out:])
    # kept sources ascend and are disjoint, inside the arena
    ends = 0
    for i in kept:
        assert case["entries"][i][0] >= ends
        ends = case["entries"][i][0] + case["entries"][i][1]
    assert ends <= case["arena_bytes"]
    dst_bytes = case["arena_bytes"] if dst is None else case["dst_bytes"]
    stored = [e[3] >> 32 for e in got["entries"][:n_out]]
    assert stored == sorted(stored, reverse=True)                     # the stored ones are a prefix
    limit = 0
    for k, i in enumerate(kept):
        new, old = got["entries"][k], case["entries"][i]
        assert stored[k] == int(new[0] + new[1] <= dst_bytes)
        if stored[k]:
            assert np.array_equal(got["arena"][new[0]:new[0] + new[1]], arena[old[0]:old[0] + old[1]])
            limit = new[0] + new[1]
    before = arena if dst is None else dst
    assert np.array_equal(got["arena"][limit:], before[limit:])       # nothing at or above the last stored blob's end
    if dst is None:
        assert stored == [1] * n_out and limit == got["cursor"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_compacting_the_result_with_all_ones_changes_nothing(case):
    arena, dst, got = run(case)
    n_out = got["n_out"]
    if n_out == 0:
        return
    size = got["arena"].size
    again = M.compact(got["arena"], size, got["entries"][:n_out], got["lengths"][:n_out], [1] * n_out)
    n_stored = sum(e[3] >> 32 for e in got["entries"][:n_out])
    assert again["n_out"] == n_stored
    assert again["entries"][:n_stored] == got["entries"][:n_stored] and again["lengths"][:n_stored] == got["lengths"][:n_stored]
    assert again["new_index"] == list(range(n_stored)) + [M.UNUSABLE] * (n_out - n_stored)
    assert np.array_equal(again["arena"], got["arena"])


def test_precedence_of_the_three_codes():
    ab = 4096
    bad = M.entry(0, 64, stored=0)                    # unusable, and below the end of the candidate in front of it
    low = M.entry(0, 64)                              # usable, out of order
    front = M.entry(1024, 64)
    arena = np.zeros(ab, np.uint8)
    for e, keep, want in ((bad, 0, M.DROPPED), (bad, 1, M.UNUSABLE), (low, 0, M.DROPPED), (low, 1, M.OUT_OF_ORDER)):
        got = M.compact(arena, ab, [front, e], [1, 2], [1, keep])
        assert got["new_index"] == [0, want] and got["n_out"] == 1 and got["cursor"] == 64
    # an unusable entry is no candidate: it does not raise the maximum
    got = M.compact(arena, ab, [M.entry(2048, 64, stored=0), M.entry(0, 64)], None, [1, 1])
    assert got["new_index"] == [M.UNUSABLE, 0] and got["lengths"] is None
    # an out-of-order candidate is one: it does
    got = M.compact(arena, ab, [M.entry(0, 1024), M.entry(512, 1024), M.entry(1024, 64)], None, [1, 1, 1])
    assert got["new_index"] == [0, M.OUT_OF_ORDER, M.OUT_OF_ORDER]


def test_the_case_list_covers_every_verdict():
    seen, unstored, moved_out, rounds = set(), 0, 0, set()
    for case in CASES:
        _, dst, got = run(case)
        seen |= {v if v < 0 else 0 for v in got["new_index"]}
        unstored += sum(1 for e in got["entries"][:got["n_out"]] if e[3] >> 32 == 0)
        moved_out += dst is not None
        rounds.add(case["round"])
    assert seen == {0, M.DROPPED, M.UNUSABLE, M.OUT_OF_ORDER}
    assert unstored >= 1 and moved_out >= 3 and rounds == {None, *M.ROUNDS}
    by_name = {c["name"]: c for c in CASES}
    # the carried maximum: the offender is in the chunk in front of its victims
    c = by_name["scan_carried_maximum"]
    got = M.compact(M.arena_of(c), c["arena_bytes"], c["entries"], c["lengths"], c["keep"])
    assert got["new_index"][1020] == 1020 and got["new_index"][1021:1040] == [M.OUT_OF_ORDER] * 19
    assert got["new_index"][1040] == 1021 and 1020 // M.CHUNK != 1039 // M.CHUNK
    # the wrapping fields are what they say
    for name in ("offset_wraps", "bytes_wrap"):
        e = by_name[f"unusable_{name}_keep_1"]["entries"][2]
        assert max(e[0], e[1]) == M.U64 - 64
