"""The scaffolding of the device oracle tests (arena.py) on the CPU: every "whole arena equals the
model" assertion of the GPU suite rests on the regions naming the bytes they say they name, on slots
that do not overlap, on guards that are there, and on check_arena seeing a single differing byte.
"""
import re

import numpy as np
import pytest

from arena import CANARY, GUARD, LAYOUTS, Region, canary_image, check_arena, place, rup16

CODES = [(1, 0), (2, 1), (8, 4), (33, 20)]
LENS = [1, 16, 17]
BLOCKS = [1, 5]


@pytest.fixture(params=[(lay, k, m, L, B) for lay in LAYOUTS for k, m in CODES for L in LENS for B in BLOCKS],
                ids=lambda p: "%s-%d-%d-%d-%d" % p)
def case(request):
    lay, k, m, L, B = request.param
    data, par = place(lay, k, m, L, B)
    return data, par, canary_image([data, par]), k, m, L, B


def test_rup16():
    assert [rup16(x) for x in (0, 1, 15, 16, 17, 1202)] == [0, 16, 16, 16, 32, 1216]


def test_index_view_and_at_name_the_same_bytes(case):
    data, par, img, k, m, L, B = case
    assert (data.rows, par.rows, data.B, par.B) == (k, m, B, B) and data.ss == par.ss
    for reg in (data, par):
        for lo, hi in ((0, L), (L, rup16(L)), (0, reg.ss)):
            want = np.array([[[reg.off + b * reg.bs + r * reg.ss + x for x in range(lo, hi)]
                              for r in range(reg.rows)] for b in range(B)], dtype=np.int64).reshape(B, reg.rows, hi - lo)
            idx = reg.index(lo, hi)
            assert idx.shape == want.shape and np.array_equal(idx, want)
            # a view writes the bytes the index names, and nothing else
            mark = img.copy()
            reg.view(mark, lo, hi)[...] = 0x11
            model = img.copy()
            model[idx] = 0x11
            assert np.array_equal(mark, model)
            for b in range(B):
                for r in range(reg.rows):
                    assert reg.at(b, r) == reg.off + b * reg.bs + r * reg.ss
                    if hi > lo:
                        assert reg.at(b, r) + lo == idx[b, r, 0]
        assert np.array_equal(reg.view(img), reg.view(img, 0, reg.ss))
    ro = img.copy()
    ro.setflags(write=False)
    assert not data.view(ro, 0, L).flags.writeable


def test_slots_do_not_overlap_and_lie_between_the_guards(case):
    data, par, img, k, m, L, B = case
    R = rup16(L)
    count = np.zeros(img.size, dtype=np.int32)
    for reg in (data, par):
        np.add.at(count, reg.index(0, R).ravel(), 1)
    assert count.max() <= 1 and count.sum() == B * (k + m) * R
    used = np.flatnonzero(count)
    assert used[0] >= GUARD and img.size - 1 - used[-1] >= GUARD
    assert (img == CANARY).all() and img.dtype == np.uint8
    for reg in (data, par):
        assert reg.off % 16 == 0 and reg.bs % 16 == 0 and reg.ss % 16 == 0 and reg.ss >= R


def test_end_is_one_past_the_last_slots_stride(case):
    data, par, img, k, m, L, B = case
    for reg in (data, par):
        if reg.rows:
            assert reg.end() == reg.at(B - 1, reg.rows - 1) + reg.ss
        else:
            assert reg.end() == reg.at(B - 1, 0) + reg.ss   # as a region of one row
    assert img.size == max(data.end(), par.end()) + GUARD


def test_regions_refuse_unaligned_offsets_and_strides():
    Region(256, 48, 16, 2, 3)
    for off, bs, ss in ((264, 48, 16), (256, 40, 16), (256, 48, 24)):
        with pytest.raises(AssertionError):
            Region(off, bs, ss, 2, 3)
    with pytest.raises(AssertionError):
        canary_image([Region(GUARD - 16, 48, 16, 2, 3)])
    with pytest.raises(ValueError):
        place("no_such_layout", 2, 1, 16, 1)


def test_check_arena_names_the_first_differing_byte(case):
    data, par, img, k, m, L, B = case
    check_arena(img.copy(), img, "equal")
    slots = np.concatenate([r.index(0, L).ravel() for r in (data, par)])
    first, last = int(slots.min()), int(slots.max())   # the first and the last byte a call may touch
    for off in (first, last, 0, GUARD - 1, img.size - GUARD, img.size - 1):
        got = img.copy()
        got[off] ^= 0x10
        with pytest.raises(AssertionError, match=re.escape("here: 1 bytes differ from the model, first at arena "
                                                           "offset %d (got 0x%02x, want 0x%02x)"
                                                           % (off, CANARY ^ 0x10, CANARY))):
            check_arena(got, img, "here")
    got = img.copy()
    got[[first, img.size - 1]] = 0
    with pytest.raises(AssertionError, match="2 bytes differ from the model, first at arena offset %d " % first):
        check_arena(got, img, "two")
