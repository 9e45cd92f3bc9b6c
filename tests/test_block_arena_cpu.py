"""CPU suite: the comparison logic of the guard-band harness (tests/helpers/block_arena.py) on hand-made arenas.  Every planted
defect must be reported, with its kind, at its (row, column), with the right count; a clean arena must pass."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import block_arena as ba  # noqa: E402

N, LD, NCOLS = 37, 64, 9
WINDOWS = [(2, 3), (6, 2)]          # columns 0-1, 5 and 8 are guards


def _bits(x):
    return np.array([x], dtype=np.float64).view(np.uint64)[0]


def _arena():
    """sentinel everywhere, the two windows hold data in rows [0, N) and +0.0 in the padding rows"""
    a = np.full((NCOLS, LD), ba.SENTINEL_BITS, dtype=np.uint64)
    rng = np.random.default_rng(0)
    for first, count in WINDOWS:
        a[first:first + count, :N] = rng.standard_normal((count, N)).view(np.uint64)
        a[first:first + count, N:] = 0
    return a


def test_sentinel_is_a_quiet_nan_with_a_payload():
    v = np.array([ba.SENTINEL_BITS], dtype=np.uint64).view(np.float64)[0]
    assert np.isnan(v) and int(ba.SENTINEL_BITS) >> 51 == 0xFFF and int(ba.SENTINEL_BITS) & ((1 << 51) - 1) != 0
    assert ba.round_up(1, 32) == 32 and ba.round_up(32, 32) == 32 and ba.round_up(33, 32) == 64


def test_clean_arena_passes_and_a_written_window_may_change():
    before = _arena()
    assert ba.find_defects(before, before.copy(), N, WINDOWS, []) == []
    after = before.copy()
    after[2:5, :N] = np.arange(3 * N, dtype=np.float64).reshape(3, N).view(np.uint64)
    assert ba.find_defects(before, after, N, WINDOWS, [(2, 3)]) == []
    ba.assert_contract(before, after, N, WINDOWS, [(2, 3)])


@pytest.mark.parametrize("row,col", [(0, 0), (N - 1, 1), (N, 5), (LD - 1, 8), (17, 5)])
def test_one_flipped_guard_element_is_found_at_its_index(row, col):
    before = _arena()
    after = before.copy()
    after[col, row] ^= np.uint64(1)                      # one payload bit: still a NaN, only a bit compare sees it
    (d,) = ba.find_defects(before, after, N, WINDOWS, WINDOWS)
    assert (d.kind, d.row, d.column, d.count) == (ba.GUARD, row, col, 1)
    assert d.was == int(ba.SENTINEL_BITS) and d.now == int(ba.SENTINEL_BITS) ^ 1
    with pytest.raises(AssertionError, match=r"guard: 1 element\(s\) differ, first at \(row %d, column %d\)" % (row, col)):
        ba.assert_contract(before, after, N, WINDOWS, WINDOWS, what="a test")


def test_first_defect_is_the_first_in_column_major_order_and_all_are_counted():
    before = _arena()
    after = before.copy()
    after[5, 40] = 0
    after[1, 63] = 0
    after[1, 3] = 0
    (d,) = ba.find_defects(before, after, N, WINDOWS, [])
    assert (d.kind, d.row, d.column, d.count) == (ba.GUARD, 3, 1, 3)


@pytest.mark.parametrize("value", [-0.0, 5e-324, 1.0, float("nan")])
@pytest.mark.parametrize("row,col", [(N, 2), (LD - 1, 4), (N + 5, 7)])
def test_nonzero_bits_in_a_padding_row_of_a_written_window(value, row, col):
    before = _arena()
    after = before.copy()
    after[col, row] = _bits(value)
    written = [w for w in WINDOWS if w[0] <= col < w[0] + w[1]]
    (d,) = ba.find_defects(before, after, N, WINDOWS, written)
    assert (d.kind, d.row, d.column, d.count) == (ba.PADDING, row, col, 1)
    # the same store into a window that was NOT declared written is a read-only violation at the same place
    (d,) = ba.find_defects(before, after, N, WINDOWS, [])
    assert (d.kind, d.row, d.column, d.count) == (ba.READ_ONLY, row, col, 1)


def test_padding_rows_of_a_written_window_are_checked_even_if_they_were_bad_before():
    before = _arena()
    before[3, N + 1] = _bits(-0.0)
    (d,) = ba.find_defects(before, before.copy(), N, WINDOWS, [(2, 3)])
    assert (d.kind, d.row, d.column) == (ba.PADDING, N + 1, 3)


def test_changed_read_only_window():
    before = _arena()
    after = before.copy()
    after[6, 11] = _bits(3.0)
    after[7, 0] = _bits(4.0)
    (d,) = ba.find_defects(before, after, N, WINDOWS, [(2, 3)])
    assert (d.kind, d.row, d.column, d.count) == (ba.READ_ONLY, 11, 6, 2)
    assert ba.find_defects(before, after, N, WINDOWS, [(6, 2)]) == []


def test_several_defects_are_all_reported():
    before = _arena()
    after = before.copy()
    after[0, 0] = 0               # guard
    after[2, N] = _bits(1.0)      # padding of the written window
    after[6, 1] = _bits(2.0)      # read-only window
    kinds = [(d.kind, d.row, d.column) for d in ba.find_defects(before, after, N, WINDOWS, [(2, 3)])]
    assert kinds == [(ba.GUARD, 0, 0), (ba.PADDING, N, 2), (ba.READ_ONLY, 1, 6)]


def test_bad_window_tables_are_refused():
    a = _arena()
    with pytest.raises(AssertionError):
        ba.find_defects(a, a, N, [(0, 3), (2, 2)], [])        # overlap
    with pytest.raises(AssertionError):
        ba.find_defects(a, a, N, [(7, 3)], [])                # outside
    with pytest.raises(AssertionError):
        ba.find_defects(a, a, N, [(0, 3)], [(1, 1)])          # written but never handed out


def test_parent_fill_is_recognisable():
    f = ba.parent_fill(5, 3)
    assert f.shape == (5, 3) and f[4, 2] == 3 * 2.0 ** 20 + 4.5 and len(np.unique(f)) == 15
