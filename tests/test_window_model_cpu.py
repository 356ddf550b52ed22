"""tests/window_model.py on examples small enough to work out by hand (no GPU, no oracle: the verdicts are written down)."""
import numpy as np
import pytest

from window_model import Verdict, WindowModel, check_separation

# three slots: 0 is close (similarity 0.9), 1 is scored and not close (0.9 as well: a tie with slot 0), 2 is outside the length window
V = Verdict(close=[True, False, False], scored=[True, True, False], sim=[0.9, 0.9, -1.0])


def test_six_positions_with_a_tie():
    w = WindowModel([2, 1, 0, 1, 0, 2])
    assert w.alive() == 6 and w.alive(1, 4) == 3
    # positions 1 (slot 1) and 2 (slot 0) tie at 0.9: the lower position wins, whatever its slot; the close ones are 2 and 4
    close, bp, bs, im, n = w.get_close(V, 0, 6)
    assert close.tolist() == [2, 4] and (bp, bs, im, n) == (1, 0.9, False, 6)
    assert w.alive() == 4 and w.alive(2, 3) == 0 and w.alive(4, 5) == 0
    # the close ones are dead: nothing close any more, the tie is between positions 1 and 3 now
    close, bp, bs, im, n = w.get_close(V, 0, 6)
    assert close.size == 0 and (bp, bs, im, n) == (1, 0.9, True, 4)
    w.kill([1])
    close, bp, bs, im, n = w.get_close(V, 0, 6)
    assert close.size == 0 and (bp, bs, im, n) == (3, 0.9, True, 3)
    # a range that holds only the unscored slot: alive, and nothing to choose
    assert w.get_close(V, 5, 6)[1:] == (-1, -1.0, True, 1)
    # the end is cut to the window's
    assert w.get_close(V, 3, 100)[1:] == (3, 0.9, True, 2)


def test_a_higher_similarity_beats_a_lower_position():
    v = Verdict(close=[False, True], scored=[True, True], sim=[0.5, 0.75])
    w = WindowModel([0, 0, 1, 0, 1])
    close, bp, bs, im, n = w.get_close(v, 0, 5)
    assert close.tolist() == [2, 4] and (bp, bs, im, n) == (2, 0.75, False, 5)
    assert w.get_close(v, 0, 5)[1:] == (0, 0.5, True, 3)


def test_a_dead_tile():
    """tiles of four positions: the middle one is killed whole, the first and the last keep one position each"""
    w = WindowModel(np.tile([0, 1, 2, 1], 3))
    w.kill([4, 5, 6, 7])
    w.kill([0, 1, 2, 9, 10, 11])
    assert (w.alive(0, 4), w.alive(4, 8), w.alive(8, 12)) == (1, 0, 1)
    assert w.alive_positions().tolist() == [3, 8]
    close, bp, bs, im, n = w.get_close(V, 0, 12)
    assert close.tolist() == [8] and (bp, bs, im, n) == (3, 0.9, False, 2)
    close, bp, bs, im, n = w.get_close(V, 4, 8)          # the dead tile alone
    assert close.size == 0 and (bp, bs, im, n) == (-1, -1.0, True, 0)


def test_kill_refuses_the_whole_call():
    w = WindowModel([0, 1, 0, 1])
    w.get_close(V, 0, 1)          # position 0 dies by being close
    for bad in ([1, 4], [1, 1], [1, 0], [-1]):
        with pytest.raises(ValueError):
            w.kill(bad)
        assert w.alive() == 3 and w.alive(1, 2) == 1          # position 1, listed first every time, is untouched
    w.kill([])
    w.kill([1, 3])
    assert w.alive_positions().tolist() == [2]


def test_empty_ranges_and_an_empty_window():
    w = WindowModel([0, 1, 0])
    for a, b in ((2, 2), (3, 1), (3, 9), (7, 9)):
        assert w.alive(a, b) == 0
        close, bp, bs, im, n = w.get_close(V, a, b)
        assert close.size == 0 and (bp, bs, im, n) == (-1, -1.0, True, 0)
    assert w.alive() == 3
    e = WindowModel(np.zeros(0, dtype=np.uint32))
    assert e.alive() == 0 and e.get_close(V, 0, 5)[1:] == (-1, -1.0, True, 0)
    with pytest.raises(ValueError):
        e.kill([0])


def test_the_separation_check():
    check_separation(V)          # bit-equal is fine, and the unscored slot's -1 is not looked at
    check_separation(Verdict([True, True, False], [True, True, True], [0.9, 0.9, 0.5]), copies=[(0, 1)])
    with pytest.raises(AssertionError):
        check_separation(V, copies=[(0, 1)])          # copies of one sequence cannot differ in their verdict
    check_separation(Verdict([False] * 3, [True] * 3, [0.5, 0.5 * (1 + 2e-6), 0.5]))
    with pytest.raises(AssertionError):
        check_separation(Verdict([False] * 2, [True] * 2, [0.5, 0.5 * (1 + 1e-7)]))
    with pytest.raises(AssertionError):
        check_separation(Verdict([False] * 2, [True] * 2, [0.5, 0.75]), copies=[(0, 1)])
    with pytest.raises(AssertionError):
        Verdict([True], [False], [-1.0])          # close and unscored cannot be
