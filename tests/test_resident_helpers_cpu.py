"""The index helpers the four resident data paths share (tacorl_amd/data/resident.py): `episode_end` in both variants,
`validate_episodes`, and the refusal of the same bad episode tables by the index classes that call it."""
import numpy as np
import pytest

from tacorl_amd.data.resident import episode_end, neighbour_csr, pick, validate_episodes

EP = np.array([[10, 19], [20, 29], [40, 49]], dtype=np.int64)  # three episodes, a gap at 30 .. 39
#                  before  start end  start end  gap start end past
STEPS = np.array([5,      10,   19,  20,   29,  35, 40,   49, 60])
BAD = {"unsorted": ([[20, 29], [10, 19]], 64), "overlapping": ([[10, 25], [20, 29]], 64), "negative": ([[-1, 9], [20, 29]], 64),
       "out_of_range": ([[10, 19], [20, 29]], 25)}


def test_episode_end_in_both_variants():
    from tacorl_amd.data.relay_replay import RelayIndex
    from tacorl_amd.data.replay import PlayIndex, TransitionIndex

    clamped = np.array([19, 19, 19, 29, 29, 29, 49, 49, 49])  # the last episode that starts at or before the step, else the first
    missing = np.array([-1, 19, 19, 29, 29, -1, 49, 49, -1])  # -1 where no episode holds the step
    assert np.array_equal(episode_end(EP, STEPS), clamped)
    assert np.array_equal(episode_end(EP, STEPS, missing=-1), missing)
    assert int(episode_end(EP, 35)) == 29 and int(episode_end(EP, 35, missing=-7)) == -7  # a scalar step, another marker
    assert episode_end(EP, STEPS, missing=-1).dtype == np.int64
    # the index classes answer through it: PlayIndex with the marker, the others clamped
    assert np.array_equal(PlayIndex(EP, 4, 4).episode_end(STEPS), missing)
    assert np.array_equal(TransitionIndex(EP).episode_end(STEPS), clamped)
    assert np.array_equal(RelayIndex(EP, max_low_level_window=2, max_high_level_window=4).episode_end(STEPS), clamped)


def test_validate_episodes_returns_the_table_and_its_length():
    ep, n = validate_episodes([[10, 19], [20, 29], [40, 49]])
    assert ep.dtype == np.int64 and ep.shape == (3, 2) and n == 50
    assert validate_episodes(EP, 64)[1] == 64
    assert validate_episodes([[3, 3]], 4)[1] == 4  # a one-frame episode at the last frame is inside
    with pytest.raises(ValueError, match="no episodes"):
        validate_episodes(np.zeros((0, 2), np.int64), 64)
    with pytest.raises(ValueError, match="sorted"):
        validate_episodes([[10, 5]], 64)  # an end before its start


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_episode_tables_are_refused(name):
    from tacorl_amd.data.play_replay import validate_play_tables
    from tacorl_amd.data.relay_replay import RelayIndex
    from tacorl_amd.data.replay import PlayIndex, TransitionIndex

    ep, n = BAD[name]
    match = "episode bounds" if name in ("negative", "out_of_range") else "sorted"
    with pytest.raises(ValueError, match=match):
        validate_episodes(ep, n)
    with pytest.raises(ValueError, match=match):
        TransitionIndex(ep, n_frames=n)
    with pytest.raises(ValueError, match=match):
        RelayIndex(ep, n_frames=n, max_low_level_window=2, max_high_level_window=4)
    ix = PlayIndex(ep, 4, 4)  # PlayIndex itself validates nothing against a dataset: validate_play_tables does
    with pytest.raises(ValueError, match=match):
        validate_play_tables(ix, n)


def test_neighbour_csr_and_pick():
    from tacorl_amd.data.neighbours import NeighbourTable

    tab, nn, ptr, val = neighbour_csr({5: [7, 9], 2: []})
    assert tab is None and sorted(nn) == [2, 5] and ptr.tolist() == [0, 0, 0, 0, 0, 0, 2] and val.tolist() == [7, 9]
    assert ptr.dtype == val.dtype == np.int64
    tab, nn, ptr, val = neighbour_csr(None)
    assert tab is None and nn == {} and ptr.tolist() == [0] and len(val) == 0 and val.dtype == np.int64
    table = NeighbourTable.from_dict({5: [7, 9]}, 16)
    tab, nn, ptr, val = neighbour_csr(table, 16)
    assert tab is table and nn is None and val.tolist() == [7, 9]
    assert int(ptr[6] - ptr[5]) == 2 and int(ptr[5]) == 0
    for bad in ({5: [16]}, {16: [1]}, {-1: [1]}, {5: [-2]}, table):  # with n_frames, every key and neighbour lies inside
        with pytest.raises(ValueError, match="nn_steps_from_step"):
            neighbour_csr(bad, 8 if bad is table else 16)
    neighbour_csr({5: [16]})  # ... and without, nothing is checked
    u = np.array([0.0, 0.5, 0.999, 1.0])
    assert pick(u, np.full(4, 4)).tolist() == [0, 2, 3, 3]      # floor(u n), u = 1 kept inside
    assert pick(u, np.zeros(4, np.int64)).tolist() == [0, 0, 0, 0]  # nothing to choose from: 0, not -1
