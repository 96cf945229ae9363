"""The neighbour table of the similar_robot_obs strategy, without a GPU: the NumPy restatement of the search + margin filter
against the file the unmodified reference class wrote (tests/golden/nn_table.npz, tools/gen_nn_table_golden.py) and against
an fp64 brute-force oracle, the NeighbourTable plumbing into the sampling indices, and the argument checks of the C ABI."""
import json

import numpy as np
import pytest

from tests import knn_ref as R


def test_host_restatement_equals_the_reference_file():
    from tacorl_amd.data.neighbours import knn_l2_host, nn_steps_from_step_host

    g = R.golden()
    got = nn_steps_from_step_host(g["robot_obs"], g["ep"], g["num_nn"], g["margin"])
    steps = np.concatenate([np.arange(s, e) for s, e in g["ep"]])
    assert sorted(g["nn"]) == steps.tolist() == sorted(got)      # exactly the range(start, end) steps: no episode end step
    assert all(got[s] == g["nn"][s] for s in steps.tolist())     # list for list, in order
    # what the fixture covers (the generator asserts the same)
    assert any(len(v) == 0 for v in g["nn"].values()) and any(len(v) > 0 for v in g["nn"].values())
    pts, _ = R.golden_points()
    rows, _ = knn_l2_host(pts, g["num_nn"])
    dt = np.abs(steps[rows] - steps[:, None])
    assert (dt == g["margin"] - 1).any() and (dt >= g["margin"]).any()
    q, s = np.nonzero(dt == g["margin"] - 1)
    assert all(int(steps[rows[a, b]]) not in g["nn"][int(steps[a])] for a, b in zip(q, s))  # dropped at |dt| = margin - 1
    # the duplicate frames: an exact copy far away in time is a surviving neighbour at distance 0
    assert 10 in g["nn"][250] and 250 in g["nn"][10]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fp32_restatement_against_fp64_oracle(seed):
    """Standard-normal points, N = 1500, D = 15, k = 32: the ordered lists may differ from the fp64 oracle's only between
    entries whose fp64 distances lie within relative 2 (D + 3) 2^-24, and for at most 1 % of the queries."""
    pts, rows32, dist32 = R.host_knn("normal", seed, 32)
    rows64, d64 = R.knn_fp64(pts, 32)
    need = R.queries_needing_allowance(rows32, rows64, d64, pts.shape[1])
    print(f"seed {seed}: {need} of {len(pts)} queries need the near-tie allowance")
    assert need <= len(pts) // 100
    ref = np.take_along_axis(d64, rows32.astype(np.int64), axis=1)
    rel = np.abs(dist32 - ref)[ref > 0] / ref[ref > 0]
    print(f"seed {seed}: max relative distance error {rel.max():.3g}")
    assert rel.max() <= (15 + 2) * 2.0 ** -24   # the one-sided bound of the D + 2 roundings behind each fp32 distance


def _table():
    from tacorl_amd.data.neighbours import NeighbourTable

    g = R.golden()
    return g, NeighbourTable.from_dict(g["nn"], n_frames=len(g["robot_obs"]))


def test_table_round_trips_through_the_reference_file_schema(tmp_path):
    from tacorl_amd.data.neighbours import NeighbourTable

    g, tab = _table()
    assert tab.to_dict() == g["nn"] and tab.n_frames == 300 and tab.ptr.numel() == 301
    path = tmp_path / "nn.json"
    tab.save_json(path, "train")
    assert path.read_text() == g["nn_json"]                       # byte for byte what the reference wrote
    tab.save_json(path, "validation")                             # merges: the train table stays
    doc = json.loads(path.read_text())
    assert list(doc) == ["train", "validation"] and doc["train"] == doc["validation"]
    back = NeighbourTable.load_json(path, "validation", 300)
    assert back.to_dict() == g["nn"]
    assert np.array_equal(back.ptr.numpy(), tab.ptr.numpy()) and np.array_equal(back.val.numpy(), tab.val.numpy())
    with pytest.raises(KeyError):
        NeighbourTable.load_json(path, "test", 300)


def test_indices_adopt_a_table_like_its_dict():
    from tacorl_amd.data.replay import PlayIndex, TransitionIndex

    g, tab = _table()
    probs = {"geometric": 0.5, "similar_robot_obs": 0.5}
    a = TransitionIndex(g["ep"], n_frames=300, goal_strategy_prob=probs, nn_steps_from_step=tab)
    b = TransitionIndex(g["ep"], n_frames=300, goal_strategy_prob=probs, nn_steps_from_step=tab.to_dict())
    assert np.array_equal(a._nn_ptr, b._nn_ptr) and np.array_equal(a._nn_val, b._nn_val)
    assert a._nn_ptr.dtype == b._nn_ptr.dtype == a._nn_val.dtype == b._nn_val.dtype == np.int64
    d = a.draw(512, np.random.default_rng(0))
    sa, sb = a.sample(None, d), b.sample(None, d)
    assert all(np.array_equal(sa[k], sb[k]) for k in sb)
    assert ((d["strategy"] == 1) & np.isin(sa["goal"], tab.val.numpy())).sum() > 50  # neighbour goals were drawn
    p = PlayIndex(g["ep"], goal_strategy_prob=probs, nn_steps_from_step=tab)
    q = PlayIndex(g["ep"], goal_strategy_prob=probs, nn_steps_from_step=tab.to_dict())
    assert np.array_equal(p._nn_ptr, q._nn_ptr) and np.array_equal(p._nn_val, q._nn_val)
    rng = np.random.default_rng(1)
    idx, dd = rng.integers(0, len(p), size=512), p.draw(512, rng)
    sp, sq = p.sample(idx, dd), q.sample(idx, dd)
    assert all(np.array_equal(sp[k], sq[k]) for k in sq)
    # the table's range validation is vectorised: one bad step anywhere is refused
    from tacorl_amd.data.neighbours import NeighbourTable
    with pytest.raises(ValueError):
        TransitionIndex(g["ep"], n_frames=300, nn_steps_from_step=NeighbourTable.from_dict({3: [300]}, n_frames=301))
    with pytest.raises(ValueError):
        TransitionIndex(g["ep"], n_frames=300, nn_steps_from_step=NeighbourTable.from_dict({300: [1]}, n_frames=301))


@pytest.mark.parametrize("build", ["host", "device"])
def test_validation_errors(build):
    """Both entry points validate before any arithmetic (and the device one before it touches a device)."""
    from tacorl_amd.data import neighbours as NB

    fn = NB.nn_steps_from_step_host if build == "host" else NB.build_nn_steps_from_step
    obs = np.zeros((40, 15), np.float32)
    ep = [[0, 19], [20, 39]]
    bad = obs.copy()
    bad[7, 3] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        fn(bad, ep, 8, 4)
    bad[7, 3] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        fn(bad, ep, 8, 4)
    with pytest.raises(ValueError, match="overlap"):
        fn(obs, [[0, 20], [20, 39]], 8, 4)
    with pytest.raises(ValueError, match="overlap"):
        fn(obs, [[20, 39], [0, 19]], 8, 4)
    with pytest.raises(ValueError, match="outside"):
        fn(obs, [[0, 19], [20, 40]], 8, 4)
    with pytest.raises(ValueError, match="num_nn"):
        fn(obs, ep, 65, 4)
    with pytest.raises(ValueError, match="num_nn"):
        fn(obs, ep, 0, 4)
    with pytest.raises(ValueError, match="columns"):
        fn(np.zeros((40, 33), np.float32), ep, 8, 4)
    bad[7, 3] = 0.0
    bad[19, 0] = np.nan   # an episode's end step is not searched: its values do not matter
    if build == "host":
        assert sorted(fn(bad, ep, 8, 4)) == list(range(0, 19)) + list(range(20, 39))


def test_knn_abi_refuses_bad_arguments_without_gpu():
    """tacorl_knn_l2 / tacorl_nn_margin_filter validate before they touch the device (nothing is launched here); the
    blocking constants that ops exports are the library's."""
    from tacorl_amd import _lib, ops

    L = _lib.lib()
    sup = L.tacorl_knn_l2_supported
    assert sup(1, 1) == 1 and sup(32, 64) == 1 and sup(15, 32) == 1
    assert sup(0, 32) == 0 and sup(33, 32) == 0 and sup(15, 0) == 0 and sup(15, 65) == 0 and sup(-1, -1) == 0
    assert L.tacorl_knn_l2_tile() == ops.KNN_TILE
    assert L.tacorl_knn_l2_query_block(32) == L.tacorl_knn_l2_query_block(1) == ops.KNN_QUERY_BLOCK
    assert L.tacorl_knn_l2_query_block(33) == L.tacorl_knn_l2_query_block(64) == ops.KNN_QUERY_BLOCK_K64
    assert L.tacorl_knn_l2_query_block(0) == 0 and L.tacorl_knn_l2_query_block(65) == 0
    P = 4096  # (never dereferenced: every call below is refused in the argument checks)

    def knn(points=P, n=100, D=15, ld=15, q0=0, nq=100, k=32, rows=P, dist=P):
        return L.tacorl_knn_l2(points, n, D, ld, q0, nq, k, rows, dist, None)

    assert knn(points=None) != 0 and knn(rows=None) != 0
    assert knn(points=P + 2) != 0 and knn(rows=P + 1) != 0 and knn(dist=P + 2) != 0
    assert knn(ld=14) != 0 and knn(D=0) != 0 and knn(D=33, ld=33) != 0
    assert knn(q0=1) != 0 and knn(q0=90, nq=11) != 0 and knn(q0=-1, nq=10) != 0 and knn(nq=0) != 0 and knn(nq=-5) != 0
    assert knn(k=0) != 0 and knn(k=65) != 0 and knn(n=0, nq=0) != 0 and knn(n=2**31, nq=1) != 0

    def filt(rows=P, nq=100, k=32, q0=0, steps=P, n=100, margin=16, out=P, count=P):
        return L.tacorl_nn_margin_filter(rows, nq, k, q0, steps, n, margin, out, count, None)

    assert filt(rows=None) != 0 and filt(steps=None) != 0 and filt(out=None) != 0 and filt(count=None) != 0
    assert filt(rows=P + 2) != 0 and filt(steps=P + 4) != 0 and filt(out=P + 4) != 0 and filt(count=P + 1) != 0
    assert filt(q0=1) != 0 and filt(q0=95, nq=6) != 0 and filt(nq=0) != 0 and filt(k=0) != 0 and filt(k=65) != 0
    assert filt(margin=-1) != 0 and filt(n=0, nq=0) != 0
