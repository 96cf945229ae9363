"""The ring of output buffers that the four resident replays inherit (tacorl_amd/data/resident.py ResidentReplay), at the
smallest shapes that exercise it: 64 frames of 8 x 8 x 3 uint8 (192 bytes: the gather moves 16-byte chunks) in two episodes,
A = 7, S = 4 for the D4RL tables, windows 2 .. 4, B = 4, slots = 3."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ("transition", "relay", "d4rl", "play")
N, EP, A, S, B, SLOTS = 64, [[0, 31], [32, 63]], 7, 4, 4, 3


def _replay(kind):
    """(replay, the batch form that uses nothing but the ring: dense for D4RL, whose fused batch holds only its draws)."""
    rs = np.random.RandomState(3)
    frames = {"rgb_static": torch.from_numpy(rs.randint(0, 256, size=(N, 8, 8, 3)).astype(np.uint8)).to(DEV)}
    acts = rs.uniform(-1, 1, size=(N, A)).astype(np.float32)
    kw = dict(device=DEV, batch_size=B, slots=SLOTS)
    if kind == "transition":
        from tacorl_amd.data.replay import HbmTransitionReplay, TransitionIndex

        return HbmTransitionReplay(frames, acts, TransitionIndex(EP, n_frames=N), **kw), True
    if kind == "relay":
        from tacorl_amd.data.relay_replay import HbmRelayReplay, RelayIndex

        return HbmRelayReplay(frames, acts, RelayIndex(EP, n_frames=N, max_low_level_window=2, max_high_level_window=4), **kw), True
    if kind == "d4rl":
        from tacorl_amd.data.d4rl_replay import D4RLWindowIndex, HbmD4RLReplay

        ends = np.zeros(N, bool)
        ends[[e for _, e in EP]] = True
        ix = D4RLWindowIndex(ends, np.zeros(N, bool), min_window_size=2, max_window_size=4, include_goal=True)
        return HbmD4RLReplay(rs.uniform(-1, 1, size=(N, S)).astype(np.float32), acts, ix, **kw), False
    from tacorl_amd.data.play_replay import HbmPlayReplay
    from tacorl_amd.data.replay import PlayIndex

    return HbmPlayReplay(frames, acts, PlayIndex(EP, 2, 4), **kw), True


def _draws(rp, first, n=B, seed=0):
    """Host draws for the n items first, first + 1, ..."""
    d = rp.index.draw(n, np.random.default_rng(seed))
    d["idx"] = np.arange(first, first + n, dtype=np.int64)
    return d


def _ring_tensors(b, out=None, path=()):
    """{path: tensor} of a batch's tensors that are views of the replay's buffers (`idx` is the draw itself, and a fused
    batch's `frames` are the dataset)."""
    out = {} if out is None else out
    for k, v in b.items():
        if torch.is_tensor(v) and k != "idx":
            out[path + (k,)] = v
        elif isinstance(v, dict) and k != "frames":
            _ring_tensors(v, out, path + (k,))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_a_dense_batch_lives_for_slots_minus_one_more(kind):
    rp, _ = _replay(kind)
    first = _ring_tensors(rp.batch(_draws(rp, 0), fused=False))
    assert first and len(rp._ring) == SLOTS
    snap = {k: v.clone() for k, v in first.items()}
    for j in range(1, SLOTS):  # slots - 1 further batches land in the other slots
        rp.batch(_draws(rp, 8 * j, seed=j), fused=False)
        assert all(torch.equal(first[k], snap[k]) for k in first), (kind, j)
    last = _ring_tensors(rp.batch(_draws(rp, 8 * SLOTS, seed=SLOTS), fused=False))  # ... and the next one in the first's
    assert sorted(last) == sorted(first)
    assert all(last[k].data_ptr() == first[k].data_ptr() and torch.equal(last[k], first[k]) for k in first)
    assert any(not torch.equal(first[k], snap[k]) for k in first)
    rp.check()


@pytest.mark.parametrize("kind", KINDS)
def test_a_larger_batch_replaces_the_ring_once(kind, monkeypatch):
    from tacorl_amd import ops

    rp, fused = _replay(kind)
    calls, note = [], ops.note_alloc
    monkeypatch.setattr(ops, "note_alloc", lambda: (calls.append(1), note())[1])
    rp.batch(_draws(rp, 0), fused=fused)
    old = [dict(s) for s in rp._ring]
    assert rp._cap == B and not calls  # a batch of the capacity allocates nothing
    epoch = ops.alloc_epoch()
    big = rp.batch(_draws(rp, 0, n=B + 2), fused=fused)
    assert rp._cap == B + 2 and len(calls) == 1 and ops.alloc_epoch() == epoch + 1
    assert all(new[k] is not was[k] and new[k].numel() * B == was[k].numel() * (B + 2) for new, was in zip(rp._ring, old) for k in was)
    assert all(v.shape[0] == B + 2 for k, v in _ring_tensors(big).items() if k[-1] != "ids")
    new = [dict(s) for s in rp._ring]
    rp.batch(_draws(rp, 8, n=B + 2, seed=1), fused=fused)  # a second batch of that size: the same buffers, no allocation
    assert len(calls) == 1 and all(s[k] is was[k] for s, was in zip(rp._ring, new) for k in was)
    rp.batch(_draws(rp, 16, seed=2), fused=fused)          # ... and a smaller one is a view of them
    assert len(calls) == 1 and rp._cap == B + 2
    rp.check()


@pytest.mark.parametrize("kind", KINDS)
def test_check_raises_after_one_item_outside_the_index(kind):
    rp, fused = _replay(kind)
    rp.batch(_draws(rp, 0), fused=fused)
    rp.check()  # nothing was clamped: no error, and the status word stays 0
    assert int(rp.status.item()) == 0
    d = _draws(rp, 4)
    d["idx"][1] = len(rp.index) + 5
    rp.batch(d, fused=fused)
    with pytest.raises(IndexError, match="clamp"):
        rp.check()
