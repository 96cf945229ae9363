"""Replay data path: play-window / goal sampling, the uint8 dataset resident in HBM (or in pinned
host memory behind a copy stream), GPU augmentations; the vector-observation (D4RL) window replay and its datamodule
(d4rl_replay.py); the relay-imitation-learning replay and its datamodule (relay_replay.py); the play-window replay sampled on
the device and its datamodule (play_replay.py)."""
from .play_replay import HbmPlayReplay, PlayDataModule, PlayWindowLoader  # noqa: F401
from .relay_replay import HbmRelayReplay, RelayIndex, RelayLoader, RILDataModule  # noqa: F401
