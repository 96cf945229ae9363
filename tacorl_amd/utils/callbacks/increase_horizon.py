"""The goal-horizon curriculum of the transition dataset (reference utils/callbacks/increase_horizon.py; config/callbacks/
increase_horizon/{linear,constant}.yaml): after every training epoch the horizon of the `increasing_horizon` goal strategy
grows by the dataset's `horizon_step`, and `train/goal_horizon` is logged.

The reference runs from `on_epoch_end`; pytorch_lightning 1.6 dropped that hook and MiniTrainer never had it, so this runs
from `on_train_epoch_end` - once per training epoch, where `on_epoch_end` fired for the train loop.  The "dataset" is the
TransitionIndex a transition datamodule (or its resident replay) holds: the object that has `goal_strategy_prob`,
`current_horizon` and `increase_horizon(epoch)`; the horizon is a launch argument of the device sampler, so the next batch
is drawn with it.  IncreaseHorizonUncertainty is not built: it needs dropout critics, which no in-scope critic has."""
import torch

from ...lightning import CallbackBase


class IncreaseHorizonLinear(CallbackBase):
    @staticmethod
    def get_dataset(trainer):
        """:7-11, over the places a datamodule of this project keeps its train index."""
        dm = getattr(trainer, "datamodule", None)
        train_ds = getattr(dm, "train_dataset", None)
        if hasattr(train_ds, "dataset"):
            train_ds = train_ds.dataset
        for cand in (train_ds, getattr(dm, "index", None), getattr(getattr(dm, "train_replay", None), "index", None),
                     getattr(getattr(dm, "replay", None), "index", None)):
            if hasattr(cand, "goal_strategy_prob"):
                return cand
        return train_ds

    def on_train_epoch_end(self, trainer, pl_module) -> None:
        train_ds = self.get_dataset(trainer)
        if hasattr(train_ds, "goal_strategy_prob"):
            pl_module.log("train/goal_horizon", torch.tensor(train_ds.current_horizon, dtype=torch.float), on_epoch=True)
            if "increasing_horizon" in train_ds.goal_strategy_prob.keys():
                train_ds.increase_horizon(epoch=pl_module.current_epoch + 1)


class IncreaseHorizonConstant(CallbackBase):
    def on_train_epoch_end(self, trainer, pl_module) -> None:
        pass
