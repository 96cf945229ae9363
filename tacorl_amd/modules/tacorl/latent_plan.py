"""What the two TACORLs (tacorl.TACORL on images, tacorl_d4rl.TACORL on vector observations) share on top of their
CQL_Offline: the frozen PlayLMP they are built from and its action decoder - adopted as `action_decoder.*`, optionally
fine-tuned with an Adam of its own whose gradients travel in the engine's arena.  The two `_step`s (segments, side graphs,
keys) stay with the classes."""
from pathlib import Path

import torch

from ... import dist as D
from ..common import register_views


class LatentPlanShell:
    def __init__(self, play_lmp_dir: str = "~/tacorl/models/play_lmp", lmp_epoch_to_load: int = -1,
                 overwrite_lmp_cfg: dict = {}, finetune_action_decoder: bool = False, action_decoder_lr: float = 1e-4, *args,
                 play_lmp=None, **kwargs):
        self.play_lmp_dir = Path(play_lmp_dir).expanduser()
        self.lmp_epoch_to_load = lmp_epoch_to_load
        self.overwrite_lmp_cfg = overwrite_lmp_cfg
        self.finetune_action_decoder = finetune_action_decoder
        self.action_decoder_lr = action_decoder_lr
        # opt-in to a full unpickle of the PlayLMP checkpoint (real PL checkpoints carry DictConfig hyper-parameters)
        self.lmp_unsafe_pickle = bool(kwargs.pop("lmp_unsafe_pickle", False))
        self.__dict__["_play_lmp"] = play_lmp  # nn.Module: must not be registered as a sub-module
        super().__init__(*args, **kwargs)

    def _adopt_decoder(self):
        """The LMP's action decoder becomes this module's `action_decoder.*` (parameters and buffers); its loss reaches the
        logged scalars; fine-tuned, its gradients join [actor | q1 | q2 | log_alpha'] in the engine's arena: with several GPUs
        the step's second all-reduce covers them - no third collective inside the first segment."""
        e, ad = self.engine, self.ad
        self._ad_pv = register_views(self, "action_decoder.", ad.blk.views)
        for k, v in ad.buffers.items():
            self.action_decoder.register_buffer(k, v)
        e.pre_metrics = [ad.finish_loss]  # (the decoder loss leaves its partial sums on the device: loss(lazy=True))
        if self.finetune_action_decoder:
            e.extend_arena(ad.blk)

    def named_gradients(self):
        out = super().named_gradients()
        if self.ad is not None and self.finetune_action_decoder:
            out.update({f"action_decoder.{k}": v for k, v in self.ad.blk.grad_views.items()})
        return out

    def configure_optimizers(self):
        o = super().configure_optimizers()
        if self.finetune_action_decoder and self.ad is not None:  # reference tacorl.py:289-300, tacorl_d4rl.py:162-173
            blk = self.ad.blk
            o.append(self._make_adam("action_decoder", [(blk, self._ad_pv, blk.views_of(blk.m), blk.views_of(blk.v))],
                                     self.action_decoder_lr))
        return o

    def _defer_ad_update(self):
        """More than one rank (or the split-graph test mode): the fine-tuned decoder's Adam step waits for the arena's
        all-reduce.  On one GPU it stays on the decoder's own branch of the step's graph."""
        return D.collectives_on(self.world_size) or getattr(self, "_force_graph_split", False)

    def _join_ad(self):
        if getattr(self, "_ad_join", None) is not None:
            torch.cuda.current_stream().wait_stream(self._ad_join)
            self._ad_join = None

    def training_step(self, batch, batch_idx=0, noise=None):
        self._step(batch, noise, optimize=True, log_type="train")
        self._tick_optimizers()

    def validation_step(self, batch, *args, noise=None, **kwargs):
        self._step(batch, noise, optimize=False, log_type="validation")
