"""The D4RL rollout evaluation (reference utils/callbacks/rollout_d4rl.py; config/callbacks/{play_lmp_d4rl,rl_d4rl}.yaml ->
`rollout:`): `val_episodes` episodes in the AntMaze environments every `val_every_n_*`, published as `val_accuracy`,
`val_episode_return` and `val_score` (the environment's get_normalized_score of the return).

The managers of evaluation/rollout_manager_d4rl.py are selected by the `_target_` leaf as in callbacks/rollout.py (RLRollout,
LatentPlanRollout, TACORL); observations are vectors, the goal is the environment's `target_goal` (vec_policy.
default_batch_obs), and the episodes run len(envs) at a time.  On an epoch without an evaluation the three `val_*` keys are
-inf (the reference stops there with a KeyError on `score`, :181)."""
from .rollout import RolloutBase, _world_rank, flat_metrics, rank_split


class Rollout(RolloutBase):
    """reference utils/callbacks/rollout_d4rl.py Rollout, with `envs` / `n_envs` / `seed` added.  `log_video` is accepted and
    ignored: video logging, `render` and wandb are not built."""

    SCORE = True

    def __init__(self, rollout_manager, val_episodes=32, skip_first_n_epochs=0, val_every_n_epochs=None,
                 val_every_n_episodes=None, val_every_n_batches=None, envs=None, n_envs=None, seed=0, log_video=False):
        self._init_schedule(rollout_manager, val_episodes, skip_first_n_epochs, val_every_n_epochs, val_every_n_episodes,
                            val_every_n_batches, envs, n_envs, seed)
        if not self.d4rl:
            raise ValueError(f"rollout_manager._target_ {dict(rollout_manager).get('_target_')!r}: the D4RL callback takes the "
                             "managers of tacorl.evaluation.rollout_manager_d4rl")

    def evaluate(self, pl_module, num_episodes=5, render=False):
        """:53-95."""
        world, rank = _world_rank()
        infos = self._run_episodes(pl_module, [(("episode", e), {}) for e in rank_split(num_episodes, world, rank)])
        self.last_infos = infos
        return flat_metrics(infos, score=True)

    def _evaluate_and_log(self, pl_module, log_type, on_step, on_epoch):
        return self.evaluate(pl_module, num_episodes=self.val_episodes)  # :105
