"""What the long-horizon rollout tests share (tests/rollout_envs.py's scripted infos carry no `successful_tasks`):

  * the synthetic start_end_tasks.json and the scripted rollout_info that tools/gen_rollout_lh_callback_golden.py answers the
    reference callback's episodes with, and tests/test_rollout_lh_cpu.py this project's;
  * ScriptedVectorEnv: a vector environment (the D4RL surface) whose episode - start, length, tasks - comes from `reset(...)`
    alone, so any slot can run any episode; float64 host arithmetic, an episode is a function of its actions' bits;
  * greedy_makespan / batch_makespan: the policy calls of a refilled and of a fixed-batch evaluation, from the lengths.
NumPy only."""
import zlib

import numpy as np

A, B, C, D, E = "open_drawer", "move_block_left", "turn_on_light", "lift_block", "close_drawer"
# 5 windows of two tasks, 4 of four, and windows of one and three that neither setting takes
START_END_TASKS = {
    "100": {"150": [A, B], "170": [A, B, C, D], "130": [A]},
    "200": {"240": [B, C], "290": [B, C, D, E], "260": [B, C, D]},
    "300": {"330": [C, A], "395": [C, A, B, E]},
    "400": {"425": [D, A], "470": [D, A, C, B], "410": [D]},
    "500": {"560": [E, B]},
}
NUM_ROLLOUTS = 7  # not divisible by 2 or 3; more than either task list holds: the modulo wraps


def scripted_info(start_step, end_step, tasks, i):
    """A rollout_info that depends on the window, its tasks and the episode's position in its rank's list alone."""
    h = zlib.crc32(repr((int(start_step), int(end_step), list(tasks), int(i))).encode())
    n = h % (len(tasks) + 1)
    return {"episode_length": 5 + (h >> 4) % 40, "episode_return": -((h >> 9) % 1000) / 8.0, "success": n == len(tasks),
            "successful_tasks": list(tasks[:n])}


def key_of(reset_info):
    """(start step, end step, tasks) of a reset_info built from tests/rollout_envs.py state_of_step."""
    ti = reset_info["task_info"]
    return int(ti["start_info"]["robot_obs"][2]), int(ti["goal_info"]["robot_obs"][2]), list(ti["tasks"])


# ------------------------------------------------------------------------------------------ environments
class ScriptedVectorEnv:
    """obs' = A obs + B a on float64 vectors; every instance has the same A, B and goal.  reset(length=, seed=, tasks=) or
    reset(task_info={"start_info", "goal_info", "tasks"}) (length and seed read off the two steps) sets the episode.  Task j of
    n is checked once, at step ceil((j + 1) length / n): it succeeds if every task before it did and obs[j] > -0.5; the
    episode is done at `length`."""

    def __init__(self, state_dim=29, action_dim=8, max_episode_steps=40):
        g = np.random.RandomState(77)
        self.A = np.eye(state_dim) * 0.9 + g.randn(state_dim, state_dim) * 0.02
        self.B = g.randn(state_dim, action_dim) * 0.1
        self.target_goal = g.randn(2)
        self.state_dim, self._max_episode_steps = state_dim, int(max_episode_steps)
        self.length, self.tasks, self.t, self.obs, self.won = 1, [], 0, np.zeros(state_dim), []

    def reset(self, task_info=None, length=5, seed=0, tasks=()):
        if task_info is not None:
            s, e = int(task_info["start_info"]["robot_obs"][2]), int(task_info["goal_info"]["robot_obs"][2])
            length, seed, tasks = 3 + (e - s) % 11, s + 31 * e, task_info["tasks"]
        self.length, self.tasks, self.t, self.won = int(length), list(tasks), 0, []
        self.obs = np.random.RandomState(int(seed)).randn(self.state_dim)
        return self.obs.astype(np.float32)

    def step(self, action):
        self.obs = self.A @ self.obs + self.B @ np.asarray(action, dtype=np.float64)
        self.t += 1
        n = len(self.tasks)
        for j in range(n):
            if self.t == -(-(j + 1) * self.length // n) and len(self.won) == j and self.obs[j] > -0.5:
                self.won.append(self.tasks[j])
        done = self.t >= self.length
        reward = -float(np.abs(self.obs[:2] - self.target_goal).sum())
        return self.obs.astype(np.float32), reward, done, {"success": n > 0 and len(self.won) == n, "successful_tasks": list(self.won)}

    def get_normalized_score(self, episode_return):
        return (episode_return + 50.0) / 50.0


# ------------------------------------------------------------------------------------------ schedules
def greedy_makespan(lengths, R):
    """Policy calls of the refill runner: episodes in order, each into the slot that frees first."""
    free = [0] * R
    for n in lengths:
        r = free.index(min(free))
        free[r] += n
    return max(free)


def batch_makespan(lengths, R):
    """Policy calls of fixed batches of R: the sum of the batches' maxima."""
    return sum(max(lengths[i: i + R]) for i in range(0, len(lengths), R))
