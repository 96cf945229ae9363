"""Deterministic toy environments with the gym API for the rollout tests: `reset(**reset_info)`, `step(action)` ->
(observation, reward, done, info), `_max_episode_steps`.  Everything is integer or float64 host arithmetic, so an episode is a
function of the bits of the actions it is stepped with.

GridImageEnv: a point on a 32 x 32 integer grid.  Its cameras render uint8 frames at a source resolution of their own as a
pure function of the integer state; an action moves the point by round(3 a[0]), round(3 a[1]); success is an L1 distance to
the goal of at most `threshold`.  `reset(task_info=...)` takes the callback's two forms: {"start_info", "goal_info", "tasks"}
(the point and the goal are read off the first two entries of robot_obs) and {"task", "index"}.

PointVectorEnv: a linear system on float64 vectors with `target_goal` and `get_normalized_score` (the D4RL surface)."""
import numpy as np

GRID = 32
TASKS = {"open_drawer": 2, "move_block_left": 3, "turn_on_light": 1}  # get_possible_tasks(): task -> number of goals


def render(state, cam_id, hw):
    """uint8 (H, W, 3): a pure function of the integer state."""
    H, W = hw
    x, y = int(state[0]), int(state[1])
    h = np.arange(H, dtype=np.int64)[:, None, None]
    w = np.arange(W, dtype=np.int64)[None, :, None]
    c = np.arange(3, dtype=np.int64)[None, None, :]
    v = (h * (3 + x) + w * (5 + y) + c * 37 + 11 * cam_id + ((h // 8 + x) * (w // 8 + y)) * 7) % 256
    return v.astype(np.uint8)


class GridImageEnv:
    def __init__(self, seed=0, cams=("rgb_static",), src_hw=(100, 100), threshold=2, max_episode_steps=20):
        g = np.random.RandomState(seed)
        self.cams, self.src_hw = list(cams), {c: tuple(src_hw[c]) if isinstance(src_hw, dict) else tuple(src_hw) for c in cams}
        self.start0, self.goal0 = g.randint(0, GRID, 2), g.randint(0, GRID, 2)
        self.threshold, self._max_episode_steps = int(threshold), int(max_episode_steps)
        self.state, self.goal, self.tasks = self.start0.copy(), self.goal0.copy(), []

    def get_possible_tasks(self):
        return dict(TASKS)

    def _obs(self):
        return {"observation": {c: render(self.state, i, self.src_hw[c]) for i, c in enumerate(self.cams)},
                "goal": {c: render(self.goal, i, self.src_hw[c]) for i, c in enumerate(self.cams)}}

    def reset(self, task_info=None):
        self.state, self.goal, self.tasks = self.start0.copy(), self.goal0.copy(), []
        if task_info is not None and "start_info" in task_info:
            self.state = np.asarray(task_info["start_info"]["robot_obs"][:2]).astype(np.int64) % GRID
            self.goal = np.asarray(task_info["goal_info"]["robot_obs"][:2]).astype(np.int64) % GRID
            self.tasks = list(task_info["tasks"])
        elif task_info is not None:
            k = sorted(TASKS).index(task_info["task"])
            self.state = np.array([(5 * k + 3) % GRID, (7 * task_info["index"] + 1) % GRID], dtype=np.int64)
            self.goal = np.array([(self.state[0] + 4) % GRID, (self.state[1] + 3 * k) % GRID], dtype=np.int64)
            self.tasks = [task_info["task"]]
        return self._obs()

    def step(self, action):
        a = np.asarray(action, dtype=np.float64)
        self.state = np.clip(self.state + np.rint(3 * a[:2]).astype(np.int64), 0, GRID - 1)
        dist = int(np.abs(self.state - self.goal).sum())
        success = dist <= self.threshold
        info = {"success": bool(success), "successful_tasks": list(self.tasks) if success else []}
        return self._obs(), -float(dist), bool(success), info


class PointVectorEnv:
    def __init__(self, seed=0, length=9, state_dim=29, action_dim=8, max_episode_steps=20):
        g = np.random.RandomState(seed)
        self.A = np.eye(state_dim) * 0.9 + g.randn(state_dim, state_dim) * 0.02
        self.B = g.randn(state_dim, action_dim) * 0.1
        self.obs0, self.target_goal = g.randn(state_dim), g.randn(2)
        self.length, self._max_episode_steps = int(length), int(max_episode_steps)
        self.t, self.obs = 0, None

    def reset(self):
        self.t, self.obs = 0, self.obs0.copy()
        return self.obs.astype(np.float32)

    def step(self, action):
        self.obs = self.A @ self.obs + self.B @ np.asarray(action, dtype=np.float64)
        self.t += 1
        reward = -float(np.abs(self.obs[:2] - self.target_goal).sum())
        done = self.t >= self.length
        return self.obs.astype(np.float32), reward, done, {"success": bool(done and reward > -2.0)}

    def get_normalized_score(self, episode_return):
        return (episode_return + 50.0) / 50.0


# ------------------------------------------------------------------------------------------ the callback fixture's script
# tools/gen_rollout_callback_golden.py drives the reference callback with a stub manager that answers every episode with
# scripted_info(key); tests/test_callbacks_rollout_cpu.py hands the same answers to this project's callback.
START_END_TASKS = {
    "100": {"120": ["open_drawer"], "140": ["open_drawer"], "190": ["open_drawer"], "110": ["open_drawer"]},
    "200": {"230": ["move_block_left"], "221": ["move_block_left", "open_drawer"], "263": ["move_block_left"]},
    "300": {"317": ["turn_on_light"], "318": ["turn_on_light"], "340": ["lift_block"], "364": ["lift_block"]},
    "400": {"417": ["close_drawer"], "450": ["lift_block"], "420": ["open_drawer"]},
}
MIN_SEQ_LEN, MAX_SEQ_LEN = 16, 64


def scripted_info(*key):
    """A rollout_info that depends on the key alone."""
    import zlib

    h = zlib.crc32(repr(key).encode())
    return {"episode_length": 5 + h % 17, "episode_return": -((h >> 5) % 1000) / 8.0, "success": bool((h >> 3) & 1)}


def state_of_step(step):
    """The robot_obs / scene_obs stored in the fixture directory's frame file of `step`."""
    s = int(step)
    return {"robot_obs": np.array([s % GRID, (7 * s) % GRID, s], dtype=np.float64),
            "scene_obs": np.array([s, 2 * s], dtype=np.float64)}


def write_state_dir(root, start_end_tasks=START_END_TASKS):
    """A frame directory in the reference's naming that holds the steps the task list names."""
    import os

    steps = {int(s) for s in start_end_tasks} | {int(e) for v in start_end_tasks.values() for e in v}
    for s in sorted(steps):
        np.savez(os.path.join(root, f"episode_{s:07d}.npz"), **state_of_step(s))
    return root
