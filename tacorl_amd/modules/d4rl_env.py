"""What the D4RL modules read from `gym.make(d4rl_env)` (reference cql_offline_lightning_d4rl.py:57,133-137,
play_lmp_d4rl.py:44,56-60): the observation width, the action width and the action bounds.  Neither `gym` nor `d4rl` is
imported: the AntMaze tasks share one robot, so the three numbers are a table of the task names."""
GOAL_DIM = 2  # the (x, y) target, hard-coded by the reference (cql_offline_lightning_d4rl.py:135, play_lmp_d4rl.py:56)

# name -> (state_dim, action_dim, action bound): the Ant's 29-d observation, 8 joint torques in [-1, 1]
ANTMAZE = {f"antmaze-{maze}-v{v}": (29, 8, 1.0)
           for maze in ("umaze", "umaze-diverse", "medium-play", "medium-diverse", "large-play", "large-diverse")
           for v in (0, 1, 2)}


def env_dims(d4rl_env, state_dim=None, action_dim=None):
    """(state_dim, action_dim, bound) of the environment; explicit state_dim / action_dim override the table, and an
    environment the table does not know needs both."""
    known = ANTMAZE.get(d4rl_env)
    if known is None and (state_dim is None or action_dim is None):
        raise ValueError(f"d4rl_env {d4rl_env!r} is not one of the AntMaze tasks ({', '.join(sorted(ANTMAZE)[:3])}, ...): "
                         "pass state_dim and action_dim")
    s, a, bound = known if known is not None else (None, None, 1.0)
    return int(state_dim if state_dim is not None else s), int(action_dim if action_dim is not None else a), float(bound)
