"""Rank-count invariance of the device noise: two ranks that each fill their own shard from the shared seed equal the
single-rank full-batch step with that seed (tests/device_noise_shard_script.py)."""
import os
import sys

import pytest

from tests.proc_util import free_port, run_group

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seeded_shards_equal_the_seeded_full_batch_step():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "tests", "device_noise_shard_script.py")]
    out = run_group(cmd, env, ROOT, timeout=420)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
