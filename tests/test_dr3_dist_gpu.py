"""The DR3 term on the N-rank path, on a single-GPU box as tests/test_dist_gpu.py runs it: two processes share cuda:0 and
reduce through gloo."""
import os
import sys

import pytest

from tests.proc_util import free_port, run_group

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_rank_halves_equal_the_full_batch_step_with_dr3():
    """CQL_Offline with with_dr3=True: two ranks on per-sample halves (B = 4) with sharded noise, hipGraph segments around the
    all-reduces, against the single-rank full-batch step (tests/dr3_shard_script.py)."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "tests", "dr3_shard_script.py")]
    out = run_group(cmd, env, ROOT, timeout=600)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
