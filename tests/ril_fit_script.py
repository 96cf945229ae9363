"""GPU half of tests/test_ril_gpu.py::test_trainer_fit_smoke, run in a fresh interpreter: MiniTrainer.fit drives two
batches of RelayImitationLearning (built through `instantiate`, as scripts/train.py builds its module) from host batches,
validates once, and a checkpoint written by the trainer loads into a fresh module (parameters, Adam state, step count)."""
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tacorl_amd import lightning as L  # noqa: E402
from tests import ril_util as U  # noqa: E402

CAMS = {"rgb_static": (84, 84)}
cfg = dict(U.ril_cfg(), _target_=U.TARGET, _recursive_=False, device="cuda:0")
torch.manual_seed(5)
mod = L.instantiate(cfg)
data = [U.make_ril_batch(70 + i, 3, CAMS) for i in range(2)]
p0 = mod.engine.blk.param.clone()
tr = L.MiniTrainer(max_epochs=1, max_steps=2, log_every_n_steps=1)
tr.fit(mod, train_dataloaders=data, val_dataloaders=data[:1])
torch.cuda.synchronize()
lm = tr.logged_metrics
for k in ("train/low_level_loss", "train/high_level_loss", "train/total_loss", "validation/total_loss"):
    assert k in lm and lm[k] == lm[k], lm
assert tr.global_step == 2 and int(mod.engine.blk.step) == 2 and not torch.equal(p0, mod.engine.blk.param)
assert all(torch.isfinite(v).all() for v in mod.state_dict().values())
with tempfile.TemporaryDirectory() as d:
    path = os.path.join(d, "last.ckpt")
    tr.save_checkpoint(path)
    torch.manual_seed(6)
    fresh = L.instantiate(cfg)
    t2 = L.MiniTrainer()
    t2._attach(fresh)
    t2.load_checkpoint(path)
a, b = mod.engine.blk, fresh.engine.blk
assert torch.equal(a.param, b.param) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v) and int(b.step) == 2
# the restored module takes the next step exactly as the original does
mod.training_step(L.move_to(data[0], mod.device), 0)
fresh.training_step(L.move_to(data[0], fresh.device), 0)
torch.cuda.synchronize()
assert torch.equal(a.param, b.param) and fresh.logged and all(mod.logged[k] == v for k, v in fresh.logged.items())
print("ALL OK")
