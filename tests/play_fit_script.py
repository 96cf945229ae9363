"""GPU half of tests/test_play_replay_gpu.py::test_trainer_fit_over_the_datamodule, run in a fresh interpreter with
tests/fake_pl on PYTHONPATH.  usage: play_fit_script.py <fused|dense>.  pytorch_lightning's Trainer.fit (the strict stand-in)
drives TACORL (decoder fine-tuned) and PlayLMP for a few steps out of a PlayDataModule - an .npz dataset with a neighbour
table, the reference's dataset configs, a train transform list, a validation loader - and the samplers' status words stay 0."""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
fused = {"fused": True, "dense": False}[sys.argv[1]]

import pytorch_lightning as pl  # noqa: E402

from tacorl_amd import lightning as L  # noqa: E402
from tacorl_amd.data.play_replay import PlayDataModule, PlayWindowLoader  # noqa: E402
from tests import cfg_util as C  # noqa: E402

assert L.LightningModuleBase is pl.LightningModule
DEV, N, HW = "cuda:0", 400, 84
g = torch.Generator().manual_seed(3)
frames = torch.randint(0, 256, (N, HW, HW, 3), dtype=torch.uint8, generator=g).numpy()
acts = np.random.RandomState(4).uniform(-1, 1, size=(N, 7)).astype(np.float32)
acts[:, -1] = np.where(acts[:, -1] >= 0, 1.0, -1.0)
rs = np.random.RandomState(5)
nn = {int(k): rs.randint(0, 300, size=rs.randint(0, 4)).tolist() for k in range(0, 300, 2)}
TM = {"transforms": {"train": {"rgb_static": [{"_target_": "tacorl.utils.transforms.RandomShiftsAug", "pad": 4},
                                              {"_target_": "tacorl.utils.transforms.ScaleImageTensor"},
                                              {"_target_": "torchvision.transforms.Normalize", "mean": [0.5], "std": [0.5]}]},
                     "validation": {"rgb_static": [{"_target_": "tacorl.utils.transforms.ScaleImageTensor"}]}}}
DS = {"_target_": "tacorl.datamodule.dataset.play_dataset.PlayDataset", "_recursive_": False, "modalities": ["rgb_static", "rel_actions_world"],
      "min_window_size": 8, "max_window_size": 16, "pad": True}
DS_GOAL = dict(DS, include_goal=True, goal_sampling_prob=0.3, goal_strategy_prob={"geometric": 0.9, "similar_robot_obs": 0.1})
strip = lambda c: {k: v for k, v in c.items() if k not in ("_target_", "_recursive_")}  # noqa: E731


def build(kind):
    from tacorl_amd.modules.play_lmp.play_lmp_for_rl import PlayLMP
    from tacorl_amd.modules.tacorl.tacorl import TACORL

    torch.manual_seed(5)
    lmp = PlayLMP(**strip(C.playlmp_cfg(device=DEV)))
    return lmp if kind == "playlmp" else TACORL(play_lmp=lmp, **strip(C.tacorl_cfg(device=DEV)))


with tempfile.TemporaryDirectory() as d:
    path = os.path.join(d, "play.npz")
    np.savez(path, **{"frames/rgb_static": frames, "actions": acts, "ep_start_end_ids_train": [[0, 149], [150, 299]],
                      "ep_start_end_ids_val": [[300, 399]]})
    for kind, ds in (("tacorl", DS_GOAL), ("playlmp", DS)):
        dm = PlayDataModule(dict(ds, path=path), batch_size=3, train_percentage=1.0, val_percentage=0.5, transform_manager=TM,
                            nn_steps_from_step=nn if kind == "tacorl" else None, steps_per_epoch=2, val_steps=1, num_workers=4,
                            shuffle_val=False, device=DEV, fused=fused, generator=torch.Generator(device=DEV).manual_seed(41),
                            _target_="tacorl.datamodule.basic_data_module.BasicDataModule")
        mod = build(kind)
        p0 = {k: v.detach().clone() for k, v in mod.state_dict().items() if v.dtype == torch.float32}
        per = len(L._as_list(mod.configure_optimizers()))  # PL >= 1.6 counts optimizer steps
        tr = pl.Trainer(max_epochs=2, log_every_n_steps=1, gpus=1)
        tr.fit(mod, datamodule=dm)
        torch.cuda.synchronize()
        tl, vl = dm.train_dataloader(), dm.val_dataloader()
        assert isinstance(tl, PlayWindowLoader) and len(tl) == 2 and len(vl) == 1 and tl.fused is fused and vl.fused is fused
        assert (tl.aug_specs is not None) and vl.aug_specs is None
        b = next(iter(tl))
        assert ("replay" in b) == fused and ("states" in b) != fused and "aug" in b and ("disp" in b) == (kind == "tacorl")
        assert "aug" not in next(iter(vl))
        assert tr.global_step == 4 * per and tr.current_epoch == 2, (tr.global_step, per)
        lm = tr.logged_metrics
        want = "train/total_loss" if kind == "playlmp" else "train/q1_loss"
        assert want in lm and np.isfinite(lm[want]), lm
        val = {k: v for k, v in lm.items() if k.startswith("val")}
        assert val and all(np.isfinite(v) for v in val.values()), lm
        sd = mod.state_dict()
        assert all(torch.isfinite(v).all() for v in sd.values() if v.dtype.is_floating_point)
        assert any(not torch.equal(p0[k].cpu(), sd[k].cpu()) for k in p0), f"{kind}: no parameter moved"
        dm.train_replay.check()
        dm.val_replay.check()
        print(f"{kind}: ok  {want}={lm[want]:.5g}")
print("ALL OK")
