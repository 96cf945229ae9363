"""The launch plan of the image-ingest stage - what stands between a batch and the encoders' image buffers - pinned on the
device: for every batch form TACORL, PlayLMP, CQL_Offline and RelayImitationLearning take, which `tacorl_pack_images*`
entry points (and TACORL's `tacorl_stage_transition`) run, in which order, over which jobs, and on which stream.

`call` is replaced on every loaded tacorl_amd module that has the name (`_lib` included: PlayLMP imports it inside its
functions) by a recorder that FORWARDS to the real entry point, so the device work runs as always, on the stream the code
chose.  A record is (entry point, arguments, issued on the default stream?): every argument but the stream, arrays as
tuples, every pointer as (name of the tensor it points into, byte offset) against the batch's tensors, module.frames[c],
engine.X3[c] and the small transition buffers; "temp" is a pointer into a tensor the staging made itself (the obs / next
rows of an augmentation table).

The expectations in PLAN were written down from a run of the commit BEFORE the five hand-kept copies of this stage were
folded into tacorl_amd/image_ingest.py; they are literals, never derived from the code under test.  tools/image_ingest_plan.py
prints them (and the image buffers' hashes) for a tree.

Shapes: B = 2, T = 3, a dataset of 16 frames, geometry GEO x GEO = the smallest square the conv stack takes whose uint8
frame is a multiple of 16 bytes (chosen on the host with ops.encoder_act_layout), GEO + 1 for the size no vector route takes
(H*W % 4 != 0, H*W*3 % 16 != 0), GEO + 4 as the source size of the resizing augmentation."""
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S, G2 = "rgb_static", "rgb_gripper"
B, T, N = 2, 3, 16


def geometry():
    from tacorl_amd import _lib, ops

    for h in range(1, 512):
        if (h * h * 3) % 16 == 0:
            try:
                ops.encoder_act_layout(1, h, h)
                return h
            except _lib.TacorlHipError:
                pass
    raise AssertionError("no geometry")


class Recorder:
    def __init__(self, monkeypatch):
        import tacorl_amd.modules.cql.cql_offline_lightning  # noqa: F401
        import tacorl_amd.modules.play_lmp.play_lmp_for_rl  # noqa: F401
        import tacorl_amd.modules.relay_imitation_learning.relay_imitation_learning  # noqa: F401
        import tacorl_amd.modules.tacorl.tacorl  # noqa: F401
        from tacorl_amd import _lib

        self.real, self.sigs, self.raw, self.bases = _lib.call, _lib._SIGS, [], {}
        for name, mod in list(sys.modules.items()):
            if name.startswith("tacorl_amd") and mod is not None and hasattr(mod, "call"):
                monkeypatch.setattr(mod, "call", self.call)

    def call(self, name, *a):
        if name.startswith("tacorl_pack_images") or name == "tacorl_stage_transition":
            dev = torch.device(DEV)
            self.raw.append((name, self._plain(name, a), torch.cuda.current_stream(dev) == torch.cuda.default_stream(dev)))
        return self.real(name, *a)

    def _plain(self, name, a):
        """Arguments as python values, read while the ctypes arrays are alive; a pointer becomes a _Ptr."""
        import ctypes as C

        out = []
        for x, ty in list(zip(a, self.sigs[name][1]))[:-1]:  # (the last argument is the stream)
            if isinstance(x, C.Array):
                out.append(tuple(_Ptr(v) if x._type_ is C.c_void_p else int(v) for v in x))
            else:
                out.append(_Ptr(getattr(x, "value", x)) if ty is C.c_void_p else int(x))
        return tuple(out)

    def name(self, prefix, t):
        if torch.is_tensor(t):
            self.bases[prefix] = (t.data_ptr(), t.data_ptr() + t.numel() * t.element_size())
        elif isinstance(t, dict):
            for k, v in t.items():
                self.name(f"{prefix}.{k}" if prefix else str(k), v)

    def _resolve(self, v):
        if isinstance(v, tuple):
            return tuple(self._resolve(x) for x in v)
        if not isinstance(v, _Ptr):
            return v
        if not v.addr:
            return None
        for name, (lo, hi) in self.bases.items():
            if lo <= v.addr < hi:
                return (name, v.addr - lo)
        return "temp"

    def take(self):
        out = [(n[len("tacorl_"):], self._resolve(a), main) for n, a, main in self.raw]
        self.raw = []
        return out


class _Ptr:
    def __init__(self, addr):
        self.addr = addr


@pytest.fixture
def rec(monkeypatch):
    return Recorder(monkeypatch)


# ------------------------------------------------------------------------------------------------------------- modules
def _strip(c):
    return {k: v for k, v in c.items() if k not in ("_target_", "_recursive_")}


def _lmp(cams, window_cams=None):
    from tacorl_amd.modules.play_lmp.play_lmp_for_rl import PlayLMP
    from tests import cfg_util as C

    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    cfg = C.playlmp_cfg(cams, T=T, device=DEV)
    if window_cams is not None:
        cfg.update(plan_recognition_modalities=list(window_cams), action_decoder_modalities=list(window_cams))
    return PlayLMP(**_strip(cfg))


def _tacorl(cams=(S,), window_cams=None):
    from tacorl_amd.modules.tacorl.tacorl import TACORL
    from tests import cfg_util as C

    lmp = _lmp(cams, window_cams)
    m = TACORL(play_lmp=lmp, **_strip(C.tacorl_cfg(cams, device=DEV)))
    m.current_epoch = 5
    return m


def _cql(obs=(S,), goal=(S,)):
    from tests import goalcams_util as GC

    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    m = GC.build(list(obs), list(goal))
    m.current_epoch = 5
    return m


def _ril():
    from tacorl_amd.modules.relay_imitation_learning.relay_imitation_learning import RelayImitationLearning
    from tests import ril_util as U

    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    return RelayImitationLearning(device=DEV, **U.ril_cfg())


# ------------------------------------------------------------------------------------------------------------- batches
def _frames(hw, cams, seed=3):
    g = torch.Generator().manual_seed(seed)
    return {c: torch.randint(0, 256, (N, hw, hw, 3), dtype=torch.uint8, generator=g).to(DEV) for c in cams}


def _actions():
    acts = np.random.RandomState(4).uniform(-1, 1, size=(N, 7)).astype(np.float32)
    acts[:, -1] = np.where(acts[:, -1] >= 0, 1.0, -1.0)
    return acts


def _f32_play(hw, cams, nchw=True):
    g = torch.Generator(device=DEV).manual_seed(5)
    u = lambda *s: torch.rand(*s, device=DEV, generator=g) * 2 - 1  # noqa: E731
    img = (3, hw, hw) if nchw else (hw, hw, 3)
    acts = u(B, T, 7)
    acts[..., -1] = torch.where(acts[..., -1] >= 0, 1.0, -1.0)
    return {"states": {c: u(B, T, *img) for c in cams}, "goal": {c: u(B, *img) for c in cams}, "actions": acts,
            "disp": torch.tensor([1, 3], device=DEV)}


def _u8_play(hw, cams, fused, aug=False, resize=None):
    """The replay feeder's batch over a dataset of N frames: gathered (B,T,H,W,3) frames, or the dataset and an id table."""
    from tacorl_amd.data.augment import AugmentSpec, draw_play_batch_augmentation
    from tacorl_amd.data.replay import HbmReplay, PlayIndex

    ix = PlayIndex([[0, N - 1]], T, T, goal_sampling_prob=0.3)
    rng = np.random.default_rng(1)
    idx, draws = rng.integers(len(ix), size=B), ix.draw(B, rng)
    hbm = HbmReplay(_frames(hw, cams), _actions(), ix, device=DEV)
    a = None
    if aug:
        g = torch.Generator(device=DEV).manual_seed(12)
        a = draw_play_batch_augmentation({c: AugmentSpec(pad=2, resize=(resize, resize) if resize else None) for c in cams},
                                         B, T, DEV, g)
    b = hbm.batch(idx, draws, aug=a, fused=fused)
    b["_keep"] = hbm  # (the batch's small tensors live in the feeder's staging ring)
    return b


def _f32_transition(hw, obs, goal):
    g = torch.Generator(device=DEV).manual_seed(6)
    u = lambda *s: torch.rand(*s, device=DEV, generator=g) * 2 - 1  # noqa: E731
    gl = {c: u(B, 3, hw, hw) for c in goal}
    acts = u(B, 7)
    acts[:, -1] = torch.where(acts[:, -1] >= 0, 1.0, -1.0)
    return {"observations": {"observation": {c: u(B, 3, hw, hw) for c in obs}, "goal": gl},
            "next_observations": {"observation": {c: u(B, 3, hw, hw) for c in obs}, "goal": gl},
            "actions": acts, "rewards": torch.tensor([1.0, 0.0], device=DEV), "terminals": torch.tensor([1, 0], device=DEV)}


def _u8_transition(hw, cams, fused, aug=False, resize=None):
    from tacorl_amd.data.augment import AugmentSpec, draw_transition_batch_augmentation
    from tacorl_amd.data.replay import HbmTransitionReplay, TransitionIndex

    ix = TransitionIndex([[0, N - 1]], n_frames=N, goal_strategy_prob={"geometric": 1.0})
    rp = HbmTransitionReplay(_frames(hw, cams), _actions(), ix, device=DEV, batch_size=B)
    a = None
    if aug:
        g = torch.Generator(device=DEV).manual_seed(14)
        a = draw_transition_batch_augmentation({c: AugmentSpec(pad=2, resize=(resize, resize) if resize else None) for c in cams},
                                               B, DEV, g)
    b = rp.batch(ix.draw(B, np.random.default_rng(13)), aug=a, fused=fused)
    b["_keep"] = rp
    return b


def _ril_batch(hw, u8):
    from tests import ril_util as U

    b = U.make_ril_batch(7, B, {S: (hw, hw)})
    if u8:
        b = U.to_uint8_hwc(b)[0]
    return {k: ({c: t.to(DEV) for c, t in v.items()} if isinstance(v, dict) else v.to(DEV)) for k, v in b.items()}


# --------------------------------------------------------------------------------------------------------------- cases
def _names(rec, mod, batch):
    rec.bases = {}
    rec.name("", {k: v for k, v in batch.items() if k not in ("_keep", "ready", "idx", "window_size")})
    for k in ("frames", "acts", "_acts", "reward"):
        if getattr(mod, k, None) is not None:
            rec.name(k, getattr(mod, k))
    e = getattr(mod, "engine", None)
    if e is not None:
        rec.name("X3", getattr(e, "X3", None))  # (absent where the staging raised before the first allocation)
        rec.name("done", getattr(e, "done", None))


def buffers(mod):
    """Every image buffer the staging filled: module.frames[c] and engine.X3[c]."""
    out = {f"frames.{c}": t for c, t in (getattr(mod, "frames", None) or {}).items()}
    e = getattr(mod, "engine", None)
    out.update({f"X3.{c}": t for c, t in (e.X3.items() if e is not None else ())})
    return out


def _run(rec, mod, batch, step):
    torch.manual_seed(7)
    torch.cuda.manual_seed(7)
    step(mod, batch)
    torch.cuda.synchronize()
    _names(rec, mod, batch)
    return rec.take()


def _train(mod, batch):
    mod.training_step(batch, 0)


def _tacorl_nhwc(mod, batch):
    mod._step(batch, None, True, "train", nchw=False)


def _playlmp_nhwc(mod, batch):
    mod._step(batch, nchw=False)


def play_forms(geo):
    """The eight forms of a play-window batch: name -> (batch builder over cameras, step)."""
    return {
        "f32_nchw": (lambda cams: _f32_play(geo, cams), None),
        "f32_nhwc": (lambda cams: _f32_play(geo, cams, nchw=False), "nhwc"),
        "f32_nchw_odd": (lambda cams: _f32_play(geo + 1, cams), None),
        "u8": (lambda cams: _u8_play(geo, cams, fused=False), None),
        "u8_aug": (lambda cams: _u8_play(geo, cams, fused=False, aug=True), None),
        "u8_aug_resize": (lambda cams: _u8_play(geo + 4, cams, fused=False, aug=True, resize=geo), None),
        "replay": (lambda cams: _u8_play(geo, cams, fused=True), None),
        "replay_aug": (lambda cams: _u8_play(geo, cams, fused=True, aug=True), None),
    }


def transition_forms(geo):
    return {
        "f32_nchw": lambda cams: _f32_transition(geo, cams, cams),
        "u8": lambda cams: _u8_transition(geo, cams, fused=False),
        "u8_aug": lambda cams: _u8_transition(geo, cams, fused=False, aug=True),
        "replay": lambda cams: _u8_transition(geo, cams, fused=True),
        "replay_aug": lambda cams: _u8_transition(geo, cams, fused=True, aug=True),
        "replay_aug_resize": lambda cams: _u8_transition(geo + 4, cams, fused=True, aug=True, resize=geo),
    }


def cases(geo):
    """name -> () -> (module, batch, step): every case of the plan."""
    out = {}
    for form, (make, how) in play_forms(geo).items():
        out[f"tacorl/{form}"] = lambda make=make, how=how: (_tacorl(), make([S]), _tacorl_nhwc if how else _train)
        out[f"playlmp/{form}"] = lambda make=make, how=how: (_lmp([S]), make([S]), _playlmp_nhwc if how else _train)
    for form in ("f32_nchw", "u8", "u8_aug", "replay", "replay_aug"):  # rgb_gripper: an engine camera outside the window
        make = play_forms(geo)[form][0]
        out[f"tacorl_engine_only_cam/{form}"] = lambda make=make: (_tacorl((S, G2), window_cams=(S,)), make([S, G2]), _train)
    for form, make in transition_forms(geo).items():
        out[f"cql/{form}"] = lambda make=make: (_cql(), make([S]), _train)
    out["cql_goalcams/f32_nchw"] = lambda: (_cql((S,), (G2,)), _f32_transition(geo, [S], [G2]), _train)
    out["cql_goalcams/replay"] = lambda: (_cql((S,), (G2,)), _u8_transition(geo, [S, G2], fused=True), _train)
    out["ril/f32_nchw"] = lambda: (_ril(), _ril_batch(geo, False), _train)
    out["ril/u8"] = lambda: (_ril(), _ril_batch(geo, True), _train)
    return out


def run_case(rec, name, geo):
    mod, batch, step = cases(geo)[name]()
    return mod, _run(rec, mod, batch, step)


PLAN = {'cql/f32_nchw': [('pack_images_batch',
                   (3,
                    (('observations.observation.rgb_static', 0), ('observations.goal.rgb_static', 0),
                     ('next_observations.observation.rgb_static', 0)),
                    (3888, 3888, 3888), (('X3.rgb_static', 0), ('X3.rgb_static', 31104), ('X3.rgb_static', 62208)),
                    (2, 2, 2), 0, 36, 36),
                   True)],
 'cql/replay': [('pack_images_u8_gather_batch',
                 (3, (('replay.frames.rgb_static', 0), ('replay.frames.rgb_static', 0), ('replay.frames.rgb_static', 0)),
                  (3888, 3888, 3888), (('replay.ids', 0), ('replay.ids', 32), ('replay.ids', 16)), (1, 1, 1),
                  (('X3.rgb_static', 0), ('X3.rgb_static', 31104), ('X3.rgb_static', 62208)), (2, 2, 2), 0, 36, 36),
                 True)],
 'cql/replay_aug': [('pack_images_u8_resize_aug_gather_batch',
                     (3,
                      (('replay.frames.rgb_static', 0), ('replay.frames.rgb_static', 0), ('replay.frames.rgb_static', 0)),
                      (3888, 3888, 3888), (('replay.ids', 0), ('replay.ids', 32), ('replay.ids', 16)), (1, 1, 1),
                      (('X3.rgb_static', 0), ('X3.rgb_static', 31104), ('X3.rgb_static', 62208)),
                      (('aug.obs.rgb_static.shift', 0), ('aug.goal.rgb_static.shift', 0), ('aug.next.rgb_static.shift', 0)),
                      (('aug.obs.rgb_static.jitter', 0), ('aug.goal.rgb_static.jitter', 0),
                       ('aug.next.rgb_static.jitter', 0)),
                      (2, 2, 2), 0, 36, 36, 36, 36, 2),
                     True)],
 'cql/replay_aug_resize': [('pack_images_u8_resize_aug_gather_batch',
                            (3,
                             (('replay.frames.rgb_static', 0), ('replay.frames.rgb_static', 0),
                              ('replay.frames.rgb_static', 0)),
                             (4800, 4800, 4800), (('replay.ids', 0), ('replay.ids', 32), ('replay.ids', 16)), (1, 1, 1),
                             (('X3.rgb_static', 0), ('X3.rgb_static', 31104), ('X3.rgb_static', 62208)),
                             (('aug.obs.rgb_static.shift', 0), ('aug.goal.rgb_static.shift', 0),
                              ('aug.next.rgb_static.shift', 0)),
                             (('aug.obs.rgb_static.jitter', 0), ('aug.goal.rgb_static.jitter', 0),
                              ('aug.next.rgb_static.jitter', 0)),
                             (2, 2, 2), 0, 40, 40, 36, 36, 2),
                            True)],
 'cql/u8': [('pack_images_u8_batch',
             (3,
              (('observations.observation.rgb_static', 0), ('observations.goal.rgb_static', 0),
               ('next_observations.observation.rgb_static', 0)),
              (3888, 3888, 3888), (('X3.rgb_static', 0), ('X3.rgb_static', 31104), ('X3.rgb_static', 62208)), (2, 2, 2), 0,
              36, 36),
             True)],
 'cql/u8_aug': [('pack_images_u8_resize_aug_gather_batch',
                 (3,
                  (('observations.observation.rgb_static', 0), ('observations.goal.rgb_static', 0),
                   ('next_observations.observation.rgb_static', 0)),
                  (3888, 3888, 3888), (None, None, None), (1, 1, 1),
                  (('X3.rgb_static', 0), ('X3.rgb_static', 31104), ('X3.rgb_static', 62208)),
                  (('aug.obs.rgb_static.shift', 0), ('aug.goal.rgb_static.shift', 0), ('aug.next.rgb_static.shift', 0)),
                  (('aug.obs.rgb_static.jitter', 0), ('aug.goal.rgb_static.jitter', 0), ('aug.next.rgb_static.jitter', 0)),
                  (2, 2, 2), 0, 36, 36, 36, 36, 2),
                 True)],
 'cql_goalcams/f32_nchw': [('pack_images_batch',
                            (2,
                             (('observations.observation.rgb_static', 0), ('next_observations.observation.rgb_static', 0)),
                             (3888, 3888), (('X3.rgb_static', 0), ('X3.rgb_static', 31104)), (2, 2), 0, 36, 36),
                            True),
                           ('pack_images_batch',
                            (1, (('observations.goal.rgb_gripper', 0),), (3888,), (('X3.rgb_gripper', 0),), (2,), 0, 36,
                             36),
                            True)],
 'cql_goalcams/replay': [('pack_images_u8_gather_batch',
                          (2, (('replay.frames.rgb_static', 0), ('replay.frames.rgb_static', 0)), (3888, 3888),
                           (('replay.ids', 0), ('replay.ids', 16)), (1, 1),
                           (('X3.rgb_static', 0), ('X3.rgb_static', 31104)), (2, 2), 0, 36, 36),
                          True),
                         ('pack_images_u8_gather_batch',
                          (1, (('replay.frames.rgb_gripper', 0),), (3888,), (('replay.ids', 32),), (1,),
                           (('X3.rgb_gripper', 0),), (2,), 0, 36, 36),
                          True)],
 'playlmp/f32_nchw': [('pack_images_batch',
                       (1, (('states.rgb_static', 0),), (3888,), (('frames.rgb_static', 0),), (6,), 0, 36, 36), True)],
 'playlmp/f32_nchw_odd': [('pack_images', (('states.rgb_static', 0), 4107, 1, ('frames.rgb_static', 0), 0, 6, 3, 37, 37),
                           True)],
 'playlmp/f32_nhwc': [('pack_images', (('states.rgb_static', 0), 3888, 0, ('frames.rgb_static', 0), 0, 6, 3, 36, 36),
                       True)],
 'playlmp/replay': [('pack_images_u8_gather_batch',
                     (1, (('replay.frames.rgb_static', 0),), (3888,), (('replay.ids', 0),), (1,),
                      (('frames.rgb_static', 0),), (6,), 0, 36, 36),
                     True)],
 'playlmp/replay_aug': [('pack_images_u8_resize_aug_gather_batch',
                         (1, (('replay.frames.rgb_static', 0),), (3888,), (('replay.ids', 0),), (1,),
                          (('frames.rgb_static', 0),), (('aug.states.rgb_static.shift', 0),),
                          (('aug.states.rgb_static.jitter', 0),), (6,), 0, 36, 36, 36, 36, 2),
                         True)],
 'playlmp/u8': [('pack_images_u8_batch',
                 (1, (('states.rgb_static', 0),), (3888,), (('frames.rgb_static', 0),), (6,), 0, 36, 36), True)],
 'playlmp/u8_aug': [('pack_images_u8_resize_aug_gather_batch',
                     (1, (('states.rgb_static', 0),), (3888,), (None,), (1,), (('frames.rgb_static', 0),),
                      (('aug.states.rgb_static.shift', 0),), (('aug.states.rgb_static.jitter', 0),), (6,), 0, 36, 36, 36,
                      36, 2),
                     True)],
 'playlmp/u8_aug_resize': [('pack_images_u8_resize_aug_gather_batch',
                            (1, (('states.rgb_static', 0),), (4800,), (None,), (1,), (('frames.rgb_static', 0),),
                             (('aug.states.rgb_static.shift', 0),), (('aug.states.rgb_static.jitter', 0),), (6,), 0, 40, 40,
                             36, 36, 2),
                            True)],
 'ril/f32_nchw': [('pack_images_batch',
                   (4,
                    (('obs.rgb_static', 0), ('low_level_goal.rgb_static', 0), ('high_level_goal.rgb_static', 0),
                     ('high_level_action.rgb_static', 0)),
                    (3888, 3888, 3888, 3888),
                    (('X3.rgb_static', 0), ('X3.rgb_static', 31104), ('X3.rgb_static', 62208), ('X3.rgb_static', 93312)),
                    (2, 2, 2, 2), 0, 36, 36),
                   True)],
 'ril/u8': [('pack_images_u8_batch',
             (4,
              (('obs.rgb_static', 0), ('low_level_goal.rgb_static', 0), ('high_level_goal.rgb_static', 0),
               ('high_level_action.rgb_static', 0)),
              (3888, 3888, 3888, 3888),
              (('X3.rgb_static', 0), ('X3.rgb_static', 31104), ('X3.rgb_static', 62208), ('X3.rgb_static', 93312)),
              (2, 2, 2, 2), 0, 36, 36),
             True)],
 'tacorl/f32_nchw': [('stage_transition', (('disp', 0), 1, ('reward', 0), ('done', 0), 2, ('actions', 0), ('acts', 0), 42),
                      False),
                     ('pack_images_window_batch',
                      (2, (('states.rgb_static', 0), ('goal.rgb_static', 0)), (3888, 3888),
                       (('frames.rgb_static', 0), ('X3.rgb_static', 31104)), (6, 2), (('X3.rgb_static', 0), None),
                       (('X3.rgb_static', 62208), None), (3, 0), 0, 36, 36),
                      True)],
 'tacorl/f32_nchw_odd': [('stage_transition',
                          (('disp', 0), 1, ('reward', 0), ('done', 0), 2, ('actions', 0), ('acts', 0), 42), False),
                         ('pack_images', (('states.rgb_static', 0), 4107, 1, ('frames.rgb_static', 0), 0, 6, 3, 37, 37),
                          True),
                         ('pack_images', (('states.rgb_static', 0), 12321, 1, ('X3.rgb_static', 0), 0, 2, 3, 37, 37), True),
                         ('pack_images', (('goal.rgb_static', 0), 4107, 1, ('X3.rgb_static', 32856), 0, 2, 3, 37, 37),
                          True),
                         ('pack_images',
                          (('states.rgb_static', 32856), 12321, 1, ('X3.rgb_static', 65712), 0, 2, 3, 37, 37), True)],
 'tacorl/f32_nhwc': [('stage_transition', (('disp', 0), 1, ('reward', 0), ('done', 0), 2, ('actions', 0), ('acts', 0), 42),
                      False),
                     ('pack_images', (('states.rgb_static', 0), 3888, 0, ('frames.rgb_static', 0), 0, 6, 3, 36, 36), True),
                     ('pack_images', (('states.rgb_static', 0), 11664, 0, ('X3.rgb_static', 0), 0, 2, 3, 36, 36), True),
                     ('pack_images', (('goal.rgb_static', 0), 3888, 0, ('X3.rgb_static', 31104), 0, 2, 3, 36, 36), True),
                     ('pack_images', (('states.rgb_static', 31104), 11664, 0, ('X3.rgb_static', 62208), 0, 2, 3, 36, 36),
                      True)],
 'tacorl/replay': [('stage_transition', (('disp', 0), 1, ('reward', 0), ('done', 0), 2, ('actions', 0), ('acts', 0), 42),
                    False),
                   ('pack_images_u8_gather_batch',
                    (4,
                     (('replay.frames.rgb_static', 0), ('replay.frames.rgb_static', 0), ('replay.frames.rgb_static', 0),
                      ('replay.frames.rgb_static', 0)),
                     (3888, 3888, 3888, 3888),
                     (('replay.ids', 0), ('replay.ids', 0), ('replay.ids', 48), ('replay.ids', 16)), (1, 3, 1, 3),
                     (('frames.rgb_static', 0), ('X3.rgb_static', 0), ('X3.rgb_static', 31104), ('X3.rgb_static', 62208)),
                     (6, 2, 2, 2), 0, 36, 36),
                    True)],
 'tacorl/replay_aug': [('stage_transition',
                        (('disp', 0), 1, ('reward', 0), ('done', 0), 2, ('actions', 0), ('acts', 0), 42), False),
                       ('pack_images_u8_resize_aug_gather_batch',
                        (4,
                         (('replay.frames.rgb_static', 0), ('replay.frames.rgb_static', 0), ('replay.frames.rgb_static', 0),
                          ('replay.frames.rgb_static', 0)),
                         (3888, 3888, 3888, 3888),
                         (('replay.ids', 0), ('replay.ids', 0), ('replay.ids', 48), ('replay.ids', 16)), (1, 3, 1, 3),
                         (('frames.rgb_static', 0), ('X3.rgb_static', 0), ('X3.rgb_static', 31104),
                          ('X3.rgb_static', 62208)),
                         (('aug.states.rgb_static.shift', 0), 'temp', ('aug.goal.rgb_static.shift', 0), 'temp'),
                         (('aug.states.rgb_static.jitter', 0), 'temp', ('aug.goal.rgb_static.jitter', 0), 'temp'),
                         (6, 2, 2, 2), 0, 36, 36, 36, 36, 2),
                        True)],
 'tacorl/u8': [('stage_transition', (('disp', 0), 1, ('reward', 0), ('done', 0), 2, ('actions', 0), ('acts', 0), 42),
                False),
               ('pack_images_u8_batch',
                (4,
                 (('states.rgb_static', 0), ('states.rgb_static', 0), ('goal.rgb_static', 0), ('states.rgb_static', 7776)),
                 (3888, 11664, 3888, 11664),
                 (('frames.rgb_static', 0), ('X3.rgb_static', 0), ('X3.rgb_static', 31104), ('X3.rgb_static', 62208)),
                 (6, 2, 2, 2), 0, 36, 36),
                True)],
 'tacorl/u8_aug': [('stage_transition', (('disp', 0), 1, ('reward', 0), ('done', 0), 2, ('actions', 0), ('acts', 0), 42),
                    False),
                   ('pack_images_u8_resize_aug_gather_batch',
                    (4,
                     (('states.rgb_static', 0), ('states.rgb_static', 0), ('goal.rgb_static', 0),
                      ('states.rgb_static', 7776)),
                     (3888, 11664, 3888, 11664), (None, None, None, None), (1, 1, 1, 1),
                     (('frames.rgb_static', 0), ('X3.rgb_static', 0), ('X3.rgb_static', 31104), ('X3.rgb_static', 62208)),
                     (('aug.states.rgb_static.shift', 0), 'temp', ('aug.goal.rgb_static.shift', 0), 'temp'),
                     (('aug.states.rgb_static.jitter', 0), 'temp', ('aug.goal.rgb_static.jitter', 0), 'temp'), (6, 2, 2, 2),
                     0, 36, 36, 36, 36, 2),
                    True)],
 'tacorl/u8_aug_resize': [('stage_transition',
                           (('disp', 0), 1, ('reward', 0), ('done', 0), 2, ('actions', 0), ('acts', 0), 42), False),
                          ('pack_images_u8_resize_aug_gather_batch',
                           (4,
                            (('states.rgb_static', 0), ('states.rgb_static', 0), ('goal.rgb_static', 0),
                             ('states.rgb_static', 9600)),
                            (4800, 14400, 4800, 14400), (None, None, None, None), (1, 1, 1, 1),
                            (('frames.rgb_static', 0), ('X3.rgb_static', 0), ('X3.rgb_static', 31104),
                             ('X3.rgb_static', 62208)),
                            (('aug.states.rgb_static.shift', 0), 'temp', ('aug.goal.rgb_static.shift', 0), 'temp'),
                            (('aug.states.rgb_static.jitter', 0), 'temp', ('aug.goal.rgb_static.jitter', 0), 'temp'),
                            (6, 2, 2, 2), 0, 40, 40, 36, 36, 2),
                           True)],
 'tacorl_engine_only_cam/f32_nchw': [('stage_transition',
                                      (('disp', 0), 1, ('reward', 0), ('done', 0), 2, ('actions', 0), ('acts', 0), 42),
                                      False),
                                     ('pack_images_batch',
                                      (3,
                                       (('states.rgb_gripper', 0), ('goal.rgb_gripper', 0), ('states.rgb_gripper', 31104)),
                                       (11664, 3888, 11664),
                                       (('X3.rgb_gripper', 0), ('X3.rgb_gripper', 31104), ('X3.rgb_gripper', 62208)),
                                       (2, 2, 2), 0, 36, 36),
                                      True),
                                     ('pack_images_window_batch',
                                      (2, (('states.rgb_static', 0), ('goal.rgb_static', 0)), (3888, 3888),
                                       (('frames.rgb_static', 0), ('X3.rgb_static', 31104)), (6, 2),
                                       (('X3.rgb_static', 0), None), (('X3.rgb_static', 62208), None), (3, 0), 0, 36, 36),
                                      True)],
 'tacorl_engine_only_cam/replay': [('stage_transition',
                                    (('disp', 0), 1, ('reward', 0), ('done', 0), 2, ('actions', 0), ('acts', 0), 42),
                                    False),
                                   ('pack_images_u8_gather_batch',
                                    (3,
                                     (('replay.frames.rgb_gripper', 0), ('replay.frames.rgb_gripper', 0),
                                      ('replay.frames.rgb_gripper', 0)),
                                     (3888, 3888, 3888), (('replay.ids', 0), ('replay.ids', 48), ('replay.ids', 16)),
                                     (3, 1, 3),
                                     (('X3.rgb_gripper', 0), ('X3.rgb_gripper', 31104), ('X3.rgb_gripper', 62208)),
                                     (2, 2, 2), 0, 36, 36),
                                    True),
                                   ('pack_images_u8_gather_batch',
                                    (4,
                                     (('replay.frames.rgb_static', 0), ('replay.frames.rgb_static', 0),
                                      ('replay.frames.rgb_static', 0), ('replay.frames.rgb_static', 0)),
                                     (3888, 3888, 3888, 3888),
                                     (('replay.ids', 0), ('replay.ids', 0), ('replay.ids', 48), ('replay.ids', 16)),
                                     (1, 3, 1, 3),
                                     (('frames.rgb_static', 0), ('X3.rgb_static', 0), ('X3.rgb_static', 31104),
                                      ('X3.rgb_static', 62208)),
                                     (6, 2, 2, 2), 0, 36, 36),
                                    True)],
 'tacorl_engine_only_cam/replay_aug': [('stage_transition',
                                        (('disp', 0), 1, ('reward', 0), ('done', 0), 2, ('actions', 0), ('acts', 0), 42),
                                        False),
                                       ('pack_images_u8_resize_aug_gather_batch',
                                        (3,
                                         (('replay.frames.rgb_gripper', 0), ('replay.frames.rgb_gripper', 0),
                                          ('replay.frames.rgb_gripper', 0)),
                                         (3888, 3888, 3888), (('replay.ids', 0), ('replay.ids', 48), ('replay.ids', 16)),
                                         (3, 1, 3),
                                         (('X3.rgb_gripper', 0), ('X3.rgb_gripper', 31104), ('X3.rgb_gripper', 62208)),
                                         ('temp', ('aug.goal.rgb_gripper.shift', 0), 'temp'),
                                         ('temp', ('aug.goal.rgb_gripper.jitter', 0), 'temp'), (2, 2, 2), 0, 36, 36, 36, 36,
                                         2),
                                        True),
                                       ('pack_images_u8_resize_aug_gather_batch',
                                        (4,
                                         (('replay.frames.rgb_static', 0), ('replay.frames.rgb_static', 0),
                                          ('replay.frames.rgb_static', 0), ('replay.frames.rgb_static', 0)),
                                         (3888, 3888, 3888, 3888),
                                         (('replay.ids', 0), ('replay.ids', 0), ('replay.ids', 48), ('replay.ids', 16)),
                                         (1, 3, 1, 3),
                                         (('frames.rgb_static', 0), ('X3.rgb_static', 0), ('X3.rgb_static', 31104),
                                          ('X3.rgb_static', 62208)),
                                         (('aug.states.rgb_static.shift', 0), 'temp', ('aug.goal.rgb_static.shift', 0),
                                          'temp'),
                                         (('aug.states.rgb_static.jitter', 0), 'temp', ('aug.goal.rgb_static.jitter', 0),
                                          'temp'),
                                         (6, 2, 2, 2), 0, 36, 36, 36, 36, 2),
                                        True)],
 'tacorl_engine_only_cam/u8': [('stage_transition',
                                (('disp', 0), 1, ('reward', 0), ('done', 0), 2, ('actions', 0), ('acts', 0), 42), False),
                               ('pack_images_u8_batch',
                                (3, (('states.rgb_gripper', 0), ('goal.rgb_gripper', 0), ('states.rgb_gripper', 7776)),
                                 (11664, 3888, 11664),
                                 (('X3.rgb_gripper', 0), ('X3.rgb_gripper', 31104), ('X3.rgb_gripper', 62208)), (2, 2, 2),
                                 0, 36, 36),
                                True),
                               ('pack_images_u8_batch',
                                (4,
                                 (('states.rgb_static', 0), ('states.rgb_static', 0), ('goal.rgb_static', 0),
                                  ('states.rgb_static', 7776)),
                                 (3888, 11664, 3888, 11664),
                                 (('frames.rgb_static', 0), ('X3.rgb_static', 0), ('X3.rgb_static', 31104),
                                  ('X3.rgb_static', 62208)),
                                 (6, 2, 2, 2), 0, 36, 36),
                                True)],
 'tacorl_engine_only_cam/u8_aug': [('stage_transition',
                                    (('disp', 0), 1, ('reward', 0), ('done', 0), 2, ('actions', 0), ('acts', 0), 42),
                                    False),
                                   ('pack_images_u8_resize_aug_gather_batch',
                                    (3, (('states.rgb_gripper', 0), ('goal.rgb_gripper', 0), ('states.rgb_gripper', 7776)),
                                     (11664, 3888, 11664), (None, None, None), (1, 1, 1),
                                     (('X3.rgb_gripper', 0), ('X3.rgb_gripper', 31104), ('X3.rgb_gripper', 62208)),
                                     ('temp', ('aug.goal.rgb_gripper.shift', 0), 'temp'),
                                     ('temp', ('aug.goal.rgb_gripper.jitter', 0), 'temp'), (2, 2, 2), 0, 36, 36, 36, 36,
                                     2),
                                    True),
                                   ('pack_images_u8_resize_aug_gather_batch',
                                    (4,
                                     (('states.rgb_static', 0), ('states.rgb_static', 0), ('goal.rgb_static', 0),
                                      ('states.rgb_static', 7776)),
                                     (3888, 11664, 3888, 11664), (None, None, None, None), (1, 1, 1, 1),
                                     (('frames.rgb_static', 0), ('X3.rgb_static', 0), ('X3.rgb_static', 31104),
                                      ('X3.rgb_static', 62208)),
                                     (('aug.states.rgb_static.shift', 0), 'temp', ('aug.goal.rgb_static.shift', 0), 'temp'),
                                     (('aug.states.rgb_static.jitter', 0), 'temp', ('aug.goal.rgb_static.jitter', 0),
                                      'temp'),
                                     (6, 2, 2, 2), 0, 36, 36, 36, 36, 2),
                                    True)]}

GEO = 36  # what geometry() returns for the conv stack (8/4, 4/2, 3/1): the literals below are written for it


@pytest.mark.parametrize("name", sorted(cases(GEO)))
def test_launch_plan(rec, name):
    assert geometry() == GEO
    _, got = run_case(rec, name, GEO)
    assert got == PLAN[name], f"{name}:\n{got}"


# -------------------------------------------------------------------------------------------------------------- errors
def _raises_before_any_launch(rec, mod, batch, step, match, exc=ValueError):
    with pytest.raises(exc, match=match):
        step(mod, batch)
    torch.cuda.synchronize()
    _names(rec, mod, batch)
    # (TACORL's small launch - reward / done / action window - goes out on the side stream ahead of the frames)
    assert [r for r in rec.take() if r[0] != "stage_transition"] == []


@pytest.mark.parametrize("kind", ["tacorl", "playlmp"])
def test_resize_on_fp32_frames_raises(rec, kind):
    b = dict(_f32_play(GEO + 4, [S]), aug={"resize": {S: (GEO, GEO)}})
    _raises_before_any_launch(rec, _tacorl() if kind == "tacorl" else _lmp([S]), b, _train, "needs the dataset's uint8 frames")


@pytest.mark.parametrize("kind", ["tacorl", "playlmp", "cql", "ril"])
def test_uint8_frame_size_not_a_multiple_of_16_raises(rec, kind):
    """(The frames are made here: the replay feeder's own gather does not take such a dataset either.)"""
    hw = GEO + 1
    assert (hw * hw * 3) % 16
    g = torch.Generator(device=DEV).manual_seed(9)
    u8 = lambda *s: torch.randint(0, 256, s, device=DEV, dtype=torch.uint8, generator=g)  # noqa: E731
    if kind in ("tacorl", "playlmp"):
        mod = _tacorl() if kind == "tacorl" else _lmp([S])
        b = dict(_f32_play(hw, [S]), states={S: u8(B, T, hw, hw, 3)}, goal={S: u8(B, hw, hw, 3)})
    elif kind == "cql":
        mod, b = _cql(), _f32_transition(hw, [S], [S])
        goal = {S: u8(B, hw, hw, 3)}
        b.update(observations={"observation": {S: u8(B, hw, hw, 3)}, "goal": goal},
                 next_observations={"observation": {S: u8(B, hw, hw, 3)}, "goal": goal})
    else:
        mod, b = _ril(), _ril_batch(hw, True)
    _raises_before_any_launch(rec, mod, b, _train, "multiple")


@pytest.mark.parametrize("kind", ["tacorl", "playlmp"])
def test_transition_replay_handed_to_a_play_window_module_raises(rec, kind):
    """HbmTransitionReplay's fused batch has no window (replay = {kind, frames, ids, B}, no "T"): the play-window staging
    fails on the missing key before anything is launched."""
    b = dict(_u8_transition(GEO, [S], fused=True), disp=torch.tensor([1, 3], device=DEV))
    _raises_before_any_launch(rec, _tacorl() if kind == "tacorl" else _lmp([S]), b, _train, "T", exc=KeyError)


@pytest.mark.parametrize("fused", [False, True])
def test_obs_and_next_take_the_draws_of_window_frames_0_and_last(fused):
    """The launch plan sees the obs / next augmentation tables only as "temp": here their CONTENT is pinned.  TACORL's obs,
    goal and next images must be, bit for bit, what the augmenting pack makes of window frame 0 with the draws [:, 0], of the
    goal frame with the goal's own draws, and of window frame T - 1 with the draws [:, T - 1]; the window images, of every
    frame with its own draw."""
    from tacorl_amd import _lib, ops

    mod, b = _tacorl(), _u8_play(GEO, [S], fused=fused, aug=True)
    _train(mod, b)
    torch.cuda.synchronize()
    if fused:
        rp = b["replay"]
        ids = rp["ids"].long()
        st, gl = rp["frames"][S][ids[: B * T]].view(B, T, GEO, GEO, 3), rp["frames"][S][ids[B * T:]]
    else:
        st, gl = b["states"][S], b["goal"][S]
    a, ag, pad = b["aug"]["states"][S], b["aug"]["goal"][S], b["aug"]["pad"][S]

    def packed(src, shift, jitter):
        src, shift, jitter = src.contiguous(), shift.contiguous(), jitter.contiguous()
        out = torch.full((src.shape[0], GEO, GEO, 3), float("nan"), device=DEV)
        ops.pack_images_u8_resize_aug_batch([(src.data_ptr(), GEO * GEO * 3, out.data_ptr(), src.shape[0], None, 1, shift, jitter)],
                                            _lib.F32, (GEO, GEO), GEO, GEO, pad)
        torch.cuda.synchronize()
        return out

    X3 = mod.engine.X3[S]
    assert X3.dtype == torch.float32 and X3.shape[0] == 3 * B
    assert torch.equal(X3[:B], packed(st[:, 0], a["shift"][:, 0], a["jitter"][:, 0])), "obs"
    assert torch.equal(X3[B: 2 * B], packed(gl, ag["shift"], ag["jitter"])), "goal"
    assert torch.equal(X3[2 * B:], packed(st[:, T - 1], a["shift"][:, T - 1], a["jitter"][:, T - 1])), "next"
    assert not torch.equal(X3[:B], packed(st[:, 0], a["shift"][:, T - 1], a["jitter"][:, T - 1]))  # (the draws do differ)
    assert torch.equal(mod.frames[S], packed(st.reshape(B * T, GEO, GEO, 3), a["shift"].reshape(B * T, 2), a["jitter"].reshape(B * T, 8)))
