"""Train-time image augmentations as GPU work (reference utils/transforms.py:265-330 and
config/datamodule/transform_manager/transforms/rl_train.yaml): the random draws are made here, as small device
tables, and applied by `tacorl_pack_images_u8_aug_batch` on the way into the encoder's image buffers."""
import torch


class AugmentSpec:
    """One camera's train pipeline: RandomShiftsAug(pad) and ColorTransform(contrast, brightness, hue, prob)
    (rl_train.yaml: pad 6 / 4, contrast 0.1, brightness 0.1, hue 0.02)."""

    def __init__(self, pad=4, brightness=0.1, contrast=0.1, hue=0.02, prob=1.0, resize=None):
        self.pad, self.brightness, self.contrast, self.hue, self.prob = int(pad), brightness, contrast, hue, prob
        # torchvision.transforms.Resize(size) ahead of the shift (rl_train.yaml:3-4,16-17: [128, 128] static, [84, 84]
        # gripper): the dataset's frames keep their camera resolution and are resized by the same launch
        self.resize = None if resize is None else (int(resize[0]), int(resize[1]))

    def draw(self, n, device, generator=None):
        """The reference's draws for n frames: shift = randint(0, 2*pad+1, (n,2)) (utils/transforms.py:288-290);
        ColorJitter.get_params: fn_idx = randperm(4), b ~ U(max(0,1-b), 1+b), c likewise, h ~ U(-hue, hue);
        ColorTransform applies it with probability `prob` (:311-314).  Returns (shift int32 (n,2), jitter f32 (n,8))."""
        g = generator
        shift = torch.randint(0, 2 * self.pad + 1, (n, 2), device=device, generator=g, dtype=torch.int32)
        u = torch.rand(n, 4, device=device, generator=g)
        b = max(0.0, 1 - self.brightness) + u[:, 0] * (1 + self.brightness - max(0.0, 1 - self.brightness))
        c = max(0.0, 1 - self.contrast) + u[:, 1] * (1 + self.contrast - max(0.0, 1 - self.contrast))
        h = (2 * u[:, 2] - 1) * self.hue
        order = torch.rand(n, 4, device=device, generator=g).argsort(dim=1).float()  # a uniform random permutation
        apply = (u[:, 3] < self.prob).float()
        return shift, torch.cat([b[:, None], c[:, None], h[:, None], order, apply[:, None]], dim=1).contiguous()


def augment_specs(transform_manager, cams, split="train"):
    """{camera: AugmentSpec or None} out of a transform manager config of the `rl` form (config/datamodule/transform_manager/
    rl.yaml: transforms.<split>.<camera> = a list of {_target_, ...}): Resize(size) -> spec.resize, RandomShiftsAug(pad) ->
    spec.pad, ColorTransform(contrast, brightness, hue, prob) -> the spec's jitter; ScaleImageTensor and Normalize(0.5, 0.5)
    are what the uint8 pack computes anyway.  Any other transform of a camera in `cams` is not built.  None: no config."""
    if transform_manager is None:
        return {c: None for c in cams}
    cfg = dict(transform_manager)
    lists = dict(dict(cfg.get("transforms", cfg) or {}).get(split) or {})
    out = {}
    for c in cams:
        kw, seen = {"pad": 0, "prob": 0.0}, False
        for t in lists.get(c) or []:
            t = dict(t)
            name = str(t.get("_target_", "")).rsplit(".", 1)[-1]
            if name == "Resize":
                size = t["size"]
                kw["resize"] = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
            elif name == "RandomShiftsAug":
                kw["pad"], seen = int(t.get("pad", 4)), True
            elif name == "ColorTransform":
                kw.update(brightness=t.get("brightness", 0.0), contrast=t.get("contrast", 0.0), hue=t.get("hue", 0.0),
                          prob=t.get("prob", 1.0))
                seen = True
            elif name == "Normalize":
                if [float(x) for x in t.get("mean", [0.5])] != [0.5] or [float(x) for x in t.get("std", [0.5])] != [0.5]:
                    raise NotImplementedError(f"transform {t.get('_target_')} of {c}: only Normalize(0.5, 0.5) is part of the pack")
            elif name != "ScaleImageTensor":  # (x / 255: part of the pack)
                raise NotImplementedError(f"transform {t.get('_target_')} of {c} is not built")
        out[c] = AugmentSpec(**kw) if seen or "resize" in kw else None
    return out


def draw_play_batch_augmentation(specs, B, T, device, generator=None):
    """batch["aug"] for a play batch: per camera a different draw for every frame of the window and for the goal frame,
    as the reference's dataset applies its transform to (T,3,H,W) windows and to the goal frame separately
    (play_dataset.py:405-412,246-247; RandomShiftsAug draws per leading index)."""
    aug = {"states": {}, "goal": {}, "pad": {}, "resize": {}}
    for cam, sp in specs.items():
        if sp.resize is not None:
            aug["resize"][cam] = sp.resize
        s, j = sp.draw(B * T, device, generator)
        aug["states"][cam] = {"shift": s.view(B, T, 2), "jitter": j.view(B, T, 8)}
        s, j = sp.draw(B, device, generator)
        aug["goal"][cam] = {"shift": s, "jitter": j}
        aug["pad"][cam] = sp.pad
    return aug


def draw_transition_batch_augmentation(specs, B, device, generator=None):
    """batch["aug"] for a transition batch: per camera three independent draws, for the observation, the next observation
    and the goal frame - the reference's transition dataset transforms the three in three separate calls
    (goal_cond_replay_buffer_dataset.py:276-282)."""
    aug = {"obs": {}, "next": {}, "goal": {}, "pad": {}, "resize": {}}
    for cam, sp in specs.items():
        if sp.resize is not None:
            aug["resize"][cam] = sp.resize
        for role in ("obs", "next", "goal"):
            s, j = sp.draw(B, device, generator)
            aug[role][cam] = {"shift": s, "jitter": j}
        aug["pad"][cam] = sp.pad
    return aug


RIL_ROLES = ("obs", "low_level_goal", "high_level_goal", "high_level_action")  # the RIL engine's image slots, in order


def draw_ril_batch_augmentation(specs, B, device, generator=None):
    """batch["aug"] for a relay-imitation-learning batch: per camera four independent draws, one per frame of the item - the
    reference's dataset calls its transform manager once per frame (relay_imitation_learning_dataset.py:85-98,121-127)."""
    aug = {role: {} for role in RIL_ROLES}
    aug.update(pad={}, resize={})
    for cam, sp in specs.items():
        if sp.resize is not None:
            aug["resize"][cam] = sp.resize
        for role in RIL_ROLES:
            s, j = sp.draw(B, device, generator)
            aug[role][cam] = {"shift": s, "jitter": j}
        aug["pad"][cam] = sp.pad
    return aug
