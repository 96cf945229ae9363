"""The launch plan of the perceptual-encoder stage, pinned without a device: which entry points the actor-critic engine, the
relay-imitation engine and their `load_images` issue, over how many problems and images, at which geometry, and which
(parameter block, camera) pairs the packed conv weights are written for and when.

The engines build on "cpu" and the capability predicates are host functions of the library, so with `call` replaced by a
recorder (on every loaded tacorl_amd module that has the name) the forward / backward dispatch runs as on the device and
yields the launch list.  The expectations in PLAN were written down from the commit BEFORE the three hand-kept copies of this
stage were folded into tacorl_amd/encoder_stage.py; they are literals, never derived from the code under test.

Records:
  (entry point, problems, images per problem, H, W[, max_wg])   encoder forward / backward launches
  ("fwd_fused_wg", ..., saves)                                 + which problems get their activations saved
  ("pack_weights", ((block, camera), ...))                     packed conv weights
  ("mlp_bwd_fused_dgrad", problems, flags) ...                 MLP backward launches (flags: prepacked | 2 * lean)
  ("ws", tag)                                                  workspace requests (tags decide who shares scratch memory)
"""
import sys

import pytest
import torch

from tacorl_amd import ops
from tacorl_amd._lib import BF16, F32

S, G, T3 = "rgb_static", "rgb_gripper", "rgb_tactile"

# entry point -> index of (images-per-problem array, H, max_wg) in its argument list
_ENC = {"tacorl_encoder_fwd_fused_wg": (6, 7, 9), "tacorl_encoder_fwd": (5, 6, None),
        "tacorl_encoder_bwd_fused_head": (4, 5, None), "tacorl_encoder_bwd_fused_conv": (5, 6, None),
        "tacorl_encoder_bwd_fused_fc_wgrad": (4, 5, None), "tacorl_encoder_bwd_fused": (6, 7, None),
        "tacorl_encoder_bwd": (6, 7, None), "tacorl_encoder_bwd_fused_pack": (2, 3, None)}


class Recorder:
    def __init__(self, monkeypatch):
        import tacorl_amd.engine  # noqa: F401
        import tacorl_amd.modules.play_lmp.play_lmp_for_rl  # noqa: F401
        import tacorl_amd.modules.relay_imitation_learning.engine  # noqa: F401

        self.log, self.blocks, self.bases = [], {}, {}
        real_ws = ops.workspace
        for name, mod in list(sys.modules.items()):
            if name.startswith("tacorl_amd") and mod is not None:
                if hasattr(mod, "call"):
                    monkeypatch.setattr(mod, "call", self.call)
                if hasattr(mod, "stream"):
                    monkeypatch.setattr(mod, "stream", lambda: None)
                if hasattr(mod, "workspace"):
                    monkeypatch.setattr(mod, "workspace", lambda nb, dev, tag="default": (self.log.append(("ws", tag)),
                                                                                          real_ws(nb, dev, tag))[1])

    def name_blocks(self, **blks):
        for name, blk in blks.items():
            for c in getattr(blk, "all_cams", blk.cams):
                self.blocks[blk.enc(c)] = (name, c)

    def take(self):
        out, self.log = self.log, []
        return out

    def _off(self, p):
        """A raw pointer as (name of the tensor it points into, byte offset)."""
        p = getattr(p, "value", p)
        for name, (lo, hi) in reversed(self.bases.items()):  # (newest first: an older entry's memory may have been reused)
            if lo <= p < hi:
                return (name, p - lo)
        raise AssertionError(f"pointer {p:#x} outside every known tensor")

    def call(self, name, *a):
        short = name[len("tacorl_"):]
        if name in _ENC:
            i_n, i_h, i_wg = _ENC[name]
            rec = (short[len("encoder_"):], a[0], tuple(a[i_n]), a[i_h], a[i_h + 1])
            if i_wg is not None:
                rec += (a[i_wg], tuple(bool(p) for p in a[5]))
            self.log.append(rec)
        elif name == "tacorl_encoder_pack_weights":
            self.log.append(("pack_weights", tuple(self.blocks[p] for p in a[1])))
        elif name in ("tacorl_pack_images_batch", "tacorl_pack_images_u8_batch"):
            jobs = tuple((self._off(s), int(p), self._off(d), int(n)) for s, p, d, n in zip(a[1], a[2], a[3], a[4]))
            self.log.append((short, jobs, a[5], a[6], a[7]))
        elif name == "tacorl_pack_images":
            self.log.append((short, self._off(a[0]), a[1], a[2], self._off(a[3]), a[4], a[5], a[7], a[8]))
        elif name == "tacorl_mlp_bwd_fused_dgrad":
            self.log.append((short, a[0], a[11]))
        elif name == "tacorl_mlp_bwd_fused_wgrad":
            self.log.append((short, a[0], a[12]))
        elif name in ("tacorl_mlp_bwd", "tacorl_mlp_bwd_fused_pack"):
            self.log.append((short, a[0]))
        return 0


@pytest.fixture
def rec(monkeypatch):
    return Recorder(monkeypatch)


def _ac(rec, obs, goal, hw, compute=BF16, img=torch.bfloat16, B=2):
    from tacorl_amd.engine import ACEngine

    e = ACEngine(obs, goal, hw, 7, B, "cpu", compute=compute, img_dtype=img)
    rec.name_blocks(actor=e.actor, q1=e.q1, q2=e.q2, tq1=e.tq1, tq2=e.tq2)
    rec.take()
    return e


def _ril(rec, cams, hw, compute=BF16, img=torch.bfloat16, B=2):
    from tacorl_amd.modules.relay_imitation_learning.engine import RILEngine

    e = RILEngine(cams, cams, hw, B, "cpu", compute=compute, img_dtype=img)
    rec.name_blocks(blk=e.blk)
    rec.take()
    return e


def _with_extra(rec, e, n=6):
    """A frozen network's problem per camera, as TACORL's LMP window adds them."""
    from tacorl_amd.engine import NetBlock

    lmp = NetBlock(e.cams, e.goal_cams, [e.E, 8, 4], [0, 0], [("h.0.weight", "h.0.bias"), ("h.1.weight", "h.1.bias")], "cpu")
    rec.name_blocks(lmp=lmp)
    e.extra_enc = [dict(cam=c, img=torch.zeros(n, *e.hw[c], 3, dtype=e.img_dtype), net=lmp, out=torch.zeros(n, 32),
                        act=torch.zeros(ops.encoder_act_layout(n, *e.hw[c])[1]), n=n) for c in e.enc_cams]
    return lmp


def _ac_plan(rec, e):
    e._encode_all()
    fwd = rec.take()
    e._encoders_backward()
    return {"fwd": fwd, "bwd": rec.take()}


def _ril_plan(rec, e):
    e._encode()
    fwd = rec.take()
    e._encoders_backward()
    return {"fwd": fwd, "bwd": rec.take()}


HW84 = {S: (84, 84), G: (84, 84)}


def case_ac_two_cams(rec):
    e = _ac(rec, [S, G], [S], HW84)
    out = _ac_plan(rec, e)
    e._prepack_backward()
    out["prepack"] = rec.take()
    e._encoders_backward()
    out["bwd_prepacked"] = rec.take()
    out["groups"], out["images"] = e._fused_groups(), e.encode_fused_only()
    out["fused_only"] = rec.take()
    out["ok"] = [(e._fused_ok(c), bool(e._fused_bwd_ok(c))) for c in e.enc_cams]
    out["problems"] = [[x[4:] for x in e._all_problems(c)] for c in e.enc_cams]
    return out


def case_ac_two_geometries(rec):
    return _ac_plan(rec, _ac(rec, [S, G], [S], {S: (84, 84), G: (64, 64)}))


def case_ac_three_cams(rec):
    e = _ac(rec, [S, G, T3], [S, G, T3], {S: (84, 84), G: (84, 84), T3: (84, 84)})
    return dict(_ac_plan(rec, e), groups=e._fused_groups())


def case_ac_ring(rec):
    e = _ac(rec, [S], [S], {S: (150, 200)})
    return dict(_ac_plan(rec, e), ok=(e._fused_ok(S), bool(e._fused_bwd_ok(S))))


def case_ac_no_fused_geometry(rec):
    e = _ac(rec, [S], [S], {S: (48, 48)})
    return dict(_ac_plan(rec, e), ok=(e._fused_ok(S), bool(e._fused_bwd_ok(S))), groups=e._fused_groups())


def case_ac_f32(rec):
    return _ac_plan(rec, _ac(rec, [S], [S], {S: (84, 84)}, compute=F32, img=torch.float32))


def case_ac_use_fused_off(rec):
    e = _ac(rec, [S, G], [S], HW84)
    e.use_fused = False
    return _ac_plan(rec, e)


def case_ac_extra(rec):
    e = _ac(rec, [S, G], [S], HW84)
    _with_extra(rec, e)
    out = {"fwd": (e._encode_all(), rec.take())[1]}
    seen = []
    out["split"] = e.encode_split(lambda: seen.append(len(rec.log)))
    out["split_fwd"], out["between"] = rec.take(), seen
    # the benchmark times the fused launches by replacing _launch_fused on the instance: every one must go through it
    spied, orig = [], e._launch_fused
    e._launch_fused = lambda c, pr, max_wg=0: (spied.append((c, len(pr), max_wg)), orig(c, pr, max_wg))[1]
    e._encode_all(), e.encode_split(lambda: None), e.encode_fused_only()
    out["spied"], out["spied_launches"] = spied, [r[:2] for r in rec.take()]
    e.extra_enc = []
    out["split_without_extra"] = e.encode_split(lambda: None)
    return out


def case_ril_two_geometries(rec):
    e = _ril(rec, [S, G], {S: (84, 84), G: (48, 48)})
    out = {"fwd": (e._encode(), rec.take())[1]}
    e.backward()
    out["bwd"] = rec.take()
    out["act_t"] = [e.enc_act_t[c] is None for c in e.cams]
    return out


def case_ril_per_layer_camera_first(rec):
    return _ril_plan(rec, _ril(rec, [G, S], {S: (84, 84), G: (48, 48)}))


def case_ril_two_cams(rec):
    return _ril_plan(rec, _ril(rec, [S, G], HW84))


def case_ril_f32(rec):
    return _ril_plan(rec, _ril(rec, [S], {S: (84, 84)}, compute=F32, img=torch.float32))


def _packs(records):
    return [r for r in records if r[0] == "pack_weights"]


def case_ac_pack_bookkeeping(rec):
    e = _ac(rec, [S, G], [S], HW84)
    lmp = _with_extra(rec, e)
    out = {"stale_at_start": e.packs_stale()}
    out["first"] = _packs((e._encode_all(), rec.take())[1])
    out["second"] = _packs((e._encode_all(), rec.take())[1])
    ops.touched(e.q1.param)
    out["stale_after_touch"] = e.packs_stale()
    out["third"] = _packs((e._encode_all(), rec.take())[1])
    out["stale_after_forward"] = e.packs_stale()
    out["late"] = _packs((e.phase_c(), rec.take())[1])
    out["stale_after_step"] = e.packs_stale()
    out["after_step"] = _packs((e._encode_all(), rec.take())[1])
    # a replayed graph: the optimiser's writes are announced, then the graph's own late pack is recorded
    ops.touched(*[b.param for b in (e.actor, e.q1, e.q2, e.tq1, e.tq2)])
    out["stale_before_written"] = e.packs_stale()
    e.packs_written()
    out["stale_after_written"] = e.packs_stale()
    ops.touched(lmp.param)  # a frozen network's parameters edited in place: no replay's late pack covers that
    e.packs_written()
    out["stale_frozen_edited"] = e.packs_stale()
    out["frozen"] = _packs((e._encode_all(), rec.take())[1])
    out["no_optimize"] = _packs((e.phase_c(optimize=False), rec.take())[1])
    return out


def case_ril_pack_bookkeeping(rec):
    e = _ril(rec, [S, G], {S: (84, 84), G: (48, 48)})
    out = {"stale_at_start": e.packs_stale()}
    out["first"] = _packs((e._encode(), rec.take())[1])
    out["second"] = _packs((e._encode(), rec.take())[1])
    ops.touched(e.blk.param)
    out["stale_after_touch"] = e.packs_stale()
    out["third"] = _packs((e._encode(), rec.take())[1])
    out["late"] = _packs((e.optimizer_step(), rec.take())[1])
    out["stale_after_step"] = e.packs_stale()
    out["after_step"] = _packs((e._encode(), rec.take())[1])
    ops.touched(e.blk.param)
    out["stale_before_written"] = e.packs_stale()
    e.packs_written()
    out["stale_after_written"] = e.packs_stale()
    return out


class _OnDevice(torch.Tensor):
    """A host tensor that answers is_cuda = True: load_images only takes addresses and strides."""
    is_cuda = property(lambda self: True)


def _images(rec, name, *shape, dtype=torch.float32, skip=0):
    t = torch.zeros(skip + int(torch.tensor(shape).prod()), dtype=dtype)
    rec.bases.pop(name, None)
    rec.bases[name] = (t.data_ptr(), t.data_ptr() + t.numel() * t.element_size())
    return t[skip:].view(*shape).as_subclass(_OnDevice)


def _load_cases(rec, e, load):
    """load(cam, tensors of the camera's slots, nchw); the cameras: S 84 x 84 with every slot, G 49 x 49 (H*W odd)."""
    for c in e.X3:
        rec.bases["X3:" + c] = (e.X3[c].data_ptr(), e.X3[c].data_ptr() + e.X3[c].numel() * e.X3[c].element_size())
    ns, B, out = len(e.X3[S]) // e.B, e.B, {}
    run = lambda *a: (load(*a), rec.take())[1]  # noqa: E731
    out["f32_nchw"] = run(S, [_images(rec, f"src{i}", B, 3, 84, 84) for i in range(ns)], True)
    out["f32_nhwc"] = run(S, [_images(rec, f"src{i}", B, 84, 84, 3) for i in range(ns)], False)
    out["u8"] = run(S, [_images(rec, f"src{i}", B, 84, 84, 3, dtype=torch.uint8) for i in range(ns)], False)
    states = _images(rec, "states", B, ns + 1, 3, 84, 84)
    out["f32_strided"] = run(S, [states[:, i] for i in range(ns)], True)
    states = _images(rec, "states", B, ns + 1, 84, 84, 3, dtype=torch.uint8)
    out["u8_strided"] = run(S, [states[:, i] for i in range(ns)], False)
    ng = len(e.X3[G]) // e.B
    out["f32_nchw_odd"] = run(G, [_images(rec, f"src{i}", B, 3, 49, 49) for i in range(ng)], True)
    out["f32_nchw_unaligned"] = run(S, [_images(rec, f"src{i}", B, 3, 84, 84, skip=1) for i in range(ns)], True)
    for key, cam, hw, skip in (("u8_size", G, (49, 49), 0), ("u8_unaligned", S, (84, 84), 8)):
        n = ng if cam == G else ns
        with pytest.raises(ValueError) as err:
            load(cam, [_images(rec, f"src{i}", B, *hw, 3, dtype=torch.uint8, skip=skip) for i in range(n)], False)
        out[key] = (str(err.value), rec.take())
    return out


def case_ac_load_images(rec):
    e = _ac(rec, [S, G], [S], {S: (84, 84), G: (49, 49)})  # S: [obs | goal | next], G: [obs | next]
    return _load_cases(rec, e, lambda c, ts, nchw: e.load_images(c, ts[0], ts[1] if c == S else None, ts[-1], nchw=nchw))


def case_ril_load_images(rec):
    e = _ril(rec, [S, G], {S: (84, 84), G: (49, 49)})
    return _load_cases(rec, e, lambda c, ts, nchw: e.load_images(c, ts, nchw=nchw))


CASES = {k[len("case_"):]: v for k, v in sorted(globals().items()) if k.startswith("case_")}

PLAN = {'ac_extra': {'between': [1],
              'fwd': [('pack_weights',
                       (('actor', 'rgb_static'), ('q1', 'rgb_static'), ('q2', 'rgb_static'), ('tq1', 'rgb_static'),
                        ('tq2', 'rgb_static'), ('lmp', 'rgb_static'))),
                      ('pack_weights',
                       (('actor', 'rgb_gripper'), ('q1', 'rgb_gripper'), ('q2', 'rgb_gripper'), ('tq1', 'rgb_gripper'),
                        ('tq2', 'rgb_gripper'), ('lmp', 'rgb_gripper'))),
                      ('fwd_fused_wg', 14, (4, 2, 4, 4, 4, 4, 6, 2, 2, 2, 2, 2, 2, 6), 84, 84, 0,
                       (True, False, True, True, False, False, False, True, False, True, True, False, False, False))],
              'spied': [('rgb_static', 14, 0), ('rgb_static', 2, 0), ('rgb_static', 12, 160), ('rgb_static', 14, 0)],
              'spied_launches': [('fwd_fused_wg', 14), ('fwd_fused_wg', 2), ('fwd_fused_wg', 12), ('fwd_fused_wg', 14)],
              'split': True,
              'split_fwd': [('fwd_fused_wg', 2, (6, 6), 84, 84, 0, (False, False)),
                            ('fwd_fused_wg', 12, (4, 2, 4, 4, 4, 4, 2, 2, 2, 2, 2, 2), 84, 84, 160,
                             (True, False, True, True, False, False, True, False, True, True, False, False))],
              'split_without_extra': False},
 'ac_f32': {'bwd': [('ws', 'mlp_bwd_genc'), ('mlp_bwd', 3), ('ws', 'enc_bwd'), ('bwd', 3, (4, 4, 4), 84, 84)],
            'fwd': [('fwd', 6, (4, 2, 4, 4, 4, 4), 84, 84)]},
 'ac_load_images': {'f32_nchw': [('pack_images_batch',
                                  ((('src0', 0), 21168, ('X3:rgb_static', 0), 2),
                                   (('src1', 0), 21168, ('X3:rgb_static', 84672), 2),
                                   (('src2', 0), 21168, ('X3:rgb_static', 169344), 2)),
                                  1, 84, 84)],
                    'f32_nchw_odd': [('pack_images', ('src0', 0), 7203, 1, ('X3:rgb_gripper', 0), 1, 2, 49, 49),
                                     ('pack_images', ('src1', 0), 7203, 1, ('X3:rgb_gripper', 28812), 1, 2, 49, 49)],
                    'f32_nchw_unaligned': [('pack_images', ('src0', 4), 21168, 1, ('X3:rgb_static', 0), 1, 2, 84, 84),
                                           ('pack_images', ('src1', 4), 21168, 1, ('X3:rgb_static', 84672), 1, 2, 84, 84),
                                           ('pack_images', ('src2', 4), 21168, 1, ('X3:rgb_static', 169344), 1, 2, 84, 84)],
                    'f32_nhwc': [('pack_images', ('src0', 0), 21168, 0, ('X3:rgb_static', 0), 1, 2, 84, 84),
                                 ('pack_images', ('src1', 0), 21168, 0, ('X3:rgb_static', 84672), 1, 2, 84, 84),
                                 ('pack_images', ('src2', 0), 21168, 0, ('X3:rgb_static', 169344), 1, 2, 84, 84)],
                    'f32_strided': [('pack_images_batch',
                                     ((('states', 0), 84672, ('X3:rgb_static', 0), 2),
                                      (('states', 84672), 84672, ('X3:rgb_static', 84672), 2),
                                      (('states', 169344), 84672, ('X3:rgb_static', 169344), 2)),
                                     1, 84, 84)],
                    'u8': [('pack_images_u8_batch',
                            ((('src0', 0), 21168, ('X3:rgb_static', 0), 2),
                             (('src1', 0), 21168, ('X3:rgb_static', 84672), 2),
                             (('src2', 0), 21168, ('X3:rgb_static', 169344), 2)),
                            1, 84, 84)],
                    'u8_size': ('uint8 frames: H*W*3 and the image pitch must be multiples of 16, tensors 16-byte aligned',
                                []),
                    'u8_strided': [('pack_images_u8_batch',
                                    ((('states', 0), 84672, ('X3:rgb_static', 0), 2),
                                     (('states', 21168), 84672, ('X3:rgb_static', 84672), 2),
                                     (('states', 42336), 84672, ('X3:rgb_static', 169344), 2)),
                                    1, 84, 84)],
                    'u8_unaligned': ('uint8 frames: H*W*3 and the image pitch must be multiples of 16, tensors 16-byte '
                                     'aligned',
                                     [])},
 'ac_no_fused_geometry': {'bwd': [('ws', 'mlp_bwdf_genc'), ('mlp_bwd_fused_dgrad', 3, 2), ('ws', 'mlp_bwdf_genc'),
                                  ('mlp_bwd_fused_wgrad', 3, 1), ('ws', 'enc_bwd'), ('bwd', 3, (4, 4, 4), 48, 48)],
                          'fwd': [('fwd', 6, (4, 2, 4, 4, 4, 4), 48, 48)],
                          'groups': [],
                          'ok': (False, False)},
 'ac_pack_bookkeeping': {'after_step': [],
                         'first': [('pack_weights',
                                    (('actor', 'rgb_static'), ('q1', 'rgb_static'), ('q2', 'rgb_static'),
                                     ('tq1', 'rgb_static'), ('tq2', 'rgb_static'), ('lmp', 'rgb_static'))),
                                   ('pack_weights',
                                    (('actor', 'rgb_gripper'), ('q1', 'rgb_gripper'), ('q2', 'rgb_gripper'),
                                     ('tq1', 'rgb_gripper'), ('tq2', 'rgb_gripper'), ('lmp', 'rgb_gripper')))],
                         'frozen': [('pack_weights', (('lmp', 'rgb_static'),)),
                                    ('pack_weights', (('lmp', 'rgb_gripper'),))],
                         'late': [('pack_weights',
                                   (('actor', 'rgb_static'), ('q1', 'rgb_static'), ('q2', 'rgb_static'),
                                    ('tq1', 'rgb_static'), ('tq2', 'rgb_static'))),
                                  ('pack_weights',
                                   (('actor', 'rgb_gripper'), ('q1', 'rgb_gripper'), ('q2', 'rgb_gripper'),
                                    ('tq1', 'rgb_gripper'), ('tq2', 'rgb_gripper')))],
                         'no_optimize': [],
                         'second': [],
                         'stale_after_forward': False,
                         'stale_after_step': False,
                         'stale_after_touch': True,
                         'stale_after_written': False,
                         'stale_at_start': False,
                         'stale_before_written': True,
                         'stale_frozen_edited': True,
                         'third': [('pack_weights', (('q1', 'rgb_static'),)), ('pack_weights', (('q1', 'rgb_gripper'),))]},
 'ac_ring': {'bwd': [('ws', 'mlp_bwdf_genc'), ('mlp_bwd_fused_dgrad', 3, 2), ('ws', 'mlp_bwdf_genc'),
                     ('mlp_bwd_fused_wgrad', 3, 1), ('ws', 'enc_bwd_fused_rgb_static'),
                     ('bwd_fused_head', 3, (4, 4, 4), 150, 200), ('bwd_fused_conv', 3, (4, 4, 4), 150, 200),
                     ('bwd_fused_fc_wgrad', 3, (4, 4, 4), 150, 200)],
             'fwd': [('pack_weights',
                      (('actor', 'rgb_static'), ('q1', 'rgb_static'), ('q2', 'rgb_static'), ('tq1', 'rgb_static'),
                       ('tq2', 'rgb_static'))),
                     ('fwd_fused_wg', 6, (4, 2, 4, 4, 4, 4), 150, 200, 0, (True, False, True, True, False, False))],
             'ok': (True, True)},
 'ac_three_cams': {'bwd': [('ws', 'mlp_bwdf_genc'), ('mlp_bwd_fused_dgrad', 3, 2), ('ws', 'mlp_bwdf_genc'),
                           ('mlp_bwd_fused_wgrad', 3, 1), ('ws', 'enc_bwd_fused_rgb_static'),
                           ('bwd_fused_head', 3, (4, 4, 4), 84, 84), ('bwd_fused_conv', 3, (4, 4, 4), 84, 84),
                           ('bwd_fused_fc_wgrad', 3, (4, 4, 4), 84, 84), ('ws', 'enc_bwd_fused_rgb_gripper'),
                           ('bwd_fused_head', 3, (4, 4, 4), 84, 84), ('bwd_fused_conv', 3, (4, 4, 4), 84, 84),
                           ('bwd_fused_fc_wgrad', 3, (4, 4, 4), 84, 84), ('ws', 'enc_bwd_fused_rgb_tactile'),
                           ('bwd_fused_head', 3, (4, 4, 4), 84, 84), ('bwd_fused_conv', 3, (4, 4, 4), 84, 84),
                           ('bwd_fused_fc_wgrad', 3, (4, 4, 4), 84, 84)],
                   'fwd': [('pack_weights',
                            (('actor', 'rgb_static'), ('q1', 'rgb_static'), ('q2', 'rgb_static'), ('tq1', 'rgb_static'),
                             ('tq2', 'rgb_static'))),
                           ('fwd_fused_wg', 6, (4, 2, 4, 4, 4, 4), 84, 84, 0, (True, False, True, True, False, False)),
                           ('pack_weights',
                            (('actor', 'rgb_gripper'), ('q1', 'rgb_gripper'), ('q2', 'rgb_gripper'), ('tq1', 'rgb_gripper'),
                             ('tq2', 'rgb_gripper'))),
                           ('fwd_fused_wg', 6, (4, 2, 4, 4, 4, 4), 84, 84, 0, (True, False, True, True, False, False)),
                           ('pack_weights',
                            (('actor', 'rgb_tactile'), ('q1', 'rgb_tactile'), ('q2', 'rgb_tactile'), ('tq1', 'rgb_tactile'),
                             ('tq2', 'rgb_tactile'))),
                           ('fwd_fused_wg', 6, (4, 2, 4, 4, 4, 4), 84, 84, 0, (True, False, True, True, False, False))],
                   'groups': [['rgb_static'], ['rgb_gripper'], ['rgb_tactile']]},
 'ac_two_cams': {'bwd': [('ws', 'mlp_bwdf_genc'), ('mlp_bwd_fused_dgrad', 3, 2), ('ws', 'mlp_bwdf_genc'),
                         ('mlp_bwd_fused_wgrad', 3, 1), ('ws', 'enc_bwd_fused_rgb_static+rgb_gripper'),
                         ('bwd_fused_head', 6, (4, 4, 4, 2, 2, 2), 84, 84),
                         ('bwd_fused_conv', 6, (4, 4, 4, 2, 2, 2), 84, 84),
                         ('bwd_fused_fc_wgrad', 6, (4, 4, 4, 2, 2, 2), 84, 84)],
                 'bwd_prepacked': [('ws', 'mlp_bwdf_genc'), ('mlp_bwd_fused_dgrad', 3, 3), ('ws', 'mlp_bwdf_genc'),
                                   ('mlp_bwd_fused_wgrad', 3, 1), ('ws', 'enc_bwd_fused_rgb_static+rgb_gripper'),
                                   ('bwd_fused_head', 6, (4, 4, 4, 2, 2, 2), 84, 84),
                                   ('bwd_fused_conv', 6, (4, 4, 4, 2, 2, 2), 84, 84),
                                   ('bwd_fused_fc_wgrad', 6, (4, 4, 4, 2, 2, 2), 84, 84)],
                 'fused_only': [('fwd_fused_wg', 12, (4, 2, 4, 4, 4, 4, 2, 2, 2, 2, 2, 2), 84, 84, 0,
                                 (True, False, True, True, False, False, True, False, True, True, False, False))],
                 'fwd': [('pack_weights',
                          (('actor', 'rgb_static'), ('q1', 'rgb_static'), ('q2', 'rgb_static'), ('tq1', 'rgb_static'),
                           ('tq2', 'rgb_static'))),
                         ('pack_weights',
                          (('actor', 'rgb_gripper'), ('q1', 'rgb_gripper'), ('q2', 'rgb_gripper'), ('tq1', 'rgb_gripper'),
                           ('tq2', 'rgb_gripper'))),
                         ('fwd_fused_wg', 12, (4, 2, 4, 4, 4, 4, 2, 2, 2, 2, 2, 2), 84, 84, 0,
                          (True, False, True, True, False, False, True, False, True, True, False, False))],
                 'groups': [['rgb_static', 'rgb_gripper']],
                 'images': 34,
                 'ok': [(True, True), (True, True)],
                 'prepack': [('ws', 'mlp_bwdf_q'), ('mlp_bwd_fused_pack', 2), ('ws', 'mlp_bwdf_qpi'),
                             ('mlp_bwd_fused_pack', 2), ('ws', 'mlp_bwdf_pi'), ('mlp_bwd_fused_pack', 1),
                             ('ws', 'mlp_bwdf_genc'), ('mlp_bwd_fused_pack', 3),
                             ('ws', 'enc_bwd_fused_rgb_static+rgb_gripper'),
                             ('bwd_fused_pack', 6, (4, 4, 4, 2, 2, 2), 84, 84)],
                 'problems': [[(4, True, 'rgb_static'), (2, False, 'rgb_static'), (4, True, 'rgb_static'),
                               (4, True, 'rgb_static'), (4, False, 'rgb_static'), (4, False, 'rgb_static')],
                              [(2, True, 'rgb_gripper'), (2, False, 'rgb_gripper'), (2, True, 'rgb_gripper'),
                               (2, True, 'rgb_gripper'), (2, False, 'rgb_gripper'), (2, False, 'rgb_gripper')]]},
 'ac_two_geometries': {'bwd': [('ws', 'mlp_bwdf_genc'), ('mlp_bwd_fused_dgrad', 3, 2), ('ws', 'mlp_bwdf_genc'),
                               ('mlp_bwd_fused_wgrad', 3, 1), ('ws', 'enc_bwd_fused_rgb_static'),
                               ('bwd_fused_head', 3, (4, 4, 4), 84, 84), ('bwd_fused_conv', 3, (4, 4, 4), 84, 84),
                               ('bwd_fused_fc_wgrad', 3, (4, 4, 4), 84, 84), ('ws', 'enc_bwd_fused_rgb_gripper'),
                               ('bwd_fused_head', 3, (2, 2, 2), 64, 64), ('bwd_fused_conv', 3, (2, 2, 2), 64, 64),
                               ('bwd_fused_fc_wgrad', 3, (2, 2, 2), 64, 64)],
                       'fwd': [('pack_weights',
                                (('actor', 'rgb_static'), ('q1', 'rgb_static'), ('q2', 'rgb_static'), ('tq1', 'rgb_static'),
                                 ('tq2', 'rgb_static'))),
                               ('fwd_fused_wg', 6, (4, 2, 4, 4, 4, 4), 84, 84, 0, (True, False, True, True, False, False)),
                               ('pack_weights',
                                (('actor', 'rgb_gripper'), ('q1', 'rgb_gripper'), ('q2', 'rgb_gripper'),
                                 ('tq1', 'rgb_gripper'), ('tq2', 'rgb_gripper'))),
                               ('fwd_fused_wg', 6, (2, 2, 2, 2, 2, 2), 64, 64, 0,
                                (True, False, True, True, False, False))]},
 'ac_use_fused_off': {'bwd': [('ws', 'mlp_bwdf_genc'), ('mlp_bwd_fused_dgrad', 3, 2), ('ws', 'mlp_bwdf_genc'),
                              ('mlp_bwd_fused_wgrad', 3, 1), ('ws', 'enc_bwd'), ('bwd', 3, (4, 4, 4), 84, 84),
                              ('ws', 'enc_bwd'), ('bwd', 3, (2, 2, 2), 84, 84)],
                      'fwd': [('fwd', 6, (4, 2, 4, 4, 4, 4), 84, 84), ('fwd', 6, (2, 2, 2, 2, 2, 2), 84, 84)]},
 'ril_f32': {'bwd': [('ws', 'ril_enc_bwd'), ('bwd', 1, (6,), 84, 84)], 'fwd': [('fwd', 2, (6, 2), 84, 84)]},
 'ril_load_images': {'f32_nchw': [('pack_images_batch',
                                   ((('src0', 0), 21168, ('X3:rgb_static', 0), 2),
                                    (('src1', 0), 21168, ('X3:rgb_static', 84672), 2),
                                    (('src2', 0), 21168, ('X3:rgb_static', 169344), 2),
                                    (('src3', 0), 21168, ('X3:rgb_static', 254016), 2)),
                                   1, 84, 84)],
                     'f32_nchw_odd': [('pack_images', ('src0', 0), 7203, 1, ('X3:rgb_gripper', 0), 1, 2, 49, 49),
                                      ('pack_images', ('src1', 0), 7203, 1, ('X3:rgb_gripper', 28812), 1, 2, 49, 49),
                                      ('pack_images', ('src2', 0), 7203, 1, ('X3:rgb_gripper', 57624), 1, 2, 49, 49),
                                      ('pack_images', ('src3', 0), 7203, 1, ('X3:rgb_gripper', 86436), 1, 2, 49, 49)],
                     'f32_nchw_unaligned': [('pack_images', ('src0', 4), 21168, 1, ('X3:rgb_static', 0), 1, 2, 84, 84),
                                            ('pack_images', ('src1', 4), 21168, 1, ('X3:rgb_static', 84672), 1, 2, 84, 84),
                                            ('pack_images', ('src2', 4), 21168, 1, ('X3:rgb_static', 169344), 1, 2, 84, 84),
                                            ('pack_images', ('src3', 4), 21168, 1, ('X3:rgb_static', 254016), 1, 2, 84,
                                             84)],
                     'f32_nhwc': [('pack_images', ('src0', 0), 21168, 0, ('X3:rgb_static', 0), 1, 2, 84, 84),
                                  ('pack_images', ('src1', 0), 21168, 0, ('X3:rgb_static', 84672), 1, 2, 84, 84),
                                  ('pack_images', ('src2', 0), 21168, 0, ('X3:rgb_static', 169344), 1, 2, 84, 84),
                                  ('pack_images', ('src3', 0), 21168, 0, ('X3:rgb_static', 254016), 1, 2, 84, 84)],
                     'f32_strided': [('pack_images_batch',
                                      ((('states', 0), 105840, ('X3:rgb_static', 0), 2),
                                       (('states', 84672), 105840, ('X3:rgb_static', 84672), 2),
                                       (('states', 169344), 105840, ('X3:rgb_static', 169344), 2),
                                       (('states', 254016), 105840, ('X3:rgb_static', 254016), 2)),
                                      1, 84, 84)],
                     'u8': [('pack_images_u8_batch',
                             ((('src0', 0), 21168, ('X3:rgb_static', 0), 2),
                              (('src1', 0), 21168, ('X3:rgb_static', 84672), 2),
                              (('src2', 0), 21168, ('X3:rgb_static', 169344), 2),
                              (('src3', 0), 21168, ('X3:rgb_static', 254016), 2)),
                             1, 84, 84)],
                     'u8_size': ('uint8 frames: H*W*3 and the image pitch must be multiples of 16, tensors 16-byte aligned',
                                 []),
                     'u8_strided': [('pack_images_u8_batch',
                                     ((('states', 0), 105840, ('X3:rgb_static', 0), 2),
                                      (('states', 21168), 105840, ('X3:rgb_static', 84672), 2),
                                      (('states', 42336), 105840, ('X3:rgb_static', 169344), 2),
                                      (('states', 63504), 105840, ('X3:rgb_static', 254016), 2)),
                                     1, 84, 84)],
                     'u8_unaligned': ('uint8 frames: H*W*3 and the image pitch must be multiples of 16, tensors 16-byte '
                                      'aligned',
                                      [])},
 'ril_pack_bookkeeping': {'after_step': [],
                          'first': [('pack_weights', (('blk', 'rgb_static'),))],
                          'late': [('pack_weights', (('blk', 'rgb_static'),))],
                          'second': [],
                          'stale_after_step': False,
                          'stale_after_touch': True,
                          'stale_after_written': False,
                          'stale_at_start': False,
                          'stale_before_written': True,
                          'third': [('pack_weights', (('blk', 'rgb_static'),))]},
 'ril_per_layer_camera_first': {'bwd': [('ws', 'ril_enc_bwd'), ('bwd', 1, (6,), 48, 48),
                                        ('ws', 'ril_enc_bwd_fused_rgb_static'), ('bwd_fused', 1, (6,), 84, 84)],
                                'fwd': [('pack_weights', (('blk', 'rgb_static'),)),
                                        ('fwd_fused_wg', 2, (6, 2), 84, 84, 0, (True, False)),
                                        ('fwd', 2, (6, 2), 48, 48)]},
 'ril_two_cams': {'bwd': [('ws', 'ril_enc_bwd_fused_rgb_static+rgb_gripper'), ('bwd_fused', 2, (6, 6), 84, 84)],
                  'fwd': [('pack_weights', (('blk', 'rgb_static'), ('blk', 'rgb_gripper'))),
                          ('fwd_fused_wg', 4, (6, 2, 6, 2), 84, 84, 0, (True, False, True, False))]},
 'ril_two_geometries': {'act_t': [True, False],
                        'bwd': [('ws', 'ril_bwd_pol_low'), ('mlp_bwd', 1), ('ws', 'ril_bwd_pol_high'), ('mlp_bwd', 1),
                                ('ws', 'ril_bwdf_genc'), ('mlp_bwd_fused_dgrad', 1, 0), ('ws', 'ril_bwdf_genc'),
                                ('mlp_bwd_fused_wgrad', 1, 0), ('ws', 'ril_enc_bwd_fused_rgb_static'),
                                ('bwd_fused', 1, (6,), 84, 84), ('ws', 'ril_enc_bwd'), ('bwd', 1, (6,), 48, 48)],
                        'fwd': [('pack_weights', (('blk', 'rgb_static'),)),
                                ('fwd_fused_wg', 2, (6, 2), 84, 84, 0, (True, False)), ('fwd', 2, (6, 2), 48, 48)]}}


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_plan_is_the_recorded_one(rec, name):
    got = CASES[name](rec)
    assert sorted(got) == sorted(PLAN[name])
    for key in got:
        assert got[key] == PLAN[name][key], (name, key)
