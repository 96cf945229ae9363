"""Builders and checks shared by the device-noise module tests (tests/test_device_noise_step_gpu.py, the two-rank script):
fixture-sized modules of the existing goldens' configurations, the restatement of every noise buffer of a module, and the
module's buffers as an injectable `noise=` tape."""
import numpy as np
import torch

from tacorl_amd import noise as N
from tests import noise_ref as R

SEED = 11
CASES = ("cql_q", "tacorl_q", "playlmp_dropout", "tacorl_d4rl_q")


def _cat(a, b, rows):
    if isinstance(a, dict):
        return {k: _cat(a[k], b[k], rows) for k in a}
    if torch.is_tensor(a) and a.dim() > 0:
        return torch.cat([a, b], dim=0)[:rows]
    return a


def golden(name):
    if name.startswith("tacorl_d4rl"):
        from tests import d4rl_cfg as K

        return K.D4rlGolden(name)
    from tests.golden_util import Golden

    return Golden(name)


def batches(name, steps, B=None):
    """`steps` batches out of the golden's two (alternating); B: that many samples out of [batch 0; batch 1]."""
    g = golden(name)
    two = [g.batch(0), g.batch(1)]
    if B is not None:
        two = [_cat(two[0], two[1], B), _cat(two[1], two[0], B)]
    return [two[i % 2] for i in range(steps)]


def build(name, seed=SEED, world_size=1, **over):
    """The module of a golden's configuration with its parameters loaded; seed None: torch's generator (the twin)."""
    from tests.test_step_gpu import ACTOR, CQL_YAML, CRITIC, build_tacorl

    g = golden(name)
    kw = dict(device_noise_seed=seed, world_size=world_size, **over)
    if name == "cql_q":  # B = 4 (the batches above), n = 2, the discrete gripper
        from tacorl_amd.modules.cql.cql_offline_lightning import CQL_Offline

        cams = sorted(g.cams)
        mod = CQL_Offline(actor=dict(ACTOR, discrete_gripper=True), critic=CRITIC, real_world=True, obs_modalities=cams,
                          goal_modalities=cams, action_dim=7, device="cuda:0", compute_dtype="f32",
                          **dict(CQL_YAML, **g.cfg.get("overrides", {}), n_action_samples=kw.pop("n_action_samples", 2)), **kw)
    elif name == "tacorl_q":
        mod = build_tacorl(g, **kw)
    elif name == "tacorl_d4rl_q":
        from tests.test_d4rl_modules_gpu import build_tacorl as build_d4rl

        mod = build_d4rl(g, **kw)
    else:
        from tacorl_amd.modules.play_lmp.play_lmp_for_rl import PlayLMP

        cams, c = sorted(g.cams), g.cfg
        pr = dict(num_heads=8, num_layers=2, encoder_hidden_size=2048, fc_hidden_size=4096, latent_plan_dim=c["latent"],
                  min_std=1e-4, dropout_p=c.get("dropout_p", 0.0), max_position_embeddings=c["T"])
        ad = dict(n_mixtures=10, num_layers=2, hidden_size=2048, out_features=7, num_classes=10, latent_plan_dim=c["latent"],
                  rnn_model="rnn_decoder", include_goal=False)
        mod = PlayLMP(plan_proposal=ACTOR, plan_recognition=pr, action_decoder=ad, plan_proposal_obs_modalities=cams,
                      plan_proposal_goal_modalities=cams, plan_recognition_modalities=cams, action_decoder_modalities=cams,
                      real_world=True, lr=1e-4, kl_beta=1e-3, device="cuda:0", compute_dtype="f32", **kw)
    mod.load_state_dict(g.params(), strict=False)
    if "epoch" in g.cfg:
        mod.current_epoch = g.cfg["epoch"]
    return mod


def noise_buffers(mod):
    """{name: (buffer, kind, draw id, n_outer, outer_major, keep_p)} of every noise buffer the module's step reads."""
    out = {}
    eng = getattr(mod, "engine", None)
    if eng is not None:
        for k, buf in {**eng.noise, **eng.extra_noise}.items():
            om = k in N.OUTER_MAJOR
            n_outer = buf.numel() // (eng.B * buf.shape[-1]) if om else 1
            out[k] = (buf, "uniform" if k[0] in "ug" else "normal", N.DRAW_IDS[k], n_outer, om, 0.0)
        return out
    for k, buf in mod.noise.items():
        out[k] = (buf, "uniform" if k[0] == "u" else "normal", N.DRAW_IDS[k], 1, False, 0.0)
    if getattr(mod, "_pr_train", False):
        for i, buf in enumerate(mod.pr.keep):
            out[f"dropout_{i}"] = (buf, "keep", N.dropout_id(i), 1, False, 1.0 - mod.pr.dropout_p)
    return out


def check_buffers(mod, B, seed, step, sample0=0):
    """Every noise buffer equals the restatement for (seed, step, draw id): uniforms and keep masks bit for bit, normals inside
    the fp32 bound.  Returns the buffers' clones (the tape for a twin, and what a resumed run must reproduce bit for bit)."""
    bufs, bad, got = noise_buffers(mod), [], {}
    assert bufs
    for k, (buf, kind, did, n_outer, om, p) in bufs.items():
        x = buf.detach().clone()
        got[k] = x
        inner = x.numel() // (B * n_outer)
        want = N.philox_restatement(seed, step, did, kind, B, inner, n_outer, sample0, om, p).reshape(-1)
        have = x.cpu().numpy().reshape(-1)
        if kind == "normal":
            if not (np.abs(have.astype(np.float64) - want) <= R.normal_bound(want)).all():
                bad.append(f"{k}: a normal outside the bound")
        elif not (have.astype(np.float64) == want.astype(np.float64)).all():
            bad.append(f"{k}: {kind} differs from the restatement")
    assert not bad, f"step {step}: " + "; ".join(bad)
    return got


def as_tape(mod, bufs, B, T=None):
    """The buffers in the layouts the `noise=` argument takes (dropout masks: the reference's - activations (T, B, *))."""
    tape = {k: v for k, v in bufs.items() if not k.startswith("dropout_")}
    masks = [bufs[k] for k in sorted((k for k in bufs if k.startswith("dropout_")), key=lambda s: int(s.split("_")[1]))]
    if masks:
        pr = mod.pr
        tape["dropout"] = [m.view(B, pr.H, T, T) if i % 4 == 1 else m.view(B, T, -1).permute(1, 0, 2) for i, m in enumerate(masks)]
    return tape


def snapshot(mod):
    return {k: v.detach().clone() for k, v in mod.state_dict().items()}, dict(mod.logged)
