"""FrameIngest and the policies' `embeddings=` way in, on the GPU: 84 x 84 networks fed from 100 x 100 uint8 frames of
tests/rollout_envs.py GridImageEnv, R in {1, 3, 4}, plan_duration 4, episodes of at most 2 * 4 + 1 steps.

  * packed images: bit-identical to what a resident replay's validation batch holds for the same frames - the frames through
    tacorl_resize_frames_u8 (the replay's store_size stage) and the uint8 pack, in place and by frame index;
  * f32 / per-layer route: embeddings bit-identical to perceptual_encoder.get_state_from_observation on the equivalent fp32
    images; bf16 fused route: against the per-layer bf16 route inside FUSED_VS_PER_LAYER;
  * a row's embedding is the same bits alone and among R; goal embeddings are kept per row until that row is reset;
  * embeddings follow a training step (PackedWeights' version rule on the fused route);
  * RLPolicy against rl_policy_restatement; LatentPlanPolicy / RelayPolicy with embeddings= against their image path."""
import numpy as np
import pytest
import torch

from tests import cfg_util as C
from tests import d4rl_cfg as K
from tests import ril_util as U
from tests import rollout_envs as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAM, SRC, HW = "rgb_static", (100, 100), (84, 84)
# tests/test_kernels_gpu.py test_encoder_fused_forward: relerr(fused, generic bf16) < 1e-2 ("vs generic bf16")
FUSED_VS_PER_LAYER = 1e-2
RTOL = 1e-4  # tests/test_vec_policy_gpu.py: a policy's actions against its restatement, relative


def _tm(cams=(CAM,), size=HW):
    lst = [{"_target_": "torchvision.transforms.Resize", "size": list(size)}, {"_target_": "tacorl.utils.transforms.ScaleImageTensor"},
           {"_target_": "torchvision.transforms.Normalize", "mean": [0.5], "std": [0.5]}]
    return {"transforms": {"validation": {c: list(lst) for c in cams}, "train": {c: list(lst) for c in cams}}}


def _relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _lmp(route, seed=5):
    torch.manual_seed(seed)
    dt = {"f32": "f32", "bf16": "bf16"}[route]
    mod = K.build(C.playlmp_cfg(device=DEV, compute_dtype=dt, image_dtype=dt))
    mod.eval()
    return mod


@pytest.fixture(scope="module")
def lmp_f32():
    return _lmp("f32")


@pytest.fixture(scope="module")
def lmp_bf16():
    return _lmp("bf16")


def _raw(R, shift=0, cams=(CAM,)):
    """R observations of R environments at different states (and different goals)."""
    out = []
    for r in range(R):
        env = E.GridImageEnv(seed=0, cams=cams, src_hw=SRC)
        out.append(env.reset(task_info={"task": sorted(E.TASKS)[r % 3], "index": r + shift}))
    return out


def _nchw(ingest, cam, lo, hi):
    """The packed images of rows [lo, hi) as the fp32 CHW tensors a caller of the image path would hand over."""
    return ingest.images(cam)[lo:hi].float().permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------ packed images
@pytest.mark.parametrize("route", ["f32", "bf16"])
def test_packed_images_are_the_resident_replays_validation_batch(route, lmp_f32, lmp_bf16):
    from tacorl_amd import encoder_stage as stage
    from tacorl_amd import ops
    from tacorl_amd.evaluation.frame_ingest import FrameIngest

    mod, R = (lmp_f32 if route == "f32" else lmp_bf16), 3
    raw = _raw(R)
    ing = FrameIngest(mod, R, _tm())
    g_rows = ing.pack(raw)
    assert g_rows == [0, 1, 2] and ing.hw[CAM] == HW and ing.src_hw[CAM] == SRC
    frames = torch.from_numpy(np.stack([o["observation"][CAM] for o in raw] + [o["goal"][CAM] for o in raw])).to(DEV)
    stored = ops.resize_frames_u8(frames, torch.zeros(2 * R, *HW, 3, dtype=torch.uint8, device=DEV))  # the replay's store_size stage
    flag, H, W = stage.image_flag(mod.img_dtype), *HW
    want = torch.zeros(2 * R, H, W, 3, dtype=mod.img_dtype, device=DEV)
    ops.pack_images_u8_batch([(stored.data_ptr(), H * W * 3, want.data_ptr(), 2 * R)], flag, H, W)
    assert torch.equal(ing.images(CAM), want)
    idx = torch.arange(2 * R, device=DEV).flip(0).contiguous()  # by frame index, as the replay's fused validation batch reads
    want_g = torch.zeros_like(want)
    ops.pack_images_u8_gather_batch([(stored.data_ptr(), H * W * 3, want_g.data_ptr(), 2 * R, idx.data_ptr(), 1)], flag, H, W)
    assert torch.equal(ing.images(CAM), want_g.flip(0))
    # ScaleImageTensor and Normalize(0.5, 0.5) of the stored frame
    ref = (stored.float() / 255 - 0.5) / 0.5
    assert torch.allclose(ing.images(CAM).float(), ref, rtol=0, atol=2 ** -7 if route == "bf16" else 1e-6)
    assert ing.launches == {"copy_h2d": 1, "tacorl_resize_frames_u8": 1, "tacorl_pack_images_u8_batch": 1}


# ------------------------------------------------------------------------------------------ embeddings
def test_f32_route_embeddings_equal_the_image_path(lmp_f32):
    from tacorl_amd.evaluation.frame_ingest import FrameIngest

    mod, R = lmp_f32, 4
    ing = FrameIngest(mod, R, _tm())
    emb = ing.step(_raw(R))
    pe = mod.perceptual_encoder
    want = pe.get_state_from_observation(observation={CAM: _nchw(ing, CAM, 0, R)}, modalities=[CAM])
    want_goal = pe.get_state_from_observation(observation={CAM: _nchw(ing, CAM, R, 2 * R)}, modalities=[CAM])
    assert torch.equal(emb.obs["lmp"][CAM], want) and torch.equal(emb.goal["lmp"][CAM], want_goal)
    assert not torch.equal(want[0], want[1]) and "tacorl_encoder_fwd_fused_wg" not in ing.launches


def test_bf16_fused_route_against_the_per_layer_route(lmp_bf16):
    from tacorl_amd.evaluation.frame_ingest import FrameIngest

    mod, R = lmp_bf16, 4
    ing = FrameIngest(mod, R, _tm())
    emb = ing.step(_raw(R))
    assert ing.launches.get("tacorl_encoder_fwd_fused_wg") == 1  # observations and goals of the step: one launch
    pe = mod.perceptual_encoder  # EncoderRunner: the per-layer entry point, bf16 images and bf16 MFMA operands
    want = pe.get_state_from_observation(observation={CAM: _nchw(ing, CAM, 0, R)}, modalities=[CAM])
    want_goal = pe.get_state_from_observation(observation={CAM: _nchw(ing, CAM, R, 2 * R)}, modalities=[CAM])
    assert float(want.norm()) > 0 and float(want_goal.norm()) > 0 and not torch.equal(want[0], want[1])
    e1, e2 = _relerr(emb.obs["lmp"][CAM], want), _relerr(emb.goal["lmp"][CAM], want_goal)
    print(f"norms: per-layer {float(want.norm()):.6g}, fused {float(emb.obs['lmp'][CAM].norm()):.6g}; "
          f"values differ in {int((emb.obs['lmp'][CAM] != want).sum())} of {want.numel()}")
    print(f"fused against per-layer bf16: observations {e1:.3g}, goals {e2:.3g} (bound {FUSED_VS_PER_LAYER})")
    assert e1 < FUSED_VS_PER_LAYER and e2 < FUSED_VS_PER_LAYER


@pytest.mark.parametrize("route", ["f32", "bf16"])
@pytest.mark.parametrize("R", [3, 4])
def test_a_row_alone_and_among_R_is_the_same_bits(route, R, lmp_f32, lmp_bf16):
    from tacorl_amd.evaluation.frame_ingest import FrameIngest

    mod = lmp_f32 if route == "f32" else lmp_bf16
    raw = _raw(R)
    emb = FrameIngest(mod, R, _tm()).step(raw)
    one = FrameIngest(mod, 1, _tm())
    for r in range(R):
        one.reset()
        alone = one.step([raw[r]])
        assert torch.equal(alone.obs["lmp"][CAM][0], emb.obs["lmp"][CAM][r]), r
        assert torch.equal(alone.goal["lmp"][CAM][0], emb.goal["lmp"][CAM][r]), r


def test_goal_embeddings_are_cached_per_row_until_that_row_is_reset(lmp_f32):
    from tacorl_amd.evaluation.frame_ingest import FrameIngest

    mod, R = lmp_f32, 3
    ing = FrameIngest(mod, R, _tm())
    first, second = _raw(R), _raw(R, shift=5)  # other states AND other goals
    g0 = {k: v.clone() for k, v in ing.step(first).goal["lmp"].items()}
    assert ing.goal_valid == [True] * R and ing.launches["copy_h2d"] == 1
    e1 = ing.step(second)
    assert torch.equal(e1.goal["lmp"][CAM], g0[CAM])  # not recomputed: the new goal frames were not even copied
    obs1 = e1.obs["lmp"][CAM].clone()
    ing.reset([1])
    assert ing.goal_valid == [True, False, True]
    e2 = ing.step(second)
    fresh = FrameIngest(mod, R, _tm()).step(second)
    assert torch.equal(e2.goal["lmp"][CAM][1], fresh.goal["lmp"][CAM][1]) and not torch.equal(e2.goal["lmp"][CAM][1], g0[CAM][1])
    assert torch.equal(e2.goal["lmp"][CAM][0], g0[CAM][0]) and torch.equal(e2.goal["lmp"][CAM][2], g0[CAM][2])
    assert torch.equal(e2.obs["lmp"][CAM], obs1)
    mask = [False, False, True]
    ing.reset(mask)
    assert ing.goal_valid == [True, True, False]
    with pytest.raises(ValueError, match="goal"):
        FrameIngest(mod, 1, _tm()).step([first[0]["observation"]])  # a network that takes a goal, an observation without one


@pytest.mark.parametrize("route", ["f32", "bf16"])
def test_embeddings_follow_a_training_step(route):
    """One optimiser step between two evaluations: the second one's embeddings are the NEW weights' - those of an ingest built
    after the step, whose packed conv weights (fused route) were made from them."""
    from tacorl_amd import lightning as L
    from tacorl_amd import synth
    from tacorl_amd.evaluation.frame_ingest import FrameIngest

    mod, R = _lmp(route, seed=6), 3
    raw = _raw(R)
    ing = FrameIngest(mod, R, _tm())
    before = ing.step(raw).obs["lmp"][CAM].clone()
    again = ing.step(raw).obs["lmp"][CAM].clone()
    assert torch.equal(before, again)
    if route == "bf16":
        assert "tacorl_encoder_fwd_fused_wg" in ing.launches
    mod.train()
    L.MiniTrainer(max_epochs=1, max_steps=1).fit(mod, train_dataloaders=[synth.make_play_batch(50, 2, 16, {CAM: HW})])
    mod.eval()
    after = ing.step(raw).obs["lmp"][CAM].clone()
    fresh = FrameIngest(mod, R, _tm()).step(raw).obs["lmp"][CAM]
    assert not torch.equal(after, before) and torch.equal(after, fresh)


# ------------------------------------------------------------------------------------------ RLPolicy
def _cql(seed=7):
    torch.manual_seed(seed)
    mod = K.build(C.cql_cfg(device=DEV, compute_dtype="f32", image_dtype="f32"))
    mod.eval()
    return mod


@pytest.fixture(scope="module")
def cql():
    return _cql()


@pytest.mark.parametrize("use_cem", [False, True])
def test_rl_policy_against_its_restatement(use_cem, cql):
    """The restatement over the module's own surfaces, one row at a time (the reference manager's loop); CEM draws injected."""
    from tacorl_amd.evaluation.vec_policy import RLPolicy, rl_policy_restatement
    from tacorl_amd.modules.cem import CEMOptimizer

    mod, R, T = cql, 3, 3
    pol = RLPolicy(mod, R, use_cem=use_cem)
    g = torch.Generator().manual_seed(3)
    obs = [{CAM: torch.rand(R, 3, *HW, generator=g) * 2 - 1} for _ in range(T)]
    goal = [{CAM: torch.rand(R, 3, *HW, generator=g) * 2 - 1} for _ in range(T)]
    cem = CEMOptimizer(q1=mod.q1, q2=mod.q2, action_dim=7, discrete_gripper=True) if use_cem else None
    eps = [torch.randn(R, 4, 256, 7, generator=g) for _ in range(T)]
    row = lambda d, r: {c: v[r: r + 1] for c, v in d.items()}  # noqa: E731

    def actor_fn(o, gl, t):
        return torch.cat([mod.actor.get_actions({"observation": row(o, r), "goal": row(gl, r)}, deterministic=True,
                                                reparameterize=False)[0] for r in range(R)])

    def cem_fn(o, gl, mean, t):
        return torch.cat([cem.get_action({"observation": row(o, r), "goal": row(gl, r)}, initial_mean=mean[r: r + 1],
                                         noise={"eps": eps[t][r: r + 1]}) for r in range(R)])

    want = rl_policy_restatement(actor_fn, obs, goal, R, cem_fn=cem_fn if use_cem else None)
    for t in range(T):
        got = pol.step(obs[t], goal[t], noise={"cem_eps": eps[t]} if use_cem else None)
        assert got.shape == (R, 7) and bool((got[:, -1].abs() == 1).all())  # the discrete gripper: -1 or +1
        assert torch.equal(got[:, -1], want["actions"][t][:, -1])
        err = _relerr(got[:, :-1], want["actions"][t][:, :-1])
        assert err < RTOL, (t, err)
    if use_cem:
        assert not torch.equal(want["actions"][0], want["initial_mean"][0])


def test_rl_policy_on_vector_observations_and_embeddings(cql):
    from tacorl_amd.evaluation.frame_ingest import FrameIngest
    from tacorl_amd.evaluation.vec_policy import RLPolicy

    torch.manual_seed(2)
    vec = K.build(K.cql_d4rl_cfg(device=DEV))
    vec.eval()
    g = torch.Generator().manual_seed(4)
    obs, goal = torch.rand(4, 29, generator=g) * 2 - 1, torch.rand(4, 2, generator=g)
    a = RLPolicy(vec, 4).step(obs, goal)
    for r in range(4):
        one = vec.actor.get_actions(torch.cat([obs[r], goal[r]]).to(DEV), deterministic=True, reparameterize=False)[0]
        assert _relerr(a[r], one) < RTOL
    with pytest.raises(ValueError, match="vector observations"):
        RLPolicy(vec, 4).step(obs, goal, embeddings=object())
    # the image module through the ingest: bit-identical to the image path fed the same pixels
    R = 3
    raw = _raw(R)
    for use_cem in (False, True):
        ing = FrameIngest(cql, R, _tm(), use_cem=use_cem)
        pol = RLPolicy(cql, R, use_cem=use_cem)
        eps = torch.randn(R, 4, 256, 7, generator=g)
        got = pol.step(None, None, noise={"cem_eps": eps}, embeddings=ing.step(raw)).clone()
        want = pol.step({CAM: _nchw(ing, CAM, 0, R)}, {CAM: _nchw(ing, CAM, R, 2 * R)}, noise={"cem_eps": eps})
        assert torch.equal(got, want), use_cem
        assert [n for n, *_ in ing.nets] == (["actor", "q1"] if use_cem else ["actor"])


# ------------------------------------------------------------------------------------------ embeddings= against images
def _episode_frames(R, T):
    """T steps of R environments driven by a fixed action tape: raw[t] is the list of R observations."""
    envs = [E.GridImageEnv(seed=0, src_hw=SRC) for _ in range(R)]
    raw = [[env.reset(task_info={"task": sorted(E.TASKS)[r % 3], "index": r}) for r, env in enumerate(envs)]]
    for t in range(T - 1):
        raw.append([env.step(np.array([((t + r) % 3 - 1) / 3.0, ((t * r) % 3 - 1) / 3.0]))[0] for r, env in enumerate(envs)])
    return raw


def test_latent_plan_policy_with_embeddings_equals_the_image_path(lmp_f32):
    from tacorl_amd.evaluation.frame_ingest import FrameIngest
    from tacorl_amd.evaluation.vec_policy import LatentPlanPolicy

    mod, R, T, dur = lmp_f32, 3, 9, 4
    raw = _episode_frames(R, T)
    ing = FrameIngest(mod, R, _tm())
    p_emb, p_img = LatentPlanPolicy(mod, R, plan_duration=dur), LatentPlanPolicy(mod, R, plan_duration=dur)
    g, ad = torch.Generator().manual_seed(8), p_emb.ad
    draws = [dict(plan_eps=torch.randn(R, ad.P, generator=g), rand_a=torch.rand(R, ad.Da, ad.K, generator=g),
                  rand_b=torch.rand(R, ad.Da, generator=g)) for _ in range(T)]
    goal_img = torch.zeros(R, 3, *HW, device=DEV)
    for t in range(T):
        if t == 6:  # row 1 starts a new episode: its plan, its decoder state and its goal embedding begin again
            for x in (p_emb, p_img, ing):
                x.reset([1])
            raw[t][1] = dict(raw[t][1], goal=raw[t][2]["goal"])
        new_goal = [r for r in range(R) if not ing.goal_valid[r]]
        emb = ing.step(raw[t])
        if new_goal:
            goal_img[new_goal] = _nchw(ing, CAM, R, R + len(new_goal))
        a = p_emb.step(None, None, noise=draws[t], embeddings=emb).clone()
        b = p_img.step({CAM: _nchw(ing, CAM, 0, R)}, {CAM: goal_img}, noise=draws[t])
        assert torch.equal(a, b), t
        assert p_emb.clock.age == p_img.clock.age
    assert torch.equal(p_emb.plan, p_img.plan)
    with pytest.raises(ValueError, match="vector observations"):
        torch.manual_seed(1)
        vec = K.build(K.playlmp_d4rl_cfg(device=DEV, dropout_p=0.0))
        LatentPlanPolicy(vec, 2).step(None, None, embeddings=emb)


def test_tacorl_policy_with_cem_and_embeddings_equals_the_image_path():
    """TACORL with use_cem: three networks in the ingest (the actor's encoders, the frozen LMP encoder, q1's encoders); the plan
    of the rows that re-plan and every action are the image path's bits, CEM draws injected."""
    from tacorl_amd.evaluation.frame_ingest import FrameIngest
    from tacorl_amd.evaluation.vec_policy import LatentPlanPolicy
    from tacorl_amd.modules.tacorl.tacorl import TACORL

    strip = lambda c: {k: v for k, v in c.items() if k not in ("_target_", "_recursive_")}  # noqa: E731
    torch.manual_seed(9)
    f32 = dict(compute_dtype="f32", image_dtype="f32")
    lmp = K.build(C.playlmp_cfg(device=DEV, **f32))
    mod = TACORL(play_lmp=lmp, **strip(C.tacorl_cfg(device=DEV, finetune_action_decoder=False)), **f32)
    mod.eval()
    R, T, dur = 3, 5, 4
    raw = _episode_frames(R, T)
    ing = FrameIngest(mod, R, _tm(), use_cem=True)
    assert [n for n, *_ in ing.nets] == ["actor", "lmp", "q1"]
    p_emb, p_img = (LatentPlanPolicy(mod, R, plan_duration=dur, use_cem=True) for _ in range(2))
    g, ad, cem = torch.Generator().manual_seed(8), p_emb.ad, p_emb.cem
    goal_img = None
    for t in range(T):
        noise = dict(rand_a=torch.rand(R, ad.Da, ad.K, generator=g), rand_b=torch.rand(R, ad.Da, generator=g),
                     cem_eps=torch.randn(R, cem.num_iterations, cem.batch_size, cem.action_dim, generator=g))
        emb = ing.step(raw[t])
        if t == 0:
            goal_img = _nchw(ing, CAM, R, 2 * R)
        a = p_emb.step(None, None, noise=noise, embeddings=emb).clone()
        b = p_img.step({CAM: _nchw(ing, CAM, 0, R)}, {CAM: goal_img}, noise=noise)
        assert torch.equal(a, b), t
        assert torch.equal(p_emb.plan, p_img.plan) and bool((p_emb.plan.abs() <= 1).all())
    assert ing.launches.get("tacorl_encoder_fwd_fused_wg") is None  # f32: the per-layer entry point


def test_relay_policy_with_embeddings_equals_the_image_path():
    from tacorl_amd.evaluation.frame_ingest import FrameIngest
    from tacorl_amd.evaluation.vec_policy import RelayPolicy
    from tacorl_amd.modules.relay_imitation_learning.relay_imitation_learning import RelayImitationLearning

    cams = ("rgb_static", "rgb_gripper")
    torch.manual_seed(11)
    mod = RelayImitationLearning(device=DEV, **U.ril_cfg(low=list(cams), high=list(cams)[::-1], num_layers=2, hidden_dim=72))
    mod.eval()
    R, T, dur = 4, 6, 4
    envs = [E.GridImageEnv(seed=0, cams=cams, src_hw=SRC) for _ in range(R)]
    raw = [env.reset(task_info={"task": sorted(E.TASKS)[r % 3], "index": r}) for r, env in enumerate(envs)]
    ing = FrameIngest(mod, R, _tm(cams))
    p_emb, p_img = RelayPolicy(mod, R, plan_duration=dur), RelayPolicy(mod, R, plan_duration=dur)
    goal_img = None
    for t in range(T):
        emb = ing.step(raw)
        if t == 0:
            goal_img = {c: _nchw(ing, c, R, 2 * R) for c in cams}
            # both cameras share the 84 x 84 geometry: the per-layer route still takes each camera's problems in one call
        a = p_emb.step(None, None, embeddings=emb).clone()
        b = p_img.step({c: _nchw(ing, c, 0, R) for c in cams}, goal_img)
        assert torch.equal(a, b), t
        raw = [env.step(a[r].cpu().numpy())[0] for r, env in enumerate(envs)]
