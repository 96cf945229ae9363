"""Generate the bidirectional-RNN plan recognition fixtures (tests/golden/*birnn*.npz) by running the UNMODIFIED
reference on CPU with `plan_recognition=tanh_net` selected (config/networks/plan_recognition/tanh_net.yaml:
PlanRecognitionTanhNetwork, a 2-layer bidirectional ReLU nn.RNN, h = 2048).

Build container only (needs the reference tree, like oracle/gen_golden.py):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_birnn_golden.py            # all cases
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_birnn_golden.py playlmp_birnn

Nothing under oracle/ changes: the harness's plan-recognition config is swapped at runtime and the cases run through
oracle.gen_golden.run_case as they are.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import gen_golden as G  # noqa: E402
from oracle import ref_harness as H  # noqa: E402

CASES = {
    # PlayLMP seq-VAE step with the bi-RNN posterior (BASELINE config 1 shape, tiny batch)
    "playlmp_birnn": dict(kind="playlmp", B=3, T=16, cams={"rgb_static": (84, 84)}, latent=16, steps=2, seed=51,
                          plan_recognition="tanh_net"),
    # TACORL Q phase over a frozen LMP whose posterior is the bi-RNN
    "tacorl_birnn_q": dict(kind="tacorl", B=3, T=16, cams={"rgb_static": (84, 84)}, latent=16, epoch=5,
                           finetune_ad=False, steps=2, seed=52, plan_recognition="tanh_net"),
    # its validation step
    "val_tacorl_birnn": dict(kind="tacorl", B=3, T=16, cams={"rgb_static": (84, 84)}, latent=16, epoch=5,
                             finetune_ad=False, steps=1, seed=53, validate=True, plan_recognition="tanh_net"),
}


def tanh_net_cfg(latent_plan_dim, seq_len=None, dropout_p=0.0):
    """config/networks/plan_recognition/tanh_net.yaml with ${latent_plan_dim} resolved (seq_len: unused by this net)."""
    assert dropout_p == 0.0
    return {
        "_target_": H.P + "plan_encoders.plan_recognition_tanh_net.PlanRecognitionTanhNetwork",
        "state_dim": None,
        "latent_plan_dim": latent_plan_dim,
        "birnn_dropout_p": 0.0,
        "min_std": 0.0001,
    }


if __name__ == "__main__":
    H.pr_cfg = tanh_net_cfg
    which = sys.argv[1:] or list(CASES)
    for n in which:
        G.run_case(n, CASES[n])
