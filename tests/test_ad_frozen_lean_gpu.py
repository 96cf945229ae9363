"""ActionDecoderLogistic.forward(frozen=True, bf16_state_only=True): the logging-only pass of TACORL writes only the bf16
hidden state - the next step's and the heads' operand - and no fp32 copy, which nobody but a backward reads.  Both forms pass a
NULL operand for h_{-1} = 0 at t = 0 (the ring GEMM skips its K tiles).  The heads must have the same bits, the launch log
the same length; a pass that a backward may follow still fills h."""
import pytest
import torch

from tests.test_action_decoder_gpu import Calls, _case, _dev, _module

pytestmark = pytest.mark.gpu

NAN = float("nan")
BF16 = 1
B, Tm, H, L, P, E = 8, 5, 256, 2, 16, 32
RING = ("tacorl_rnn_linear_fwd_batch_ext", "tacorl_rnn_linear_fwd_batch")


def _forward(ad, d, log, **kw):
    ad._ensure(B, Tm)
    ad.heads.fill_(NAN)
    for t in ad.h:
        t.fill_(NAN)
    for t in ad.hb:
        t[: B * Tm].view(torch.int16).fill_(-1)  # 0xFFFF: a bf16 NaN
    log.take()
    ad.forward(d["plan"], d["emb"], E, B, Tm + 1, Tm, BF16, **kw)
    torch.cuda.synchronize()
    return (ad.heads[:, :ad.NH].clone(), [t[: B * Tm].clone() for t in ad.hb], [t.clone() for t in ad.h], log.take())


def test_frozen_forward_without_fp32_state(monkeypatch):
    _dev()
    log = Calls(monkeypatch)
    W, _, d = _case(B, Tm, H, P, E, L, seed=5)
    ad = _module(H, P, E, L, W)
    _forward(ad, d, log, frozen=True)  # (the first frozen pass also refreshes the bf16 weight mirrors: two more calls)
    heads0, hb0, h0, log0 = _forward(ad, d, log, frozen=True)
    heads1, hb1, h1, log1 = _forward(ad, d, log, frozen=True, bf16_state_only=True)
    assert torch.isfinite(heads0).all()
    assert torch.equal(heads1.view(torch.int32), heads0.view(torch.int32))
    for l in range(L):
        assert torch.isfinite(hb0[l].float()).all() and torch.equal(hb1[l].view(torch.int16), hb0[l].view(torch.int16)), l
        assert torch.isfinite(h0[l]).all(), "the plain frozen pass fills h"
        assert torch.isnan(h1[l]).all(), "bf16_state_only: h is left as it was"
        assert torch.equal(hb0[l], h0[l].to(torch.bfloat16))
    assert len(log1) == len(log0)
    ring0, ring1 = [a for n, a in log0 if n in RING], [a for n, a in log1 if n in RING]
    assert len(ring0) == len(ring1) == Tm + 2 * (L - 1)
    # both forms: a NULL operand exactly for the recurrent problems at t = 0 (launch 0: layer 0; launch 2: layer 1)
    for ring in (ring0, ring1):
        nulls = [[not v for v in a[1]] for a in ring]
        assert nulls[0] == [True] and nulls[2][0] is False and sum(nulls[2]) == 1
        assert sum(sum(n) for n in nulls) == L
    # the recurrent problems (activation ReLU) carry no fp32 output, the projections (identity) keep theirs
    for a in ring1:
        n, ys, acts = a[0], a[8], a[16]
        assert [bool(ys[p]) for p in range(n)] == [acts[p] == 0 for p in range(n)]
    assert all(all(bool(v) for v in a[8]) for a in ring0)


def test_non_frozen_forward_still_fills_h(monkeypatch):
    _dev()
    log = Calls(monkeypatch)
    W, _, d = _case(B, Tm, H, P, E, L, seed=6)
    ad = _module(H, P, E, L, W)
    ref = _forward(ad, d, log)
    got = _forward(ad, d, log, bf16_state_only=True)  # (ignored unless frozen: a backward may follow)
    for l in range(L):
        assert torch.isfinite(got[2][l]).all() and torch.equal(got[2][l], ref[2][l])
    assert torch.equal(got[0], ref[0])
