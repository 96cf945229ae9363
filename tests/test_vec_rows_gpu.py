"""tacorl_vec_rows - the vector-observation step's row assembly (csrc/rl_ops.hip: the policy rows [state | goal] of obs and
next, the Q rows [state | goal | action] of XQ, XQpi and XT, one launch) - bit for bit against torch indexing, the bf16 mirrors
against torch's round-to-nearest-even conversion.  Every pad column up to the leading dimension is exactly 0; canary values in
front of and behind every output buffer are intact; a block whose pointer is NULL is not written.

Shapes: the D4RL one (S, G, A) = (29, 2, 16) - lds 32, ldq 48, one pad column each - and a ragged (5, 2, 3) - lds 8, ldq 12 -
at B 1 and 3, n 1 and 4, and one B whose item count exceeds a single launch's grid (tacorl_vec_rows_max_blocks() workgroups of
256 threads, one thread per row and four columns), so that the grid-stride loop runs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EINVAL = -22
CANARY, GUARD = -7.25, 64  # (exact in bf16 too)


def _dev():
    from tacorl_amd import _lib

    _lib.call("tacorl_hip_init", 0)
    return torch.device("cuda:0")


def _al4(x):
    return (x + 3) // 4 * 4


def _expected(obs, goal, acts_main, act_pi, act_next, n, lds, ldq):
    """The five blocks by torch indexing (reference tacorl_d4rl.py:68-89 get_rl_batch, cql_offline_lightning_d4rl.py:160-200
    expand_obs: sample-major rows k B + b)."""
    pad = lambda t, ld: torch.cat([t, torch.zeros(t.shape[0], ld - t.shape[1])], 1)  # noqa: E731
    s, nx = torch.cat([obs[:, 0], goal], 1), torch.cat([obs[:, -1], goal], 1)
    return [pad(s, lds), pad(nx, lds), pad(torch.cat([s.repeat(3 * n + 1, 1), acts_main], 1), ldq),
            pad(torch.cat([s, act_pi], 1), ldq), pad(torch.cat([nx, act_next], 1), ldq)]


def _guarded(rows, ld, dtype, dev):
    whole = torch.full((rows * ld + 2 * GUARD,), CANARY, dtype=dtype, device=dev)
    return whole, whole[GUARD: GUARD + rows * ld].view(rows, ld)


def _call(ins, outs, mirrors, B, T, S, G, A, n, lds, ldq):
    from tacorl_amd import _lib, ops

    ptrs = lambda ts: ops.ptr_array([None if t is None else t for t in ts])  # noqa: E731
    return _lib.lib().tacorl_vec_rows(*[ops.ptr(t) for t in ins], ptrs(outs), ptrs(mirrors) if mirrors is not None else None,
                                      B, T, S, G, A, n, lds, ldq, ops.stream())


def _inputs(B, T, S, G, A, n, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return r(B, T, S), r(B, G), r((3 * n + 1) * B, A), r(B, A), r(B, A)


def _grid_cap_B(S, G, A, n):
    """The smallest B (rounded up to an odd number) whose items exceed one grid: (3 n + 5) B rows x max(lds, ldq) / 4."""
    from tacorl_amd import _lib

    cap = _lib.lib().tacorl_vec_rows_max_blocks() * 256
    w4 = max(_al4(S + G), _al4(S + G + A)) // 4
    return (cap // ((3 * n + 5) * w4) + 1) | 1


CASES = [(*sga, B, n) for sga in ((29, 2, 16), (5, 2, 3)) for B in (1, 3) for n in (1, 4)] + [(5, 2, 3, "grid", 1)]


@pytest.mark.parametrize("S,G,A,B,n", CASES)
def test_vec_rows(S, G, A, B, n):
    dev = _dev()
    T = 8 if S == 29 else 3
    if B == "grid":
        from tacorl_amd import _lib

        B = _grid_cap_B(S, G, A, n)
        assert (3 * n + 5) * B * (max(_al4(S + G), _al4(S + G + A)) // 4) > _lib.lib().tacorl_vec_rows_max_blocks() * 256
    lds, ldq = _al4(S + G), _al4(S + G + A)
    cpu = _inputs(B, T, S, G, A, n, seed=B + S + n)
    ins = [t.to(dev) for t in cpu]
    want = _expected(*cpu, n, lds, ldq)
    rows = [B, B, (3 * n + 1) * B, B, B]
    f32 = [_guarded(r, ld, torch.float32, dev) for r, ld in zip(rows, (lds, lds, ldq, ldq, ldq))]
    b16 = [_guarded(r, ld, torch.bfloat16, dev) for r, ld in zip(rows, (lds, lds, ldq, ldq, ldq))]
    assert _call(ins, [v for _, v in f32], [v for _, v in b16], B, T, S, G, A, n, lds, ldq) == 0
    torch.cuda.synchronize()
    names = ("s_obs", "s_next", "xq", "xqpi", "xt")
    for name, (whole, view), (wb, vb), w in zip(names, f32, b16, want):
        got = view.cpu()
        assert torch.equal(got, w), f"{name}: {int((got != w).sum())} of {w.numel()} floats differ"
        assert torch.equal(vb.cpu(), w.to(torch.bfloat16)), f"{name}: the bf16 mirror is not torch's rounding of the rows"
        width = S + G + (A if name.startswith("x") else 0)
        assert width < w.shape[1] and float(got[:, width:].abs().max()) == 0.0 and float(vb[:, width:].float().abs().max()) == 0.0
        for t in (whole, wb):
            c = t.cpu().float()
            assert (c[:GUARD] == CANARY).all() and (c[-GUARD:] == CANARY).all(), f"{name}: a canary was overwritten"


def test_vec_rows_null_blocks_and_refusals():
    """Policy rows alone (the step's first phase), Q rows alone (its second), fp32 without mirrors: blocks whose pointer is NULL
    stay untouched.  Leading dimensions too narrow or no multiple of 4, a misaligned output, a Q block without its actions,
    B = 0: EINVAL before anything is launched."""
    dev = _dev()
    B, T, S, G, A, n = 3, 4, 5, 2, 3, 2
    lds, ldq = 8, 12
    cpu = _inputs(B, T, S, G, A, n, seed=11)
    ins = [t.to(dev) for t in cpu]
    want = _expected(*cpu, n, lds, ldq)
    rows = [B, B, (3 * n + 1) * B, B, B]
    for keep in ((0, 1), (2, 3, 4)):
        bufs = [_guarded(r, ld, torch.float32, dev) for r, ld in zip(rows, (lds, lds, ldq, ldq, ldq))]
        outs = [v if i in keep else None for i, (_, v) in enumerate(bufs)]
        assert _call(ins, outs, None, B, T, S, G, A, n, lds, ldq) == 0
        torch.cuda.synchronize()
        for i, ((whole, view), w) in enumerate(zip(bufs, want)):
            if i in keep:
                assert torch.equal(view.cpu(), w)
            else:
                assert (whole == CANARY).all()
    bufs = [_guarded(r, ld, torch.float32, dev) for r, ld in zip(rows, (lds, lds, ldq, ldq, ldq))]
    outs = [v for _, v in bufs]
    ok = dict(B=B, T=T, S=S, G=G, A=A, n=n, lds=lds, ldq=ldq)
    for bad in (dict(lds=4), dict(lds=10), dict(ldq=8), dict(ldq=14), dict(B=0), dict(T=0)):
        a = dict(ok, **bad)
        assert _call(ins, outs, None, *[a[k] for k in ("B", "T", "S", "G", "A", "n", "lds", "ldq")]) == EINVAL, bad
    assert _call(ins, [outs[0][:, 1:]] + outs[1:], None, *ok.values()) == EINVAL  # 4-byte aligned fp32 output
    assert _call(ins[:2] + [None] + ins[3:], outs, None, *ok.values()) == EINVAL  # XQ without acts_main
    torch.cuda.synchronize()
    for whole, _ in bufs:
        assert (whole == CANARY).all()
