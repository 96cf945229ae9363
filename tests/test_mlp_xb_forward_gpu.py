"""The many-row fused MLP forward writes the weight gradients' layer-0 bf16 operand (tacorl_mlp_fwd_fused_gather_xb): the
[Mp][128] image mlp_x_to_bf16_kernel otherwise converts from the fp32 rows with a launch of its own behind the backward chain.

Two problems of the Q head (71 -> 256 -> 256 -> 256 -> 1, SiLU) with 2088 and 2300 rows - the 32-row many-row kernels, Mp > M
for both - whose input is gathered from three segments (32 | 32 | 7 columns, the first two with a row modulo), ldx = 72.
  * every byte of each problem's [Mp][128] region equals bf16(x) zero-padded;
  * the weight gradients with "xb is current" (lean bit 1) equal, bit for bit, those of the call that converts x itself -
    and do not read x (it is NaN in that call);
  * the bit is refused for a workspace no forward was given.
The values of those gradients are tests/test_mlp_fp64_gpu.py's business (B2, against fp64)."""
import pytest
import torch

from tests import mlp_ref as R
from tests.test_mlp_fp64_gpu import _flat, _grad_views

pytestmark = pytest.mark.gpu

NAN = float("nan")
SITE, MS, MODS = "q_head", [2088, 2300], [261, 230]


def _dev():
    from tacorl_amd import _lib

    _lib.call("tacorl_hip_init", 0)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def run():
    from tacorl_amd import ops

    dev = _dev()
    probs = [R.problem(SITE, m, seed=i) for i, m in enumerate(MS)]
    dims, acts, ld = probs[0]["dims"], probs[0]["acts"], probs[0]["ld"]
    assert (dims[0], ld) == (71, 72)
    fl = [_flat(p, dev) for p in probs]
    flats, fb = [f[0] for f in fl], [f[1] for f in fl]
    segs, xs = [], []
    for p, mod in zip(probs, MODS):  # columns 0..31 and 32..63 repeat every `mod` rows; 64..70 per row, pitch 8
        M = p["M"]
        a, b = p["x"][:mod, :32].contiguous().to(dev), p["x"][:mod, 32:64].contiguous().to(dev)
        act = torch.full((M, 8), 3.0, device=dev)
        act[:, :7] = p["x"][:, 64:71].to(dev)
        segs.append([(a, 0, 32, 0, mod), (b, 0, 32, 32, mod), (act, 0, 8, 64, 0)])
        r = torch.arange(M, device=dev) % mod
        xs.append(torch.cat([a[r], b[r], act[:, :7]], 1))
    tag = "t_mlp_xb_forward"
    nb = ops.L.lib().tacorl_mlp_bwd_fused_ws_bytes(2, ops.int_array(MS), len(dims) - 1, ops.int_array(dims))
    ws = ops.workspace(nb, dev, tag)
    ws.fill_(0xFF)
    xb_ptr = ops.mlp_bwd_fused_xb(MS, dims, tag, dev)
    assert all(v is not None for v in xb_ptr) and ops.workspace(nb, dev, tag) is ws
    bufs = [torch.full((ops.mlp_act_layout(m, dims, acts)[2],), NAN, device=dev) for m in MS]
    x_out = [torch.full((m, ld), NAN, device=dev) for m in MS]
    assert ops.mlp_lean_ok(2, dims, ld, dims[-1], ld, 1)
    ops.mlp_fwd_gather(segs, x_out, ld, flats, fb, bufs, MS, dims, acts, lean=True, xb_out=xb_ptr)
    torch.cuda.synchronize()
    xb = []
    for m, ptr in zip(MS, xb_ptr):
        off, Mp = ptr - ws.data_ptr(), R.padded(m)
        xb.append(ws[off: off + Mp * 128 * 2].clone().view(torch.int16).view(Mp, 128))
    douts = [p["d_out"].to(dev).contiguous() for p in probs]
    NL = dims[-1]
    ops.mlp_bwd_fused_dgrad(flats, bufs, douts, NL, None, ld, MS, dims, acts, tag, lean=True)

    def wgrad(x, xb_current, tag_=tag):
        gr = [torch.full_like(f, NAN) for f in flats]
        ops.mlp_bwd_fused_wgrad(x, ld, bufs, douts, NL, gr, MS, dims, acts, tag_, lean=True, xb_current=xb_current)
        torch.cuda.synchronize()
        return gr

    return dict(dev=dev, xs=xs, x_out=x_out, xb=xb, wgrad=wgrad, ld=ld, ws=ws, xb_ptr=xb_ptr)


def test_forward_writes_the_whole_bf16_image(run):
    for p, (M, x) in enumerate(zip(MS, run["xs"])):
        Mp = R.padded(M)
        assert Mp > M
        exp = torch.zeros(Mp, 128, dtype=torch.bfloat16, device=run["dev"])
        exp[:M, :71] = x.to(torch.bfloat16)
        assert torch.equal(run["xb"][p], exp.view(torch.int16)), p
        assert torch.equal(run["x_out"][p][:, :71], x) and bool((run["x_out"][p][:, 71:] == 0).all()), p


def test_gradients_with_and_without_the_conversion_launch(run):
    poison = [torch.full_like(x, NAN) for x in run["x_out"]]
    with_bit = run["wgrad"](poison, True)      # reads the forward's image, never x
    image = [run["ws"][ptr - run["ws"].data_ptr():][: R.padded(m) * 256].clone() for m, ptr in zip(MS, run["xb_ptr"])]
    converted = run["wgrad"](run["x_out"], False)  # converts x itself, as before
    for p in range(len(MS)):
        for g in (with_bit[p], converted[p]):  # (the block's alignment gaps keep their NaN prefill)
            v = _grad_views(g, R.SITES[SITE][0])
            assert all(torch.isfinite(t).all() for t in v["dW"] + v["db"]), p
        assert torch.equal(with_bit[p].view(torch.int32), converted[p].view(torch.int32)), p
        now = run["ws"][run["xb_ptr"][p] - run["ws"].data_ptr():][: R.padded(MS[p]) * 256]
        assert torch.equal(now, image[p]), "the conversion launch writes the image the forward wrote"
    # a weight-gradient call uses the forward's image up: the bit needs a new forward of that entry
    from tacorl_amd._lib import TacorlHipError

    with pytest.raises(TacorlHipError, match=r"\(-22\)"):
        run["wgrad"](run["x_out"], True)


def test_the_bit_is_refused_for_a_workspace_no_forward_wrote(run):
    from tacorl_amd._lib import TacorlHipError

    with pytest.raises(TacorlHipError, match=r"\(-22\)"):
        run["wgrad"](run["x_out"], True, "t_mlp_xb_forward_other")
