"""PlanRecognitionTanhNetwork on HIP kernels (reference networks/plan_encoders/plan_recognition_tanh_net.py, selected by
config/networks/plan_recognition/tanh_net.yaml): a 2-layer bidirectional ReLU nn.RNN (batch_first, h0 = 0, both biases)
whose output at the last position, [B][2H], feeds mean_fc and variance_fc (2H -> A each); std = softplus(var) + min_std.

Parameters keep the reference's state-dict names (birnn_model.{weight_ih,weight_hh,bias_ih,bias_hh}_l{0,1}{,_reverse},
mean_fc.*, variance_fc.*); mean_fc and variance_fc are stored back to back so the two heads are one contraction.

Two exact prunings of the reference's computation:
  * only x[:, -1] reaches the heads, and layer 2's reverse direction produces position T-1 in its FIRST step, from the
    zero state: relu(W_ih_l1_reverse [h1f_{T-1} | h1r_{T-1}] + b_ih + b_hh).  Its other T-1 steps are never computed and
    weight_hh_l1_reverse gets a zero gradient (it never touches the output);
  * layer 2's forward direction needs layer 1's reverse output at every t, so layer 1 runs to completion first.
Chain: the input projection of layer 1 (both directions, one launch), T layer-1 steps (both directions in one launch per
step: times s and T-1-s), layer 2's input projection (one K = 2H GEMM over the interleaved [T][B][2H] layer-1 output),
T layer-2 forward steps, the heads.  The reverse step of layer 2 depends only on layer 1 and runs beside that chain.

Storage (fp32, time-major, a step's state is one [B][*] slab): y1 holds [T + 2] slabs of [B][2H] - slab t + 1 is time t
([fwd | rev] columns), slabs 0 and T + 1 stay zero: the h_{-1} of the forward and the h_T of the reverse direction, so
every step (and every weight gradient) is the same GEMM; y2 holds layer 2's forward state the same way ([T + 1] slabs of
[B][H], slab 0 zero), except that its last step writes straight into h2cat = [h2f_{T-1} | h2r] [B][2H], the heads' input.
bf16 (`_ring_ok`): the recurrence, both projections, the reverse step and the BPTT chains run on the LDS-DMA ring GEMM
(tacorl_rnn_linear_ld: row strides over the interleaved state, layer 1's input term as the K extension, the next step's bf16
operand written in the epilogue) and the square weight gradients on tacorl_rnn_wgrad(_batch) from those bf16 copies; the
narrow contractions (heads, d emb, the input weights of layer 1) and every shape the ring refuses take the generic GEMMs,
which are also the fp32 path.
"""
import ctypes as C

import torch

from .. import ops
from .._lib import ACT_NONE, ACT_RELU, BF16, call, ptr
from ..blocks import TensorBlock


class PlanRecognitionBiRNN:
    def __init__(self, state_dim, latent_plan_dim, device, hidden_dim=2048, min_std=1e-4, birnn_dropout_p=0.0,
                 trainable=True, **unused):
        if birnn_dropout_p:
            raise NotImplementedError("PlanRecognitionTanhNetwork: birnn_dropout_p > 0 is not implemented on the HIP path")
        self.D_in = self.D = state_dim
        self.Hd, self.A, self.latent_plan_dim, self.min_std = hidden_dim, latent_plan_dim, latent_plan_dim, min_std
        self.dropout_p = 0.0
        H, D, A = hidden_dim, state_dim, latent_plan_dim
        spec = []
        for l, din in ((0, D), (1, 2 * H)):
            for sfx in ("", "_reverse"):
                spec += [(f"birnn_model.weight_ih_l{l}{sfx}", (H, din)), (f"birnn_model.weight_hh_l{l}{sfx}", (H, H)),
                         (f"birnn_model.bias_ih_l{l}{sfx}", (H,)), (f"birnn_model.bias_hh_l{l}{sfx}", (H,))]
        spec += [("mean_fc.weight", (A, 2 * H)), ("variance_fc.weight", (A, 2 * H)), ("mean_fc.bias", (A,)),
                 ("variance_fc.bias", (A,))]
        self.blk = TensorBlock(spec, device, trainable=trainable)
        off = self.blk.off
        # (mean_fc | variance_fc back to back - one [2A][2H] matrix for the heads' input gradient - unless alignment padding
        # separates them: odd H * A)
        self._heads_stacked = off["variance_fc.weight"][0] == off["mean_fc.weight"][0] + 2 * H * A
        self.dev = device
        self._shape = None

    def _w(self, name, grad=False):
        return self.blk.g("birnn_model." + name) if grad else self.blk.p("birnn_model." + name)

    def _ensure(self, B, T):
        if self._shape == (B, T):
            return
        ops.note_alloc()
        f = lambda *s: torch.zeros(*s, device=self.dev)  # noqa: E731
        H, D = self.Hd, self.D
        self.embT = f(T * B, D)
        self.p1 = f(T * B, 2 * H)
        self.y1 = f((T + 2) * B, 2 * H)   # slabs 0 and T + 1: zero states, never written
        self.p2 = f(T * B, H)
        self.y2 = f((T + 1) * B, H)       # slab 0: zero state
        self.h2cat = f(B, 2 * H)
        self.bhh_r = f(B, H)
        self.head = f(B, 2 * self.A)
        self.y1b = self.y2b = self.xext = None  # (bf16 copies of the ring path: _ensure_ring)
        self._shape = (B, T)

    def _ensure_ring(self, B, T):
        if self.y1b is not None:
            return
        ops.note_alloc()
        bf = lambda *s: torch.zeros(*s, device=self.dev, dtype=torch.bfloat16)  # noqa: E731
        H = self.Hd
        self.y1b, self.y2b, self.xext = bf((T + 2) * B, 2 * H), bf((T + 1) * B, H), bf(T * B, 128)

    def stage_dropout(self, B, T, masks=None):
        """(no dropout sites: birnn_dropout_p is 0 on this path)"""

    def fused_inference_ok(self, T, ld_emb, compute):
        return False

    def _ring_ok(self, B, T, compute):
        """bf16 and a shape the ring GEMM takes: K = H and 2H multiples of 128, N = H of 64, D <= 128 (one K-extension tile),
        every weight 16-byte aligned in the bf16 mirror."""
        H, L = self.Hd, ops.L.lib()
        if compute != BF16 or self.D > 128 or H % 128:
            return False
        if any(o % 8 for o, _, _ in self.blk.off.values()):
            return False
        return bool(L.tacorl_rnn_linear_ld_supported(B, H, H, 2 * H, 2 * H) and L.tacorl_rnn_linear_ld_supported(T * B, 2 * H, H, 2 * H, H))

    def _wb(self, name):
        """Address of `birnn_model.<name>` in the bf16 mirror."""
        return self._pb.data_ptr() + 2 * self.blk.off["birnn_model." + name][0]

    def prepare_inference(self):
        """Weight-only preparation of the bf16 ring path: the bf16 mirror of the parameter block and layer 1's input weights
        as K-padded [H][128] extension operands.  Depends on nothing a step computes (a caller may issue it on a side stream)."""
        H, D, blk = self.Hd, self.D, self.blk
        if getattr(self, "_pb", None) is None:
            ops.note_alloc()
            self._pb = torch.zeros(blk.param.numel(), device=self.dev, dtype=torch.bfloat16)
            self._wext = [torch.zeros(H, 128, device=self.dev, dtype=torch.bfloat16) for _ in range(2)]
        call("tacorl_to_bf16_batch", 1, ops.ptr_array([blk.param]), ops.ptr_array([self._pb]),
             (C.c_long * 1)(blk.param.numel() // 4 * 4), ops.stream())
        for d, sfx in enumerate(("", "_reverse")):
            call("tacorl_pad_to_bf16", self._w("weight_ih_l0" + sfx), D, ptr(self._wext[d]), 128, H, D, ops.stream())

    _WT = (("weight_hh_l0", 1), ("weight_hh_l0_reverse", 1), ("weight_hh_l1", 1), ("weight_ih_l1", 2),
           ("weight_ih_l1_reverse", 2))  # (W^T operands of the bf16 BPTT: name, input width / H)

    def prepare_backward(self, B):
        """Weight-only preparation of the bf16 backward: W^T as bf16 for every ring BPTT / projection GEMM (one launch)."""
        H = self.Hd
        if getattr(self, "_wt", None) is None:
            ops.note_alloc()
            self._wt = {n: torch.zeros(k * H * H, device=self.dev, dtype=torch.bfloat16) for n, k in self._WT}
        call("tacorl_transpose_to_bf16_batch", len(self._WT), ops.ptr_array([self._w(n) for n, _ in self._WT]),
             ops.ptr_array([self._wt[n] for n, _ in self._WT]), ops.int_array([H] * len(self._WT)),
             ops.int_array([k * H for _, k in self._WT]), ops.stream())
        return True

    def _ring(self, xs, ldx, ws_, ys, ybs, ldy, M, K, N, act, bs=None, b2s=None, adds=None, ld_add=0, xexts=None, wexts=None,
              masks=None):
        arr = lambda v: ops.ptr_array(v) if v is not None else None  # noqa: E731
        call("tacorl_rnn_linear_ld", len(xs), ops.ptr_array(xs), ldx, ops.ptr_array(ws_), arr(bs), arr(b2s), arr(adds), ld_add,
             arr(xexts), arr(wexts), arr(masks), ops.ptr_array(ys), arr(ybs), ldy, M, K, N, act, ops.stream())

    # ------------------------------------------------------------------------ GEMM helpers (library entry points)
    def _fwd(self, xs, ldx, ws_, bs, adds, ld_add, ys, ldy, Ms, K, N, act, compute):
        n = len(xs)
        nb = ops.L.lib().tacorl_linear_add_fwd_ws_bytes(n, ops.int_array(Ms), K, N)
        ws = ops.workspace(nb, self.dev, "birnn_fwd")
        call("tacorl_linear_add_fwd", n, ops.ptr_array(xs), ldx, ops.ptr_array(ws_), ops.ptr_array(bs),
             ops.ptr_array(adds) if adds is not None else None, ld_add, ops.ptr_array(ys), ldy, ops.int_array(Ms), K, N, act,
             compute, ptr(ws), ws.numel(), ops.stream())

    def _dgrad(self, dzs, ld_dz, ws_, outs, ld_out, Ms, O, I, compute, srcs=None, ld_src=0, act=ACT_NONE, adds=None, ld_add=0):
        n = len(dzs)
        nb = ops.L.lib().tacorl_linear_dgrad_ws_bytes(n, ops.int_array(Ms), O, I)
        ws = ops.workspace(nb, self.dev, "birnn_dgrad")
        call("tacorl_linear_dgrad_splitk", n, ops.ptr_array(dzs), ld_dz, ops.ptr_array(ws_), ops.ptr_array(outs), ld_out,
             ops.ptr_array(srcs) if srcs is not None else None, ld_src, act,
             ops.ptr_array(adds) if adds is not None else None, ld_add, ops.int_array(Ms), O, I, compute,
             ptr(ws), ws.numel(), ops.stream())

    def _wgrad(self, xs, ldx, dzs, ld_dz, Ms, K, O, dws, dbs, compute):
        n = len(xs)
        nb = ops.L.lib().tacorl_linear_wgrad_ws_bytes(n, ops.int_array(Ms), K, O)
        ws = ops.workspace(nb, self.dev, "birnn_wgrad")
        call("tacorl_linear_wgrad", n, ops.ptr_array(xs), ldx, ops.ptr_array(dzs), ld_dz, ops.int_array(Ms), K, O,
             ops.ptr_array(dws), ops.ptr_array(dbs), 0, compute, ptr(ws), ws.numel(), ops.stream())

    # ------------------------------------------------------------------------ forward
    def forward(self, emb, ld_emb, B, T, compute, inference=False, sample=None, prepared=False, frozen=False, train=False):
        """emb: device tensor/pointer of [B*T][ld_emb] per-frame embeddings (batch-major rows b*T+t, first D columns used).
        Returns the (B, 2A) head buffer [mean | var_raw]; with sample=(eps, plan) also plan = tanh(mean + eps * std).
        bf16 ring path: prepared=True - prepare_inference() was already issued for the current weights; frozen=True - the
        weights only change through torch in-place ops, so the preparation is re-issued only when the parameter block's
        version counter moved (TACORL's frozen LMP).  (inference / train change nothing: no dropout on this network.)"""
        self._ensure(B, T)
        H, D, A, blk = self.Hd, self.D, self.A, self.blk
        emb_p = emb.data_ptr() if isinstance(emb, torch.Tensor) else (emb.value if hasattr(emb, "value") else int(emb))
        at = lambda base, floats: base + 4 * floats  # noqa: E731
        call("tacorl_birnn_swap_rows", emb_p, ld_emb, ptr(self.embT), D, B, T, D, ops.stream())
        self._ringed = self._ring_ok(B, T, compute)
        if self._ringed:
            ver = blk.param._version
            if not prepared and not (frozen and getattr(self, "_prep_version", None) == ver):
                self.prepare_inference()
            self._prep_version = ver if frozen else None
            self._forward_ring(B, T)
        else:
            self._forward_generic(B, T, compute)
        # mean_fc | variance_fc: one launch
        h2 = self.h2cat.data_ptr()
        self._fwd([h2, h2], 2 * H, [blk.p("mean_fc.weight"), blk.p("variance_fc.weight")],
                  [blk.p("mean_fc.bias"), blk.p("variance_fc.bias")], None, 0, [self.head.data_ptr(), at(self.head.data_ptr(), A)],
                  2 * A, [B, B], 2 * H, A, ACT_NONE, compute)
        if sample is not None:
            eps, plan = sample
            call("tacorl_pr_sample", ptr(self.head), ptr(eps), ptr(plan), None, None, B, A, float(self.min_std), ops.stream())
        return self.head

    def _forward_ring(self, B, T):
        """bf16: every step one ring-GEMM launch (layer 1: both directions, the input term as the K extension)."""
        self._ensure_ring(B, T)
        H = self.Hd
        S1, S2, SX = B * 2 * H, B * H, B * 128
        y1, y2, p2, h2 = self.y1.data_ptr(), self.y2.data_ptr(), self.p2.data_ptr(), self.h2cat.data_ptr()
        y1b, y2b, xe = self.y1b.data_ptr(), self.y2b.data_ptr(), self.xext.data_ptr()
        f4 = lambda base, n: base + 4 * n  # noqa: E731
        f2 = lambda base, n: base + 2 * n  # noqa: E731
        call("tacorl_pad_to_bf16", ptr(self.embT), self.D, xe, 128, T * B, self.D, ops.stream())
        wext = [t.data_ptr() for t in self._wext]
        for s in range(T):
            tr = T - 1 - s
            self._ring([f2(y1b, s * S1), f2(y1b, (tr + 2) * S1 + H)], 2 * H, [self._wb("weight_hh_l0"), self._wb("weight_hh_l0_reverse")],
                       [f4(y1, (s + 1) * S1), f4(y1, (tr + 1) * S1 + H)], [f2(y1b, (s + 1) * S1), f2(y1b, (tr + 1) * S1 + H)],
                       2 * H, B, H, H, ACT_RELU, bs=[self._w("bias_hh_l0"), self._w("bias_hh_l0_reverse")],
                       b2s=[self._w("bias_ih_l0"), self._w("bias_ih_l0_reverse")], xexts=[f2(xe, s * SX), f2(xe, tr * SX)],
                       wexts=wext)
        # layer 2 reverse (its one step: both biases in the epilogue), then the projection and the forward recurrence
        self._ring([f2(y1b, T * S1)], 2 * H, [self._wb("weight_ih_l1_reverse")], [f4(h2, H)], None, 2 * H, B, 2 * H, H, ACT_RELU,
                   bs=[self._w("bias_ih_l1_reverse")], b2s=[self._w("bias_hh_l1_reverse")])
        self._ring([f2(y1b, S1)], 2 * H, [self._wb("weight_ih_l1")], [p2], None, H, T * B, 2 * H, H, ACT_NONE,
                   bs=[self._w("bias_ih_l1")])
        for t in range(T):
            last = t == T - 1
            self._ring([f2(y2b, t * S2)], H, [self._wb("weight_hh_l1")], [h2 if last else f4(y2, (t + 1) * S2)],
                       None if last else [f2(y2b, (t + 1) * S2)], 2 * H if last else H, B, H, H, ACT_RELU,
                       bs=[self._w("bias_hh_l1")], adds=[f4(p2, t * S2)], ld_add=H)

    def _forward_generic(self, B, T, compute):
        H, D, blk = self.Hd, self.D, self.blk
        S1, S2 = B * 2 * H, B * H  # slab strides (floats) of y1 / p1 and of y2 / p2
        y1, p1, y2, p2 = self.y1.data_ptr(), self.p1.data_ptr(), self.y2.data_ptr(), self.p2.data_ptr()
        at = lambda base, floats: base + 4 * floats  # noqa: E731
        # layer 1 input projection, both directions: p1[t][b] = [x W_ih_l0^T + b_ih_l0 | x W_ih_l0r^T + b_ih_l0r]
        et = self.embT.data_ptr()
        self._fwd([et, et], D, [self._w("weight_ih_l0"), self._w("weight_ih_l0_reverse")],
                  [self._w("bias_ih_l0"), self._w("bias_ih_l0_reverse")], None, 0, [p1, at(p1, H)], 2 * H, [T * B, T * B], D,
                  H, ACT_NONE, compute)
        # layer 1 recurrence: step s = forward time s (state slab s -> s + 1) and reverse time T-1-s (slab T+1-s -> T-s)
        for s in range(T):
            tr = T - 1 - s
            self._fwd([at(y1, s * S1), at(y1, (tr + 2) * S1 + H)], 2 * H,
                      [self._w("weight_hh_l0"), self._w("weight_hh_l0_reverse")],
                      [self._w("bias_hh_l0"), self._w("bias_hh_l0_reverse")],
                      [at(p1, s * S1), at(p1, tr * S1 + H)], 2 * H,
                      [at(y1, (s + 1) * S1), at(y1, (tr + 1) * S1 + H)], 2 * H, [B, B], H, H, ACT_RELU, compute)
        # layer 2 reverse direction: its output at T-1 is its first step (zero state) - [B] rows, beside the chain below
        ops.copy_cols(blk.param, blk.off["birnn_model.bias_hh_l1_reverse"][0], H, self.bhh_r, 0, H, B, H, src_row_mod=1)
        self._fwd([at(y1, T * S1)], 2 * H, [self._w("weight_ih_l1_reverse")], [self._w("bias_ih_l1_reverse")],
                  [self.bhh_r.data_ptr()], H, [at(self.h2cat.data_ptr(), H)], 2 * H, [B], 2 * H, H, ACT_RELU, compute)
        # layer 2 input projection over the whole sequence: one K = 2H GEMM over the interleaved layer-1 output
        self._fwd([at(y1, S1)], 2 * H, [self._w("weight_ih_l1")], [self._w("bias_ih_l1")], None, 0, [p2], H, [T * B], 2 * H,
                  H, ACT_NONE, compute)
        # layer 2 forward recurrence; the last step writes h2f_{T-1} into the heads' input
        for t in range(T):
            last = t == T - 1
            self._fwd([at(y2, t * S2)], H, [self._w("weight_hh_l1")], [self._w("bias_hh_l1")], [at(p2, t * S2)], H,
                      [self.h2cat.data_ptr() if last else at(y2, (t + 1) * S2)], 2 * H if last else H, [B], H, H, ACT_RELU,
                      compute)

    # ------------------------------------------------------------------------ backward
    def backward(self, d_head, B, T, compute, wgrad_stream=None, prepared=False):
        """d_head: (B, 2A) gradient w.r.t. [mean | var_raw].  Fills self.blk.grad and returns the (B*T, D) gradient w.r.t.
        the input embeddings (batch-major rows b*T+t).  wgrad_stream: the weight gradients - read only by the optimiser -
        are issued on that stream beside the dependent input-gradient chain; the caller joins it.  Every buffer they read is
        written once per backward, before they are issued.  prepared: prepare_backward() was issued for the current weights."""
        H, D, A, blk = self.Hd, self.D, self.A, self.blk
        ring = bool(getattr(self, "_ringed", False))
        if getattr(self, "_bshape", None) != (B, T, ring):
            ops.note_alloc()
            f = lambda *s: torch.zeros(*s, device=self.dev)  # noqa: E731
            self.dz2cat = f(B, 2 * H)         # [dZ of h2f_{T-1} | dZ of h2r]
            self.dz2 = f(T * B, H)            # layer 2 forward dZ, time-major
            self.dr = f(B, 2 * H)             # the reverse step's input gradient onto y1 at T-1
            self.dy1 = f(T * B, 2 * H)        # gradient onto layer 1's interleaved output
            self.dz1 = f((T + 2) * B, 2 * H)  # layer 1 dZ, slab t + 1 = time t; slabs 0 and T + 1 stay zero
            self.dxt, self.dxt0, self.dx = f(T * B, D), f(T * B, D), f(B * T, D)
            self.dhead_tmp = f(B, 2 * H)
            if ring:  # bf16 copies the ring GEMMs read (dz1b: zero slabs as dz1)
                bf = lambda *s: torch.zeros(*s, device=self.dev, dtype=torch.bfloat16)  # noqa: E731
                self.dz2b, self.dz2rb, self.dz1b = bf(T * B, H), bf(B, H), bf((T + 2) * B, 2 * H)
            self._bshape = (B, T, ring)
        S1, S2 = B * 2 * H, B * H
        at = lambda base, floats: base + 4 * floats  # noqa: E731
        y1, dz2 = self.y1.data_ptr(), self.dz2.data_ptr()
        h2, dz2c, dh = self.h2cat.data_ptr(), self.dz2cat.data_ptr(), d_head.data_ptr()

        def side(fn):
            if wgrad_stream is None:
                return fn()
            wgrad_stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(wgrad_stream):
                fn()

        # heads: dZ at the last position, through the ReLU of both layer-2 directions
        if self._heads_stacked:
            self._dgrad([dh], 2 * A, [blk.p("mean_fc.weight")], [dz2c], 2 * H, [B], 2 * A, 2 * H, compute, srcs=[h2],
                        ld_src=2 * H, act=ACT_RELU)
        else:
            tmp = self.dhead_tmp.data_ptr()
            self._dgrad([dh], 2 * A, [blk.p("mean_fc.weight")], [tmp], 2 * H, [B], A, 2 * H, compute)
            self._dgrad([at(dh, A)], 2 * A, [blk.p("variance_fc.weight")], [dz2c], 2 * H, [B], A, 2 * H, compute, srcs=[h2],
                        ld_src=2 * H, act=ACT_RELU, adds=[tmp], ld_add=2 * H)
        side(lambda: self._wgrad([h2, h2], 2 * H, [dh, at(dh, A)], 2 * A, [B, B], 2 * H, A,
                                 [blk.g("mean_fc.weight"), blk.g("variance_fc.weight")],
                                 [blk.g("mean_fc.bias"), blk.g("variance_fc.bias")], compute))
        ops.copy_cols(self.dz2cat, 0, 2 * H, self.dz2, (T - 1) * S2, H, B, H)

        def rev_grads():  # layer 2 reverse step: W_ih from its [B] rows; b_hh = b_ih gradient; W_hh never touches the output
            self._wgrad([at(y1, T * S1)], 2 * H, [at(dz2c, H)], 2 * H, [B], 2 * H, H, [self._w("weight_ih_l1_reverse", True)],
                        [self._w("bias_ih_l1_reverse", True)], compute)
            ops.copy_cols(blk.grad, blk.off["birnn_model.bias_ih_l1_reverse"][0], H, blk.grad,
                          blk.off["birnn_model.bias_hh_l1_reverse"][0], H, 1, H)
            blk.grad_views["birnn_model.weight_hh_l1_reverse"].zero_()
        side(rev_grads)
        if ring:
            self._backward_ring(B, T, side, prepared)
        else:
            self._backward_generic(B, T, compute, side)
        et = self.embT.data_ptr()
        side(lambda: self._wgrad([et, et], D, [at(self.dz1.data_ptr(), S1), at(self.dz1.data_ptr(), S1 + H)], 2 * H, [T * B, T * B],
                                 D, H, [self._w("weight_ih_l0", True), self._w("weight_ih_l0_reverse", True)],
                                 [self._w("bias_ih_l0", True), self._w("bias_ih_l0_reverse", True)], compute))
        # input gradient (time-major), both directions, then back to the batch-major rows of the embeddings
        dz1 = self.dz1.data_ptr()
        self._dgrad([at(dz1, S1)], 2 * H, [self._w("weight_ih_l0")], [self.dxt0.data_ptr()], D, [T * B], H, D, compute)
        self._dgrad([at(dz1, S1 + H)], 2 * H, [self._w("weight_ih_l0_reverse")], [self.dxt.data_ptr()], D, [T * B], H, D,
                    compute)
        ops.copy_cols(self.dxt0, 0, D, self.dxt, 0, D, T * B, D, accumulate=True)
        call("tacorl_birnn_swap_rows", ptr(self.dxt), D, ptr(self.dx), D, T, B, D, ops.stream())
        return self.dx

    def _backward_ring(self, B, T, side, prepared):
        """bf16: the reverse step's input gradient, the BPTT of layer 2, the projection onto layer 1 and the BPTT of both layer-1
        directions (one launch per step) on the ring GEMM with W^T operands; square weight gradients from the bf16 copies."""
        H = self.Hd
        if not prepared:
            self.prepare_backward(B)
        S1, S2 = B * 2 * H, B * H
        f4 = lambda base, n: base + 4 * n  # noqa: E731
        f2 = lambda base, n: base + 2 * n  # noqa: E731
        y1, y2, dz1, dz2, dy1, dz2c = (t.data_ptr() for t in (self.y1, self.y2, self.dz1, self.dz2, self.dy1, self.dz2cat))
        y1b, y2b, dz1b, dz2b, dz2rb = (t.data_ptr() for t in (self.y1b, self.y2b, self.dz1b, self.dz2b, self.dz2rb))
        wt = {n: t.data_ptr() for n, t in self._wt.items()}
        call("tacorl_pad_to_bf16", ptr(self.dz2cat), 2 * H, f2(dz2b, (T - 1) * S2), H, B, H, ops.stream())
        call("tacorl_pad_to_bf16", f4(dz2c, H), 2 * H, dz2rb, H, B, H, ops.stream())
        self._ring([dz2rb], H, [wt["weight_ih_l1_reverse"]], [self.dr.data_ptr()], None, 2 * H, B, H, 2 * H, ACT_NONE)
        for t in range(T - 2, -1, -1):
            self._ring([f2(dz2b, (t + 1) * S2)], H, [wt["weight_hh_l1"]], [f4(dz2, t * S2)], [f2(dz2b, t * S2)], H, B, H, H,
                       ACT_NONE, masks=[f4(y2, (t + 1) * S2)])
        L = ops.L.lib()
        wg = bool(L.tacorl_rnn_wgrad_supported(T * B, self.Hd, 2 * self.Hd))

        def l2_grads():
            if wg:
                call("tacorl_rnn_wgrad", dz2b, H, f2(y1b, S1), 2 * H, T * B, H, 2 * H, self._w("weight_ih_l1", True),
                     self._w("bias_ih_l1", True), 0, ops.stream())
                call("tacorl_rnn_wgrad", dz2b, H, y2b, H, T * B, H, H, self._w("weight_hh_l1", True), self._w("bias_hh_l1", True), 0,
                     ops.stream())
            else:
                self._l2_wgrad_generic(B, T, BF16)
        side(l2_grads)
        self._ring([dz2b], H, [wt["weight_ih_l1"]], [dy1], None, 2 * H, T * B, H, 2 * H, ACT_NONE)
        ops.copy_cols(self.dr, 0, 2 * H, self.dy1, (T - 1) * S1, 2 * H, B, 2 * H, accumulate=True)
        for k in range(T):
            t = T - 1 - k
            self._ring([f2(dz1b, (t + 2) * S1), f2(dz1b, k * S1 + H)], 2 * H, [wt["weight_hh_l0"], wt["weight_hh_l0_reverse"]],
                       [f4(dz1, (t + 1) * S1), f4(dz1, (k + 1) * S1 + H)], [f2(dz1b, (t + 1) * S1), f2(dz1b, (k + 1) * S1 + H)],
                       2 * H, B, H, H, ACT_NONE, adds=[f4(dy1, t * S1), f4(dy1, k * S1 + H)], ld_add=2 * H,
                       masks=[f4(y1, (t + 1) * S1), f4(y1, (k + 1) * S1 + H)])

        def l1_grads():
            if wg:
                call("tacorl_rnn_wgrad_batch", 2, ops.ptr_array([f2(dz1b, S1), f2(dz1b, S1 + H)]), 2 * H,
                     ops.ptr_array([y1b, f2(y1b, 2 * S1 + H)]), 2 * H, ops.int_array([T * B, T * B]), H, H,
                     ops.ptr_array([self._w("weight_hh_l0", True), self._w("weight_hh_l0_reverse", True)]),
                     ops.ptr_array([self._w("bias_hh_l0", True), self._w("bias_hh_l0_reverse", True)]), 0, ops.stream())
            else:
                self._l1_wgrad_generic(B, T, BF16)
        side(l1_grads)

    def _l2_wgrad_generic(self, B, T, compute):
        H, S1 = self.Hd, B * 2 * self.Hd
        y1, y2, dz2 = self.y1.data_ptr(), self.y2.data_ptr(), self.dz2.data_ptr()
        self._wgrad([y1 + 4 * S1], 2 * H, [dz2], H, [T * B], 2 * H, H, [self._w("weight_ih_l1", True)],
                    [self._w("bias_ih_l1", True)], compute)
        # (W_hh pairs dZ_t with h_{t-1}: slab t of y2, slab 0 the zero state)
        self._wgrad([y2], H, [dz2], H, [T * B], H, H, [self._w("weight_hh_l1", True)], [self._w("bias_hh_l1", True)], compute)

    def _l1_wgrad_generic(self, B, T, compute):
        # W_hh: forward pairs dZ_t with h_{t-1} (slab t), reverse pairs dZ_t with h_{t+1} (slab t + 2)
        H, S1 = self.Hd, B * 2 * self.Hd
        y1, dz1 = self.y1.data_ptr(), self.dz1.data_ptr()
        at = lambda base, floats: base + 4 * floats  # noqa: E731
        self._wgrad([y1, at(y1, 2 * S1 + H)], 2 * H, [at(dz1, S1), at(dz1, S1 + H)], 2 * H, [T * B, T * B], H, H,
                    [self._w("weight_hh_l0", True), self._w("weight_hh_l0_reverse", True)],
                    [self._w("bias_hh_l0", True), self._w("bias_hh_l0_reverse", True)], compute)

    def _backward_generic(self, B, T, compute, side):
        H = self.Hd
        S1, S2 = B * 2 * H, B * H
        at = lambda base, floats: base + 4 * floats  # noqa: E731
        y2, dz1, dz2, dy1, dz2c = (t.data_ptr() for t in (self.y2, self.dz1, self.dz2, self.dy1, self.dz2cat))
        y1 = self.y1.data_ptr()
        # layer 2 reverse step: input gradient onto y1 at T-1
        self._dgrad([at(dz2c, H)], 2 * H, [self._w("weight_ih_l1_reverse")], [self.dr.data_ptr()], 2 * H, [B], H, 2 * H, compute)
        # layer 2 forward BPTT: dZ_t = (dZ_{t+1} W_hh) * [h_t > 0]
        for t in range(T - 2, -1, -1):
            self._dgrad([at(dz2, (t + 1) * S2)], H, [self._w("weight_hh_l1")], [at(dz2, t * S2)], H, [B], H, H, compute,
                        srcs=[at(y2, (t + 1) * S2)], ld_src=H, act=ACT_RELU)
        side(lambda: self._l2_wgrad_generic(B, T, compute))
        # gradient onto layer 1's output: dZ2 W_ih_l1 at every t, plus the reverse step's term at T-1
        if T > 1:
            self._dgrad([dz2], H, [self._w("weight_ih_l1")], [dy1], 2 * H, [(T - 1) * B], H, 2 * H, compute)
        self._dgrad([at(dz2, (T - 1) * S2)], H, [self._w("weight_ih_l1")], [at(dy1, (T - 1) * S1)], 2 * H, [B], H, 2 * H,
                    compute, adds=[self.dr.data_ptr()], ld_add=2 * H)
        # layer 1 BPTT, both directions per launch: forward time t = T-1-k (from t + 1), reverse time k (from k - 1)
        for k in range(T):
            t = T - 1 - k
            self._dgrad([at(dz1, (t + 2) * S1), at(dz1, k * S1 + H)], 2 * H,
                        [self._w("weight_hh_l0"), self._w("weight_hh_l0_reverse")],
                        [at(dz1, (t + 1) * S1), at(dz1, (k + 1) * S1 + H)], 2 * H, [B, B], H, H, compute,
                        srcs=[at(y1, (t + 1) * S1), at(y1, (k + 1) * S1 + H)], ld_src=2 * H, act=ACT_RELU,
                        adds=[at(dy1, t * S1), at(dy1, k * S1 + H)], ld_add=2 * H)
        side(lambda: self._l1_wgrad_generic(B, T, compute))
