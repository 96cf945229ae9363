"""The perceptual-encoder stage of a training step, stated once for the actor-critic step (engine.py), the relay-imitation
step (modules/relay_imitation_learning/engine.py) and the PlayLMP step (modules/play_lmp/play_lmp_for_rl.py): which
kernels apply, the packed conv weights, which cameras share a launch, and the forward / backward dispatch.  It begins at the
NHWC image buffers that image_ingest.py fills.

An encoder problem is the 7-tuple (image pointer, parameter block, out, act, images, needs_backward, camera); a parameter
block is anything with `.param` (the flat fp32 tensor) and `.enc(camera[, flat])` (address of that camera's encoder in it).
Nothing here computes anything: it decides which entry point of the library runs over which problems.
"""
import torch

from . import ops
from ._lib import BF16, F32, call

EF_MAXP = 16  # problems of one fused forward launch (the kernel's problem table)
EBW_MAXP = 8  # problems of one fused backward launch sequence


def image_flag(img_dtype):
    return BF16 if img_dtype == torch.bfloat16 else F32


# ------------------------------------------------------------- 1. which kernels apply
def fused_fwd_ok(hw, compute, img_dtype):
    """The fused single-launch forward: bf16 images + bf16 MFMA + a templated camera geometry."""
    return compute == BF16 and img_dtype == torch.bfloat16 and bool(ops.L.lib().tacorl_encoder_fused_supported(*hw))


def fused_bwd_ok(hw, compute, img_dtype, n_imgs):
    """The per-image LDS-resident conv backward over problems of n_imgs images each.  It may exist for fewer geometries than
    the fused forward; where it does not, the problems that have a backward take the per-layer path."""
    return fused_fwd_ok(hw, compute, img_dtype) and ops.L.lib().tacorl_encoder_bwd_fused_ws_bytes(
        len(n_imgs), ops.int_array(n_imgs), *hw) > 0


def fused_saves(hw, compute, img_dtype, n_imgs):
    """Does the fused forward leave activations that this backward can read?  (Act format 2 - a geometry of encoder_ring.hip
    without the LDS-resident backward: the fused launch saves fp32 activations, which the per-layer backward reads.)"""
    return fused_bwd_ok(hw, compute, img_dtype, n_imgs) or (
        fused_fwd_ok(hw, compute, img_dtype) and ops.L.lib().tacorl_encoder_fused_act_format(*hw) == 2)


# ------------------------------------------------------------ 2. packed conv weights
class PackedWeights:
    """Packed conv weights of the fused encoder forward (bf16 MFMA fragments in the kernel's register order), one buffer per
    (parameter block, camera).

    The validity rule: a packed copy is current while the block's torch version counter (ops.touched) is the one recorded
    when it was packed.  A step packs the networks its optimiser moves BEHIND its Adam launch, at the end of the step - in
    the shadow of whatever else still runs there - instead of in front of the encoder forward at the head of the next step's
    chain; in front of a forward only what something else has written since is packed again (pack_stale), so frozen networks
    are packed once, not every step.  A captured graph replays that late pack but no python: after a replay the owner records
    it (written), and before one it asks whether something else wrote the parameters (stale) - then the graph is dropped."""

    def __init__(self, device):
        self.dev, self.buf, self.ver = device, {}, {}

    def buffer(self, blk, c):
        if (blk, c) not in self.buf:
            ops.note_alloc()
            self.buf[(blk, c)] = torch.empty(ops.L.lib().tacorl_encoder_fused_wpk_bytes(), dtype=torch.uint8, device=self.dev)
        return self.buf[(blk, c)]

    def pack(self, pairs):
        """One pack launch over the (block, camera) pairs, whatever their stamps say."""
        pairs = list(pairs)
        if not pairs:
            return
        call("tacorl_encoder_pack_weights", len(pairs), ops.ptr_array([b.enc(c) for b, c in pairs]),
             ops.ptr_array([self.buffer(b, c) for b, c in pairs]), ops.stream())
        for b, c in pairs:
            self.ver[(b, c)] = b.param._version

    def pack_stale(self, pairs):
        self.pack([(b, c) for b, c in pairs if self.ver.get((b, c)) != b.param._version])

    def _packed(self, blocks, cams):
        return [(b, c) for b in blocks for c in cams if (b, c) in self.ver]

    def stale(self, blocks, cams):
        """Would a replayed step read a packed copy that no longer matches its parameter block?"""
        return any(self.ver[(b, c)] != b.param._version for b, c in self._packed(blocks, cams))

    def written(self, blocks, cams):
        """The step's tail launch (eager, or the replayed graph's) has just re-packed these blocks: record it."""
        for b, c in self._packed(blocks, cams):
            self.ver[(b, c)] = b.param._version


# ---------------------------------------------------------------- 3. geometry grouping
def geometry_groups(cams, hw, ok, n_problems, limit):
    """Cameras that share ONE launch (sequence): the cameras of one geometry for which ok(c) holds, when their problems
    together - n_problems(c) each - fit `limit` (EF_MAXP forward: C4's two 128 x 128 cameras, 7 problems each, are one launch
    over 5 504 images instead of two over 2 752, one prologue and one tail; EBW_MAXP backward: the conv-backward launches
    cost ~6-10 us each before their first image); every other camera alone.
    Two cases no compiled geometry reaches follow the actor-critic engine's rule: cameras with the fused forward but
    without the LDS-resident backward do not merge (pass the backward's predicate as ok), and a geometry whose cameras do
    not all fit the limit is not merged in part."""
    groups, out = {}, []
    for c in cams:
        groups.setdefault((tuple(hw[c]), bool(ok(c))), []).append(c)
    for (_, good), cs in groups.items():
        out += [cs] if good and sum(n_problems(c) for c in cs) <= limit else [[c] for c in cs]
    return out


# ---------------------------------------------------------------- 4. forward dispatch
def problem_src(x):
    """The optional 8th field of a problem: the device address of its fp32-source table entry (SourceTable), or None - its
    images are the packed NHWC buffer at x[0]."""
    return x[7] if len(x) > 7 else None


class SourceTable:
    """Device table of fp32 CHW sources that the fused forward converts itself (tacorl_encoder_fwd_fused_src): the launch -
    possibly a captured graph node - holds the address of an ENTRY, and `fill`, an eager launch in front of it, writes into
    the entry where this step's batch tensor lies.  Only forward-only problems of the 84 x 84 fused kernel qualify (`ok`)."""

    def __init__(self, device, n):
        self.esz = int(ops.L.lib().tacorl_encoder_src_entry_bytes())
        self.n, self.buf = n, torch.zeros(n * self.esz, dtype=torch.uint8, device=device)

    def entry(self, i):
        return self.buf.data_ptr() + i * self.esz

    @staticmethod
    def ok(base, img_pitch, hw):
        """base: device address; img_pitch in floats; the images themselves contiguous (3, H, W) fp32."""
        H, W = hw
        return bool(ops.L.lib().tacorl_encoder_src_supported(ops.C.c_void_p(base), img_pitch, H * W, W, H, W))

    def fill(self, sources, hw):
        """sources: [(base address, image pitch in floats)] for entries 0 .. len - 1."""
        H, W = hw
        n, Lg = len(sources), ops.C.c_long * len(sources)
        assert 0 < n <= self.n
        call("tacorl_encoder_src_fill", ops.ptr(self.buf), n, ops.ptr_array([b for b, _ in sources]), Lg(*[p for _, p in sources]),
             Lg(*[H * W] * n), Lg(*[W] * n), H, W, ops.stream())


class FrontTable:
    """TACORL's step front on the fp32-source route as one device table at a fixed address (tacorl_step_front): per camera
    the SourceTable entries [window | next], the pack jobs [obs; goal] of the engine cameras, the transition's sources and
    destinations.  A step's entries are a PLAN - (sources, jobs, disp, disp dtype code, reward, done, B, action window source,
    destination, element count, (H, W)): sources [(base address, image pitch in floats)] with entry k = camera k // 2's
    [window | next][k % 2], jobs image_ingest.PackJob (src, pitch, dst, n), every pointer a raw device address (None: absent).
    `accept` validates and assembles a plan on the host, `commit` issues the ONE fill launch only when the assembled bytes
    differ from the bytes last written (`shadow`; the owner drops it - `invalidate` - where it reallocates or changes route):
    the table holds addresses, sources and destinations alike, and the contents behind them are read by `launch` - a
    captured graph node - every step."""

    def __init__(self, device):
        L = ops.L.lib()
        self.nbytes, self.esz = int(L.tacorl_step_front_table_bytes()), int(L.tacorl_encoder_src_entry_bytes())
        offs = (ops.C.c_long * 15)()
        call("tacorl_step_front_offsets", offs)
        self.src_off = int(offs[0])
        self.buf = torch.zeros(self.nbytes, dtype=torch.uint8, device=device)
        self.host = ops.C.create_string_buffer(self.nbytes)
        self.plan = self.bytes = self.shadow = self.grid = None

    def entry(self, cam, which):
        """Device address of camera number `cam`'s source entry: which = 0 the window's frames, 1 the next observations."""
        return self.buf.data_ptr() + self.src_off + (2 * cam + which) * self.esz

    def invalidate(self):
        self.shadow = None

    def accept(self, plan):
        """Does the table take this plan (tacorl_step_front_supported's rules)?  Then its bytes are kept for `commit`.  Pure
        host; a plan equal to the last accepted one costs a tuple comparison."""
        if plan != self.plan:
            sources, jobs, disp, disp_dtype, reward, done, B, acts_src, acts_dst, n_acts, hw = plan
            Ls, Lj = ops.C.c_long * len(sources), ops.C.c_long * len(jobs)
            if ops.L.lib().tacorl_step_front_assemble(
                    self.host, len(sources), ops.ptr_array([b for b, _ in sources]), Ls(*[p for _, p in sources]), len(jobs),
                    ops.ptr_array([j.src for j in jobs]), Lj(*[j.pitch for j in jobs]), ops.ptr_array([j.dst for j in jobs]),
                    ops.int_array([j.n for j in jobs]), disp, disp_dtype, reward, done, B, acts_src, acts_dst, n_acts, *hw) != 0:
                return False
            self.plan, self.bytes = plan, self.host.raw
            self.grid = (len(jobs), max([j.n for j in jobs], default=0), B, n_acts, *hw)
        return True

    def commit(self):
        """The accepted plan onto the device table, on the current stream (behind the previous step's readers of the table).
        Returns whether a fill was issued."""
        if self.bytes == self.shadow:
            return False
        call("tacorl_step_front_fill", ops.ptr(self.buf), self.bytes, ops.stream())
        self.shadow = self.bytes
        return True

    def launch(self):
        """The front of the step over the table as it stands (graph-capturable)."""
        call("tacorl_step_front", ops.ptr(self.buf), *self.grid, ops.stream())


def launch_fused(pr, packs, hw, max_wg=0):
    """One fused encoder launch over the problems pr (each carries its camera: cameras of one geometry may share a launch)
    on at most max_wg workgroups (0: one per CU); activations are saved only for the problems a backward follows."""
    srcs = [problem_src(x) for x in pr]
    if any(srcs):  # fp32 CHW sources (problem_src): the same launch, the kernel converts those problems' images itself
        assert not any(s_ and x[5] for s_, x in zip(srcs, pr)), "a problem with a backward reads the packed image"
        call("tacorl_encoder_fwd_fused_src", len(pr), ops.ptr_array([x[0] for x in pr]), ops.ptr_array(srcs),
             ops.ptr_array([packs.buffer(x[1], x[6]) for x in pr]), ops.ptr_array([x[1].enc(x[6]) for x in pr]),
             ops.ptr_array([x[2] for x in pr]), ops.ptr_array([x[3] if x[5] else None for x in pr]),
             ops.int_array([x[4] for x in pr]), *hw, int(max_wg), ops.stream())
        return
    call("tacorl_encoder_fwd_fused_wg", len(pr), ops.ptr_array([x[0] for x in pr]),
         ops.ptr_array([packs.buffer(x[1], x[6]) for x in pr]), ops.ptr_array([x[1].enc(x[6]) for x in pr]),
         ops.ptr_array([x[2] for x in pr]), ops.ptr_array([x[3] if x[5] else None for x in pr]),
         ops.int_array([x[4] for x in pr]), *hw, int(max_wg), ops.stream())


def encode(groups, problems, hw, compute, img_dtype, packs, fused, saves, launch, pack_per_camera=True, per_layer_last=False):
    """Every encoder forward of the camera groups: per group ONE fused launch - launch(first camera, problems) - over the
    problems it takes, in front of it a pack of what is stale; the per-layer path for the cameras fused(c) does not hold for
    (fp32 mode, no templated geometry) and for the problems whose backward could not read the fused launch's activations
    (saves(c) false).  problems(c): the 7-tuples of camera c.
    The two steps' launch orders are kept as they were measured: pack_per_camera - one pack launch per camera (several
    blocks) or one per group (one block); per_layer_last - the per-layer launches behind every fused launch, or in line."""
    def per_layer(pr):
        for c in dict.fromkeys(x[6] for x in pr):
            prc = [x for x in pr if x[6] == c]
            call("tacorl_encoder_fwd", len(prc), ops.ptr_array([x[0] for x in prc]), ops.ptr_array([x[1].enc(c) for x in prc]),
                 ops.ptr_array([x[2] for x in prc]), ops.ptr_array([x[3] for x in prc]), ops.int_array([x[4] for x in prc]),
                 *hw[c], image_flag(img_dtype), compute, ops.stream())

    slow = []
    for cs in groups:
        pr = [x for c in cs for x in problems(c)]
        if fused(cs[0]):
            unsaved = lambda x: x[5] and not saves(x[6])  # noqa: E731
            slow += [x for x in pr if unsaved(x)]
            pr = [x for x in pr if not unsaved(x)]
            pairs = list(dict.fromkeys((x[1], x[6]) for c in cs for x in pr if x[6] == c))
            for part in ([[p for p in pairs if p[1] == c] for c in cs] if pack_per_camera else [pairs]):
                packs.pack_stale(part)
            launch(cs[0], pr)
        else:
            slow += pr
        if not per_layer_last:
            per_layer(slow)
            slow = []
    per_layer(slow)
