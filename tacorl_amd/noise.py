"""A step's noise as a pure function of (seed, step, draw id, global sample index, position inside the sample).

`tacorl_noise_fill` (csrc/noise_ops.hip) computes it on the GPU, one launch for all of a step's buffers; this file holds the
ONE table of draw ids, the builder of the kernel's segment table, the host-side generator state `DeviceNoise`, and
`philox_restatement`: the same function in NumPy integer / fp64 arithmetic (no torch import at module level, so the
CPU tests can use it).

Counter layout (Philox4x32-10, key = (seed & 0xffffffff, seed >> 32)):

    counter = (j >> 2, sample0 + b, draw_id << 16 | k, step)        element j of sample b, outer index k, takes word j & 3

so a rank that holds samples [sample0, sample0 + B_local) of the batch draws exactly the rows the one-rank step draws for them
(dist.py: noise is sharded by sample), and (seed, step) is the generator's whole state.
"""
import ctypes as C

import numpy as np

# Draw ids: APPEND ONLY - an id is part of every element's counter, so a changed id changes every run's noise.
DRAW_IDS = {
    "eps_pi": 0, "eps_next": 1, "eps_cur": 2, "eps_nxt": 3, "u_rand": 4,          # ACEngine: policy / CQL samples
    "g_pi": 5, "g_next": 6, "g_cur": 7, "g_nxt": 8,                                # ... discrete-gripper Gumbel uniforms
    "eps_pr": 9,                                                                   # TACORL: the plan-recognition sample
    "eps_plan": 10, "u_plan": 11,                                                  # PlayLMP: posterior sample, random plan
    # rollouts (RowNoise; 96 = DROPOUT_BASE + DROPOUT_MAX): the decoder's mixture uniforms, the sampled plan, CEM's population
    "ro_rand_a": 96, "ro_rand_b": 97, "ro_plan": 98, "ro_cem": 99,
}
# The plan recognition's keep masks in the reference's order: [embedding] + per layer [attention, dropout1, ffn, dropout2]
# -> ids DROPOUT_BASE + i (i < DROPOUT_MAX; a 15-layer transformer fits).  The rollout ids follow them; the next free id is 100.
# (PlayLMP's training step samples nothing from the action decoder - its logging pass is a loss - so no ids for that.)
DROPOUT_BASE, DROPOUT_MAX = 32, 64

NORMAL, UNIFORM, KEEP = 0, 1, 2
MAX_SEGS = 64
_KINDS = {"normal": NORMAL, "uniform": UNIFORM, "keep": KEEP}
# draws whose buffers are (n_outer, B, inner) - outer-major; every other one is (B, inner) (keep masks: batch-major)
OUTER_MAJOR = ("eps_cur", "eps_nxt", "g_cur", "g_nxt", "u_rand")


def dropout_id(i):
    if not 0 <= i < DROPOUT_MAX:
        raise ValueError(f"dropout mask {i}: ids for {DROPOUT_MAX} masks are reserved")
    return DROPOUT_BASE + i


class Segment:
    """One destination buffer of a fill: n_outer x B_local x inner elements at `offset` of the f32 (normal, uniform) or
    the u8 (keep) base; (B_local, n_outer, inner) or - outer_major - (n_outer, B_local, inner)."""

    def __init__(self, offset, kind, draw_id, B_local, inner, n_outer=1, outer_major=False, keep_p=0.0):
        self.offset, self.kind = int(offset), _KINDS.get(kind, kind)
        self.draw_id, self.B_local, self.inner, self.n_outer = int(draw_id), int(B_local), int(inner), int(n_outer)
        self.outer_major, self.keep_p = bool(outer_major), float(keep_p)

    @property
    def groups(self):
        return self.n_outer * self.B_local * ((self.inner + 3) // 4)

    @property
    def numel(self):
        return self.n_outer * self.B_local * self.inner


class _Row(C.Structure):  # tacorl_noise_seg
    _fields_ = [("offset", C.c_int), ("kind", C.c_int), ("draw_id", C.c_int), ("n_outer", C.c_int), ("B_local", C.c_int),
                ("inner", C.c_int), ("outer_major", C.c_int), ("keep_p", C.c_float), ("group0", C.c_int), ("reserved", C.c_int)]


class SegmentTable:
    """The host table `tacorl_noise_fill` takes (tacorl_noise_table): built once per batch shape, where the buffers are
    carved.  n_f32 / n_u8: sizes of the two destination buffers in elements (the entry point refuses a segment past them)."""

    def __init__(self, segments, n_f32, n_u8=0):
        self.segments = list(segments)
        if not 1 <= len(self.segments) <= MAX_SEGS:
            raise ValueError(f"{len(self.segments)} segments: a fill takes 1..{MAX_SEGS}")
        self.n_f32, self.n_u8 = int(n_f32), int(n_u8)

        class _Table(C.Structure):
            _fields_ = [("n_f32", C.c_int), ("n_u8", C.c_int), ("n_groups", C.c_int), ("reserved", C.c_int),
                        ("seg", _Row * len(self.segments))]

        t, g = _Table(), 0
        for r, s in zip(t.seg, self.segments):
            if not (0 <= s.draw_id <= 65535 and 1 <= s.n_outer <= 65535):
                raise ValueError(f"draw id {s.draw_id} / n_outer {s.n_outer}: 16 bits of the counter each")
            (r.offset, r.kind, r.draw_id, r.n_outer, r.B_local, r.inner, r.outer_major, r.keep_p, r.group0) = (
                s.offset, s.kind, s.draw_id, s.n_outer, s.B_local, s.inner, int(s.outer_major), s.keep_p, g)
            g += s.groups
        t.n_f32, t.n_u8, t.n_groups = self.n_f32, self.n_u8, g
        self.n_groups, self.c_table = g, t

    def __len__(self):
        return len(self.segments)


def table_for(flat_numel, entries, B_local, u8_numel=0, u8_entries=()):
    """Segment table of carved buffers.  entries: (name or draw id, kind, offset, shape) with shape (B, inner..) or - for an
    OUTER_MAJOR name - (n_outer, B, inner..); u8_entries: (draw id, offset, inner, keep_p) keep masks, batch-major."""
    segs = []
    for name, kind, off, shape in entries:
        did = DRAW_IDS[name] if isinstance(name, str) else int(name)
        om = isinstance(name, str) and name in OUTER_MAJOR
        n_outer = int(np.prod(shape)) // (B_local * int(shape[-1])) if om else 1
        inner = int(shape[-1]) if om else int(np.prod(shape)) // B_local
        assert n_outer * B_local * inner == int(np.prod(shape)), (name, shape, B_local)
        segs.append(Segment(off, kind, did, B_local, inner, n_outer, om))
    for did, off, inner, p in u8_entries:
        segs.append(Segment(off, KEEP, did, B_local, inner, keep_p=p))
    return SegmentTable(segs, flat_numel, u8_numel)


class DeviceNoise:
    """The generator's whole state: (seed, step).  fill() launches the kernel for the current step on the current stream;
    advance() moves to the next step (once per step that draws, training and validation alike)."""

    def __init__(self, seed, step=0):
        seed, step = int(seed), int(step)
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"device noise seed {seed}: 64 bits")
        self.seed = seed
        self.step = 0
        self._set_step(step)

    def _set_step(self, step):
        if not 0 <= step < 1 << 32:
            raise ValueError(f"device noise step {step}: the counter holds 32 bits of it")
        self.step = step

    def fill(self, table, base_f32, base_u8=None, sample0=0):
        from . import _lib

        _lib.call("tacorl_noise_fill", C.byref(table.c_table), len(table), _lib.ptr(base_f32), _lib.ptr(base_u8), self.seed,
                  self.step, int(sample0), _lib.stream())

    def advance(self):
        self._set_step(self.step + 1)

    def state(self):
        return {"seed": self.seed, "step": self.step}


# ------------------------------------------------------------------------------------------ a rollout step's draws
ROWS_MAX, ROWS_SEGS = 64, 4   # TACORL_NOISE_ROWS_MAX, TACORL_NOISE_ROWS_SEGS
BY_STEP, BY_PLAN = 0, 1       # which of a row's two numbers is a segment's step word


class RowSegment:
    """One (R, inner) row-major buffer at `offset` of the f32 base.  which: BY_STEP or BY_PLAN; rows: the rows that are drawn
    (None: all of them) - the others are not written."""

    def __init__(self, offset, kind, draw_id, inner, which=BY_STEP, rows=None):
        self.offset, self.kind = int(offset), _KINDS.get(kind, kind)
        self.draw_id = DRAW_IDS[draw_id] if isinstance(draw_id, str) else int(draw_id)
        self.inner, self.which, self.rows = int(inner), int(which), rows


class _RowsSeg(C.Structure):  # tacorl_noise_rows_seg
    _fields_ = [("offset", C.c_int), ("kind", C.c_int), ("draw_id", C.c_int), ("inner", C.c_int), ("which", C.c_int),
                ("reserved", C.c_int), ("mask", C.c_ulonglong)]


class _Rows(C.Structure):  # tacorl_noise_rows
    _fields_ = [("n_rows", C.c_int), ("n_seg", C.c_int), ("n_f32", C.c_int), ("reserved", C.c_int),
                ("episode", C.c_uint * ROWS_MAX), ("step", C.c_uint * ROWS_MAX), ("plan_no", C.c_uint * ROWS_MAX),
                ("seg", _RowsSeg * ROWS_SEGS)]


def rows_table(rows, segments, n_f32):
    """The host struct `tacorl_noise_fill_rows` takes.  rows: (episodes, steps, plan numbers), one entry per row each."""
    episodes, steps, plan_nos = ([int(v) for v in x] for x in rows)
    R = len(episodes)
    if not (1 <= R <= ROWS_MAX and len(steps) == R and len(plan_nos) == R):
        raise ValueError(f"{R} episodes, {len(steps)} steps, {len(plan_nos)} plan numbers: 1..{ROWS_MAX} rows, one of each per row")
    if len(segments) > ROWS_SEGS:
        raise ValueError(f"{len(segments)} segments: a rollout fill takes up to {ROWS_SEGS}")
    if any(not 0 <= v < 1 << 32 for x in (episodes, steps, plan_nos) for v in x):
        raise ValueError("episode / step / plan number: the counter holds 32 bits of each")
    t = _Rows()
    t.n_rows, t.n_seg, t.n_f32 = R, len(segments), int(n_f32)
    for r in range(R):
        t.episode[r], t.step[r], t.plan_no[r] = episodes[r], steps[r], plan_nos[r]
    for c, s in zip(t.seg, segments):
        mask = (1 << R) - 1 if s.rows is None else sum({1 << int(r) for r in s.rows})
        c.offset, c.kind, c.draw_id, c.inner, c.which, c.mask = s.offset, s.kind, s.draw_id, s.inner, s.which, mask
    return t


class RowNoise:
    """The rollouts' generator: its whole state is the seed, every draw is keyed by the row's own (episode, step or plan
    number).  fill() is one asynchronous launch on the current stream; the table travels in the launch arguments."""

    def __init__(self, seed):
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"device noise seed {seed}: 64 bits")
        self.seed = seed

    def fill(self, rows, segments, base):
        from . import _lib

        t = rows_table(rows, segments, base.numel())
        _lib.call("tacorl_noise_fill_rows", C.byref(t), _lib.ptr(base), self.seed, _lib.stream())


def rank_sample0(B_local, world_size):
    """First global sample of this rank's shard: rank x B_local, the rank taken from the process group when one exists."""
    if world_size <= 1:
        return 0
    import torch.distributed as dist

    return dist.get_rank() * B_local if dist.is_available() and dist.is_initialized() else 0


# ------------------------------------------------------------------------------------------ the restatement (NumPy)
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 block function.  counter: (..., 4), key: (2,) or (..., 2) of 32-bit values; returns uint32 (..., 4)."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k = np.asarray(key, dtype=np.uint64) & _MASK
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _MASK)
        k0, k1 = (k0 + np.uint64(_W0)) & _MASK, (k1 + np.uint64(_W1)) & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def philox_words(seed, step, draw_id, B_local, inner, n_outer=1, sample0=0):
    """uint32 (B_local, n_outer, ceil(inner / 4), 4): the output words of every group of four."""
    if not (0 <= draw_id <= 65535 and 1 <= n_outer <= 65535 and 0 <= step < 1 << 32):
        raise ValueError("draw id / n_outer: 16 bits, step: 32 bits")
    qn = (inner + 3) // 4
    ctr = np.zeros((B_local, n_outer, qn, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(qn, dtype=np.uint64)[None, None, :]
    ctr[..., 1] = (np.uint64(sample0) + np.arange(B_local, dtype=np.uint64))[:, None, None]
    ctr[..., 2] = (np.uint64(draw_id << 16) | np.arange(n_outer, dtype=np.uint64))[None, :, None]
    ctr[..., 3] = np.uint64(step)
    return philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64))


def uniform_from_words(w):
    """fp64 (exactly representable in fp32): (w >> 8) 2^-24."""
    return (np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def normal_from_words(w):
    """fp64 Box-Muller on the word pairs (0,1) and (2,3) of (..., 4) words: outputs (r cos, r sin) per pair."""
    w = np.asarray(w, dtype=np.uint32) >> np.uint32(8)
    a, b = w[..., 0::2], w[..., 1::2]
    r = np.sqrt(-2.0 * np.log((a.astype(np.float64) + 1.0) * 2.0 ** -24))
    th = 2.0 * np.pi * (b.astype(np.float64) * 2.0 ** -24)
    out = np.empty(w.shape, dtype=np.float64)
    out[..., 0::2], out[..., 1::2] = r * np.cos(th), r * np.sin(th)
    return out


def philox_restatement(seed, step, draw_id, kind, B_local, inner, n_outer=1, sample0=0, outer_major=False, keep_p=0.0):
    """What `tacorl_noise_fill` writes for one segment, in the segment's own layout: (B_local, n_outer, inner) or - with
    outer_major - (n_outer, B_local, inner).  normal: fp64 (the kernel's fp32 value lies within tests/noise_ref.py's bound);
    uniform: fp64 values that are exact fp32 numbers; keep: uint8."""
    kind = _KINDS.get(kind, kind)
    w = philox_words(seed, step, draw_id, B_local, inner, n_outer, sample0)
    if kind == NORMAL:
        v = normal_from_words(w)
    else:
        v = uniform_from_words(w)
        if kind == KEEP:
            v = (v.astype(np.float32) < np.float32(keep_p)).astype(np.uint8)
    v = v.reshape(B_local, n_outer, -1)[..., :inner]
    return np.ascontiguousarray(v.transpose(1, 0, 2)) if outer_major else v


def philox_rows_restatement(seed, draw_id, kind, episodes, numbers, inner):
    """What `tacorl_noise_fill_rows` writes for one segment whose mask holds every row: (R, 1, inner), row r from the counter
    (q, episodes[r], draw_id << 16, numbers[r]).  normal: fp64; uniform: fp64 values that are exact fp32 numbers."""
    kind = _KINDS.get(kind, kind)
    if kind not in (NORMAL, UNIFORM):
        raise ValueError("a rollout segment is normal or uniform")
    ep, nr = np.asarray(episodes, dtype=np.uint64).ravel(), np.asarray(numbers, dtype=np.uint64).ravel()
    if not (0 <= draw_id <= 65535 and ep.shape == nr.shape and inner >= 1 and (ep < 1 << 32).all() and (nr < 1 << 32).all()):
        raise ValueError("draw id: 16 bits; episodes / numbers: 32 bits, one of each per row")
    qn = (inner + 3) // 4
    ctr = np.zeros((ep.size, 1, qn, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(qn, dtype=np.uint64)[None, None, :]
    ctr[..., 1] = ep[:, None, None]
    ctr[..., 2] = np.uint64(draw_id << 16)
    ctr[..., 3] = nr[:, None, None]
    w = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64))
    v = normal_from_words(w) if kind == NORMAL else uniform_from_words(w)
    return v.reshape(ep.size, 1, -1)[..., :inner]
