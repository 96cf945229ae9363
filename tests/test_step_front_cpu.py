"""The front table of TACORL's fp32-source step, host side only (no GPU): what tacorl_step_front_supported takes and refuses,
the table's size and field offsets against literals, the bytes tacorl_step_front_assemble writes, and the stand-alone
program tests/native/step_front_host_check.cpp built with the host sanitizers (address, undefined) and run here.
Addresses are made up and never dereferenced: nothing is launched."""
import ctypes as C
import os
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = W = 84
IMG, B, T = 3 * H * W, 3, 2
STATES, GOAL, X3 = 0x10000000, 0x20000000, 0x30000000
DISP, REWARD, DONE, ACTS, ACTS_DST = 0x40000000, 0x40001000, 0x40002000, 0x40003000, 0x40004000


def _lib():
    from tacorl_amd import _lib, build

    build.build(verbose=False)
    return _lib.lib()


def _eligible():
    return dict(src=[(STATES, IMG), (STATES + 4 * (T - 1) * IMG, T * IMG)],
                jobs=[(STATES, T * IMG, X3, B), (GOAL, IMG, X3 + 2 * B * IMG, B)],
                disp=DISP, dtype=1, reward=REWARD, done=DONE, B=B, acts=ACTS, acts_dst=ACTS_DST, n_acts=B * T * 7, hw=(H, W))


def _args(c, with_done):
    P, Lg = C.c_void_p, C.c_long
    ns, nj = len(c["src"]), len(c["jobs"])
    a = [ns, (P * ns)(*[s for s, _ in c["src"]]), (Lg * ns)(*[p for _, p in c["src"]]), nj, (P * nj)(*[j[0] for j in c["jobs"]]),
         (Lg * nj)(*[j[1] for j in c["jobs"]]), (P * nj)(*[j[2] for j in c["jobs"]]), (C.c_int * nj)(*[j[3] for j in c["jobs"]]),
         c["disp"], c["dtype"], c["reward"]]
    return a + ([c["done"]] if with_done else []) + [c["B"], c["acts"], c["acts_dst"], c["n_acts"], *c["hw"]]


def _ok(L, **changes):
    return bool(L.tacorl_step_front_supported(*_args({**_eligible(), **changes}, False)))


def test_validation_accepts_the_eligible_case_and_refuses_the_rest():
    L = _lib()
    e = _eligible()
    assert _ok(L)
    assert all(_ok(L, dtype=d) for d in (0, 1, 2, 3))
    assert _ok(L, acts=None, acts_dst=None, n_acts=0)
    # a misaligned base: a source, a pack source, a destination
    assert not _ok(L, src=[(STATES + 4, IMG), e["src"][1]])
    assert not _ok(L, jobs=[e["jobs"][0], (GOAL + 4, IMG, X3 + 2 * B * IMG, B)])
    assert not _ok(L, jobs=[(STATES, T * IMG, X3 + 8, B), e["jobs"][1]])
    # a pitch that is no multiple of four floats
    assert not _ok(L, src=[e["src"][0], (e["src"][1][0], T * IMG + 2)])
    assert not _ok(L, jobs=[(STATES, T * IMG + 2, X3, B), e["jobs"][1]])
    # dtype codes, counts, half an action window, another geometry (the sources are the 84 x 84 encoder's)
    assert not _ok(L, dtype=4) and not _ok(L, dtype=-1)
    assert not _ok(L, B=0) and not _ok(L, jobs=[e["jobs"][0], (GOAL, IMG, X3 + 2 * B * IMG, 0)]) and not _ok(L, n_acts=-1)
    assert not _ok(L, acts_dst=None) and not _ok(L, disp=None) and not _ok(L, reward=None)
    assert not _ok(L, hw=(64, 64)) and not _ok(L, hw=(85, 85))
    assert not _ok(L, src=[e["src"][0]] * 9) and not _ok(L, jobs=[e["jobs"][0]] * 9)
    assert _ok(L, src=[e["src"][0]] * 8, jobs=[e["jobs"][0]] * 8)


def test_table_size_offsets_and_assembled_bytes():
    L = _lib()
    assert L.tacorl_step_front_table_bytes() == 544 and L.tacorl_encoder_src_entry_bytes() == 32
    offs = (C.c_long * 15)()
    assert L.tacorl_step_front_offsets(offs) == 0
    #                     src  pack_src pack_dst pack_pitch pack_n disp reward done acts_src acts_dst n_acts dtype  B  njobs HW
    assert list(offs) == [0, 256, 320, 384, 448, 480, 488, 496, 504, 512, 520, 528, 532, 536, 540]
    host = C.create_string_buffer(b"\xab" * 544, 544)
    assert L.tacorl_step_front_assemble(host, *_args(_eligible(), True)) == 0
    raw = host.raw
    q = lambda off, n=1: list(struct.unpack_from(f"<{n}q", raw, off))  # noqa: E731
    i = lambda off, n=1: list(struct.unpack_from(f"<{n}i", raw, off))  # noqa: E731
    assert q(0, 4) == [STATES, IMG, H * W, W] and q(32, 4) == [STATES + 4 * IMG, T * IMG, H * W, W]
    assert raw[64:256] == bytes(192)  # (the other cameras' entries)
    assert q(256, 8) == [STATES, GOAL] + [0] * 6 and q(320, 8) == [X3, X3 + 2 * B * IMG] + [0] * 6
    assert q(384, 8) == [T * IMG, IMG] + [0] * 6 and i(448, 8) == [B, B] + [0] * 6
    assert q(480, 6) == [DISP, REWARD, DONE, ACTS, ACTS_DST, B * T * 7] and i(528, 4) == [1, B, 2, H * W]
    # equal entries -> equal bytes (what the skip of the fill compares); a moved address -> other bytes; a refused case
    # writes nothing
    again = C.create_string_buffer(544)
    assert L.tacorl_step_front_assemble(again, *_args(_eligible(), True)) == 0 and again.raw == raw
    moved = {**_eligible(), "disp": DISP + 64}
    assert L.tacorl_step_front_assemble(again, *_args(moved, True)) == 0 and again.raw != raw
    before = again.raw
    assert L.tacorl_step_front_assemble(again, *_args({**_eligible(), "dtype": 7}, True)) != 0 and again.raw == before
    # a launch entry point refuses a table that was never assembled, and grids that no table has, before it launches
    assert L.tacorl_step_front_fill(C.c_void_p(0x50000000), C.create_string_buffer(544), None) != 0
    assert L.tacorl_step_front(None, 2, B, B, 0, H, W, None) != 0 and L.tacorl_step_front(C.c_void_p(0x50000000), 9, B, B, 0, H, W, None) != 0
    assert L.tacorl_step_front(C.c_void_p(0x50000000), 2, 0, B, 0, H, W, None) != 0 and L.tacorl_step_front(C.c_void_p(0x50000000), 2, B, 0, 0, H, W, None) != 0


def test_host_side_under_the_sanitizers(tmp_path):
    """tests/native/step_front_host_check.cpp - its own main over step_front_table.h's validation and assembly - built with
    -fsanitize=address,undefined for the host and run: a clean exit, no sanitizer report."""
    from tacorl_amd import build

    exe = str(tmp_path / "step_front_host_check")
    src = os.path.join(ROOT, "tests", "native", "step_front_host_check.cpp")
    subprocess.run([build.HIPCC, "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-O1", "-g",
                    src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "step_front_host_check: ok" in r.stdout, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
