"""GPU (-m gpu): the hand-over of a chunk of work lists.  The lists of ONE oh_frames_upload call share one device arena, one `ready`
event and one pinned summary block (openhevc_amd/csrc/engine_handover.hip); they are still executed, released and freed one by one
and in any order, and the arena returns to the engine's pool with the last of them.

The lists are small (416x240 and 64x64, both geometries in one call) and cover I, P and B pictures, sparse and dense residuals, one
list whose boundary strengths are derived from the motion field and one list in page-locked memory that the GPU pulls.  Their CPU
checker's pictures (oh_or_frame) and the pictures decoded from each list uploaded alone are computed once per module."""
import ctypes as C

import numpy as np
import pytest

from openhevc_amd import frame as F
from oracle_lib import host_pic_array, oracle

pytestmark = pytest.mark.gpu

GEOMETRIES = ((416, 240), (64, 64))
# slice type, knobs, pinned; cycled over the lists of a chunk (seeds differ from list to list)
KINDS = [
    (0, {}, False),                                                   # I
    (2, {"sparse_pct": 100}, False),                                  # B, every block as levels: the copy stops short of the pool
    (1, {}, False),                                                   # P
    (2, {"split_pct": 85, "cbf_pct": 95, "skip_pct": 0}, False),      # B, dense
    (2, {"bs_from_motion": 1, "intra_pct": 25}, False),               # B, boundary strengths from the motion field behind the group's copy
    (2, {"intra_pct": 30}, True),                                     # B in page-locked memory, packed grids: pulled, a group of its own
    (2, {"sparse_pct": 60}, False),                                   # B, mixed
]
N_LISTS = 33


def geometry_of(i):
    return 1 if i % 3 == 2 else 0


def assert_same(want, got, tag):
    for c in range(len(want.planes)):
        a, b = want.visible(c), got.visible(c)
        if not np.array_equal(a, b):
            ys, xs = np.nonzero(a != b)
            raise AssertionError(f"{tag}: plane {c} differs at {len(ys)} samples, first (x={xs[0]}, y={ys[0]}): want {a[ys[0], xs[0]]} got {b[ys[0], xs[0]]}")


class World:
    """one engine; per geometry two reference pictures and the start content of a current picture; N_LISTS lists (host ids: references
    0 and 1, current picture 2), each with a current picture of its own on the engine, its checker picture and its picture decoded alone"""

    def __init__(self, eng=None):
        from openhevc_amd.engine import Engine, remap_frame
        self.eng = e = eng or Engine(0)
        self.params = [F.pic_params(w, h) for w, h in GEOMETRIES]
        self.recs = [F.Recorder(p) for p in self.params]
        rng = np.random.default_rng(10)
        self.host = [{k: F.HostPic(p, rng=rng) for k in range(3)} for p in self.params]
        self.ref_ids = []
        for p, host in zip(self.params, self.host):
            ids = [e.pic_alloc(p), e.pic_alloc(p)]
            for k in (0, 1):
                e.pic_upload(ids[k], host[k])
            self.ref_ids.append(ids)
        self.copies, self.frames, self.cur, self.want, self.alone = [], [], [], [], []
        for i in range(N_LISTS):
            g = geometry_of(i)
            st, knobs, pinned = KINDS[i % len(KINDS)]
            f = self.recs[g].synth(F.synth_params(st, 9100 + i, **knobs), 2, [0, 1])
            fc = F.FrameCopy(f, pinned_by=e.L if pinned else None)
            assert bool(fc.frame.flags & F.OH_FRAME_PINNED) == pinned
            self.copies.append(fc)
            self.cur.append(e.pic_alloc(self.params[g]))
            self.frames.append(remap_frame(fc.frame, {0: self.ref_ids[g][0], 1: self.ref_ids[g][1], 2: self.cur[i]}))
            want = {k: v.copy() for k, v in self.host[g].items()}
            assert oracle().oh_or_frame(C.byref(fc.frame), host_pic_array(want)) == 0
            self.want.append(want[2])
        # every list uploaded alone (a chunk of one), the way oh_frame_upload always worked
        self.reset_pictures(range(N_LISTS))
        for i in range(N_LISTS):
            df = e.frame_upload(self.frames[i])
            e.frame_execute(df)
            e.frame_release(df)
        e.sync()
        for i in range(N_LISTS):
            self.alone.append(self.download(i))
            assert_same(self.want[i], self.alone[i], f"list {i} uploaded alone against the checker")

    def reset_pictures(self, which):
        for i in which:
            self.eng.pic_upload(self.cur[i], self.host[geometry_of(i)][2])

    def download(self, i):
        return self.eng.pic_download(self.cur[i], self.params[geometry_of(i)])

    def check(self, which, tag):
        for i in which:
            got = self.download(i)
            assert_same(self.want[i], got, f"{tag}: list {i} against the checker")
            assert_same(self.alone[i], got, f"{tag}: list {i} against the same list uploaded alone")

    def close(self):
        self.eng.close()
        for r in self.recs:
            r.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


@pytest.mark.parametrize("n", [1, 2, 9, 33])
def test_lists_of_one_upload_call_decode_like_lists_uploaded_alone(world, n):
    """n lists in ONE oh_frames_upload call: 9 has the pulled list in its middle, which cuts the chunk into three staging groups, 33
    crosses OH_MAX_BATCH (two chunks).  One oh_frames_execute
    call takes pictures of one geometry, so the lists are executed in one call per geometry; then again, every geometry split into two
    subsets, the later lists first.  Every picture equals the checker's and the one decoded from the same list uploaded alone."""
    e = world.eng
    dfs = e.frames_upload(world.frames[:n])
    by_geometry = [[i for i in range(n) if geometry_of(i) == g] for g in range(len(GEOMETRIES))]
    world.reset_pictures(range(n))
    for idx in by_geometry:
        if idx:
            e.frames_execute([dfs[i] for i in idx])
    e.sync()
    world.check(range(n), f"{n} lists, one execute per geometry")
    world.reset_pictures(range(n))
    for idx in by_geometry:
        for part in (idx[len(idx) // 2:], idx[:len(idx) // 2]):
            if part:
                e.frames_execute([dfs[i] for i in reversed(part)])
    e.sync()
    world.check(range(n), f"{n} lists, two subsets in reverse order")
    for i, df in enumerate(dfs):                                   # let go one by one, some stream-ordered and some after a wait
        (e.frame_free if i % 5 == 3 else e.frame_release)(df)
    e.sync()


def test_arenas_level_off_when_a_chunks_lists_go_one_by_one_in_any_order(world):
    """64 chunks of 8 lists; the lists of a chunk are released or freed in a shuffled order, two of them before the others are executed
    (never executed themselves), the rest after their execute; a sync every 8 chunks.  The arenas alive level off (after chunk 64 no
    more than after chunk 16, plus 2) and the last chunk's pictures are right."""
    e = world.eng
    lists = [i for i in range(N_LISTS) if geometry_of(i) == 0][:8]
    rng = np.random.default_rng(64)
    seen = {}
    for chunk in range(64):
        last = chunk == 63
        if last:
            world.reset_pictures(lists)
        dfs = e.frames_upload([world.frames[i] for i in lists])
        order = [int(k) for k in rng.permutation(8)]
        early = [] if last else order[:2]
        for n, k in enumerate(early):
            (e.frame_free if n == 0 and chunk % 4 == 0 else e.frame_release)(dfs[k])
        rest = [k for k in order if k not in early]
        e.frames_execute([dfs[k] for k in rest])
        for n, k in enumerate(rest):
            (e.frame_free if n == 3 and chunk % 4 == 1 else e.frame_release)(dfs[k])
        if chunk % 8 == 7:
            e.sync()
        if chunk in (15, 63):
            seen[chunk] = e.memory()
    assert seen[63]["arenas"] <= seen[15]["arenas"] + 2, seen
    assert seen[63]["deferred"] == 0, seen
    world.check(lists, "chunk 64")


def test_a_malformed_list_in_a_chunk_fails_the_whole_call_on_the_host(world):
    """a chunk of 8 whose list 5 has a non-zero count with a NULL array: OH_E_ARG, every out[i] null, and the engine holds what it held
    before the call (nothing was taken from the pools and nothing was enqueued)"""
    e = world.eng
    lists = [i for i in range(N_LISTS) if geometry_of(i) == 0][:8]
    frames = []
    for i in lists:
        g = F.OhFrame()
        C.memmove(C.byref(g), C.byref(world.frames[i]), C.sizeof(F.OhFrame))
        frames.append(g)
    if frames[5].n_pu:
        frames[5].pu = C.cast(None, type(frames[5].pu))
    else:
        assert frames[5].n_tu > 0
        frames[5].tu = C.cast(None, type(frames[5].tu))
    e.sync()
    before = e.memory()
    n = len(frames)
    fs = (C.POINTER(F.OhFrame) * n)(*[C.pointer(f) for f in frames])
    out = (C.c_void_p * n)(*([1] * n))
    rc = e.L.oh_frames_upload(e.h, fs, n, out)
    assert rc == -2, rc                                            # OH_E_ARG
    assert "NULL array" in e.L.oh_engine_last_error(e.h).decode()
    assert all(out[i] is None for i in range(n)), list(out)
    assert e.memory() == before
    # the engine goes on: the same lists, well-formed, decode
    world.reset_pictures(lists)
    dfs = e.frames_upload([world.frames[i] for i in lists])
    e.frames_execute(dfs)
    for df in dfs:
        e.frame_release(df)
    e.sync()
    world.check(lists, "after the refused chunk")
