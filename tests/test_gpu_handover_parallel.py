"""GPU (-m gpu): the hand-over of a chunk whose lists are checked and counted on all the engine's host threads and whose staging copy is
claimed piece by piece (openhevc_amd/csrc/handover_host.h, engine_handover.hip).  What the threads share must not show in a single
sample: chunks of 1, 3, 32 and 33 lists decode like the CPU checker and like the same lists uploaded alone — with 0, 1, 2 (the default)
and 5 helper threads, and with two engines handing over from two threads at once — and the pool of pinned staging buffers levels off.

The lists, their checker pictures and the pictures decoded from each list uploaded alone are those of test_gpu_chunk_handover.py (World:
small 416x240 and 64x64 lists of every kind, one of them pulled from page-locked memory), made once per module.  No test provokes a
fault: a malformed list is refused on the host before anything is enqueued, which test_gpu_chunk_handover.py covers."""
import threading

import pytest

import test_gpu_chunk_handover as T
from forced_engine import forced_engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    w = T.World()
    yield w
    w.close()


class Mirror(T.World):
    """a second engine with pictures of its own for the lists of `world` (the checker's pictures and the lists themselves are shared)"""

    def __init__(self, world):
        from openhevc_amd.engine import Engine, remap_frame
        self.eng = e = Engine(0)
        self.params, self.host, self.copies, self.want, self.alone, self.recs = world.params, world.host, world.copies, world.want, world.alone, []
        self.ref_ids, self.cur, self.frames = [], [], []
        for p, host in zip(self.params, self.host):
            ids = [e.pic_alloc(p), e.pic_alloc(p)]
            for k in (0, 1):
                e.pic_upload(ids[k], host[k])
            self.ref_ids.append(ids)
        for i, fc in enumerate(self.copies):
            g = T.geometry_of(i)
            self.cur.append(e.pic_alloc(self.params[g]))
            self.frames.append(remap_frame(fc.frame, {0: self.ref_ids[g][0], 1: self.ref_ids[g][1], 2: self.cur[i]}))


def decode_chunk(w, n, frames=None):
    """lists 0 .. n-1 (frames: other copies of the same lists) in ONE oh_frames_upload call, one execute per geometry, every list released"""
    e = w.eng
    dfs = e.frames_upload((frames or w.frames)[:n])
    for g in range(len(T.GEOMETRIES)):
        idx = [i for i in range(n) if T.geometry_of(i) == g]
        if idx:
            e.frames_execute([dfs[i] for i in idx])
    for df in dfs:
        e.frame_release(df)


@pytest.mark.parametrize("n", [1, 3, 32, 33])
def test_a_chunk_counted_on_all_host_threads_decodes_like_lists_uploaded_alone(world, n):
    """1: the submitting thread alone, no helper woken; 3: fewer lists than threads at 5 helpers, as many at 2; 32: a full chunk, its
    lists claimed from the cursor; 33: a full chunk and a chunk of one behind it.  Every picture equals the checker's and the one
    decoded from the same list uploaded alone."""
    world.reset_pictures(range(n))
    decode_chunk(world, n)
    world.eng.sync()
    world.check(range(n), f"{n} lists in one call")


@pytest.mark.parametrize("helpers", [0, 1, 5])
def test_a_full_chunk_with_other_numbers_of_helper_threads(helpers):
    """OHEVC_COPY_THREADS is read when an engine is created: a world of its own per value.  0: no helper at all, the submitting thread
    runs the same code alone; 1 and 5: fewer and more threads than the default's three."""
    with forced_engine(OHEVC_COPY_THREADS=helpers) as e:
        w = T.World(e)
        try:
            w.reset_pictures(range(32))
            decode_chunk(w, 32)
            w.eng.sync()
            w.check(range(32), "32 lists in one call")
        finally:
            w.close()


def test_two_engines_hand_over_chunks_from_two_threads_at_once(world):
    """every engine has its own helper threads and its own scratch: two Python threads (the calls release the interpreter lock) hand
    over four chunks of 32 each at the same time; both sets of pictures are right"""
    second = Mirror(world)
    try:
        errors = []
        start = threading.Barrier(2)

        def run(w):
            try:
                start.wait(timeout=60)
                for k in range(4):
                    if k == 3:
                        w.reset_pictures(range(32))      # the pictures checked are the last chunk's, from their start content
                    decode_chunk(w, 32)
                w.eng.sync()
            except Exception as ex:          # noqa: BLE001 — reported by the asserting thread
                errors.append(ex)

        threads = [threading.Thread(target=run, args=(w,)) for w in (world, second)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        world.check(range(32), "first engine")
        second.check(range(32), "second engine")
    finally:
        second.close()


def staged_copies(world, recs):
    """the first 32 lists with the page-locked ones among them copied into ordinary memory: every list is staged, the chunk is ONE group"""
    from openhevc_amd import frame as F
    from openhevc_amd.engine import remap_frame
    frames, keep = [], []
    for i in range(32):
        st, knobs, pinned = T.KINDS[i % len(T.KINDS)]
        if not pinned:
            frames.append(world.frames[i])
            continue
        g = T.geometry_of(i)
        keep.append(F.FrameCopy(recs[g].synth(F.synth_params(st, 9100 + i, **knobs), 2, [0, 1])))
        assert not keep[-1].frame.flags & F.OH_FRAME_PINNED
        frames.append(remap_frame(keep[-1].frame, {0: world.ref_ids[g][0], 1: world.ref_ids[g][1], 2: world.cur[i]}))
    return frames, keep


def test_staging_buffers_level_off_over_many_chunks(world):
    """40 chunks of 32 small lists, a sync every 8 chunks: the engine holds no more pinned staging buffers after chunk 40 than after
    chunk 10 (a chunk's staging buffer is reused, never added per chunk).

    The chunks are 32 STAGED lists, one group and so one staging buffer per chunk, which is what the check is about.  With the four
    page-locked lists of the first 32 left in, each pulled through a buffer of its own, a chunk asks for nine buffers in one burst and
    the pool ends as large as the largest number the copy stream happened to leave busy within a burst: measured 4 after chunk 10 and
    5 after chunk 40, twice, with the engine's buffer pool exactly as it was before this test existed — a race between the host and the
    copy stream in which no buffer is lost, and not what this test is for.  The engine is a fresh one, so that buffers left by other
    tests do not make the bound easy."""
    fresh = Mirror(world)                      # an engine whose pool starts empty: what it holds after chunk 10 is what these chunks need
    try:
        e = fresh.eng
        frames, keep = staged_copies(fresh, world.recs)
        seen = {}
        for chunk in range(40):
            if chunk == 39:
                fresh.reset_pictures(range(32))
            decode_chunk(fresh, 32, frames)
            if chunk % 8 == 7:
                e.sync()
            if chunk in (9, 39):
                seen[chunk] = e.memory()
        e.sync()
        assert seen[39]["stages"] <= seen[9]["stages"], seen
        fresh.check(range(32), "chunk 40")
        del keep
    finally:
        fresh.close()
