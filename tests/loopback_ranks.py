"""Three ranks of ONE process exchanging tiles through the library's loop-back hub (rfw_hip_comm_init_loopback): run by
tests/test_gpu_parity.py::test_library_exchange_through_the_loopback_hub in a process of its own.
    python3 tests/loopback_ranks.py <gather format 0|1|2> <present rank, -1 = every rank de-tiles>
What the ranks end up with is the single-GPU frame, bit for bit — after every frame, and again after six frames in flight over three frame
slots per rank (the slots' gathers chained by the same events as with ncclAllGather).  Every rank runs its render() calls on a thread of
its own, as ranks of one process do: a rank's call returns once every rank has joined the gather.  Then the failure only N > 1 has: a rank
that never renders its frame is reported by the others' render() calls."""
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
fmt, present_rank = int(sys.argv[1]), int(sys.argv[2])


class raises:  # (pytest.raises without pytest)
    def __init__(self, exc, match=None):
        self.exc, self.match = exc, match

    def __enter__(self):
        return self

    def __exit__(self, t, v, tb):
        assert t is not None and issubclass(t, self.exc), f"expected {self.exc.__name__}, got {t}"
        assert self.match is None or self.match in str(v), (self.match, str(v))
        return True


from rfw_rs_amd import BackendError, HipBackend, Scene
w, h, world = 200, 136, 3
scene = Scene().build("soup", 1500, 5, 0.0, 4)
scene.set_aspect(w / h)
base = scene.view(w, h)
from rfw_rs_amd import pod
views = []
for k in range(6):                                       # six different images: the camera slides sideways
    v = pod.CameraView3D.from_buffer_copy(base)
    v.pos.x += 0.07 * k; v.p1.x += 0.07 * k
    views.append(v)
full = HipBackend.init(w, h, 1.0)
scene.sync(full)
ref = []
for v in views:
    full.reset_accumulation()
    full.render(v)
    pres = full.host_frame(presented=True)
    full.download_frame(pres); full.wait_downloads()
    ref.append((full.accumulator().copy(), full.framebuffer().copy(), pres.copy()))
ranks = []
key = 0x10C0 + fmt * 16 + (present_rank + 1)
for r in range(world):
    be = HipBackend.init(w, h, 1.0, rank=r, world=world, tile_size=32, frames_in_flight=3)
    be.set_option("gather_format", fmt)
    be.set_option("present_rank", present_rank)
    be.set_option("p2p_timeout_ms", 5000)
    scene.mark_all_changed()
    scene.sync(be)
    be.comm_init_loopback(key, r, world)
    ranks.append(be)

def check(i, what):
    acc, frame, pres = ref[i]
    for r, be in enumerate(ranks):
        # (an all-gather leaves every rank's tiles on every rank: the presenting rank de-tiles at once, the others when somebody reads)
        if fmt == 0:
            assert np.array_equal(be.accumulator().view(np.uint32), acc.view(np.uint32)), (what, i, r)
        elif fmt == 1:
            want = frame[..., :3].astype(np.float16).astype(np.float32)
            assert np.array_equal(be.framebuffer()[..., :3].view(np.uint32), want.view(np.uint32)), (what, i, r)
        else:
            dst = be.host_frame(presented=True)
            be.download_frame(dst); be.wait_downloads()
            assert np.array_equal(dst, pres), (what, i, r)

def render_all(order, v):
    """every rank of `order` calls render(v) on a thread of its own, started in that order (a rank returns once all have joined the
    gather); returns what each call raised, None where it returned"""
    errors = [None] * len(order)

    def run(k, be):
        try:
            be.render(v)
        except BackendError as e:
            errors[k] = e
    threads = [threading.Thread(target=run, args=(k, be)) for k, be in enumerate(order)]
    for t in threads:
        t.start()
        time.sleep(0.002)
    for t in threads:
        t.join()
    return errors


for i, v in enumerate(views):                          # one frame at a time
    assert render_all(ranks, v) == [None] * world
    check(i, "frame by frame")
for rep in range(3):                                   # six frames in flight over three slots per rank, ranks issued in changing order
    for i, v in enumerate(views):
        errs = render_all(ranks if (i + rep) % 2 == 0 else ranks[::-1], v); assert errs == [None] * world, (rep, i, errs)
    check(len(views) - 1, "six frames in flight")
# a rank that never arrives: the others' render() calls fail once p2p_timeout_ms has passed
for be in ranks:
    be.set_option("p2p_timeout_ms", 300)
errors = render_all(ranks[:2], views[0])
for e in errors:
    with raises(BackendError, match="did not arrive"):
        if e is not None:
            raise e
for be in ranks + [full]:
    be.close()

print("LOOPBACK OK", fmt, present_rank)
