"""The render scale (include/rfw_hip.h rfw_hip_create, DESIGN.md "Render scale", csrc/resample.inc): a backend created for a window of
W x H under a scale traces at (RW, RH) = (max(1, int(W scale)), max(1, int(H scale))) and presents at W x H.

The yardstick is a TWIN: a second backend created at (RW, RH, 1.0) with the same scene, options, views and calls.  Everything inside runs
at the render size, so the scaled backend's accumulator must equal the twin's bit for bit, and its window frame must equal the
restatement below — the filter of include/rfw_hip.h in Python ints and one numpy float32 operation per step — of the twin's frame, bit
for bit: there are no tolerances in this file.  Frames of a few thousand pixels, so that tests/test_render_scale_on_cpu.py can run the
file on the emulated library too."""
import ctypes as C

import numpy as np
import pytest

from rfw_rs_amd import BackendError, HipBackend, RenderMode, Scene

gpu = pytest.mark.gpu
F1 = np.float32(1.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def render_size(w, h, scale):
    return max(1, int(w * scale)), max(1, int(h * scale))  # the product in double, truncated


# ---------------------------------------------------------------- the restatement of the filter
def taps(R, N, x, filt):
    """the ordered tap list [(source index, weight)] of window index x; weight None: a single tap of weight 1, a copy"""
    if filt == 0:
        return [(((2 * x + 1) * R) // (2 * N), None)]
    if R <= N:
        num = (2 * x + 1) * R - N
        if num < 0:
            return [(0, None)]
        i0, rem = divmod(num, 2 * N)
        f = np.float32(rem) / np.float32(2 * N)
        if f == 0 or i0 == R - 1:
            return [(i0, None)]
        return [(i0, F1 - f), (i0 + 1, f)]
    out = []
    for j in range((x * R) // N, ((x + 1) * R - 1) // N + 1):
        o = min((x + 1) * R, (j + 1) * N) - max(x * R, j * N)
        assert o > 0  # a tap of weight zero never exists
        out.append((j, np.float32(o) / np.float32(R)))
    assert 2 <= len(out) <= 5
    return out


def apply(value, lst):
    """s = v_0 w_0, then s = s + v_k w_k in list order, per channel; value(j): float32 array of source index j"""
    if lst[0][1] is None:
        return value(lst[0][0]).copy()
    s = None
    for j, w in lst:
        v = value(j) * w
        s = v if s is None else s + v
    return s


def restatement(src, W, H, filt):
    """src: (RH, RW, 4) float32 -> (H, W, 4): the vertical list applied to the horizontal results of the source rows"""
    src = np.ascontiguousarray(src, np.float32)
    RH, RW = src.shape[:2]
    with np.errstate(all="ignore"):
        hor = np.empty((RH, W, 4), np.float32)
        for x in range(W):
            hor[:, x, :] = apply(lambda j: src[:, j, :], taps(RW, W, x, filt))
        out = np.empty((H, W, 4), np.float32)
        for y in range(H):
            out[y] = apply(lambda j: hor[j], taps(RH, H, y, filt))
    assert out.dtype == np.float32
    return out


# ---------------------------------------------------------------- scaled backend and twin
_SCENE = []


def cornell():
    if not _SCENE:
        _SCENE.append(Scene().build("cornell"))
    return _SCENE[0]


def backend(w, h, scale, options=(), **init):
    scene = cornell()
    be = HipBackend.init(w, h, scale, max_path_length=2, **init)
    for k, v in options:
        be.set_option(k, v)
    scene.mark_all_changed()
    scene.sync(be)
    return be


class Pair:
    """a backend of a W x H window under `scale`, and its twin at the render size with scale 1"""

    def __init__(self, w, h, scale, options=(), aspect=None, **init):
        self.w, self.h, self.aspect = w, h, aspect or w / h
        self.rw, self.rh = render_size(w, h, scale)
        self.be = backend(w, h, scale, options, **init)
        self.twin = backend(self.rw, self.rh, 1.0, options, **init)
        self.view = self.views(1)[0]

    def views(self, n):
        """n views for the RENDER size (what rfw asks the camera for), one spread angle"""
        scene, out = cornell(), []
        for k in range(n):
            scene.set_camera([0.0, 0.0, -3.4 + 0.1 * k] if k else [0.0, 0.0, -3.4], [0.05 * k, 0.0, 1.0], fov=40.0, aspect=self.aspect)
            out.append(scene.view(self.rw, self.rh))
        return out

    def check(self, filt, frame=None):
        got = self.be.framebuffer() if frame is None else self.be.framebuffer_at(frame)
        src = self.twin.framebuffer() if frame is None else self.twin.framebuffer_at(frame)
        assert src.shape == (self.rh, self.rw, 4) and got.shape == (self.h, self.w, 4)
        assert src[..., :3].any()  # (the frame shows something)
        want = restatement(src, self.w, self.h, filt)
        bad = np.argwhere(bits(got) != bits(want))
        assert len(bad) == 0, (len(bad), bad[:4])

    def close(self):
        self.be.close()
        self.twin.close()


SHAPES = [(64, 64, 0.5), (70, 37, 0.61), (40, 24, 1.5), (33, 21, 2.3), (16, 16, 4.0), (3, 2, 0.4)]
RENDER = [(32, 32), (42, 22), (60, 36), (75, 48), (64, 64), (1, 1)]


@gpu
@pytest.mark.parametrize("shape,want", list(zip(SHAPES, RENDER)))
def test_render_size_accumulator_and_window_frame(shape, want):
    w, h, scale = shape
    assert render_size(w, h, scale) == want
    p = Pair(w, h, scale)
    try:
        assert p.be.render_size() == want and (p.be.render_width, p.be.render_height) == want and (p.be.width, p.be.height) == (w, h)
        for n in (1, 2, 3):
            p.be.render(p.view)
            p.twin.render(p.view)
            if n in (1, 3):  # the accumulator after 1 and after 3 samples
                acc = p.be.accumulator()
                assert acc.shape == (want[1], want[0], 4) and same(acc, p.twin.accumulator())
        p.check(1)  # the default filter
        for filt in (0, 1):  # the option applies from the next frame and the image goes on: sample 4, 5
            p.be.set_option("scale_filter", filt)
            p.be.render(p.view)
            p.twin.render(p.view)
            assert p.be.frame_stats()["sample_count"] == p.twin.frame_stats()["sample_count"] >= 4
            p.check(filt)
            assert same(p.be.accumulator(), p.twin.accumulator())
    finally:
        p.close()


@gpu
def test_wide_window_row():
    """a window row so wide that (2 W + 1) RW passes 2^32: the stage's 64-bit index arithmetic (one row of small tiles keeps the frame small)"""
    w, h, scale = 160000, 1, 0.1
    assert render_size(w, h, scale) == (16000, 1) and (2 * w + 1) * 16000 >= 1 << 32
    p = Pair(w, h, scale, aspect=1.0, tile_size=8)
    try:
        p.be.render(p.view)
        p.twin.render(p.view)
        p.check(1)  # (bilinear: quotient, remainder and fraction of the wide numerator)
        assert same(p.be.accumulator(), p.twin.accumulator())
    finally:
        p.close()


@gpu
def test_same_size_path():
    """a scale that truncates to the window size is the path without a scale: frame and accumulator, and the sizes of the debug taps"""
    a, b = backend(64, 64, 1.004, [("denoise", 1)]), backend(64, 64, 1.0, [("denoise", 1)])
    try:
        assert a.render_size() == (64, 64)
        view = cornell().view(64, 64)
        for be in (a, b):
            be.render(view)
            be.render(view)
        assert same(a.framebuffer(), b.framebuffer()) and same(a.accumulator(), b.accumulator())
        ga, gb = a.denoise_guide(), b.denoise_guide()
        assert all(x.shape == (64, 64, 4) and same(x, y) for x, y in zip(ga, gb))
        assert len(a.debug_read("dn_guide", 1 << 20)) == len(b.debug_read("dn_guide", 1 << 20)) == 48 * 64 * 64
    finally:
        a.close()
        b.close()


def test_nan_containment_of_the_restatement():
    """the yardstick itself: a tap of weight zero does not exist, so a NaN or Inf source pixel spoils exactly the window pixels whose
    footprint contains it (no device needed)"""
    src = np.linspace(0.0, 1.0, 8 * 8 * 4, dtype=np.float32).reshape(8, 8, 4)
    src[2, 3] = np.nan
    src[6, 5] = np.inf

    def spoiled(n, filt):
        out = restatement(src, n, n, filt)
        return {(int(y), int(x)) for y, x in np.argwhere(~np.isfinite(out).all(axis=-1))}

    def block(y0, y1, x0, x1):
        return {(y, x) for y in range(y0, y1 + 1) for x in range(x0, x1 + 1)}
    # 16 x 16, bilinear: interior source index c weighs in window indices 2c - 1 ... 2c + 2
    assert spoiled(16, 1) == block(3, 6, 5, 8) | block(11, 14, 9, 12)
    # 16 x 16, nearest: source index c is window indices 2c, 2c + 1
    assert spoiled(16, 0) == block(4, 5, 6, 7) | block(12, 13, 10, 11)
    # 4 x 4, area: window index x averages source indices 2x, 2x + 1
    assert spoiled(4, 1) == {(1, 1), (3, 2)}
    # 4 x 4, nearest: source indices 1, 3, 5, 7 only: rows 2 and 6 are never read
    assert spoiled(4, 0) == set()
    # ... and a finite source is reproduced where the sizes agree
    assert same(restatement(src[:, :, :], 8, 8, 1)[0], src[0])


@gpu
@pytest.mark.parametrize("case", ["albedo", "filtered_ssao", "denoise_temporal"])
def test_finalisers(case):
    options = [("denoise", 2), ("denoise_temporal", 4)] if case == "denoise_temporal" else []
    mode = {"albedo": RenderMode.ALBEDO, "filtered_ssao": RenderMode.FILTERED_SSAO, "denoise_temporal": RenderMode.DEFAULT}[case]
    p = Pair(64, 64, 0.5, options)
    try:
        for image in range(3):
            for be in (p.be, p.twin):
                be.reset_accumulation()
                be.render(p.view, None, mode)
            p.check(1)
            assert same(p.be.accumulator(), p.twin.accumulator())
        if case == "denoise_temporal":  # the history lives at the render size
            assert p.be.denoise_history().shape == (32, 32, 4) and same(p.be.denoise_history(), p.twin.denoise_history())
    finally:
        p.close()


@gpu
def test_batches_and_samples():
    p = Pair(64, 64, 0.5, max_batch=2)
    try:
        views = p.views(2)
        p.be.render_batch(views)
        p.twin.render_batch(views)
        for f in range(2):
            p.check(1, frame=f)
            assert same(p.be.accumulator_at(f), p.twin.accumulator_at(f))
        assert not same(p.be.framebuffer_at(0), p.be.framebuffer_at(1))
        p.be.render_samples(views[1], 2)
        p.twin.render_samples(views[1], 2)
        p.check(1)
        assert same(p.be.accumulator(), p.twin.accumulator())
    finally:
        p.close()


@gpu
def test_frame_slots():
    p = Pair(64, 64, 0.5, frames_in_flight=3)
    try:
        for v in p.views(5):
            p.be.render(v)
            p.twin.render(v)
            p.check(1)
            assert same(p.be.accumulator(), p.twin.accumulator())
    finally:
        p.close()


@gpu
def test_resize_changes_the_scale():
    scene = cornell()
    be, twin = backend(64, 64, 1.0), backend(32, 32, 1.0)
    try:
        scene.set_camera([0.0, 0.0, -3.4], [0.0, 0.0, 1.0], fov=40.0, aspect=1.0)
        v64, v32 = scene.view(64, 64), scene.view(32, 32)
        be.render(v64)
        be.render(v64)
        first, first_acc = be.framebuffer(), be.accumulator()
        be.resize((64, 64), 0.5)  # only the scale changes: a resize of the render size
        assert be.render_size() == (32, 32) and (be.width, be.height) == (64, 64)
        fb = be.framebuffer()
        assert fb.shape == (64, 64, 4) and not fb.any() and not be.accumulator().any()  # zeros before the next render
        be.render(v32)
        twin.render(v32)
        assert same(be.framebuffer(), restatement(twin.framebuffer(), 64, 64, 1)) and same(be.accumulator(), twin.accumulator())
        be.resize((64, 64), 1.0)
        assert be.render_size() == (64, 64) and not be.framebuffer().any()
        be.render(v64)
        be.render(v64)
        assert same(be.framebuffer(), first) and same(be.accumulator(), first_acc)
    finally:
        be.close()
        twin.close()


def ortho(w, h):
    """glam orthographic_rh(-w/2, w/2, -h/2, h/2, 10, -10) as 16 column-major floats: Camera2D::from_width_height"""
    m = np.zeros((4, 4), np.float64)
    m[0, 0], m[1, 1], m[2, 2], m[2, 3], m[3, 3] = 2.0 / w, 2.0 / h, 1.0 / 20.0, 0.5, 1.0
    return np.ascontiguousarray(m.T.reshape(16).astype(np.float32))


def pixel_matrix(w, h):
    """rfw-font's instance matrix scale(1, -1, 1) * translate(-w/2, -h/2, 0): vertex (x, y) lands on pixel column x, row y"""
    m = np.eye(4)
    m[0, 3], m[1, 1], m[1, 3] = -w / 2.0, -1.0, h / 2.0
    return np.ascontiguousarray(m.T.reshape(16).astype(np.float32))


@gpu
def test_2d_layer_at_the_window_resolution():
    p = Pair(64, 64, 0.5)
    plain = backend(64, 64, 0.5)  # an identical scaled backend without 2D data
    try:
        colour = (0.25, 0.5, 0.75, 1.0)
        corners = [(16, 8), (48, 8), (16, 24), (48, 8), (48, 24), (16, 24)]  # window columns 16 ... 47, rows 8 ... 23
        p.be.set_2d_mesh(0, np.array([[x, y, 0.0, 0.0, 0.0, 0.0, *colour] for x, y in corners], np.float32))
        p.be.set_2d_instances(0, pixel_matrix(64, 64).reshape(1, 16))
        p.be.synchronize()
        p.be.render(p.view, ortho(64, 64))
        p.twin.render(p.view)
        plain.render(p.view)
        got, back = p.be.framebuffer(), plain.framebuffer()
        inside = np.zeros((64, 64), bool)
        inside[8:24, 16:48] = True
        assert p.be.overlay_stats()["drawn"] == 2
        assert np.array_equal(bits(got[inside][:, :3]), np.broadcast_to(bits(np.array(colour[:3], np.float32)), (32 * 16, 3)))
        assert np.array_equal(bits(got[inside][:, 3]), bits(back[inside][:, 3]))  # dst.w is never touched
        assert np.array_equal(bits(got[~inside]), bits(back[~inside]))
        assert same(back, restatement(p.twin.framebuffer(), 64, 64, 1))
        assert same(p.be.accumulator(), p.twin.accumulator())  # the accumulator never sees the 2D layer
    finally:
        p.close()
        plain.close()


@gpu
def test_presented_frame():
    p = Pair(70, 37, 0.61)
    try:
        p.be.render(p.view)
        fb = p.be.framebuffer()
        steps = p.be.srgb_steps()
        pres, facc, ffb = p.be.host_frame(presented=True), p.be.host_frame(accumulator=True), p.be.host_frame()
        assert pres.shape == (37, 70, 4) and facc.shape == (22, 42, 4) and ffb.shape == (37, 70, 4)
        p.be.download_frame(pres)
        p.be.download_frame(facc, accumulator=True)
        p.be.download_frame(ffb)
        p.be.wait_downloads()
        enc = lambda x: np.searchsorted(steps, x, side="right").astype(np.uint8)
        want = np.stack([enc(fb[..., 2]), enc(fb[..., 1]), enc(fb[..., 0]), np.full(fb.shape[:2], 255, np.uint8)], axis=-1)
        assert np.array_equal(pres, want) and len(np.unique(pres[..., :3])) > 8
        assert same(ffb, fb) and same(facc, p.be.accumulator())
        for a in (pres, facc, ffb):
            p.be.free_host_frame(a)
    finally:
        p.close()


BAD_SCALES = [0.0, -1.0, float("nan"), float("inf"), 4.5]


@gpu
def test_refusals():
    for s in BAD_SCALES:
        with pytest.raises(BackendError, match=r"rfw_hip_create failed: \S"):
            HipBackend.init(64, 64, s)
    with pytest.raises(BackendError, match=r"rfw_hip_create failed: \S"):
        HipBackend.init(8192, 8192, 4.0)
    with pytest.raises(BackendError, match=r"rfw_hip_create failed: \S"):
        HipBackend.init(64, 64, 0.5, world=2)
    p = Pair(64, 64, 0.5)
    try:
        p.be.render(p.view)
        before, acc = p.be.framebuffer(), p.be.accumulator()
        for size, s in [((64, 64), s) for s in BAD_SCALES] + [((8192, 8192), 4.0)]:
            with pytest.raises(BackendError, match="rfw_hip error -1"):
                p.be.resize(size, s)
            assert p.be.render_size() == (32, 32) and (p.be.width, p.be.height) == (64, 64)
            assert same(p.be.framebuffer(), before) and same(p.be.accumulator(), acc)  # the previous frame's bits
        buf = np.zeros((64, 64, 4), np.float32)  # a window-sized buffer for the accumulator of a scaled backend
        assert p.be._l.rfw_hip_read_accumulator(p.be._h, buf.ctypes.data, buf.size) == -1
        assert p.be._l.rfw_hip_read_accumulator(p.be._h, buf.ctypes.data, 32 * 32 * 4) == 0
        assert p.be._l.rfw_hip_read_framebuffer(p.be._h, buf.ctypes.data, 32 * 32 * 4) == -1
        with pytest.raises(BackendError, match="rfw_hip error -1"):
            p.be.set_option("scale_filter", 2)
        for call in (lambda: p.be.comm_init_loopback(0x5ca1e, 0, 1), lambda: p.be.set_slab_output(0), lambda: p.be.p2p_export(),
                     lambda: p.be.assemble_frame(0), lambda: p.be.comm_init(bytes(128), 0, 1)):
            with pytest.raises(BackendError, match="rfw_hip error -3"):  # RFW_HIP_E_STATE
                call()
        assert same(p.be.framebuffer(), before)
    finally:
        p.close()
    # a resize to a scale that changes the size on an instance that exchanges its frame: refused, untouched
    be = backend(64, 64, 1.0)
    try:
        be.comm_init_loopback(0x5ca1f, 0, 1)
        with pytest.raises(BackendError, match="rfw_hip error -3"):
            be.resize((64, 64), 0.5)
        assert be.render_size() == (64, 64)
        be.resize((64, 64), 1.004)  # truncates to the window: no scaled frame, nothing to refuse
    finally:
        be.close()
