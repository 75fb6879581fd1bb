"""The display transform (include/rfw_hip.h option "tonemap", DESIGN.md "Display transform", csrc/display.inc): exposure, automatic exposure
from a luminance histogram, and three tone-map curves over the finished frame of a path-traced image.

The yardstick is the restatement below — the header's definition in Python ints and one numpy float32 operation per step: the histogram,
the resolve, the adaptation and the curves.  Synthetic frames go through HipBackend.debug_display (the very launches a frame issues);
rendered frames are held against the restatement of a TWIN's frame: a second backend with the same scene and calls and "tonemap" 0.
Comparisons are on bits, except that a NaN matches any NaN (the default NaN's sign differs between x86 numpy and the device).  Frames of a
few thousand pixels, so that tests/test_display_on_cpu.py can run the file on the emulated library too."""
import numpy as np
import pytest

from rfw_rs_amd import BackendError, HipBackend, RenderMode, Scene

gpu = pytest.mark.gpu
f32 = np.float32
F1 = f32(1.0)
CR, CG, CB = f32(0.2126), f32(0.7152), f32(0.0722)
ONE_BITS = 0x3F800000

DEFAULTS = dict(tonemap=0, exposure=1.0, tonemap_white=4.0, auto_exposure=0, exposure_key=0.18, exposure_min=1.0 / 64.0, exposure_max=64.0,
                exposure_low=50, exposure_high=95, exposure_speed=0.125)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def as_float(u):
    return np.array([u], np.uint32).view(np.float32)[0]


def bits_of(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def differing(a, b):
    """positions where a and b differ in bits and are not both NaN"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.argwhere((bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b)))


def same(a, b):
    return len(differing(a, b)) == 0


def same_scalar(a, b):
    return bits_of(a) == bits_of(b) or (np.isnan(a) and np.isnan(b))


# ---------------------------------------------------------------- the restatement
def luminance(frame):
    c = np.ascontiguousarray(frame, np.float32)
    with np.errstate(all="ignore"):
        r, g, b = c[..., 0] * c[..., 0], c[..., 1] * c[..., 1], c[..., 2] * c[..., 2]
        Y = CR * r
        Y = Y + CG * g
        Y = Y + CB * b
    assert Y.dtype == np.float32
    return Y


def histogram(frame):
    Y = luminance(frame).reshape(-1)
    with np.errstate(invalid="ignore"):
        counts = Y >= f32(2.0 ** -16)  # NaN, zero, negatives and denormals do not count
    b = np.minimum(255, (bits(Y[counts]).astype(np.int64) >> 20) - 888)
    assert (b >= 0).all()
    return np.bincount(b, minlength=256).astype(np.uint32)


def resolve(hist, o, prev):
    """(E, E*, q, N) from the 256 counts under the options o; prev: the previous exposure or None"""
    c = [int(x) for x in hist]
    N = sum(c)
    lo, hi = (N * int(o["exposure_low"])) // 100, (N * int(o["exposure_high"])) // 100
    S, cum = 0, 0
    for k in range(256):
        S += k * max(0, min(cum + c[k], hi) - max(cum, lo))
        cum += c[k]
    C = hi - lo
    q = 0
    if C == 0:
        target = prev if prev is not None else F1
    else:
        q = (S * 256) // C
        lfix = ((q + 128) << 12) - (16 << 23)
        kfix = bits_of(f32(o["exposure_key"])) - ONE_BITS
        e = ONE_BITS + kfix - lfix
        e = max(bits_of(f32(o["exposure_min"])), min(bits_of(f32(o["exposure_max"])), e))
        target = as_float(e)
    if prev is None:
        E = target
    else:
        d = f32(target) - f32(prev)
        d = d * f32(o["exposure_speed"])
        E = f32(prev) + d
    return f32(E), f32(target), q, N


def curve(lin, E, o):
    k = int(o["tonemap"])
    with np.errstate(all="ignore"):
        v = lin * f32(E)
        if k == 1:
            m = v
        elif k == 2:
            W = f32(o["tonemap_white"])
            t = v / (W * W)
            t = F1 + t
            n = v * t
            dd = F1 + v
            m = n / dd
        else:
            n = f32(2.51) * v
            n = n + f32(0.03)
            n = v * n
            dd = f32(2.43) * v
            dd = dd + f32(0.59)
            dd = v * dd
            dd = dd + f32(0.14)
            m = n / dd
            m = np.where(m < 0, f32(0.0), m)  # compares: a NaN passes through
            m = np.where(m > 1, F1, m)
        out = np.sqrt(m)
    assert out.dtype == np.float32
    return out


def apply(frame, E, o):
    c = np.ascontiguousarray(frame, np.float32)
    out = c.copy()  # w is copied
    with np.errstate(all="ignore"):
        for ch in range(3):
            out[..., ch] = curve(c[..., ch] * c[..., ch], E, o)
    return out


def transform(frame, o, prev=None):
    """the whole stage: (frame out, counts, (E, E*, q, N)); the counts and the resolve only with automatic exposure"""
    if int(o["tonemap"]) == 0:
        return np.ascontiguousarray(frame, np.float32).copy(), np.zeros(256, np.uint32), (f32(0), f32(0), 0, 0)
    if int(o["auto_exposure"]):
        hist = histogram(frame)
        st = resolve(hist, o, prev)
    else:
        hist, st = np.zeros(256, np.uint32), (f32(o["exposure"]), f32(o["exposure"]), 0, 0)
    return apply(frame, st[0], o), hist, st


def check_state(got, want):
    assert got is not None
    assert same_scalar(got["exposure"], want[0]) and same_scalar(got["target"], want[1]) and (got["q"], got["n"]) == (want[2], want[3]), (got, want)


# ---------------------------------------------------------------- options
def configure(be, **changes):
    """every option of the stage to its default, then `changes`; in an order in which no intermediate state is refused"""
    o = dict(DEFAULTS, **changes)
    be.set_option("exposure_min", 2.0 ** -20)
    be.set_option("exposure_max", o["exposure_max"])
    be.set_option("exposure_min", o["exposure_min"])
    be.set_option("exposure_low", 0)
    be.set_option("exposure_high", o["exposure_high"])
    be.set_option("exposure_low", o["exposure_low"])
    for k in ("tonemap", "exposure", "tonemap_white", "auto_exposure", "exposure_key", "exposure_speed"):
        be.set_option(k, o[k])
    return o


# ---------------------------------------------------------------- synthetic frames
def pixel_with_luminance(T):
    """(x, 0, z) whose luminance is exactly the float T > 0"""
    T = f32(T)
    with np.errstate(all="ignore"):
        x0 = np.sqrt(T / CR)
        xs = (np.full(96, bits_of(x0), np.int64) - np.arange(96)).astype(np.uint32).view(np.float32)
        Y0 = CR * (xs * xs)
        delta = T - Y0
        ok = delta >= 0
        z0 = np.sqrt(np.where(ok, delta, 0) / CB).astype(np.float32)
        zs = (bits(z0).astype(np.int64)[:, None] + np.arange(-4, 5)[None, :]).clip(0).astype(np.uint32).view(np.float32)
        Y = Y0[:, None] + CB * (zs * zs)
    hit = np.argwhere((bits(Y) == bits_of(T)) & ok[:, None])
    assert len(hit), T
    i, j = hit[0]
    p = np.array([xs[i], 0.0, zs[i, j], 1.0], np.float32)
    assert bits_of(luminance(p[None])[0]) == bits_of(T)
    return p


_EDGES = []


def edge_pixels():
    """per bin k its lower edge exactly and the largest float below it: 512 pixels, of which [2 k] lands in bin k and [2 k + 1] in bin k - 1
    (k = 0: below 2^-16, it does not count)"""
    if not _EDGES:
        px = []
        for k in range(256):
            edge = (888 + k) << 20
            px.append(pixel_with_luminance(as_float(edge)))
            px.append(pixel_with_luminance(as_float(edge - 1)))
        _EDGES.append(np.stack(px))
    return _EDGES[0]


def content(kind, n):
    rng = np.random.default_rng(1000 * KINDS.index(kind) + n)
    if kind == "ramp":  # every bin, exactly on its edges; the first 64 pixels are 64 DISTINCT bins (one wavefront)
        e = edge_pixels()
        order = np.concatenate([np.arange(0, 512, 8), np.setdiff1d(np.arange(512), np.arange(0, 512, 8))])
        px = e[order][np.arange(n) % 512]
    elif kind == "special":
        sp = np.array([pixel_with_luminance(2.0 ** 16), pixel_with_luminance(as_float(bits_of(f32(2.0 ** 16)) - 1)),
                       [np.inf, 0.5, 0.5, 1.0], [0.5, -np.inf, 0.0, 1.0], [np.nan, 0.5, 0.5, 0.0], [0.5, 0.5, np.nan, 1.0],
                       [0.0, 0.0, 0.0, 1.0], [-0.0, 0.0, -0.0, 1.0], [-0.5, -0.25, -2.0, 1.0], [-3.0, 0.5, 0.0, 0.5],
                       [1e-20, 1e-20, 1e-20, 1.0], [1e-30, 2e-23, 0.0, 1.0], [1.0e-19, 0.0, 1.1e-19, 1.0],
                       pixel_with_luminance(2.0 ** -16), pixel_with_luminance(as_float(bits_of(f32(2.0 ** -16)) - 1)),
                       [1.0e19, 1.0e19, 1.0e19, 1.0], [2.0e19, 0.0, 0.0, 1.0]], np.float32)
        fill = np.exp(rng.normal(-1.0, 2.0, (n, 4))).astype(np.float32)
        px = np.where((np.arange(n) % 3 == 0)[:, None], sp[(np.arange(n) // 3) % len(sp)], fill)
    elif kind == "black":
        px = np.zeros((n, 4), np.float32)
        px[:, 3] = 1.0
    elif kind == "onebin":  # different values, one bin: Y of a grey s is about s^2, [0.286, 0.3025] lies inside [0.28125, 0.3125)
        s = rng.uniform(0.535, 0.55, n).astype(np.float32)
        px = np.stack([s, s, s, np.ones(n, np.float32)], axis=-1)
    elif kind == "equal":  # a whole wavefront in one bin, one value
        px = np.tile(np.array([0.75, 0.5, 0.25, 1.0], np.float32), (n, 1))
    else:  # "hdr": a wide spread of ordinary values
        px = np.exp(rng.normal(-1.0, 2.5, (n, 4))).astype(np.float32)
    return np.ascontiguousarray(px, np.float32)


SIZES = [(1, 1), (63, 1), (65, 3), (257, 5), (64, 64)]
KINDS = ["ramp", "special", "black", "onebin", "equal", "hdr"]
AUTO = dict(tonemap=3, auto_exposure=1)

_BE = []


def shared_backend():
    if not _BE:
        _BE.append(HipBackend.init(16, 16, 1.0))
    return _BE[0]


def check_display(be, frame, o, prev=None):
    got, hist, state = be.debug_display(frame, 0.0 if prev is None else float(prev))
    want, whist, wstate = transform(frame, o, None if prev is None else f32(prev))
    assert np.array_equal(hist, whist), np.argwhere(hist != whist)[:8]
    if int(o["tonemap"]):
        check_state(state, wstate)
    bad = differing(got, want)
    assert len(bad) == 0, (len(bad), bad[:4])
    assert np.array_equal(bits(got[..., 3]), bits(frame[..., 3]))  # w is copied
    return wstate


@gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_synthetic_frames(kind, size):
    w, h = size
    be = shared_backend()
    frame = content(kind, w * h).reshape(h, w, 4)
    hist = histogram(frame)
    if kind == "ramp" and w * h >= 512:
        assert (hist > 0).all()  # every bin
    if kind == "ramp" and w * h >= 64:
        assert len(np.unique(np.minimum(255, (bits(luminance(frame).reshape(-1)[:64]).astype(np.int64) >> 20) - 888))) == 64
    if kind in ("onebin", "equal"):
        assert np.count_nonzero(hist) == 1 and hist.sum() == w * h
    if kind == "black":
        assert hist.sum() == 0
    o = configure(be, **AUTO)
    st = check_display(be, frame, o)
    st2 = check_display(be, frame, o, prev=0.37)
    if kind == "black":  # N = 0: E stays at the previous value, or 1
        assert bits_of(st[0]) == bits_of(F1) and bits_of(st2[0]) == bits_of(f32(0.37)) and st[3] == 0
    for k in (1, 2):
        check_display(be, frame, configure(be, tonemap=k, auto_exposure=1), prev=2.5)


def test_the_yardsticks_own_edges():
    """the restatement itself (no device needed): the bin edges, what does not count, and the inverse of the binning's log"""
    e = edge_pixels()
    Y = luminance(e)
    assert bits_of(Y[0]) == bits_of(f32(2.0 ** -16)) and bits_of(Y[1]) == bits_of(f32(2.0 ** -16)) - 1
    for k in (0, 1, 17, 254, 255):
        h = histogram(e[2 * k][None])
        assert h[k] == 1 and h.sum() == 1
        h = histogram(e[2 * k + 1][None])
        assert h.sum() == (0 if k == 0 else 1) and (k == 0 or h[k - 1] == 1)
    big = np.array([[np.inf, 0, 0, 1], [1e19, 1e19, 1e19, 1], [np.nan, 1, 1, 1], [0, 0, 0, 1], [1e-20, 0, 0, 1]], np.float32)
    assert list(np.nonzero(histogram(big))[0]) == [255] and histogram(big)[255] == 2
    # a frame whose pixels all sit at the centre of bin 128 + 5 (Y = 2^0 * (1 + 5.5 / 8)) is exposed to key / Y exactly
    o = dict(DEFAULTS, **AUTO, exposure_low=0, exposure_high=100, exposure_key=0.25)
    hist = np.zeros(256, np.uint32)
    hist[133] = 10
    E, target, q, N = resolve(hist, o, None)
    assert (q, N) == (133 * 256, 10) and bits_of(E) == bits_of(target)
    # log2 E* = log2 key - log2' Y with log2' the piecewise-linear log of the binning: -2 - 5.5 / 8 -> mantissa 1 - 5.5/8 of the octave below
    assert bits_of(target) == ONE_BITS - (2 << 23) - ((5 << 20) + (1 << 19))


VARIANTS = [
    dict(AUTO, exposure_low=0, exposure_high=100),
    dict(AUTO, exposure_low=50, exposure_high=95),
    dict(AUTO, exposure_low=99, exposure_high=100),      # with N < 100: C == 1, the one brightest pixel (C == 0 needs lo == hi, N == 0 here)
    dict(AUTO, exposure_low=98, exposure_high=99),       # with N < 50: lo == hi == N - 1, C == 0
    dict(AUTO, exposure_min=4.0, exposure_max=8.0),       # the clamp from below (the frames below want less than 4) ...
    dict(AUTO, exposure_min=2.0 ** -12, exposure_max=2.0 ** -9),  # ... and from above
    dict(AUTO, exposure_speed=1.0),
    dict(AUTO, exposure_speed=0.125, exposure_key=0.5),
    dict(AUTO, tonemap=1),
    dict(AUTO, tonemap=2),
    dict(AUTO, tonemap=2, tonemap_white=1.5),
    dict(tonemap=1, exposure=0.25),
    dict(tonemap=2, exposure=8.0, tonemap_white=11.0),
    dict(tonemap=3, exposure=0.25),
    dict(tonemap=3, exposure=8.0),
    dict(tonemap=0, exposure=8.0, auto_exposure=1),       # off: the frame comes back as it went in
]


@gpu
@pytest.mark.parametrize("variant", range(len(VARIANTS)))
def test_options(variant):
    be = shared_backend()
    o = configure(be, **VARIANTS[variant])
    for kind, (w, h) in (("hdr", (65, 3)), ("hdr", (9, 7)), ("special", (257, 5)), ("onebin", (64, 2))):
        frame = content(kind, w * h).reshape(h, w, 4)
        a = check_display(be, frame, o)
        b = check_display(be, frame, o, prev=3.0)
        c = check_display(be, frame, o, prev=2.0 ** -11)
        if int(o["tonemap"]) and int(o["auto_exposure"]):
            if o["exposure_low"] == 99 and kind == "hdr" and w * h < 100:
                top = int(np.nonzero(histogram(frame))[0][-1])
                assert a[3] == w * h and a[2] == 256 * top  # C == 1: q is the brightest pixel's bin
            if o["exposure_low"] == 98 and w * h < 50:
                assert a[3] == w * h and a[2] == 0 and bits_of(a[0]) == bits_of(F1) and bits_of(b[0]) == bits_of(f32(3.0))  # C == 0
            if o["exposure_min"] == 4.0 and kind == "hdr":
                assert bits_of(a[1]) in (bits_of(f32(4.0)), bits_of(f32(8.0)))
            if o["exposure_max"] == 2.0 ** -9:
                assert bits_of(a[1]) in (bits_of(f32(2.0 ** -12)), bits_of(f32(2.0 ** -9)))
            if o["exposure_speed"] == 1.0 and a[3] > 1:
                assert bits_of(b[1]) == bits_of(a[1])
            assert bits_of(a[0]) == bits_of(a[1])  # no previous exposure: E = E*
    configure(be)


def test_clamps_are_hit_from_both_sides():
    """the yardstick: a dark frame wants more than exposure_max, a bright one less than exposure_min (no device needed)"""
    o = dict(DEFAULTS, **AUTO, exposure_low=0, exposure_high=100)
    dark, bright = np.zeros(256, np.uint32), np.zeros(256, np.uint32)
    dark[8], bright[250] = 100, 100
    assert bits_of(resolve(dark, o, None)[1]) == bits_of(f32(64.0)) and bits_of(resolve(bright, o, None)[1]) == bits_of(f32(1.0 / 64.0))


# ---------------------------------------------------------------- rendered frames: a backend and its twin
_SCENE = []


def cornell():
    if not _SCENE:
        _SCENE.append(Scene().build("cornell"))
    return _SCENE[0]


W, H = 48, 40


def backend(w=W, h=H, scale=1.0, options=(), **init):
    scene = cornell()
    be = HipBackend.init(w, h, scale, max_path_length=2, **init)
    for k, v in options:
        be.set_option(k, v)
    scene.mark_all_changed()
    scene.sync(be)
    return be


def views(n, w=W, h=H):
    scene, out = cornell(), []
    for k in range(n):
        scene.set_camera([0.0, 0.0, -3.4 + 0.35 * k], [0.06 * k, -0.03 * k, 1.0], fov=40.0, aspect=w / h)
        out.append(scene.view(w, h))
    return out


class Pair:
    """a backend with the display transform on, and its twin: the same scene, options and calls, "tonemap" 0"""

    def __init__(self, display, options=(), w=W, h=H, scale=1.0, **init):
        self.be, self.twin = backend(w, h, scale, options, **init), backend(*HipBackend_render_size(w, h, scale), 1.0, options, **init)
        self.o = configure(self.be, **display)
        self.prev = None  # the restatement's adaptation state

    def both(self, call):
        for be in (self.be, self.twin):
            call(be)

    def check(self, frame=None):
        """the latest frame against the restatement of the twin's; advances the restatement's state"""
        src = self.twin.framebuffer()
        assert src[..., :3].any()
        want, hist, st = transform(src, self.o, self.prev)
        if int(self.o["tonemap"]) and int(self.o["auto_exposure"]):
            self.prev = st[0]
            assert np.array_equal(self.be.display_histogram(), hist)
        if int(self.o["tonemap"]):
            check_state(self.be.display_state(), st)
        got = self.be.framebuffer() if frame is None else frame
        bad = differing(got, want)
        assert len(bad) == 0, (len(bad), bad[:4])
        assert not same(want, src)  # (the transform shows)
        assert same(self.be.accumulator(), self.twin.accumulator())  # the accumulator never sees it
        return want, st

    def close(self):
        self.be.close()
        self.twin.close()


def HipBackend_render_size(w, h, scale):
    return max(1, int(w * scale)), max(1, int(h * scale))


@gpu
@pytest.mark.parametrize("display", [dict(tonemap=1, exposure=8.0), dict(tonemap=2, exposure=0.25, tonemap_white=2.0), dict(tonemap=3, exposure=2.0)])
def test_manual_exposure(display):
    p = Pair(display)
    try:
        v = views(1)[0]
        for _ in range(3):  # samples of one image
            p.both(lambda be: be.render(v))
            p.check()
    finally:
        p.close()


@gpu
def test_automatic_exposure_adapts_across_images():
    p = Pair(AUTO)
    try:
        seen = []
        for v in views(6):
            p.both(lambda be: be.render(v))
            _, st = p.check()
            seen.append(bits_of(st[0]))
        assert len(set(seen)) > 3  # (the exposure moves)
        # reset_accumulation and a new sample of the same image keep the state
        p.both(lambda be: be.reset_accumulation())
        p.both(lambda be: be.render(v))
        _, st = p.check()
        assert bits_of(st[0]) != bits_of(st[1])  # still adapting: E is not E*
        p.both(lambda be: be.render(v))
        p.check()
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("case", ["denoise", "denoise_temporal", "substreams"])
def test_finalisers_and_substreams(case):
    options = {"denoise": [("denoise", 2)], "denoise_temporal": [("denoise", 2), ("denoise_temporal", 4)], "substreams": []}[case]
    p = Pair(AUTO, options, **({"streams": 2} if case == "substreams" else {}))
    try:
        for v in views(3):
            p.both(lambda be: be.reset_accumulation())
            for _ in range(2):
                p.both(lambda be: be.render(v))
                p.check()
        if case == "denoise_temporal":  # the history never sees the transform
            assert same(p.be.denoise_history(), p.twin.denoise_history())
    finally:
        p.close()


@gpu
def test_render_samples_batches_and_data_views():
    p = Pair(AUTO, max_batch=2)
    try:
        vs = views(2)
        p.both(lambda be: be.render_samples(vs[0], 2))
        p.check()
        p.both(lambda be: be.render(vs[1]))
        p.check()
        before = p.be.display_state()
        # data views and batches finalise as without the option and leave the state alone
        for mode in (RenderMode.ALBEDO, RenderMode.FILTERED_SSAO):
            p.both(lambda be: be.render(vs[0], None, mode))
            assert same(p.be.framebuffer(), p.twin.framebuffer()) and same(p.be.accumulator(), p.twin.accumulator())
        p.both(lambda be: be.render_batch(vs))
        for f in range(2):
            assert same(p.be.framebuffer_at(f), p.twin.framebuffer_at(f))
        check_state(p.be.display_state(), (before["exposure"], before["target"], before["q"], before["n"]))
        p.both(lambda be: be.render(vs[1]))
        p.check()
    finally:
        p.close()


@gpu
def test_frame_slots_share_one_state_in_call_order():
    one, p = Pair(AUTO), Pair(AUTO, frames_in_flight=3)
    try:
        vs = views(6)
        seq = {}
        for name, q in (("one", one), ("slots", p)):
            seq[name] = []
            for v in vs:
                q.both(lambda be: be.render(v))
                _, st = q.check()
                seq[name].append(bits_of(st[0]))
        assert seq["one"] == seq["slots"]
        # three more frames with nothing read in between: the chain is ordered on the device
        for v in vs[:3]:
            p.be.render(v)
        for v in vs[:3]:
            p.twin.render(v)
            _, _, st = transform(p.twin.framebuffer(), p.o, p.prev)
            p.prev = st[0]
        check_state(p.be.display_state(), st)
        assert same(p.be.framebuffer(), apply(p.twin.framebuffer(), st[0], p.o))
    finally:
        one.close()
        p.close()


# the render scale's filter (include/rfw_hip.h rfw_hip_create), as tests/test_gpu_render_scale.py restates it
def taps(R, N, x, filt):
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
        out.append((j, np.float32(o) / np.float32(R)))
    return out


def weighted(value, lst):
    if lst[0][1] is None:
        return value(lst[0][0]).copy()
    s = None
    for j, w in lst:
        v = value(j) * w
        s = v if s is None else s + v
    return s


def resampled(src, Wn, Hn, filt):
    src = np.ascontiguousarray(src, np.float32)
    RH, RW = src.shape[:2]
    with np.errstate(all="ignore"):
        hor = np.empty((RH, Wn, 4), np.float32)
        for x in range(Wn):
            hor[:, x, :] = weighted(lambda j: src[:, j, :], taps(RW, Wn, x, filt))
        out = np.empty((Hn, Wn, 4), np.float32)
        for y in range(Hn):
            out[y] = weighted(lambda j: hor[j], taps(RH, Hn, y, filt))
    return out


@gpu
def test_render_scale_resamples_the_transformed_frame():
    p = Pair(AUTO, w=2 * W, h=2 * H, scale=0.5)
    try:
        assert p.be.render_size() == (W, H) and (p.twin.width, p.twin.height) == (W, H)
        for v in views(2):
            p.both(lambda be: be.render(v))
            want, hist, st = transform(p.twin.framebuffer(), p.o, p.prev)
            p.prev = st[0]
            check_state(p.be.display_state(), st)
            got = p.be.framebuffer()
            assert got.shape == (2 * H, 2 * W, 4)
            bad = differing(got, resampled(want, 2 * W, 2 * H, 1))
            assert len(bad) == 0, (len(bad), bad[:4])
            assert same(p.be.accumulator(), p.twin.accumulator())
    finally:
        p.close()


def ortho(w, h):
    m = np.zeros((4, 4), np.float64)
    m[0, 0], m[1, 1], m[2, 2], m[2, 3], m[3, 3] = 2.0 / w, 2.0 / h, 1.0 / 20.0, 0.5, 1.0
    return np.ascontiguousarray(m.T.reshape(16).astype(np.float32))


def pixel_matrix(w, h):
    m = np.eye(4)
    m[0, 3], m[1, 1], m[1, 3] = -w / 2.0, -1.0, h / 2.0
    return np.ascontiguousarray(m.T.reshape(16).astype(np.float32))


@gpu
def test_2d_layer_stays_untransformed_and_presentation_encodes_the_result():
    p = Pair(dict(tonemap=3, exposure=4.0))
    try:
        colour = (0.25, 0.5, 0.75, 1.0)
        corners = [(8, 4), (24, 4), (8, 12), (24, 4), (24, 12), (8, 12)]  # columns 8 ... 23, rows 4 ... 11
        p.be.set_2d_mesh(0, np.array([[x, y, 0.0, 0.0, 0.0, 0.0, *colour] for x, y in corners], np.float32))
        p.be.set_2d_instances(0, pixel_matrix(W, H).reshape(1, 16))
        p.be.synchronize()
        v = views(1)[0]
        p.be.render(v, ortho(W, H))
        p.twin.render(v)
        want = apply(p.twin.framebuffer(), f32(4.0), p.o)
        got = p.be.framebuffer()
        inside = np.zeros((H, W), bool)
        inside[4:12, 8:24] = True
        assert p.be.overlay_stats()["drawn"] == 2
        assert np.array_equal(bits(got[inside][:, :3]), np.broadcast_to(bits(np.array(colour[:3], np.float32)), (16 * 8, 3)))  # the layer as it is without the option
        assert same(got[~inside], want[~inside])
        assert same(p.be.accumulator(), p.twin.accumulator())
        # the presented bytes are the encoding of the transformed frame
        steps = p.be.srgb_steps()
        pres = p.be.host_frame(presented=True)
        p.be.download_frame(pres)
        p.be.wait_downloads()
        enc = lambda x: np.searchsorted(steps, x, side="right").astype(np.uint8)
        assert np.array_equal(pres, np.stack([enc(got[..., 2]), enc(got[..., 1]), enc(got[..., 0]), np.full((H, W), 255, np.uint8)], axis=-1))
        p.be.free_host_frame(pres)
    finally:
        p.close()


@gpu
def test_what_drops_the_state_and_what_turns_the_stage_off():
    p = Pair(AUTO)
    try:
        vs = views(3)
        assert p.be.display_state() is None  # nothing before the first transformed frame
        for v in vs[:2]:
            p.both(lambda be: be.render(v))
            p.check()
        assert p.prev is not None
        for key in DEFAULTS:  # every option set drops the state, also to the value it has
            p.be.set_option(key, p.o[key])
            assert p.be.display_state() is None
            p.prev = None
            p.both(lambda be: be.render(vs[2]))
            _, st = p.check()
            assert bits_of(st[0]) == bits_of(st[1])  # no previous exposure: E = E*
            p.both(lambda be: be.render(vs[0]))
            _, st = p.check()
            assert bits_of(st[0]) != bits_of(st[1])  # ... and the next frame adapts from it
        # resize drops it too
        p.both(lambda be: be.resize((W, H), 1.0))
        assert p.be.display_state() is None
        p.prev = None
        p.both(lambda be: be.render(vs[1]))
        _, st = p.check()
        assert bits_of(st[0]) == bits_of(st[1])
        # "tonemap" 0 after use: the twin's frame again, nothing reported
        p.be.set_option("tonemap", 0)
        p.both(lambda be: be.render(vs[1]))
        assert same(p.be.framebuffer(), p.twin.framebuffer()) and same(p.be.accumulator(), p.twin.accumulator())
        assert p.be.display_state() is None
    finally:
        p.close()


NAN, INF = float("nan"), float("inf")
REFUSED = [
    ("tonemap", [-1, 4, 1.5, NAN, INF]),
    ("exposure", [0.0, -1.0, 2.0 ** -21, 2.0 ** 20 * 1.001, NAN, INF]),
    ("tonemap_white", [0.0, -4.0, NAN, INF, 1e-60]),
    ("auto_exposure", [2, -1, 0.5, NAN]),
    ("exposure_key", [0.0, 2.0 ** -11, 2.0 ** 10 * 1.001, NAN, INF]),
    ("exposure_min", [0.0, 2.0 ** -21, 65.0, NAN, INF]),          # (above exposure_max = 64)
    ("exposure_max", [1.0 / 128.0, 2.0 ** 20 * 1.001, NAN, INF]),  # (below exposure_min = 1 / 64)
    ("exposure_low", [-1, 95, 96, 50.5, NAN, INF]),                # (not below exposure_high = 95)
    ("exposure_high", [50, 49, 101, 94.5, NAN, INF]),              # (not above exposure_low = 50)
    ("exposure_speed", [0.0, -0.5, 1.001, NAN, INF, 1e-60]),
]


@gpu
def test_refusals():
    be = shared_backend()
    o = configure(be, tonemap=3, exposure=2.0)
    frame = content("hdr", 35).reshape(5, 7, 4)
    for key, values in REFUSED:
        for v in values:
            with pytest.raises(BackendError, match="rfw_hip error -1"):
                be.set_option(key, v)
    check_display(be, frame, o)  # a refused value changes nothing
    # the ends of the ranges are accepted
    for key, values in (("exposure", [2.0 ** -20, 2.0 ** 20]), ("exposure_key", [2.0 ** -10, 2.0 ** 10]), ("exposure_speed", [1.0]),
                        ("exposure_max", [2.0 ** 20, 1.0 / 64.0]), ("exposure_min", [1.0 / 64.0, 2.0 ** -20]), ("exposure_high", [100, 51]), ("exposure_low", [0, 50])):
        for v in values:
            be.set_option(key, v)
    with pytest.raises(BackendError, match="rfw_hip error -1"):
        be._check(be._l.rfw_hip_debug_display(be._h, None, 4, 4, 0.0, None, None, None))
    configure(be)
