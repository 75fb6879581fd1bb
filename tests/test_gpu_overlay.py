"""The 2D layer (include/rfw_hip.h set_2d_mesh / set_2d_instances / render's view_2d, DESIGN.md "2D layer", csrc/overlay.inc): the trait's 2D
meshes drawn over the finalised frame.

The restatement below rasterises in exact Python / int64 integers from the device's own snapped vertices (debug tap "ov_prims"), so coverage
has to agree on EVERY pixel: a pixel it does not cover must keep the bits of the background, which comes from a twin backend of the same
scene and options that never received 2D data.  It shades in float64 from the vertices, textures and matrices the test set and composites
in painter order.  Small frames (64 x 64, and 70 x 37 with partial tiles and a partial bin on both edges), so that
tests/test_overlay_on_cpu.py can run the file on the emulated library too.

The colour bound: the largest |frame - want| / max(1, |want|) over the cases of this file, measured on the emulated library against the
float64 restatement, is 1.67e-5 (test_texture_array_layer: the float32 texel coordinate u * 1024 - 0.5 of a 1024-wide layer carries 2^-14
of a texel, which the bilinear weights hand on to the colour); times 4, rounded up to one significant digit: 7e-5 (the rule of
tests/test_gpu_denoise_motion.py).  By kind of case: untextured 9.3e-8 at most (130 translucent layers), the 16 x 8 texture at its native
size 1.9e-6.  The MI355X runs the same float32 operations without contraction; its own largest figure,
printed by this file in a recorded run: 1.67e-5, the same case."""
import numpy as np
import pytest

from rfw_rs_amd import BackendError, HipBackend, Scene, pod

pytestmark = pytest.mark.gpu
W = H = 64
BOUND = 7e-5
WORST = [0.0]  # the largest figure seen so far in this process (printed by every comparison)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- matrices (column-major storage: m.reshape(4, 4).T is [row, column])
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


def cols(m):
    return np.asarray(m, np.float64).reshape(4, 4).T


def vert(x, y, u=0.0, v=0.0, c=(1.0, 1.0, 1.0, 1.0), z=0.0):
    return [x, y, z, 0.0, u, v, *c]  # (the fourth column is where Vertex2D keeps `tex`: ignored)


def tri(p0, p1, p2, c=(1.0, 1.0, 1.0, 1.0), uv=((0, 0), (0, 0), (0, 0))):
    return [vert(*p, *t, c) for p, t in zip((p0, p1, p2), uv)]


def quad(x0, y0, x1, y1, c=(1.0, 1.0, 1.0, 1.0), uv=(0.0, 0.0, 1.0, 1.0)):
    """two triangles sharing the diagonal (x0, y1) - (x1, y0)"""
    a, b, cc, d = (x0, y0), (x1, y0), (x1, y1), (x0, y1)
    ta, tb, tc, td = (uv[0], uv[1]), (uv[2], uv[1]), (uv[2], uv[3]), (uv[0], uv[3])
    return tri(a, b, d, c, (ta, tb, td)) + tri(b, cc, d, c, (tb, tc, td))


# ---------------------------------------------------------------- the scene and its twin
class Pair:
    """a backend that gets 2D data and a twin of the same scene and options that never does"""

    def __init__(self, w=W, h=H, textures=None, texture_array=None, options=(), **init):
        self.w, self.h = w, h
        self.scene = Scene().build("cornell")
        self.scene.set_aspect(w / h)
        self.view = self.scene.view(w, h)
        self.keep = []
        self.bes = []
        for _ in range(2):
            be = HipBackend.init(w, h, 1.0, max_path_length=2, **init)
            if texture_array is not None:
                be.set_option("texture_array", texture_array)
            for k, v in options:
                be.set_option(k, v)
            self.scene.mark_all_changed()
            self.scene.sync(be)
            self.bes.append(be)
        self.be, self.twin = self.bes
        self.textures = None
        if textures is not None:
            self.set_textures(textures)
        self.meshes = {}

    def set_textures(self, textures, changed=None):
        """textures: [(texels (h, w, 4) uint8 in the byte order of `fmt`, fmt)]; both backends get them (the twin has the same scene)"""
        self.textures = textures
        tds = []
        for texels, fmt in textures:
            t = np.ascontiguousarray(texels)
            self.keep.append(t)
            tds.append(pod.TextureData(t.shape[1], t.shape[0], 1, t.ctypes.data_as(pod.C.POINTER(pod.C.c_uint8)), fmt))
        for be in self.bes:
            be.set_textures(tds, changed)
            be.synchronize()

    def mesh(self, id, vertices, tex=None, matrices=None):
        v = np.asarray(vertices, np.float32).reshape(-1, 10)
        old = self.meshes.get(id, (None, None, None))
        self.meshes[id] = (v, tex, old[2] if matrices is None else [np.asarray(m, np.float32) for m in matrices])
        self.be.set_2d_mesh(id, v, tex)
        if matrices is not None:
            self.be.set_2d_instances(id, np.stack(self.meshes[id][2]) if len(matrices) else None)

    def instances(self, id, matrices):
        v, tex, _ = self.meshes[id]
        self.meshes[id] = (v, tex, [np.asarray(m, np.float32) for m in matrices])
        self.be.set_2d_instances(id, np.stack(self.meshes[id][2]) if len(matrices) else None)

    def frame(self, view_2d, mode=0, n=1, view=None):
        """synchronize, render n samples on both; returns (frame, background)"""
        self.be.synchronize()
        for _ in range(n):
            self.be.render(view or self.view, view_2d, mode)
            self.twin.render(view or self.view, None, mode)
        return self.be.framebuffer(), self.twin.framebuffer()

    def close(self):
        for be in self.bes:
            be.close()


# ---------------------------------------------------------------- the restatement
def stored_level0(texels, texture_array):
    """level 0 as the device keeps it: as handed over, or point-resampled to 1024 x 1024 (the source texel of the destination texel's centre)"""
    if not texture_array or texels.shape[:2] == (1024, 1024):
        return texels
    th, tw = texels.shape[:2]
    sy = ((2 * np.arange(1024) + 1) * th) // 2048
    sx = ((2 * np.arange(1024) + 1) * tw) // 2048
    return texels[sy][:, sx]


def sample(texels, fmt, u, v):
    """bilinear, repeat, byte / 255, channels in r, g, b, a order whichever way the bytes lie"""
    th, tw = texels.shape[:2]
    t = texels.astype(np.float64) / 255.0
    if fmt == 0:  # B, G, R, A bytes
        t = t[..., [2, 1, 0, 3]]
    x, y = u * tw - 0.5, v * th - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    ix, iy = x0.astype(np.int64), y0.astype(np.int64)
    t00, t10 = t[iy % th, ix % tw], t[iy % th, (ix + 1) % tw]
    t01, t11 = t[(iy + 1) % th, ix % tw], t[(iy + 1) % th, (ix + 1) % tw]
    return (t00 * (1 - fx) + t10 * fx) * (1 - fy) + (t01 * (1 - fx) + t11 * fx) * fy


def restate(bg, prims, meshes, textures=None, texture_array=0, w=W, h=H):
    """(want (h, w, 4) float64 with the background's values where nothing is drawn, touched (h, w) bool, blends (h, w) fragments per pixel)"""
    out = bg.astype(np.float64)
    touched = np.zeros((h, w), bool)
    blends = np.zeros((h, w), np.int64)
    n_tex = len(textures) if textures else 0
    py, px = np.mgrid[0:h, 0:w].astype(np.int64)
    cx, cy = 256 * px + 128, 256 * py + 128
    for p in prims:
        if p["dropped"]:
            continue
        verts, tex, _ = meshes[int(p["mesh"])]
        v = verts[3 * int(p["triangle"]): 3 * int(p["triangle"]) + 3].astype(np.float64)
        X, Y = [int(a) for a in p["X"]], [int(a) for a in p["Y"]]
        order = [0, 1, 2]
        S = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
        assert S != 0
        if S < 0:
            order, S = [0, 2, 1], -S
        E, inside = [], np.ones((h, w), bool)
        for i in range(3):
            a, b = order[i], order[(i + 1) % 3]
            dx, dy = X[b] - X[a], Y[b] - Y[a]
            e = dx * (cy - Y[a]) - dy * (cx - X[a])  # exact: int64, |e| < 2^48
            owns = dy < 0 or (dy == 0 and dx > 0)    # a left edge, or a top edge
            inside &= (e >= 0) if owns else (e > 0)
            E.append(e)
        if not inside.any():
            continue
        lam = [E[1][inside] / S, E[2][inside] / S, E[0][inside] / S]  # vertex order[k] weighs lam[k]
        att = sum(lam[k][:, None] * v[order[k]][None, 4:] for k in range(3))  # u, v, r, g, b, a
        src = att[:, 2:6]
        if tex is not None:
            assert tex < n_tex
            texels, fmt = textures[tex]
            src = src * sample(stored_level0(texels, texture_array), fmt, att[:, 0], att[:, 1])
        a = src[:, 3]
        keep = np.isfinite(a) & (a > 0)
        dst = out[inside]
        opaque = keep & (a >= 1)
        blend = keep & ~opaque
        dst[opaque, :3] = src[opaque, :3]
        dst[blend, :3] = a[blend, None] * src[blend, :3] + (1 - a[blend, None]) * dst[blend, :3]
        out[inside] = dst
        t = np.zeros((h, w), bool)
        t[inside] = keep
        touched |= t
        blends += t
    return out, touched, blends


def check(frame, bg, want, touched, what=""):
    """untouched pixels keep the background's bits; touched ones are within BOUND of the restatement; alpha always keeps its bits"""
    assert np.array_equal(bits(frame)[~touched], bits(bg)[~touched]), f"{what}: a pixel outside the restated coverage changed"
    assert np.array_equal(bits(frame[..., 3]), bits(bg[..., 3])), f"{what}: dst.w changed"
    f, g = frame[touched][:, :3].astype(np.float64), want[touched][:, :3]
    err = np.abs(f - g) / np.maximum(1.0, np.abs(g))
    worst = float(err.max()) if err.size else 0.0
    WORST[0] = max(WORST[0], worst)
    print(f"overlay {what}: {int(touched.sum())} pixels, largest |frame - want| / max(1, |want|) = {worst:.3g} (so far {WORST[0]:.3g}, bound {BOUND:g})")
    assert np.all(np.isfinite(f)) and worst <= BOUND, (what, worst)


def draw_and_check(pair, view_2d, mode=2, what="", texture_array=0, n=1):
    frame, bg = pair.frame(view_2d, mode, n)
    prims = pair.be.overlay_prims()
    want, touched, blends = restate(bg, prims, pair.meshes, pair.textures, texture_array, pair.w, pair.h)
    check(frame, bg, want, touched, what)
    return frame, bg, prims, touched, blends


# ---------------------------------------------------------------- 1. nothing set is nothing done
@pytest.mark.parametrize("mode,denoise", [(0, 0), (2, 0), (6, 0), (0, 3)])
def test_nothing_set_is_nothing_done(mode, denoise):
    pair = Pair(options=(("denoise", denoise),) if denoise else ())
    be, twin = pair.be, pair.twin
    pres, pres_twin = be.host_frame(presented=True), twin.host_frame(presented=True)

    def same(what):
        twin.render(pair.view, None, mode)
        twin.download_frame(pres_twin); twin.wait_downloads()
        be.download_frame(pres); be.wait_downloads()
        assert np.array_equal(bits(be.framebuffer()), bits(twin.framebuffer())), what
        assert np.array_equal(bits(be.accumulator()), bits(twin.accumulator())), what
        assert np.array_equal(pres, pres_twin), what
        assert be.overlay_stats() == {"drawn": 0, "dropped": 0, "bin_words": 0}, what
        assert len(be.overlay_prims()) == 0
        a, b = be.frame_stats(), twin.frame_stats()
        assert a.keys() == b.keys() and all(a[k] == b[k] for k in a if not k.startswith("ms_")), what  # no extra stage, no extra time slot

    v2 = ortho(W, H)
    be.render(pair.view, v2, mode); same("no 2D data")
    be.set_2d_mesh(7, None); be.set_2d_instances(7, None); be.synchronize()
    be.render(pair.view, v2, mode); same("an empty mesh")
    be.set_2d_mesh(3, quad(8, 8, 40, 40)); be.synchronize()
    be.render(pair.view, v2, mode); same("a mesh without instances")
    be.set_2d_instances(3, [pixel_matrix(W, H)]); be.synchronize()
    be.render(pair.view, None, mode); same("view_2d = None")
    be.render(pair.view, v2, mode)
    assert be.overlay_stats()["drawn"] == 2 and not np.array_equal(bits(be.framebuffer()), bits(twin.framebuffer()))
    pair.close()


# ---------------------------------------------------------------- 2. the transform and the snap
def snapped_f64(verts, matrix, view_2d, w, h):
    """rint(256 * pixel position) in float64, per vertex: (n, 2)"""
    p = np.concatenate([verts[:, :3].astype(np.float64), np.ones((len(verts), 1))], axis=1)
    clip = (cols(view_2d) @ (cols(matrix) @ p.T)).T
    x = (clip[:, 0] / clip[:, 3] * 0.5 + 0.5) * w
    y = (0.5 - 0.5 * clip[:, 1] / clip[:, 3]) * h
    return np.stack([np.rint(x * 256), np.rint(y * 256)], axis=1)


def test_the_transform_and_the_snap():
    rng = np.random.default_rng(5)
    # 64 x 64: a quarter-pixel grid under Camera2D and the font's pixel matrix — every operation is exact in float32
    pair = Pair()
    g = rng.integers(-40, 4 * 64 + 40, size=(60, 3, 2)) / 4.0
    verts = [v for t in g for v in tri(*[tuple(p) for p in t], c=(0.2, 0.9, 0.4, 0.5))]
    pair.mesh(1, verts, None, [pixel_matrix(W, H)])
    _, _, prims, _, _ = draw_and_check(pair, ortho(W, H), what="quarter-pixel grid")
    want = snapped_f64(pair.meshes[1][0], pixel_matrix(W, H), ortho(W, H), W, H).reshape(-1, 3, 2)
    live = prims["dropped"] == 0
    assert live.sum() >= 55
    assert np.array_equal(prims["X"][live], want[live, :, 0].astype(np.int32)) and np.array_equal(prims["Y"][live], want[live, :, 1].astype(np.int32))
    assert np.array_equal(prims["triangle"], np.arange(60)) and np.all(prims["mesh"] == 1) and np.all(prims["instance"] == 0)
    pair.close()
    # 70 x 37 and a rotated, scaled instance: within one unit everywhere, equal nearly everywhere
    w, h = 70, 37
    pair = Pair(w, h)
    g = rng.uniform(-10, 80, size=(80, 3, 2))
    verts = [v for t in g for v in tri(*[tuple(p) for p in t], c=(0.9, 0.3, 0.1, 0.7))]
    c, s = np.cos(0.3) * 0.8, np.sin(0.3) * 0.8
    rot = np.eye(4); rot[0, 0], rot[0, 1], rot[1, 0], rot[1, 1], rot[0, 3], rot[1, 3] = c, -s, s, c, 6.0, -9.0
    m = (cols(pixel_matrix(w, h)) @ rot).T.reshape(16).astype(np.float32)
    pair.mesh(1, verts, None, [m])
    _, _, prims, _, _ = draw_and_check(pair, ortho(w, h), what="70 x 37 rotated")
    want = snapped_f64(pair.meshes[1][0], m, ortho(w, h), w, h).reshape(-1, 3, 2)
    live = prims["dropped"] == 0
    got = np.stack([prims["X"], prims["Y"]], axis=2)[live].astype(np.float64)
    assert live.sum() >= 70 and np.abs(got - want[live]).max() <= 1 and (got == want[live]).mean() >= 0.99
    pair.close()


def test_dropped_primitives_and_both_windings():
    pair = Pair()
    pm, v2 = pixel_matrix(W, H), ortho(W, H)
    wneg = np.array(pm); wneg[15] = -1.0            # w = -1
    far = np.array(pm); far[12] += 20000.0          # |x_pix| > 16384
    good_ccw = tri((10, 10), (30, 10), (10, 30), c=(1.0, 0.0, 0.0, 1.0))
    good_cw = tri((40, 40), (40, 60), (60, 40), c=(0.0, 1.0, 0.0, 1.0))
    pair.mesh(0, good_ccw + good_cw + tri((5, 5), (9, 9), (13, 13)), None, [pm, np.zeros(16, np.float32), wneg, far])
    pair.mesh(1, tri((np.nan, 5), (20, 5), (5, 20)) + tri((5, 5), (20, 5), (5, 20), c=(0.0, 0.0, 1.0, 0.5)), None, [pm])
    frame, bg, prims, touched, _ = draw_and_check(pair, v2, what="dropped")
    assert list(prims["dropped"]) == [0, 0, 1] + [1] * 9 + [1, 0]  # zero area; zero matrix, w <= 0, too far (3 each); NaN vertex
    assert list(prims["instance"]) == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3 + [0, 0]
    assert pair.be.overlay_stats()["drawn"] == 3 and pair.be.overlay_stats()["dropped"] == 11
    assert touched[15, 15] and touched[50, 45] and np.all(frame[15, 15, :3] == (1, 0, 0)) and np.all(frame[50, 45, :3] == (0, 1, 0)), "both windings are drawn"
    pair.close()


# ---------------------------------------------------------------- 3. the fill rule
@pytest.mark.parametrize("size", [(64, 64), (70, 37)])
def test_the_fill_rule(size):
    w, h = size
    pair = Pair(w, h)
    pm, v2 = pixel_matrix(w, h), ortho(w, h)
    half = (0.9, 0.2, 0.6, 0.5)
    # vertices exactly on pixel centres: a translucent quad of two triangles
    pair.mesh(0, quad(4.5, 3.5, 20.5, 17.5, half), None, [pm])
    frame, bg, _, touched, blends = draw_and_check(pair, v2, what="quad on pixel centres")
    # top and left edges own their pixels, bottom and right do not: centres 4.5 .. 19.5 x 3.5 .. 16.5
    want = np.zeros((h, w), bool); want[3:17, 4:20] = True
    assert np.array_equal(touched, want) and blends.max() == 1, "every covered pixel exactly once, the diagonal without a seam"
    assert np.all(np.abs(frame[want][:, :3] - (0.5 * np.array(half[:3]) + 0.5 * bg[want][:, :3])) <= 1e-6)
    # two abutting quads and thin slivers that cover no centre
    pair.mesh(0, quad(2, 2, 11.5, 9, half) + quad(11.5, 2, 23, 9, (0.1, 0.8, 0.3, 0.5))
              + tri((30.6, 1.0), (30.9, 30.0), (30.7, 30.0), half) + tri((1.0, 20.6), (40.0, 20.9), (40.0, 20.7), half), None, [pm])
    frame, bg, prims, touched, blends = draw_and_check(pair, v2, what="abutting quads, slivers")
    want = np.zeros((h, w), bool); want[2:9, 2:23] = True
    assert np.array_equal(touched, want) and blends.max() == 1 and not prims["dropped"].any(), "the shared edge: once; the slivers: nothing"
    # a triangle partly outside every frame edge (negative coordinates too), and one that spans every tile and bin
    pair.mesh(0, tri((-30.0, -20.0), (w + 25.0, h * 0.4), (w * 0.3, h + 40.0), (0.3, 0.3, 0.9, 0.25))
              + tri((-3.0 * w, -h), (3.0 * w, -h), (w / 2.0, 4.0 * h), (1.0, 1.0, 0.2, 0.125)), None, [pm])
    frame, bg, prims, touched, blends = draw_and_check(pair, v2, what="outside every edge, spanning the frame")
    assert touched.all() and blends.max() == 2 and blends.min() == 1 and pair.be.overlay_stats()["drawn"] == 2
    pair.close()


# ---------------------------------------------------------------- 4. order
def test_order():
    rng = np.random.default_rng(11)
    pair = Pair(70, 37)
    w, h = 70, 37
    pm, v2 = pixel_matrix(w, h), ortho(w, h)
    verts = []
    for k in range(130):  # all of them over the pixels around (30, 18): 63 | 64, 65 and 127 | 128 lie in different ballot words
        c = (*rng.uniform(0.05, 1.0, 3), rng.uniform(0.2, 0.8))
        o = rng.uniform(-6, 6, 2)
        verts += tri((10 + o[0], 4 + o[1]), (58 + o[0], 12 + o[1]), (24 + o[0], 34 + o[1]), c)
    pair.mesh(0, verts, None, [pm])
    frame, bg, prims, touched, blends = draw_and_check(pair, v2, what="130 translucent layers")
    assert blends.max() == 130 and pair.be.overlay_stats()["bin_words"] == 2 * 1 * 3
    # two meshes with ids out of insertion order, three instances of one mesh
    pair.mesh(0, [], None, [])
    shift = lambda dx, dy: (cols(pm) @ np.array([[1, 0, 0, dx], [0, 1, 0, dy], [0, 0, 1, 0], [0, 0, 0, 1.0]])).T.reshape(16).astype(np.float32)
    pair.mesh(9, quad(5, 5, 40, 30, (1.0, 0.1, 0.1, 0.6)), None, [pm])
    pair.mesh(4, quad(20, 10, 60, 35, (0.1, 0.1, 1.0, 0.6)), None, [shift(0, 0), shift(-8, -6), shift(5, 2)])
    frame, bg, prims, touched, blends = draw_and_check(pair, v2, what="meshes by id, instances by index")
    assert list(prims["mesh"]) == [4] * 6 + [9] * 2 and list(prims["instance"]) == [0, 0, 1, 1, 2, 2, 0, 0]
    assert blends.max() == 4
    pair.close()


# ---------------------------------------------------------------- 5. texture
def texture(seed, tw=16, th=8):
    t = np.random.default_rng(seed).integers(0, 256, size=(th, tw, 4), dtype=np.uint8)
    t[:, : tw // 2, 3] = 255
    return t


@pytest.mark.parametrize("fmt", [0, 1])
def test_texture_native_size(fmt):
    pair = Pair(textures=[(texture(1), fmt), (texture(2), fmt)], texture_array=0)
    pm, v2 = pixel_matrix(W, H), ortho(W, H)
    tint = (0.9, 0.7, 0.5, 0.8)
    pair.mesh(0, quad(2, 2, 30, 20, uv=(0.1, 0.2, 0.9, 0.8)) + quad(32, 2, 62, 20, tint, uv=(0.0, 0.0, 1.0, 1.0)) + quad(2, 24, 62, 60, tint, uv=(-1.3, -0.6, 2.4, 1.7)), 0, [pm])
    pair.mesh(1, quad(40, 30, 60, 50, uv=(0.0, 0.0, 1.0, 1.0)), 1, [pm])
    frame, bg, prims, touched, _ = draw_and_check(pair, v2, what=f"texture format {fmt}")
    assert touched.sum() > 2500, "texture id 0 is usable"
    pair.mesh(1, quad(40, 30, 60, 50), 2, None)  # a texture that does not exist: not drawn
    frame, bg, prims, touched, _ = draw_and_check(pair, v2, what="tex_id beyond the count")
    assert list(prims["dropped"]) == [0] * 6 + [1] * 2
    # an edit with `changed` bits shows in the next frame
    before = frame.copy()
    pair.set_textures([(texture(3), fmt), (texture(2), fmt)], changed=[0])
    frame, bg, prims, touched, _ = draw_and_check(pair, v2, what="edited texture")
    assert not np.array_equal(bits(frame), bits(before))
    pair.close()


def test_texture_array_layer():
    pair = Pair(textures=[(texture(4), 0)], texture_array=1)
    pair.mesh(0, quad(3, 3, 61, 40, (1.0, 0.8, 0.9, 0.9), uv=(-0.2, 0.0, 1.2, 1.0)), 0, [pixel_matrix(W, H)])
    draw_and_check(pair, ortho(W, H), what="the stored 1024 x 1024 layer", texture_array=1)
    pair.close()


# ---------------------------------------------------------------- 6. blend
def test_blend():
    pair = Pair()
    pm, v2 = pixel_matrix(W, H), ortho(W, H)
    pair.mesh(0, quad(2, 2, 14, 14, (0.5, 0.6, 0.7, 0.0)) + quad(16, 2, 28, 14, (0.5, 0.6, 0.7, -0.5))
              + quad(30, 2, 42, 14, (0.25, 1.5, -0.75, 1.0)) + quad(44, 2, 56, 14, (0.25, 1.5, -0.75, 3.0)), None, [pm])
    frame, bg, prims, touched, _ = draw_and_check(pair, v2, what="alpha 0, < 0, 1, > 1")
    assert not touched[2:14, 2:28].any() and np.array_equal(bits(frame[2:14, 2:28]), bits(bg[2:14, 2:28]))
    assert np.all(frame[2:14, 30:42, :3] == np.float32([0.25, 1.5, -0.75])) and np.all(frame[2:14, 44:56, :3] == np.float32([0.25, 1.5, -0.75]))
    pair.close()
    # a NaN pixel of the finalised frame under an opaque quad becomes src; under a translucent one it stays NaN.  The NaN comes out of the
    # accumulator: a sky whose red is NaN, seen by a camera that looks away from the box, so every camera ray misses
    pair = Pair(options=(("sky_r", float("nan")),))
    pair.scene.set_camera([0.0, 0.0, -1000.0], [0.0, 0.0, -1.0])
    pair.view = pair.scene.view(W, H)
    pair.mesh(0, quad(2, 2, 16, 30, (0.125, 0.25, 0.5, 1.0)) + quad(16, 2, 30, 30, (0.125, 0.25, 0.5, 0.5)), None, [pm])
    frame, bg = pair.frame(v2, 0)
    assert np.all(np.isnan(bg[..., 0])) and np.all(np.isnan(pair.be.accumulator()[..., 0])), "the frame under the quads is NaN before the layer"
    assert np.all(frame[2:30, 2:16, :3] == np.float32([0.125, 0.25, 0.5])) and np.all(np.isnan(frame[2:30, 16:30, 0])) and np.all(np.isfinite(frame[2:30, 16:30, 1:3]))
    assert np.array_equal(bits(frame[..., 3]), bits(bg[..., 3])), "dst.w keeps its bits"
    outside = np.ones((H, W), bool); outside[2:30, 2:30] = False
    assert np.array_equal(bits(frame)[outside], bits(bg)[outside])
    pair.close()


# ---------------------------------------------------------------- 7. only the frame changes
def test_only_the_frame_changes():
    pair = Pair()
    be, twin = pair.be, pair.twin
    pm, v2 = pixel_matrix(W, H), ortho(W, H)
    pair.mesh(0, quad(6, 6, 50, 40, (0.9, 0.9, 0.1, 0.5)), None, [pm])
    be.synchronize()
    steps = be.srgb_steps()
    pres = be.host_frame(presented=True)
    for n in (1, 2, 3):
        be.render(pair.view, v2); twin.render(pair.view)
        if n == 2:
            continue
        assert np.array_equal(bits(be.accumulator()), bits(twin.accumulator())), n
        frame, bg = be.framebuffer(), twin.framebuffer()
        want, touched, _ = restate(bg, be.overlay_prims(), pair.meshes)
        check(frame, bg, want, touched, f"path traced, {n} samples")  # applied to each re-finalised frame, not accumulated
        be.download_frame(pres); be.wait_downloads()
        enc = np.searchsorted(steps, frame[..., :3], side="right").astype(np.uint8)
        assert np.array_equal(pres[..., :3], enc[..., ::-1]) and np.all(pres[..., 3] == 255), "the presented frame encodes the composited frame"
    pair.close()
    # the temporal history never sees the overlay
    pair = Pair(options=(("denoise", 1), ("denoise_temporal", 16)))
    be, twin = pair.be, pair.twin
    pair.mesh(0, quad(6, 6, 50, 40, (0.9, 0.9, 0.1, 0.5)), None, [pm])
    be.synchronize()
    for k in range(4):
        be.reset_accumulation(); twin.reset_accumulation()
        be.render(pair.view, v2); twin.render(pair.view)
        assert np.array_equal(bits(be.denoise_history()), bits(twin.denoise_history())), k
        frame, bg = be.framebuffer(), twin.framebuffer()
        want, touched, _ = restate(bg, be.overlay_prims(), pair.meshes)
        check(frame, bg, want, touched, f"temporal denoiser, image {k}")
    pair.close()


# ---------------------------------------------------------------- 8. plumbing
def glyphs(k):
    """the "glyph mesh" of frame k: k + 1 small quads"""
    v = []
    for j in range(k + 1):
        v += quad(4 + 7 * j, 6 + k, 9 + 7 * j, 14 + k, (1.0, 1.0 - 0.1 * j, 0.2 * k, 0.75))
    return v


@pytest.mark.parametrize("streams", [1, 2])
def test_frames_in_flight(streams):
    w, h = W, H
    scene = Scene().build("cornell")
    views = []
    for k in range(6):
        scene.set_camera([0.05 * k, 0.0, -3.5], [0.0, 0.0, 1.0], fov=40.0, aspect=1.0)
        views.append(scene.view(w, h))
    fly = HipBackend.init(w, h, 1.0, max_path_length=2, frames_in_flight=3, streams=streams, tile_size=16)
    one = HipBackend.init(w, h, 1.0, max_path_length=2, streams=streams, tile_size=16)
    for be in (fly, one):
        scene.mark_all_changed(); scene.sync(be)
    pm, v2 = cols(pixel_matrix(w, h)), ortho(w, h)

    def edit(be, k):
        t = np.eye(4); t[0, 3], t[1, 3] = 2.0 * k, 3.0 * k
        be.set_2d_mesh(2, glyphs(k)); be.set_2d_instances(2, [(pm @ t).T.reshape(16).astype(np.float32)]); be.synchronize()

    want = []
    for k in range(6):  # one frame at a time
        edit(one, k); one.render(views[k], v2, 2)
        want.append(one.framebuffer())
        assert one.overlay_stats()["drawn"] == 2 * (k + 1)
    assert not np.array_equal(bits(want[4]), bits(want[5]))
    bufs = [fly.host_frame() for _ in range(6)]
    for k in range(6):  # six frames without a wait: every edit is synchronised while earlier frames are still in flight
        edit(fly, k); fly.render(views[k], v2, 2)
        fly.download_frame(bufs[k])
        assert fly.overlay_stats()["drawn"] == 2 * (k + 1) and len(fly.overlay_prims()) == 2 * (k + 1), "the taps follow the slot of the latest frame"
    fly.wait_downloads()
    for k in range(6):
        assert np.array_equal(bits(bufs[k]), bits(want[k])), f"frame {k}: a frame shows the 2D state of the synchronize() before its render()"
    fly.close(); one.close()


def test_resize_batches_removal_and_the_limit():
    pair = Pair(max_batch=2)
    be, twin = pair.be, pair.twin
    pm, v2 = pixel_matrix(W, H), ortho(W, H)
    pair.mesh(0, quad(6, 6, 50, 40, (0.9, 0.9, 0.1, 0.5)), None, [pm])
    draw_and_check(pair, v2, what="before the resize")
    # render_batch and render_samples draw no overlay
    be.render_batch([pair.view, pair.view]); twin.render_batch([pair.view, pair.view])
    for f in range(2):
        assert np.array_equal(bits(be.framebuffer_at(f)), bits(twin.framebuffer_at(f)))
    be.render_samples(pair.view, 2); twin.render_samples(pair.view, 2)
    assert np.array_equal(bits(be.framebuffer()), bits(twin.framebuffer())) and be.overlay_stats()["drawn"] == 0
    for size in ((70, 37), (W, H)):
        for b in (be, twin):
            b.resize(size)
        pair.w, pair.h = size
        pair.scene.set_aspect(size[0] / size[1])
        pair.view = pair.scene.view(*size)
        pair.instances(0, [pixel_matrix(*size)])
        draw_and_check(pair, ortho(*size), what=f"resized to {size}")
    pair.instances(0, [])  # n = 0 removes
    frame, bg = pair.frame(v2, 2)
    assert np.array_equal(bits(frame), bits(bg)) and be.overlay_stats()["drawn"] == 0
    # more than 2^20 triangles over all instances: refused by synchronize(), nothing large allocated before
    be.set_2d_instances(0, np.tile(pm, ((1 << 19) + 1, 1)))
    with pytest.raises(BackendError, match="2\\^20"):
        be.synchronize()
    be.set_2d_instances(0, [pm]); be.synchronize()
    be.render(pair.view, v2, 2)
    assert be.overlay_stats()["drawn"] == 2
    pair.close()


# ---------------------------------------------------------------- 9. host: Camera2D, Quad2D, the Scene's 2D objects through synchronize
def test_host_scene_2d():
    for w, h, s in ((64, 64, 1.0), (70, 37, 1.0), (1920, 1080, 1.5)):
        got = Scene.camera_2d_view(w, h, s).astype(np.float64).reshape(4, 4).T
        l, r, b, t, n, f = -w * s / 2, w * s / 2, -h * s / 2, h * s / 2, 10.0, -10.0
        want = np.array([[2 / (r - l), 0, 0, -(l + r) / (r - l)], [0, 2 / (t - b), 0, -(t + b) / (t - b)], [0, 0, 1 / (n - f), n / (n - f)], [0, 0, 0, 1]])
        assert np.abs(got - want).max() <= 1e-7, (w, h, s)
    assert np.array_equal(Scene.camera_2d_view(W, H), ortho(W, H))
    scene = Scene().build("cornell")
    mesh = scene.add_2d_quad((10.0, 12.0), (30.0, 40.0), 0.5, None, (0.2, 0.4, 0.6, 0.5))
    v, tex = scene.mesh_2d(mesh)
    assert tex is None and v["vertex"].tolist() == [[10, 12, 0.5], [30, 12, 0.5], [30, 40, 0.5], [10, 12, 0.5], [30, 40, 0.5], [10, 40, 0.5]]
    assert v["uv"].tolist() == [[0, 0], [1, 0], [1, 1], [0, 0], [1, 1], [0, 1]] and np.all(v["color"] == np.float32([0.2, 0.4, 0.6, 0.5]))
    assert scene.mesh_2d(scene.add_2d_quad((0, 0), (1, 1), 0.0, 3))[1] == 3
    # through synchronize_system: changed 2D meshes and instance lists reach the backend; a removed instance is a zero matrix
    pair = Pair()
    pm = pixel_matrix(W, H)
    far = np.array(pm); far[12] += 16.0
    slot0, slot1 = scene.add_2d_instance(mesh, pm), scene.add_2d_instance(mesh, far)
    assert (slot0, slot1) == (0, 1)
    scene.set_aspect(1.0)
    for be in pair.bes:
        scene.mark_all_changed()
        scene.sync(be)
    pair.be.set_2d_mesh(mesh + 1, None)  # (the second quad wants texture 3, which does not exist here)
    pair.twin.set_2d_mesh(mesh, None); pair.twin.set_2d_mesh(mesh + 1, None)
    fv = np.zeros((6, 10), np.float32)
    fv[:, 0:3], fv[:, 4:6], fv[:, 6:10] = v["vertex"], v["uv"], v["color"]
    pair.meshes[mesh] = (fv, None, [pm, far])
    pair.view = scene.view(W, H)
    _, _, prims, touched, blends = draw_and_check(pair, Scene.camera_2d_view(W, H), what="the Scene's quad, two instances")
    assert list(prims["instance"]) == [0, 0, 1, 1] and not prims["dropped"].any() and blends.max() == 2 and touched[12:40, 10:46].all() and touched.sum() == 28 * 36
    scene.remove_2d_instance(mesh, 0)
    scene.set_2d_matrix(mesh, 1, pm)
    scene.sync(pair.be)
    pair.be.render(pair.view, Scene.camera_2d_view(W, H), 2)
    prims = pair.be.overlay_prims()
    assert list(prims["dropped"]) == [1, 1, 0, 0] and pair.be.overlay_stats() == {"drawn": 2, "dropped": 2, "bin_words": 1}
    pair.close()
