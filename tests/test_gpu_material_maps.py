"""Option "material_maps" (include/rfw_hip.h, DESIGN.md "Material maps"): k_shade honours the materials' metallic-roughness, sheen and emissive
maps, which shade.comp tests the flags of and never reads.

Scenes are the gallery or quads of Scene.add_quad; materials and textures are re-sent straight through HipBackend.set_materials /
set_textures after scene.sync(be) (a recorder with the backend's table hands the scene's own records over), then synchronize().  No
blue-noise tables; accumulators are compared as uint32.  The yardstick of the map step itself (rfw_hip_debug_eval_shading op 6) is the numpy
restatement below: texel_at, texture_sample, fetchTexelTrilinear and the option's formulas in float32, one operation at a time.  Frames of
64 x 48 pixels or fewer, so that tests/test_material_maps_on_cpu.py can run the file on the emulated library too."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_l2
from rfw_rs_amd import BackendError, HipBackend, Scene, pod
from rfw_rs_amd.scene import BackendTable

pytestmark = pytest.mark.gpu
f32 = np.float32
F1 = f32(1.0)
INV255 = f32(1.0) / f32(255.0)
DIFFUSE, NORMAL, ROUGHNESS, METALLIC, EMISSIVE, SHEEN = 1, 2, 4, 8, 16, 32
BGRA8, RGBA8 = 0, 1
W, H = 64, 48


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------- what the scene hands a backend, recorded
class Recorder:
    """a backend that keeps the materials and textures it is handed: .materials (pod.DeviceMaterial), .textures ((w, h, levels, bytes, format))"""

    def __init__(self):
        self.materials, self.textures = [], []
        vp, u32 = C.c_void_p, C.c_uint32
        self._cbs = []

        def cb(restype, *argtypes):
            def deco(fn):
                f = C.CFUNCTYPE(restype, *argtypes)(fn)
                self._cbs.append(f)
                return f
            return deco

        @cb(C.c_int, vp, C.POINTER(pod.DeviceMaterial), u32, vp)
        def set_materials(_, ptr, n, changed):
            self.materials = [pod.DeviceMaterial.from_buffer_copy(ptr[k]) for k in range(n)]
            return 0

        @cb(C.c_int, vp, C.POINTER(pod.TextureData), u32, vp)
        def set_textures(_, ptr, n, changed):
            self.textures = []
            for k in range(n):
                t = ptr[k]
                texels, w, h = 0, t.width, t.height
                for _l in range(max(t.mip_levels, 1)):
                    if w == 0 or h == 0:
                        break
                    texels += w * h
                    w >>= 1; h >>= 1
                raw = np.frombuffer(C.string_at(t.bytes, texels * 4), np.uint8).copy()
                self.textures.append((t.width, t.height, t.mip_levels, raw, t.format))
            return 0

        @cb(C.c_int, vp, vp, u32, vp)
        def ignore4(_, a, n, c):
            return 0

        @cb(C.c_int, vp, u32, vp)
        def ignore_mesh(_, i, d):
            return 0

        @cb(C.c_int, vp, vp, u32)
        def ignore3(_, a, n):
            return 0

        @cb(C.c_int, vp, vp)
        def ignore2(_, a):
            return 0

        @cb(C.c_int, vp)
        def ignore1(_):
            return 0

        cast = lambda f: C.cast(f, C.c_void_p)
        t = BackendTable()
        t.instance = None
        t.set_3d_mesh = t.set_3d_instances = cast(ignore_mesh)
        t.unload_3d_meshes = cast(ignore3)
        t.set_materials, t.set_textures = cast(set_materials), cast(set_textures)
        t.synchronize = cast(ignore1)
        t.set_point_lights = t.set_spot_lights = t.set_area_lights = t.set_directional_lights = t.set_skins = cast(ignore4)
        t.set_skybox = cast(ignore2)
        self._table = t

    def table(self):
        return self._table

    def last_error(self):
        return "recorder"


def recorded(scene):
    r = Recorder()
    scene.mark_all_changed()
    scene.sync(r)
    scene.mark_all_changed()
    return r.materials, r.textures


def copy_of(m):
    return pod.DeviceMaterial.from_buffer_copy(m)


def texture_data(textures):
    """pod.TextureData records over (w, h, levels, bytes, format) tuples (the tuples keep the bytes alive)"""
    return [pod.TextureData(w, h, levels, raw.ctypes.data_as(C.POINTER(C.c_uint8)), fmt) for w, h, levels, raw, fmt in textures]


def uniform_texture(rgba, w=4, h=4):
    return (w, h, 1, np.tile(np.array(rgba, np.uint8), w * h), RGBA8)


def set_scalars(m, metallic=None, roughness=None, sheen=None):
    """the scalar BYTES of a material (parameters[0]: metallic, subsurface, specular, roughness; [1]: specular tint, anisotropic, sheen, sheen tint)"""
    if metallic is not None:
        m.parameters[0] = (m.parameters[0] & ~0xFF) | metallic
    if roughness is not None:
        m.parameters[0] = (m.parameters[0] & ~(0xFF << 24)) | (roughness << 24)
    if sheen is not None:
        m.parameters[1] = (m.parameters[1] & ~(0xFF << 16)) | (sheen << 16)


def resend(be, materials=None, textures=None, changed=None):
    if textures is not None:
        be.set_textures(texture_data(textures))
    if materials is not None:
        be.set_materials(materials, changed)
    be.synchronize()
    be.reset_accumulation()


def render(be, view, samples):
    for _ in range(samples):
        be.render(view)
    return be.accumulator().copy()


GALLERY_FLOOR, GALLERY_PANEL, GALLERY_LAMP = 1, 3, 4  # build_gallery's materials: plain, textured (floor, left wall), bump, emissive-mapped panel, lamp


def gallery(w=W, h=H, texture_array=1, **options):
    scene = Scene().build("gallery")
    scene.set_aspect(w / h)
    materials, textures = recorded(scene)
    assert len(materials) == 5 and len(textures) == 3
    assert materials[GALLERY_PANEL].flags == EMISSIVE and list(materials[GALLERY_PANEL].color[:3]) == [4.0, 3.0, 2.0]
    assert materials[GALLERY_FLOOR].flags == DIFFUSE and max(materials[GALLERY_LAMP].color[:3]) > 1.0
    be = HipBackend.init(w, h, 1.0, **options)
    be.set_option("texture_array", texture_array)
    scene.sync(be)
    return scene, be, scene.view(w, h), materials, textures


# ---------------------------------------------------------------- 1. off and inert
def test_off_and_inert_cases_are_todays_frames():
    """never set, 0, and 1 on the gallery — whose only parameter map is the emissive map of the panel of colour (4, 3, 2), which is not live"""
    frames = []
    for value in (None, 0, 1):
        scene, be, view, _, _ = gallery(max_path_length=3)
        if value is not None:
            be.set_option("material_maps", value)
        frames.append(render(be, view, 2))
        assert be.frame_stats()["sample_count"] == 2
        be.close()
    assert frames[0][..., :3].any()
    assert same(frames[0], frames[1]) and same(frames[0], frames[2])


# ---------------------------------------------------------------- 2. the map step, restated
def f2i(x):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), 0, np.clip(np.trunc(x.astype(np.float64)), -2147483648.0, 2147483647.0)).astype(np.int64)


class Tex:
    def __init__(self, w, h, levels, raw, fmt):
        self.w, self.h, self.mips, self.format = w, h, levels, fmt
        self.data = np.ascontiguousarray(raw).view("<u4")


def texel_at(t, level, x, y):
    w, h, off = t.w, t.h, 0
    for _ in range(level):
        off += w * h
        w >>= 1; h >>= 1
    xi, yi = np.mod(x, w), np.mod(y, h)  # (C's remainder, plus the divisor where it is negative)
    p = t.data[off + yi * w + xi].astype(np.uint32)
    c = [(((p >> s) & 255).astype(np.float32) * INV255).astype(np.float32) for s in (0, 8, 16, 24)]
    return np.stack([c[2], c[1], c[0], c[3]] if t.format == BGRA8 else c, axis=-1)


def mix4(a, b, t):
    t = t[:, None]
    s = (F1 - t).astype(np.float32)
    return ((a * s).astype(np.float32) + (b * t).astype(np.float32)).astype(np.float32)


def texture_sample(t, u, v, lod):
    out = np.zeros((len(u), 4), np.float32)
    if t.mips == 0 or t.w == 0 or t.h == 0:
        return out
    level = np.clip(f2i(lod), 0, t.mips - 1)
    for L in np.unique(level):
        k = level == L
        L = int(L)
        w, h = t.w >> L, t.h >> L
        uu, vv = u[k], v[k]
        if L == 0:
            x = ((uu * f32(w)).astype(np.float32) - f32(0.5)).astype(np.float32)
            y = ((vv * f32(h)).astype(np.float32) - f32(0.5)).astype(np.float32)
            x0, y0 = np.floor(x), np.floor(y)
            fx, fy = (x - x0).astype(np.float32), (y - y0).astype(np.float32)
            ix, iy = f2i(x0), f2i(y0)
            t00, t10, t01, t11 = texel_at(t, 0, ix, iy), texel_at(t, 0, ix + 1, iy), texel_at(t, 0, ix, iy + 1), texel_at(t, 0, ix + 1, iy + 1)
            out[k] = mix4(mix4(t00, t10, fx), mix4(t01, t11, fx), fy)
        else:
            out[k] = texel_at(t, L, f2i(np.floor((uu * f32(w)).astype(np.float32))), f2i(np.floor((vv * f32(h)).astype(np.float32))))
    return out


def fetch_texel_trilinear(t, lam, u, v):
    level0 = np.minimum(f2i(lam), t.mips - 1)
    level1 = np.minimum(level0 + 1, t.mips - 1)
    f = (lam - np.floor(lam)).astype(np.float32)[:, None]
    p0 = texture_sample(t, u, v, level0.astype(np.float32))
    p1 = texture_sample(t, u, v, level1.astype(np.float32))
    return (((F1 - f).astype(np.float32) * p0).astype(np.float32) + (f * p1).astype(np.float32)).astype(np.float32)


def char2flt(x, s):
    return (((x >> s) & 255).astype(np.float32) * INV255).astype(np.float32)


def restated_maps(cases, texs):
    """op 6 of rfw_hip_debug_eval_shading on (n, 48) cases under the textures `texs`: (n, 7)"""
    u32 = cases.view(np.uint32)
    n = len(cases)
    colour = cases[:, 0:3]
    p0, p1, flags = u32[:, 12], u32[:, 13], u32[:, 16]
    mr_map, em_map, sh_map = (u32[:, k].view(np.int32).astype(np.int64) for k in (19, 20, 21))
    tu, tv, lam = cases[:, 27], cases[:, 28], cases[:, 29]
    r = char2flt(p0, 24)
    metallic, roughness, sheen = char2flt(p0, 0), np.maximum(f32(0.01), r), char2flt(p1, 16)
    Le, live = np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
    lod = f2i(lam).astype(np.float32)
    for index, t in enumerate(texs):
        k = ((flags & (ROUGHNESS | METALLIC)) != 0) & (mr_map == index)
        c = texture_sample(t, tu[k], tv[k], lod[k])
        rk, mk = (flags[k] & ROUGHNESS) != 0, (flags[k] & METALLIC) != 0
        roughness[k] = np.where(rk, np.maximum(f32(0.01), (r[k] * c[:, 1]).astype(np.float32)), roughness[k])
        metallic[k] = np.where(mk, (metallic[k] * c[:, 2]).astype(np.float32), metallic[k])
        k = ((flags & SHEEN) != 0) & (sh_map == index)
        c = texture_sample(t, tu[k], tv[k], lod[k])
        sheen[k] = (sheen[k] * c[:, 0]).astype(np.float32)
        k = ((flags & EMISSIVE) != 0) & (em_map == index) & ~(colour > F1).any(axis=1)
        Le[k] = fetch_texel_trilinear(t, lam[k], tu[k], tv[k])[:, :3]
        live[k] = F1
    return np.column_stack([metallic, roughness, sheen, Le, live]).astype(np.float32)


def random_cases(n, n_textures, seed):
    rng = np.random.default_rng(seed)
    cases = np.zeros((n, 48), np.float32)
    u32 = cases.view(np.uint32)
    colour = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    bright = rng.random(n) < 0.3
    colour[bright, rng.integers(0, 3, bright.sum())] = rng.uniform(1.0, 4.0, bright.sum()).astype(np.float32)
    colour[rng.random(n) < 0.05] = F1  # exactly 1 does not exceed 1
    cases[:, 0:3] = colour
    cases[:, 3] = F1
    u32[:, 12:16] = rng.integers(0, 1 << 32, (n, 4), dtype=np.uint64).astype(np.uint32)  # scalar bytes over the whole range
    u32[:, 16] = rng.integers(0, 64, n).astype(np.uint32)                                # every subset of the flag bits
    u32[:, 17:22] = rng.integers(-1, n_textures + 1, (n, 5)).astype(np.int32).view(np.uint32)  # -1 and n_textures: not live
    cases[:, 27:29] = rng.uniform(-2.0, 3.0, (n, 2)).astype(np.float32)
    cases[:, 29] = rng.uniform(-2.0, 7.0, n).astype(np.float32)
    whole = rng.random(n) < 0.1  # texel centres, edges and whole levels too
    cases[whole, 27:30] = np.round(cases[whole, 27:30] * 4.0) / 4.0
    return cases


def array_layer(w, h, raw):
    """gpu-rt's texture array, as set_textures keeps a texture under "texture_array" = 1: level 0 point-resampled to 1024 x 1024 (the source
    texel of the destination texel's centre), four more levels by a 2 x 2 box filter per channel, rounded to nearest"""
    src = raw.reshape(-1, 4)[: w * h].reshape(h, w, 4)
    k = np.arange(1024)
    level = src[((2 * k + 1) * h) // 2048][:, ((2 * k + 1) * w) // 2048]
    levels = [level]
    for _ in range(4):
        a = levels[-1].astype(np.uint32)
        levels.append(((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) // 4).astype(np.uint8))
    return np.concatenate([l.reshape(-1) for l in levels])


def source_textures(seed=5):
    rng = np.random.default_rng(seed)
    def texels(w, h, levels):
        return rng.integers(0, 256, 4 * sum((w >> l) * (h >> l) for l in range(levels))).astype(np.uint8)
    return [(8, 4, 1, texels(8, 4, 1), RGBA8), (16, 16, 3, texels(16, 16, 3), BGRA8), (5, 3, 1, texels(5, 3, 1), RGBA8)]


@pytest.mark.parametrize("texture_array", [0, 1])
def test_the_map_step_against_a_numpy_restatement(texture_array):
    sources = source_textures()
    if texture_array:
        sources = sources[1:2]
    scene = Scene().build("cornell")
    be = HipBackend.init(16, 16, 1.0)
    be.set_option("texture_array", texture_array)
    scene.sync(be)
    be.set_textures(texture_data(sources))
    be.synchronize()
    texs = [Tex(1024, 1024, 5, array_layer(w, h, raw), fmt) if texture_array else Tex(w, h, levels, raw, fmt) for w, h, levels, raw, fmt in sources]
    cases = random_cases(4000, len(sources), 11 + texture_array)
    for value in (0, 1):  # the hook applies the maps whatever the option says
        be.set_option("material_maps", value)
        got = be.eval_shading(6, cases)
        want = restated_maps(cases, texs)
        bad = np.argwhere(bits(got[:, :7]) != bits(want))
        assert len(bad) == 0, (len(bad), bad[:5], got[bad[:5, 0], :7], want[bad[:5, 0]])
        assert not got[:, 7:].any()
    live = want[:, 6] == 1
    assert 0.05 < live.mean() < 0.5 and (want[live, 3:6] > 0).any() and not want[~live, 3:6].any()
    be.close()


def test_the_map_step_needs_a_synchronized_scene():
    be = HipBackend.init(16, 16, 1.0)
    with pytest.raises(BackendError):
        be.eval_shading(6, np.zeros((1, 48), np.float32))
    be.close()


# ---------------------------------------------------------------- 3. a uniform map is the scalar it spells
@pytest.mark.parametrize("texture_array", [1, 0])
def test_a_uniform_map_is_the_scalar_it_spells(texture_array):
    """0 and 255 are the two bytes the sampler's blends return unchanged under every weight: 255 * (1 / 255f) == 1, c (1 - f) + c f == c for c in {0, 1}"""
    scene, be, view, materials, textures = gallery(texture_array=texture_array, max_path_length=3)
    twin = HipBackend.init(W, H, 1.0, max_path_length=3)
    twin.set_option("texture_array", texture_array)
    scene.mark_all_changed()
    scene.sync(twin)
    be.set_option("material_maps", 1)

    def pair(flags, slot, rgba, scalars):
        mapped = [copy_of(m) for m in materials]
        m = mapped[GALLERY_FLOOR]
        set_scalars(m, metallic=255, roughness=255, sheen=255)
        m.flags |= flags
        setattr(m, slot, len(textures))
        resend(be, mapped, textures + [uniform_texture(rgba)])
        plain = [copy_of(m) for m in materials]
        set_scalars(plain[GALLERY_FLOOR], metallic=255, roughness=255, sheen=255)
        set_scalars(plain[GALLERY_FLOOR], **scalars)
        resend(twin, plain)
        return render(be, view, 2), render(twin, view, 2)

    seen = []
    for g in (0, 255):
        for b in (0, 255):
            a, want = pair(ROUGHNESS | METALLIC, "metallic_roughness_map", (7, g, b, 9), dict(roughness=g, metallic=b))
            assert same(a, want), (g, b)
            seen.append(want)
    for r in (0, 255):
        a, want = pair(SHEEN, "sheen_map", (r, 7, 9, 11), dict(sheen=r))
        assert same(a, want), r
    assert not same(seen[0], seen[3]) and not same(seen[1], seen[2])  # the scalars show in the frame
    be.close(); twin.close()


# ---------------------------------------------------------------- quads that fill the frame
def quad_scene(w, h, behind=False):
    """one quad at z = 0 facing -z, a little larger than the frame of a camera at z = -3 (behind: z = +3, looking back); no lights, no sky.
    Returns the scene, the view, the quad's mesh id, its material's index and the materials."""
    scene = Scene().build("cornell")
    material = next(i for i in range(scene.counts()["materials"]) if max(scene.material(i)["color"][:3]) <= 1.0)
    for m in range(scene.counts()["meshes"]):
        scene.remove_mesh(m)
    z = 3.0 if behind else -3.0
    scene.set_camera((0.0, 0.0, z), (0.0, 0.0, -1.0 if behind else 1.0), fov=40.0, aspect=w / h)
    v = scene.view(w, h)
    pos, p1, right, up = (np.array(x.tolist()) for x in (v.pos, v.p1, v.right, v.up))
    corners = [p1, p1 + right, p1 + up, p1 + right + up]
    on_plane = [pos + (c - pos) * (-pos[2] / (c[2] - pos[2])) for c in corners]
    ex, ey = max(abs(c[0]) for c in on_plane), max(abs(c[1]) for c in on_plane)
    mesh = scene.add_quad((0.0, 0.0, -1.0), (0.0, 0.0, 0.0), 2.1 * ey, 2.1 * ex, material)  # (for this normal the quad's width runs along y)
    materials, _ = recorded(scene)
    return scene, v, mesh, material, materials


def attach(scene, w, h, **options):
    be = HipBackend.init(w, h, 1.0, **options)
    scene.mark_all_changed()
    scene.sync(be)
    be.set_skybox(pod.TextureData())  # an empty texture: the constant sky colour, 0
    for kind in ("point", "spot", "area", "directional"):
        getattr(be, f"set_{kind}_lights")([])
    be.synchronize()
    return be


def with_uvs(scene, mesh):
    """the quad's mesh with u, v = 0 ... 1 over its x, y extent and tangents along x in the triangle records (Scene.add_quad, as Quad3D::new,
    leaves the uvs 0, and the tangents derived from them are no directions); returns (pod.MeshData3D, the array it points into)"""
    d = scene.mesh_data(mesh)
    tris = np.frombuffer(C.string_at(d.triangles, d.num_triangles * 176), np.float32).reshape(-1, 44).copy()
    xs, ys = tris[:, [0, 4, 8]], tris[:, [1, 5, 9]]
    tris[:, [3, 7, 11]] = (xs - xs.min()) / (xs.max() - xs.min())
    tris[:, [15, 19, 23]] = (ys - ys.min()) / (ys.max() - ys.min())
    tris[:, 28:40] = np.tile(np.array([1.0, 0.0, 0.0, 1.0], np.float32), 3)  # tangent0 .. 2: along u (without uvs the mesh has none, and no BSDF sample)
    tris[:, 42] = 0.0                                                       # lod: lambda = log2(spread / |cos|), far below level 0
    out = pod.MeshData3D.from_buffer_copy(d)
    out.triangles = C.cast(tris.ctypes.data, C.POINTER(pod.RTTriangle))
    return out, tris


# ---------------------------------------------------------------- 4. texel by texel
@pytest.mark.parametrize("texture_array, neither_most, each_least", [(1, 0.05, 0.40), (0, 0.25, 0.25)])
def test_the_map_is_honoured_texel_by_texel(texture_array, neither_most, each_least):
    scene, view, mesh, mat, materials = quad_scene(W, H)
    be = attach(scene, W, H, max_path_length=1)
    be.set_option("texture_array", texture_array)
    data, keep = with_uvs(scene, mesh)
    be.set_3d_mesh(mesh, data)
    be.set_point_lights([pod.PointLight(pod.Vec3(0.0, 0.0, -2.0), 30.0, pod.Vec3(10.0, 10.0, 10.0), 0.0)])
    texels = np.zeros((16, 16, 4), np.uint8)
    texels[:, :8] = (3, 255, 0, 255)   # left half: G, B = 255, 0
    texels[:, 8:] = (3, 0, 255, 255)   # right half: 0, 255
    texture = (16, 16, 1, texels.reshape(-1), RGBA8)

    def frame(flags, roughness, metallic, option):
        ms = [copy_of(m) for m in materials]
        m = ms[mat]
        m.color[0] = m.color[1] = m.color[2] = 0.8
        set_scalars(m, metallic=metallic, roughness=roughness)
        m.flags, m.metallic_roughness_map = flags, 0
        be.set_option("material_maps", option)
        resend(be, ms, [texture])
        return render(be, view, 2)

    A = frame(0, 255, 0, 0)
    B = frame(0, 0, 255, 0)
    mapped = frame(ROUGHNESS | METALLIC, 255, 255, 1)
    differ = (bits(A) != bits(B)).any(axis=-1)
    assert differ.mean() >= 0.5, differ.mean()
    is_a, is_b = (bits(mapped) == bits(A)).all(axis=-1), (bits(mapped) == bits(B)).all(axis=-1)
    only_a, only_b, neither = (is_a & ~is_b).mean(), (is_b & ~is_a).mean(), (~is_a & ~is_b).mean()
    print(f"texture_array {texture_array}: pixels equal to A only {only_a:.3f}, to B only {only_b:.3f}, to neither {neither:.3f}")
    assert neither <= neither_most and only_a >= each_least and only_b >= each_least
    assert same(frame(ROUGHNESS | METALLIC, 255, 0, 0), A)  # the flags alone change nothing
    be.close()


# ---------------------------------------------------------------- 5. emission, exactly
def test_emission_exactly():
    w, h, n = 32, 24, 3
    scene, view, mesh, mat, materials = quad_scene(w, h)
    be = attach(scene, w, h, max_path_length=1)
    texture = uniform_texture((255, 0, 255, 255))

    def frame(colour, option, v=view, clamp=10.0):
        ms = [copy_of(m) for m in materials]
        m = ms[mat]
        m.color[0] = m.color[1] = m.color[2] = colour
        m.flags, m.emissive_map = EMISSIVE, 0
        be.set_option("material_maps", option)
        be.set_option("clamp_value", clamp)
        resend(be, ms, [texture])
        return render(be, v, n)

    assert not frame(0.5, 0).any()
    assert same(frame(0.5, 1), np.broadcast_to(np.array([n, 0, n, 0], np.float32), (h, w, 4)))
    assert same(frame(0.5, 1, clamp=0.5), np.broadcast_to(np.array([0.5 * n, 0, 0.5 * n, 0], np.float32), (h, w, 4)))
    assert same(frame(2.0, 1), frame(2.0, 0))  # a colour above 1: today's behaviour in full
    be.close()
    scene, back, mesh, mat, materials = quad_scene(w, h, behind=True)
    be = attach(scene, w, h, max_path_length=1)
    assert not frame(0.5, 1, back).any()
    be.set_option("material_maps", 1)
    be.render(back, None, 3)  # (GBUFFER: the quad does fill the frame from behind)
    assert (be.accumulator()[..., 3] > 0).all()
    be.close()


# ---------------------------------------------------------------- 6. emission lights the scene by bounces
def test_emission_lights_the_scene_by_bounces():
    """The gallery with nothing else that shines: no light lists, no sky box, the lamp's colour and the panel's lowered to 0.8 — the panel's
    emissive map (texture 0) is then live.  A sanity bound, not a measurement: the panel subtends a large solid angle from the floor."""
    scene, be, view, materials, textures = gallery(max_path_length=2)
    be.set_skybox(pod.TextureData())
    for kind in ("point", "spot", "area", "directional"):
        getattr(be, f"set_{kind}_lights")([])
    ms = [copy_of(m) for m in materials]
    for k in (GALLERY_PANEL, GALLERY_LAMP):
        ms[k].color[0] = ms[k].color[1] = ms[k].color[2] = 0.8
    resend(be, ms)
    be.render(view, None, 3)  # GBUFFER: the hit point and t
    g = be.accumulator()
    floor = (g[..., 3] > 0) & (np.abs(g[..., 1]) < 1e-4)
    assert floor.mean() > 0.1
    off = render(be, view, 4)
    assert not off[floor][:, :3].any()
    be.set_option("material_maps", 1)
    on = render(be, view, 4)
    assert be.frame_stats()["sample_count"] == 4
    assert np.isfinite(on).all() and (on[floor][:, :3] >= 0).all()
    lit = (on[floor][:, :3] > 0).any(axis=-1).mean()
    print(f"floor pixels lit by the panel after 4 samples: {lit:.3f}")
    assert lit >= 0.1
    be.close()


# ---------------------------------------------------------------- 7. the option's contract
def test_the_options_contract():
    scene, be, view, _, _ = gallery(max_path_length=2)
    want = render(be, view, 2)
    be.reset_accumulation()
    be.render(view)
    for bad in (2, -1, 0.5, float("nan")):
        with pytest.raises(BackendError):
            be.set_option("material_maps", bad)
    be.set_option("material_maps", 0)  # the same value: the image goes on
    be.render(view)
    assert be.frame_stats()["sample_count"] == 2 and same(be.accumulator(), want)
    be.set_option("material_maps", 1)
    be.render(view)
    assert be.frame_stats()["sample_count"] == 1
    for bad in (2, float("nan")):
        with pytest.raises(BackendError):
            be.set_option("material_maps", bad)
    be.set_option("material_maps", 1)
    be.render(view)
    assert be.frame_stats()["sample_count"] == 2 and same(be.accumulator(), want)  # (no live map in the gallery)
    be.close()


# ---------------------------------------------------------------- 8. everywhere k_shade runs
def mapped_gallery(**options):
    scene, be, view, materials, textures = gallery(max_path_length=3, **options)
    ms = [copy_of(m) for m in materials]
    ms[GALLERY_FLOOR].flags |= ROUGHNESS | METALLIC
    ms[GALLERY_FLOOR].metallic_roughness_map = len(textures)
    set_scalars(ms[GALLERY_FLOOR], metallic=255, roughness=255)
    noise = (16, 16, 1, np.random.default_rng(3).integers(0, 256, 16 * 16 * 4).astype(np.uint8), RGBA8)
    be.set_option("material_maps", 1)
    resend(be, ms, textures + [noise])
    return scene, be, view


def gallery_views(scene, n):
    out = []
    for k in range(n):
        scene.set_camera([0.4 + 0.3 * k, 1.5, -5.5], [-0.05, -0.05, 1.0], fov=60.0, aspect=W / H)
        out.append(scene.view(W, H))
    return out


def test_everywhere_k_shade_runs():
    scene, batch, view = mapped_gallery(max_batch=3)
    views = gallery_views(scene, 3)
    batch.render_batch(views)
    for f, v in enumerate(views):
        _, fresh, _ = mapped_gallery()
        fresh.render(v)
        assert same(batch.accumulator_at(f), fresh.accumulator()), f
        if f == 0:
            fresh.set_option("material_maps", 0)
            fresh.render(v)
            assert not same(fresh.accumulator(), batch.accumulator_at(0))  # the map shows
        fresh.close()
    batch.render_samples(views[1], 2)
    _, two, _ = mapped_gallery()
    two.render(views[1]); two.render(views[1])
    rel = rel_l2(batch.accumulator(), two.accumulator())
    print(f"render_samples against two render() calls: rel-L2 {rel:.3e}")
    assert batch.frame_stats()["sample_count"] == 2 and rel <= 1e-6
    batch.close()
    _, slots, _ = mapped_gallery(frames_in_flight=3)
    _, streams, _ = mapped_gallery(streams=2)
    for k, v in enumerate(views + views[:2]):  # more frames than slots
        two.render(v); slots.render(v); streams.render(v)
        assert same(slots.accumulator(), two.accumulator()), k
        assert same(streams.accumulator(), two.accumulator()), k
    two.close(); slots.close(); streams.close()


# ---------------------------------------------------------------- 9. edits select the kernel
def test_edits_select_the_kernel():
    scene, be, view, materials, textures = gallery(max_path_length=3)
    be.set_option("material_maps", 1)
    first = render(be, view, 2)
    edited = [copy_of(m) for m in materials]
    m = edited[GALLERY_FLOOR]
    m.flags |= ROUGHNESS | METALLIC
    m.metallic_roughness_map = 0  # the albedo checker as a metallic-roughness map
    resend(be, edited, changed=[GALLERY_FLOOR])
    assert not same(render(be, view, 2), first)
    resend(be, [copy_of(m) for m in materials], changed=[GALLERY_FLOOR])
    assert same(render(be, view, 2), first)
    # the kernel follows the table as uploaded: an element under a clear `changed` bit is not looked at, whatever it holds
    bare = [copy_of(m) for m in materials]
    bare[GALLERY_PANEL].flags = 0  # no parameter-map flag anywhere
    resend(be, bare)
    plain = render(be, view, 2)
    mapped = [copy_of(m) for m in bare]
    mapped[GALLERY_FLOOR].flags |= ROUGHNESS | METALLIC
    mapped[GALLERY_FLOOR].metallic_roughness_map = 0
    resend(be, mapped, changed=[GALLERY_FLOOR])
    with_map = render(be, view, 2)
    assert not same(with_map, plain)
    resend(be, bare, changed=[GALLERY_LAMP])  # the floor's entry is stale here and its bit is clear: the device keeps the mapped floor
    assert same(render(be, view, 2), with_map)
    be.close()
