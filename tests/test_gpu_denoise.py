"""Option "denoise" (include/rfw_hip.h, DESIGN.md "Denoiser"): the guided a-trous filter of the path-traced frame (csrc/denoise.inc).

Off by default and then bit for bit what it was; on, it changes the finalised frame only.  The guide is held against what the render modes
already pin to the oracle, the filter against a float64 numpy restatement of its formula fed with the device's own accumulator and guide.
Small frames, so that tests/test_denoise_on_cpu.py can run the file on the emulated library too.

test_the_formula_restated: the bound is 1e-5 * max(1, |want|), the one mode 6's filter is held to.  Largest |frame - want| / max(1, |want|)
measured over the scenes of that test and n = 1, 3, the same figures on the emulated library and on the MI355X (same float32 operations,
no contraction): k = 1: 4.4e-7, k = 2: 3.7e-7, k = 3: 4.6e-7, k = 4: 6.3e-7, k = 5: 7.6e-7."""
import threading
import time

import numpy as np
import pytest

from rfw_rs_amd import BackendError, HipBackend, RenderMode, Scene
from conftest import rel_l2

pytestmark = pytest.mark.gpu
W = H = 64
K_PLANE, NORMAL_POWER, ALBEDO_FLOOR = 0.02, 32, 1e-3  # csrc/denoise.inc: kDnPlane, 2^kDnNormalSquarings, kDnAlbedoFloor
DEFAULT_COLOUR = 32.0                                  # csrc/kernels.h: kDenoiseDefaultColour
TAPS = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
SCENES = [("cornell", ()), ("soup", (1500, 5, 0.0, 4)), ("gallery", ())]


def make(kind="cornell", *args, w=W, h=H, **options):
    scene = Scene().build(kind, *args) if kind else Scene()
    be = HipBackend.init(w, h, 1.0, **options)
    scene.sync(be)
    return scene, be, scene.view(w, h)


def attach(scene, w=W, h=H, denoise=0, colour=None, **options):
    """another backend of the same scene (everything is sent again)"""
    be = HipBackend.init(w, h, 1.0, **options)
    scene.mark_all_changed()
    scene.sync(be)
    if denoise:
        be.set_option("denoise", denoise)
    if colour is not None:
        be.set_option("denoise_colour", colour)
    return be


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def floor_scene(extra_quads=(), camera=((0.0, 2.0, 3.0), (0.0, -1.0, -1.0))):
    """a wide floor at y = 0 (and the given quads), one of the Cornell box's diffuse materials, no lights"""
    scene = Scene().build("cornell")
    diffuse = next(i for i in range(scene.counts()["materials"]) if max(scene.material(i)["color"][:3]) <= 1.0)
    for m in range(scene.counts()["meshes"]):
        scene.remove_mesh(m)
    scene.add_quad((0.0, 1.0, 0.0), (0.0, 0.0, 0.0), 400.0, 400.0, diffuse)
    for n, p, a, b in extra_quads:
        scene.add_quad(n, p, a, b, diffuse)
    scene.set_camera(camera[0], camera[1])
    return scene


def wall_on_the_floor():
    """a floor (y = 0) and a wall standing on it (z = -1, facing +z)"""
    return floor_scene([((0.0, 0.0, 1.0), (0.0, 100.0, -1.0), 400.0, 200.0)], camera=((0.0, 1.5, 1.5), (0.0, -1.0, -0.9)))


def render(be, view, n):
    for _ in range(n):
        be.render(view)
    return be


# ---------------------------------------------------------------- 1. off is untouched
def test_off_is_untouched():
    scene, be, view = make()
    fresh = render(attach(scene), view, 2)
    acc, fb = fresh.accumulator(), fresh.framebuffer()
    render(be, view, 2)  # the default
    assert np.array_equal(bits(be.accumulator()), bits(acc)) and np.array_equal(bits(be.framebuffer()), bits(fb))
    be.set_option("denoise", 0)
    be.reset_accumulation()
    render(be, view, 2)
    assert np.array_equal(bits(be.accumulator()), bits(acc)) and np.array_equal(bits(be.framebuffer()), bits(fb))
    be.set_option("denoise", 3)
    render(be, view, 2)
    assert np.array_equal(bits(be.accumulator()), bits(acc)), "a changed value starts a new image; the accumulator is the raw sum"
    assert not np.array_equal(bits(be.framebuffer()), bits(fb)), "the filter does change the frame"
    be.set_option("denoise", 0)
    render(be, view, 2)
    assert np.array_equal(bits(be.accumulator()), bits(acc)) and np.array_equal(bits(be.framebuffer()), bits(fb)), "3 -> 0: a fresh instance's bits"
    # the accumulator under the filter, after 1 and after 3 samples
    on, off = attach(scene, denoise=3), attach(scene)
    for n in (1, 2, 3):
        on.render(view)
        off.render(view)
        if n != 2:
            assert np.array_equal(bits(on.accumulator()), bits(off.accumulator())), n
    for key, value in (("denoise", 6), ("denoise", -1), ("denoise", 2.5), ("denoise_colour", 0)):
        with pytest.raises(BackendError):
            be.set_option(key, value)
    for b in (be, fresh, on, off):
        b.close()


def hit_materials(be, w=W, h=H):
    """(h, w) material index of the triangle the latest frame's camera ray hit (0 on a miss): k_primary's hit slab, de-tiled with the numpy
    twin, and the device's triangle records (176 bytes, material index in word 41).  After a frame of modes 1-6, which leave the slab alone."""
    from rfw_rs_amd import dist
    _, slot = dist.slab_index_map(w, h, 1)
    n = int(slot.max()) + 1
    hits = np.frombuffer(be.debug_read("hit0", 16 * n).tobytes(), np.uint32).reshape(-1, 4)[slot.reshape(-1)]
    hit = hits[:, 0].view(np.int32) >= 0
    tri = np.where(hit, hits[:, 1], 0)
    records = np.frombuffer(be.debug_read("triangles", 176 * (int(tri.max()) + 1)).tobytes(), np.int32).reshape(-1, 44)
    return np.where(hit, records[tri, 41], 0).reshape(h, w)


# ---------------------------------------------------------------- 2. the guide, against what the render modes pin to the oracle
@pytest.mark.parametrize("kind,args", SCENES)
def test_guide_matches_the_render_modes(kind, args):
    scene, be, view = make(kind, *args)
    be.set_option("denoise", 1)
    be.render(view)
    g0, g1, g2 = be.denoise_guide()
    other = attach(scene)
    other.render(view, mode=RenderMode.SSAO)
    ao_guide = np.frombuffer(other.debug_read("ao_guide", W * H * 16).tobytes(), np.float32).reshape(H, W, 4)
    assert np.array_equal(bits(g0), bits(ao_guide)), "(faced gN, t) is mode 5's guide"
    hit = g0[..., 3] > 0.0
    assert hit.any()
    other.render(view, mode=RenderMode.ALBEDO)
    albedo = other.accumulator()
    assert np.array_equal(bits(g2[hit][:, :3]), bits(albedo[hit][:, :3])), "albedo is mode 2's value"
    other.render(view, mode=RenderMode.GBUFFER)
    assert np.array_equal(bits(g1[..., :3]), bits(other.accumulator()[..., :3])), "P is mode 3's value"
    assert np.all(g1[..., 3] == 0.0)
    # f: off on misses and on lights (a colour component above 1 and no emissive map), from the material of the triangle each camera ray hit
    mats = [scene.material(i) for i in range(scene.counts()["materials"])]
    emitter = np.array([max(m["color"][:3]) > 1.0 and m["emissive_tex"] < 0 for m in mats])
    light = np.zeros((H, W), bool)
    light[hit] = emitter[hit_materials(other)[hit]]
    assert np.array_equal(g2[..., 3], (hit & ~light).astype(np.float32))
    if kind == "cornell":
        assert light.any(), "the Cornell light is in view and passes through"
    for b in (be, other):
        b.close()


# ---------------------------------------------------------------- 3. the formula, restated in float64
def shifted(a, oy, ox):
    """out[y, x] = a[y + oy, x + ox], and where that lies inside the frame"""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    inside = np.zeros((h, w), bool)
    ys, xs = slice(max(0, -oy), min(h, h - oy)), slice(max(0, -ox), min(w, w - ox))
    yq, xq = slice(max(0, -oy) + oy, min(h, h - oy) + oy), slice(max(0, -ox) + ox, min(w, w - ox) + ox)
    out[ys, xs] = a[yq, xq]
    inside[ys, xs] = True
    return out, inside


def atrous_restated(acc, n, guide, passes, sigma_c):
    """DESIGN.md "Denoiser", in float64: returns the frame's rgb where f = 1 (elsewhere 0) and f."""
    g0, g1, g2 = (g.astype(np.float64) for g in guide)
    f = g2[..., 3] > 0.0
    N, t, P = g0[..., :3], np.where(f, g0[..., 3], 1.0), g1[..., :3]
    a = np.maximum(g2[..., :3], ALBEDO_FLOOR)
    x = np.where(f[..., None], acc[..., :3].astype(np.float64) / n / a, 0.0)
    for i in range(passes):
        s, sigma = 2 ** i, sigma_c * 2.0 ** -i / np.sqrt(n)
        sw, sx = np.zeros(f.shape), np.zeros(x.shape)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                xq, inside = shifted(x, dy * s, dx * s)
                fq, Nq, Pq = shifted(f, dy * s, dx * s)[0], shifted(N, dy * s, dx * s)[0], shifted(P, dy * s, dx * s)[0]
                wn = np.maximum(0.0, (N * Nq).sum(-1)) ** NORMAL_POWER
                wp = np.maximum(0.0, 1.0 - np.abs((N * (Pq - P)).sum(-1)) / (K_PLANE * t))
                wc = np.exp(-((x - xq) ** 2).sum(-1) / sigma ** 2)
                w = np.where(inside & fq & f, TAPS[dx + 2] * TAPS[dy + 2] * wn * wp * wc, 0.0)
                sw += w
                sx += w[..., None] * xq
        x = np.where(f[..., None], sx / np.where(f, sw, 1.0)[..., None], 0.0)
    return np.sqrt(x * a) * f[..., None], f


def cornell_70x37():
    scene = Scene().build("cornell")
    scene.set_aspect(70 / 37)
    return scene


# name: (scene, width, height).  70 x 37 is no multiple of the 16-pixel tile: tiles that hang over the right and bottom edges, sub-images of
# unequal size at steps 2 .. 16, windows that start left of / above the frame
FORMULA_SCENES = {"cornell": (lambda: Scene().build("cornell"), W, H), "gallery": (lambda: Scene().build("gallery"), W, H),
                  "wall": (wall_on_the_floor, W, H), "cornell_70x37": (cornell_70x37, 70, 37)}


@pytest.mark.parametrize("name", sorted(FORMULA_SCENES))
def test_the_formula_restated(name):
    """The wall scene is the issue's named edge case (neighbouring pixels whose normals are at right angles, asserted from the guide).  Its
    quads carry no tangents, so k_shade's BSDF sample has no valid pdf there and no path leaves the first hit: the path-traced image of
    floor_scene is black whatever lights it, and on it the check covers the guide, f, the pass-through and 0 = 0 only.  The same edge WITH
    light is the Cornell box's floor against its back wall, asserted below as well."""
    build, w, h = FORMULA_SCENES[name]
    scene = build()
    view = scene.view(w, h)
    be, raw = attach(scene, w, h), attach(scene, w, h)
    worst = {}
    for n in (1, 3):
        raw.reset_accumulation()
        render(raw, view, n)
        raw_fb = raw.framebuffer()
        for k in range(1, 6):
            be.set_option("denoise", k)  # (a changed value: a new image)
            render(be, view, n)
            acc, fb, guide = be.accumulator(), be.framebuffer(), be.denoise_guide()
            assert np.array_equal(bits(acc), bits(raw.accumulator()))
            want, f = atrous_restated(acc, n, guide, k, DEFAULT_COLOUR)
            assert f.sum() > w * h // 4, "there is something to filter"
            N = guide[0][..., :3]
            right_angles = (np.abs((N[1:] * N[:-1]).sum(-1)) == 0.0) & f[1:] & f[:-1]
            if name != "gallery":  # the edge case is among the restated pixels: neighbours whose normals are at right angles
                assert right_angles.any()
            if name != "wall":
                assert np.any(want[f] > 0.0)
            dev = np.abs(fb[..., :3] - want) / np.maximum(1.0, np.abs(want))
            worst[k] = max(worst.get(k, 0.0), float(dev[f].max()))
            print(f"denoise formula {name} n={n} k={k}: max |frame - want| / max(1, |want|) = {dev[f].max():.3e}")
            assert np.all(dev[f] <= 1e-5), (name, n, k, float(dev[f].max()))
            assert np.array_equal(bits(fb[~f]), bits(raw_fb[~f])), "pass-through pixels are k_assemble's"
            assert np.array_equal(bits(fb[..., 3]), bits(raw_fb[..., 3])), "w is k_assemble's"
            assert not np.any(np.isnan(fb))
    print("denoise formula", name, "worst per k:", {k: f"{v:.2e}" for k, v in worst.items()})
    be.close()
    raw.close()


def test_both_kernel_forms_give_the_same_bits():
    """Option "denoise_form" (a measurement knob): 1 = every pass one thread per pixel with 25 taps from memory, 2 = every pass tiled through
    LDS.  Same taps in the same order, so the same bits — on a frame that is no multiple of the tile."""
    scene = cornell_70x37()
    view = scene.view(70, 37)
    frames = []
    for form in (1, 2, 0):
        be = attach(scene, 70, 37, denoise=5)
        be.set_option("denoise_form", form)
        frames.append(render(be, view, 2).framebuffer())
        be.close()
    assert np.array_equal(bits(frames[0]), bits(frames[1])) and np.array_equal(bits(frames[2]), bits(frames[1]))
    with pytest.raises(BackendError):
        be = attach(scene)
        be.set_option("denoise_form", 3)


# ---------------------------------------------------------------- 4. a vanishing colour width is the identity
def test_a_vanishing_colour_width_is_the_identity():
    scene, raw, view = make()
    be = attach(scene, denoise=5, colour=1e-6)
    raw.render(view)
    be.render(view)
    want, fb = raw.framebuffer(), be.framebuffer()
    dev = np.abs(fb - want) / np.maximum(1.0, np.abs(fb))
    print(f"denoise identity: max deviation {dev.max():.3e}")
    assert np.all(dev <= 1e-6), float(dev.max())
    be.close()
    raw.close()


# ---------------------------------------------------------------- 5. it denoises
@pytest.mark.parametrize("kind", ["cornell", "gallery"])
def test_it_denoises(kind):
    """e(img) = rel-L2 against the undenoised frame after 1024 samples, over the filtered pixels: at one sample per pixel the denoised frame
    is closer than the raw one (k = 3 and k = 5, default options).  The ratios at 1, 4, 16 and 64 samples are printed (DESIGN.md quotes them)."""
    scene, raw, view = make(kind)
    dn5, dn3 = attach(scene, denoise=5), attach(scene, denoise=3)
    marks = (1, 4, 16, 64)
    raws, dens = {}, {}
    f = None
    for n in range(1, 1025):
        raw.render(view)
        if n <= marks[-1]:
            dn5.render(view)
        if n in marks:
            raws[n], dens[n] = raw.framebuffer()[..., :3], dn5.framebuffer()[..., :3]
        if n == 1:
            dn3.render(view)
            f = dn5.denoise_guide()[2][..., 3] > 0.0  # (sample 0's filtered pixels; the jitter moves a few edge pixels per sample)
    ref = raw.framebuffer()[..., :3]
    e = lambda img: rel_l2(img[f], ref[f])
    for n in marks:
        print(f"denoise {kind} {n} spp: e(raw) = {e(raws[n]):.4f}, e(k = 5) = {e(dens[n]):.4f}, ratio {e(dens[n]) / e(raws[n]):.3f}")
    e3 = e(dn3.framebuffer()[..., :3])
    print(f"denoise {kind} 1 spp: e(k = 3) = {e3:.4f}, ratio {e3 / e(raws[1]):.3f}")
    assert e(dens[1]) < e(raws[1])
    assert e3 < e(raws[1])
    for b in (raw, dn5, dn3):
        b.close()


# ---------------------------------------------------------------- 6. everywhere mode 0 runs
def test_frame_slots_and_sub_streams_give_the_same_bits():
    scene = Scene().build("cornell")
    view = scene.view(W, H)
    plain = render(attach(scene, denoise=3, tile_size=16), view, 2)
    want = plain.framebuffer()
    for options in ({"frames_in_flight": 3}, {"streams": 2}, {"frames_in_flight": 3, "streams": 2}):
        be = render(attach(scene, denoise=3, tile_size=16, **options), view, 2)
        assert np.array_equal(bits(be.framebuffer()), bits(want)), options
        assert np.array_equal(bits(np.stack(be.denoise_guide())), bits(np.stack(plain.denoise_guide()))), options
        be.close()
    plain.close()


def test_render_samples_and_the_presented_frame():
    scene = Scene().build("cornell")
    view = scene.view(W, H)
    one = attach(scene, denoise=3, max_batch=4)
    one.render_samples(view, 4)
    seq = render(attach(scene, denoise=3), view, 4)
    assert rel_l2(one.accumulator(), seq.accumulator()) <= 1e-6
    assert np.array_equal(bits(np.stack(one.denoise_guide())), bits(np.stack(seq.denoise_guide()))), "the guide is the LAST sample's"
    fb = one.framebuffer()
    print(f"denoise render_samples: rel-L2 of the frames {rel_l2(fb, seq.framebuffer()):.3e}")
    assert rel_l2(fb, seq.framebuffer()) <= 1e-6
    raw = attach(scene, max_batch=4)
    raw.render_samples(view, 4)
    assert not np.array_equal(bits(fb), bits(raw.framebuffer()))
    # the presented BGRA8 image is the sRGB encoding of the denoised float frame
    steps = one.srgb_steps()
    pres = one.host_frame(presented=True)
    one.download_frame(pres)
    one.wait_downloads()
    enc = lambda x: np.searchsorted(steps, x, side="right").astype(np.uint8)
    want = np.stack([enc(fb[..., 2]), enc(fb[..., 1]), enc(fb[..., 0]), np.full(fb.shape[:2], 255, np.uint8)], axis=-1)
    assert np.array_equal(pres.reshape(want.shape), want)
    flt = one.host_frame()
    one.download_frame(flt)
    one.wait_downloads()
    assert np.array_equal(bits(flt), bits(fb))
    accd = one.host_frame()
    one.download_frame(accd, accumulator=True)
    one.wait_downloads()
    assert np.array_equal(bits(accd), bits(one.accumulator()))
    for b in (one, seq, raw):
        b.close()


def test_the_other_modes_ignore_the_option():
    scene = Scene().build("cornell")
    view = scene.view(W, H)
    on, off = attach(scene, denoise=5), attach(scene)
    for mode in range(1, 7):
        on.render(view, mode=mode)
        off.render(view, mode=mode)
        assert np.array_equal(bits(on.accumulator()), bits(off.accumulator())), mode
        assert np.array_equal(bits(on.framebuffer()), bits(off.framebuffer())), mode
    # a batch of frames finalises unfiltered
    on.close()
    off.close()
    on, off = attach(scene, denoise=5, max_batch=2), attach(scene, max_batch=2)
    on.render_batch([view, view])
    off.render_batch([view, view])
    for frame in range(2):
        assert np.array_equal(bits(on.framebuffer_at(frame)), bits(off.framebuffer_at(frame))), frame
    on.close()
    off.close()


def test_ranks_through_the_loopback_hub_finalise_unfiltered():
    w, h, world = 96, 64, 3
    scene = Scene().build("cornell")
    scene.set_aspect(w / h)
    view = scene.view(w, h)
    full = HipBackend.init(w, h, 1.0)
    scene.sync(full)
    full.render(view)
    acc, fb = full.accumulator(), full.framebuffer()
    ranks = []
    for r in range(world):
        be = HipBackend.init(w, h, 1.0, rank=r, world=world, tile_size=32)
        be.set_option("p2p_timeout_ms", 5000)
        be.set_option("denoise", 3)
        scene.mark_all_changed()
        scene.sync(be)
        be.comm_init_loopback(0x40E7, r, world)
        ranks.append(be)
    errors = []

    def run(be):
        try:
            be.render(view)
        except Exception as e:  # (reported below)
            errors.append(e)
    threads = [threading.Thread(target=run, args=(be,)) for be in ranks]
    for t in threads:
        t.start()
        time.sleep(0.002)
    for t in threads:
        t.join()
    assert not errors, errors
    for be in ranks:  # the gathered RGB (w does not travel)
        assert np.array_equal(bits(be.accumulator()[..., :3]), bits(acc[..., :3]))
        assert np.array_equal(bits(be.framebuffer()[..., :3]), bits(fb[..., :3]))
    for be in ranks + [full]:
        be.close()
