"""rfw_hip_render's `mode` (rfw_backend::RenderMode; include/rfw_hip.h RFW_HIP_RENDER_*, DESIGN.md "Render modes").

Mode 0 and unknown values path trace exactly as before; modes 1-4 add the primary hit's normal, albedo, position + t or view-space position
per sample and finalise the linear mean; 5 traces ambient occlusion rays through the shadow queue; 6 filters 5's result.  Small frames, so
that tests/test_render_modes_on_cpu.py can run the file on the emulated library too."""
import threading
import time

import numpy as np
import pytest

from oracle.bindings import Oracle
from rfw_rs_amd import HipBackend, RenderMode, Scene, pod

pytestmark = pytest.mark.gpu
W = H = 64


def make(kind="cornell", *args, w=W, h=H, **options):
    scene = Scene().build(kind, *args) if kind else Scene()
    be = HipBackend.init(w, h, 1.0, **options)
    scene.sync(be)
    return scene, be, scene.view(w, h)


def attach(scene, w=W, h=H, **options):
    """another backend of the same scene (everything is sent again)"""
    be = HipBackend.init(w, h, 1.0, **options)
    scene.mark_all_changed()
    scene.sync(be)
    return be


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def oracle_of(scene, w=W, h=H):
    orc = Oracle(w, h)
    scene.mark_all_changed()
    scene.sync(orc)
    return orc


def primary_hits(scene, view, w=W, h=H):
    """the camera rays of sample 0 and their closest hits (the oracle's tree; t_min 1e-4 as k_primary)"""
    orc = oracle_of(scene, w, h)
    o, d = orc.primary_rays(view, 0)
    return orc, o, d, orc.intersect(o, d)


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


# ---------------------------------------------------------------- 1. mode 0 and unknown values are untouched
def test_default_and_unknown_modes_path_trace_as_before():
    scene, be, view = make()
    ref = attach(scene)
    for _ in range(2):
        ref.render(view)
    want = ref.accumulator()
    for mode in (0, 7, 1000, RenderMode.DEFAULT):
        be.reset_accumulation()
        for _ in range(2):
            be.render(view, mode=mode)
        assert np.array_equal(bits(be.accumulator()), bits(want)), mode
    # no residue: three albedo frames, then a path-traced image equals a fresh instance's
    for _ in range(3):
        be.render(view, mode=RenderMode.ALBEDO)
    be.render(view)
    fresh = attach(scene)
    fresh.render(view)
    assert np.array_equal(bits(be.accumulator()), bits(fresh.accumulator()))
    assert np.array_equal(bits(be.framebuffer()), bits(fresh.framebuffer()))


def test_the_trait_discriminants():
    assert [m.value for m in RenderMode] == list(range(7))
    assert [m.name for m in RenderMode] == ["DEFAULT", "NORMAL", "ALBEDO", "GBUFFER", "SCREEN_SPACE", "SSAO", "FILTERED_SSAO"]


# ---------------------------------------------------------------- 2. modes 1-4 against the oracle's hits
@pytest.mark.parametrize("kind,args", [("cornell", ()), ("soup", (1500, 5, 0.0, 4)), ("gallery", ())])
def test_position_modes_match_the_oracle(kind, args):
    scene, be, view = make(kind, *args)
    _, o, d, hits = primary_hits(scene, view)
    miss = hits["inst"] < 0
    be.render(view, mode=RenderMode.GBUFFER)
    g = be.accumulator().reshape(-1, 4)
    assert np.array_equal(g[miss], np.zeros_like(g[miss])), "a miss is (0, 0, 0, 0)"
    assert not np.any(np.all(g[~miss] == 0.0, axis=1)), "every hit pixel has a value"
    t = hits["t"][~miss].astype(np.float32)
    P = (o[~miss] + t[:, None] * d[~miss]).astype(np.float32)
    scale = np.maximum(np.linalg.norm(P, axis=1), 1.0)
    assert np.all(np.abs(g[~miss, 3] - t) <= 1e-5 * scale)
    assert np.all(np.abs(g[~miss, :3] - P).max(axis=1) <= 1e-5 * scale)
    # view space: (dot(P - pos, r), dot(P - pos, u), dot(P - pos, d), 1) with the view's normalised right, up and direction
    be.render(view, mode=RenderMode.SCREEN_SPACE)
    s = be.accumulator().reshape(-1, 4)
    assert np.array_equal(s[miss], np.zeros_like(s[miss]))
    axis = lambda v: np.array([v.x, v.y, v.z], np.float64) / np.linalg.norm([v.x, v.y, v.z])
    rel = P.astype(np.float64) - np.array([view.pos.x, view.pos.y, view.pos.z])
    want = np.stack([rel @ axis(view.right), rel @ axis(view.up), rel @ axis(view.direction)], axis=1)
    assert np.all(np.abs(s[~miss, :3] - want).max(axis=1) <= 2e-5 * scale)
    assert np.all(s[~miss, 3] == 1.0)
    assert np.all(s[~miss, 2] > 0.0)  # in front of the camera


def f32(x):
    return np.asarray(x, np.float32)


def instance_normal_matrices(scene):
    """transpose(inverse(M)) of every instance in instance-id order (meshes by id, their slots in order), from the scene's own matrices"""
    out = []
    for mesh in range(scene.counts()["meshes"]):
        slot = 0
        while True:
            try:
                m, _ = scene.instance_matrix(mesh, slot)
            except KeyError:
                break
            out.append(np.linalg.inv(m.astype(np.float64)).T[:3, :3])
            slot += 1
    return np.array(out)


def device_hits(be, w=W, h=H):
    """the device's camera-ray hits of the latest frame as (inst, tri) per pixel: k_primary's slab, de-tiled with the numpy twin"""
    from rfw_rs_amd import dist
    _, slot = dist.slab_index_map(w, h, 1)
    n = int(slot.max()) + 1
    hit = np.frombuffer(be.debug_read("hit0", 16 * n).tobytes(), np.uint32).reshape(-1, 4)
    return hit[slot.reshape(-1), 0].view(np.int32), hit[slot.reshape(-1), 1].view(np.int32)


def restate_normal_and_albedo(scene, orc, d, hits, view):
    """Modes 1 and 2 per sample, restated in numpy from the oracle's triangle records, the scene's materials and instance matrices and the
    oracle's texture sampler, in k_shade's order of float32 operations at bounce 0.  Returns (N, albedo, back facing, normal-mapped)."""
    rec = orc.triangles()[hits["tri"]]
    q = lambda k: rec[:, 4 * k:4 * k + 4]
    q0, q1, q2, q3, q4, q5, q6, T0, T1, T2 = (q(k) for k in range(10))
    q10 = rec[:, 40:44].view(np.uint32)
    quant = lambda x: np.floor(np.maximum(x * f32(65535.0), f32(0.0))).astype(np.uint32)  # f2u(65535 u), as k_primary stores it
    u = quant(hits["u"]).astype(np.float32) * f32(1.0 / 65535.0)
    v = quant(hits["v"]).astype(np.float32) * f32(1.0 / 65535.0)
    w = f32(1.0) - u - v
    c = lambda a: a[:, None]
    N = c(w) * q4[:, :3] + c(u) * q5[:, :3] + c(v) * q6[:, :3]
    T = c(w) * T0[:, :3] + c(u) * T1[:, :3] + c(v) * T2[:, :3]
    Tw = w * T0[:, 3] + u * T1[:, 3] + v * T2[:, 3]
    nm = instance_normal_matrices(scene)[hits["inst"]]
    xf = lambda a: np.einsum("nij,nj->ni", nm, a.astype(np.float64))
    unit = lambda a: f32(a / np.linalg.norm(np.asarray(a, np.float64), axis=-1, keepdims=True))
    gN, N, T = unit(xf(q3[:, :3])), unit(xf(N)), unit(xf(T))
    B = f32(np.cross(N, T)) * c(Tw)
    mats = [scene.material(i) for i in range(scene.counts()["materials"])]
    mat = q10[:, 1]
    colour = f32([mats[k]["color"][:3] for k in mat])
    maps = ("diffuse_tex", "normal_tex", "metallic_roughness_tex", "emissive_tex", "sheen_tex")
    normal_mapped = np.zeros(len(mat), bool)
    for i in range(len(mat)):
        m = mats[mat[i]]
        light = max(m["color"][:3]) > 1.0 and m["emissive_tex"] < 0
        if light or not any(m[t] >= 0 for t in maps):
            continue
        lam = np.sqrt(q10[i:i + 1, 2].view(np.float32)[0]) + np.log2(f32(view.spread_angle) * (f32(1.0) / abs(np.dot(d[i], N[i]))))
        tu = w[i] * q0[i, 3] + u[i] * q1[i, 3] + v[i] * q2[i, 3]
        tv = w[i] * q3[i, 3] + u[i] * q4[i, 3] + v[i] * q5[i, 3]
        if m["diffuse_tex"] >= 0:
            colour[i] = colour[i] * orc.sample_texture(m["diffuse_tex"], tu, tv, lam, trilinear=True)[:3]
        if m["normal_tex"] >= 0:
            mm = (orc.sample_texture(m["normal_tex"], tu, tv, float(int(lam)))[:3] - f32(0.5)) * f32(2.0)
            N[i] = unit((T[i] * mm[0] + B[i] * mm[1]) + N[i] * mm[2])
            normal_mapped[i] = True
    back = np.einsum("ij,ij->i", d, gN) >= 0.0
    N[back] = -N[back]
    return N, colour, back, normal_mapped


@pytest.mark.parametrize("kind,args", [("cornell", ()), ("soup", (1500, 5, 0.0, 4)), ("gallery", ())])
def test_normal_and_albedo_modes_restated(kind, args):
    scene, be, view = make(kind, *args)
    orc, o, d, hits = primary_hits(scene, view)
    miss = hits["inst"] < 0
    be.render(view, mode=RenderMode.NORMAL)
    inst, tri = device_hits(be)
    assert np.array_equal(inst, hits["inst"]) and np.array_equal(tri[~miss], hits["tri"][~miss]), "the same hits on every pixel"
    n = be.accumulator().reshape(-1, 4)
    be.render(view, mode=RenderMode.ALBEDO)
    a = be.accumulator().reshape(-1, 4)
    for img in (n, a):
        assert np.array_equal(img[miss], np.zeros_like(img[miss])), "a miss is (0, 0, 0, 0)"
        assert np.all(img[~miss, 3] == 0.0)
    N, colour, back, normal_mapped = restate_normal_and_albedo(scene, orc, d[~miss], hits[~miss], view)
    assert np.abs(n[~miss, :3] - N).max() <= 1e-5, np.abs(n[~miss, :3] - N).max()
    assert np.abs(a[~miss, :3] - colour).max() <= 1e-5, np.abs(a[~miss, :3] - colour).max()
    if kind == "soup":
        assert back.any() and (~back).any(), "both faces of the soup are seen"
    if kind == "gallery":
        assert normal_mapped.any(), "the bump-mapped material is seen"
        assert len(np.unique(colour, axis=0)) > 20, "the diffuse map shows"
    if kind == "cornell":
        assert np.any(a[~miss, :3].max(axis=1) > 1.0), "the light shows its stored colour"


def test_samples_accumulate_and_finalise_linearly():
    scene, be, view = make("cornell")
    orc = oracle_of(scene)
    per = []
    for s in range(3):  # the restated per-sample normals of samples 0, 1, 2 (each its own jittered camera rays)
        o, d = orc.primary_rays(view, s)
        hits = orc.intersect(o, d)
        hit = hits["inst"] >= 0
        img = np.zeros((W * H, 4), np.float32)
        img[hit, :3] = restate_normal_and_albedo(scene, orc, d[hit], hits[hit], view)[0]
        per.append(img.reshape(H, W, 4))
    for _ in range(3):
        be.render(view, mode=RenderMode.NORMAL)
    acc = be.accumulator()
    assert np.abs(acc - ((per[0] + per[1]) + per[2])).max() <= 3e-5
    fb = be.framebuffer()
    assert np.array_equal(bits(fb), bits(acc * np.float32(1.0) / np.float32(3.0)))
    assert np.any(fb[..., :3] < 0.0) and not np.any(np.isnan(fb))  # no sqrt: negative components survive
    steps = be.srgb_steps()
    pres = be.host_frame(presented=True)
    be.download_frame(pres)
    be.wait_downloads()
    enc = lambda x: np.searchsorted(steps, x, side="right").astype(np.uint8)
    want = np.stack([enc(fb[..., 2]), enc(fb[..., 1]), enc(fb[..., 0]), np.full(fb.shape[:2], 255, np.uint8)], axis=-1)
    assert np.array_equal(pres.reshape(want.shape), want)


# ---------------------------------------------------------------- 3. AO ray by ray against the oracle's any-hit
def ao_rays(be):
    r = np.frombuffer(be.debug_read("ao_rays", 32 * W * H * 4).tobytes(), np.float32).reshape(-1, 8)
    return r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7].view(np.uint32)


@pytest.mark.parametrize("kind,args", [("cornell", ()), ("soup", (1500, 5, 0.0, 4))])
def test_ao_against_the_oracle_any_hit(kind, args):
    scene, be, view = make(kind, *args)
    orc, o, d, hits = primary_hits(scene, view)
    hit = hits["inst"] >= 0
    be.set_option("ao_samples", 1)
    be.render(view, mode=RenderMode.SSAO)
    acc = be.accumulator().reshape(-1, 4)
    ro, tmax, rd, px = ao_rays(be)
    assert np.array_equal(px, np.flatnonzero(hit)), "one ray per hit pixel"
    P = o[px] + hits["t"][px][:, None] * d[px]
    lo, hi = P.min(axis=0), P.max(axis=0)
    assert np.all(np.linalg.norm(ro - P, axis=1) <= 1e-3 * max(np.linalg.norm(hi - lo), 1.0))
    assert np.all(np.abs(np.linalg.norm(rd, axis=1) - 1.0) <= 1e-6)
    assert np.all(tmax > 0.0) and np.all(tmax == tmax[0])
    # about the faced geometric normal (the filter guide holds it): the ray leaves the side the camera sees
    guide = np.frombuffer(be.debug_read("ao_guide", W * H * 16).tobytes(), np.float32).reshape(-1, 4)
    assert np.all(np.einsum("ij,ij->i", rd, guide[px, :3]) > 0.0)
    assert np.all(np.einsum("ij,ij->i", d[px], guide[px, :3]) <= 0.0)
    assert np.array_equal(guide[px, 3], hits["t"][px]) and np.all(guide[~hit] == 0.0)
    occ = orc.occludes(ro, rd, tmax, 1e-3)
    assert np.array_equal(acc[px, 0], (1 - occ).astype(np.float32))
    assert np.all(acc[px, 0] == acc[px, 1]) and np.all(acc[px, 3] == 0.0)
    assert np.array_equal(acc[~hit], np.zeros_like(acc[~hit]))
    be.set_option("ao_samples", 4)
    be.render(view, mode=RenderMode.SSAO)
    a4 = be.accumulator().reshape(-1, 4)[hit, 0]
    assert set(np.unique(a4).tolist()) <= {0.0, 0.25, 0.5, 0.75, 1.0}


def test_ao_on_closed_form_scenes():
    # a floor alone: nothing occludes
    scene = floor_scene()
    be = attach(scene)
    view = scene.view(W, H)
    be.render(view, mode=RenderMode.SSAO)
    a = be.accumulator()
    assert np.all(a[..., 0] == 1.0), "the open floor is not occluded"
    # its rays are cosine-distributed about +y: cos^2 and the azimuth are uniform (chi-square, 16 bins, p ~ 1e-4)
    be.set_option("ao_samples", 8)
    dirs = []
    for _ in range(4):
        be.render(view, mode=RenderMode.SSAO)
        dirs.append(ao_rays(be)[2])
    d = np.concatenate(dirs)
    assert np.all(d[:, 1] > 0.0)
    for x in (d[:, 1] ** 2, (np.arctan2(d[:, 2], d[:, 0]) + np.pi) / (2 * np.pi)):
        counts = np.histogram(x, bins=16, range=(0.0, 1.0))[0]
        e = len(x) / 16.0
        assert ((counts - e) ** 2 / e).sum() < 45.0, counts
    # the camera between the floor and a ceiling that covers it, radius far beyond the gap: everything is occluded
    scene = floor_scene([((0.0, -1.0, 0.0), (0.0, 0.05, 0.0), 400.0, 400.0)], camera=((0.0, 0.025, 0.0), (0.0, -1.0, -0.2)))
    be = attach(scene)
    be.set_option("ao_radius", 1e4)
    be.render(scene.view(W, H), mode=RenderMode.SSAO)
    assert np.all(be.accumulator()[..., :3] == 0.0)


def test_ao_next_to_a_wall_matches_a_monte_carlo_estimate():
    """A floor (y = 0) and a wall (z = -1, facing +z): a floor point at height h = z + 1 in front of the wall is occluded along a
    cosine-weighted direction about +y iff the direction leaves towards the wall and meets it within the radius: -d_z > h / radius.  The
    device's AO, every round of 8 rays over 8 samples, against a numpy Monte-Carlo estimate of the same geometry, within 4 sigma."""
    scene = floor_scene([((0.0, 0.0, 1.0), (0.0, 100.0, -1.0), 400.0, 200.0)], camera=((0.0, 1.5, 1.5), (0.0, -1.0, -0.9)))
    be = attach(scene)
    view = scene.view(W, H)
    radius, samples, rays = 1.0, 8, 8
    be.render(view, mode=RenderMode.GBUFFER)
    P = be.accumulator().reshape(-1, 4)
    floor = (P[:, 3] > 0.0) & (np.abs(P[:, 1]) < 1e-4) & (P[:, 2] > -1.0)
    h = P[floor, 2].astype(np.float64) + 1.0
    assert floor.sum() > 1000 and (h < radius).mean() > 0.3, "the band near the wall is in view"
    be.set_option("ao_samples", rays)
    be.set_option("ao_radius", radius)
    be.render(view, mode=RenderMode.SSAO)
    first = be.accumulator().reshape(-1, 4)[floor, 0]
    assert np.any((first > 0.0) & (first < 1.0)), "the rounds of one sample go in different directions"
    for _ in range(samples - 1):
        be.render(view, mode=RenderMode.SSAO)
    ao = be.framebuffer().reshape(-1, 4)[floor, 0].astype(np.float64)
    rng = np.random.default_rng(7)
    r0, r1 = rng.random(200000), rng.random(200000)
    dz = np.sqrt(1.0 - r1) * np.sin(2.0 * np.pi * r0)  # a horizontal component of a cosine-weighted direction about +y
    occluded_beyond = np.sort(-dz[dz < 0.0])               # a ray towards the wall is occluded iff -d_z > h / radius
    p = 1.0 - (len(occluded_beyond) - np.searchsorted(occluded_beyond, h / radius, side="right")) / len(dz)
    k = samples * rays
    sigma = np.sqrt((p * (1.0 - p)).sum() / k) / len(p)
    assert abs(ao.mean() - p.mean()) <= 4.0 * sigma, (ao.mean(), p.mean(), sigma)
    assert p.min() < 0.8 and p.max() > 0.99  # (the band does hold partly occluded points)


# ---------------------------------------------------------------- 5. mode 6
def filter_restated(acc, n, guide):
    ao = acc[..., 0] / np.float32(n)
    N, t = guide[..., :3].astype(np.float64), guide[..., 3].astype(np.float64)
    h, w = ao.shape
    out = np.zeros((h, w), np.float64)
    for y in range(h):
        for x in range(w):
            if t[y, x] <= 0.0:
                continue
            y0, y1, x0, x1 = max(0, y - 3), min(h, y + 4), max(0, x - 3), min(w, x + 4)
            c = np.maximum(0.0, (N[y0:y1, x0:x1] * N[y, x]).sum(-1)) ** 8
            wt = c * np.maximum(0.0, 1.0 - np.abs(t[y, x] - t[y0:y1, x0:x1]) / (0.05 * t[y, x]))
            wt[t[y0:y1, x0:x1] <= 0.0] = 0.0
            out[y, x] = (wt * ao[y0:y1, x0:x1]).sum() / wt.sum()
    return out


def test_filtered_ao():
    scene, be, view = make("cornell")
    ref = attach(scene)
    for _ in range(3):
        be.render(view, mode=RenderMode.FILTERED_SSAO)
        ref.render(view, mode=RenderMode.SSAO)
    acc = be.accumulator()
    assert np.array_equal(bits(acc), bits(ref.accumulator()))
    guide = np.frombuffer(be.debug_read("ao_guide", W * H * 16).tobytes(), np.float32).reshape(H, W, 4)
    fb = be.framebuffer()
    want = filter_restated(acc, 3, guide)
    assert np.abs(fb[..., 0] - want).max() <= 1e-5
    assert np.array_equal(fb[..., 0], fb[..., 1]) and np.all(fb[..., 3] == 0.0)
    # smoother than the unfiltered estimate on the partly occluded walls
    raw = ref.framebuffer()[..., 0]
    hit = guide[..., 3] > 0.0
    assert np.var(fb[..., 0][hit]) < 0.5 * np.var(raw[hit]) or np.var(raw[hit]) == 0.0
    # the open floor stays 1
    scene = floor_scene()
    be = attach(scene)
    be.render(scene.view(W, H), mode=RenderMode.FILTERED_SSAO)
    assert np.all(be.framebuffer()[..., 0] == 1.0)


# ---------------------------------------------------------------- 6. slots, streams, exchange
def test_modes_over_frame_slots_and_samples():
    scene, be, view = make("cornell", frames_in_flight=3, max_batch=4)
    fresh = {}
    for mode in (RenderMode.DEFAULT, RenderMode.ALBEDO, RenderMode.SSAO):
        one = attach(scene)
        for _ in range(2):
            one.render(view, mode=mode)
        fresh[mode] = one.accumulator()
    for mode in (RenderMode.ALBEDO, RenderMode.DEFAULT, RenderMode.SSAO, RenderMode.ALBEDO):
        for _ in range(2):
            be.render(view, mode=mode)
        assert np.array_equal(bits(be.accumulator()), bits(fresh[mode])), mode
    # render_samples has no mode: after an albedo image it starts a path-traced one
    be.render(view, mode=RenderMode.ALBEDO)
    be.render_samples(view, 2)
    one = attach(scene, max_batch=4)
    one.render_samples(view, 2)
    assert np.array_equal(bits(be.accumulator()), bits(one.accumulator()))


@pytest.mark.parametrize("mode", [RenderMode.ALBEDO, RenderMode.SSAO])
def test_sub_streams_and_repeats_give_the_same_bits(mode):
    out = []
    for streams in (1, 2, 2):
        scene, be, view = make("cornell", tile_size=16, streams=streams)
        for _ in range(2):
            be.render(view, mode=mode)
        out.append((be.accumulator(), be.framebuffer()))
    for acc, fb in out[1:]:
        assert np.array_equal(bits(acc), bits(out[0][0])) and np.array_equal(bits(fb), bits(out[0][1]))


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_ranks_through_the_loopback_hub(fmt):
    w, h, world = 96, 64, 3
    scene = Scene().build("cornell")
    scene.set_aspect(w / h)
    view = scene.view(w, h)
    full = HipBackend.init(w, h, 1.0)
    scene.sync(full)
    ranks = []
    for r in range(world):
        be = HipBackend.init(w, h, 1.0, rank=r, world=world, tile_size=32)
        be.set_option("gather_format", fmt)
        be.set_option("p2p_timeout_ms", 5000)
        scene.mark_all_changed()
        scene.sync(be)
        be.comm_init_loopback(0x40D0 + fmt, r, world)
        ranks.append(be)
    for mode in (RenderMode.NORMAL, RenderMode.SSAO):
        full.render(view, mode=mode)
        acc, fb = full.accumulator(), full.framebuffer()
        pres = full.host_frame(presented=True)
        full.download_frame(pres)
        full.wait_downloads()
        errors = []

        def run(be):
            try:
                be.render(view, mode=mode)
            except Exception as e:  # (reported below)
                errors.append(e)
        threads = [threading.Thread(target=run, args=(be,)) for be in ranks]
        for t in threads:
            t.start()
            time.sleep(0.002)
        for t in threads:
            t.join()
        assert not errors, errors
        for be in ranks:
            if fmt == 0:  # the gathered RGB (w does not travel)
                assert np.array_equal(bits(be.accumulator()[..., :3]), bits(acc[..., :3])), mode
                assert np.array_equal(bits(be.framebuffer()[..., :3]), bits(fb[..., :3])), mode
            elif fmt == 1:
                assert np.array_equal(be.framebuffer()[..., :3], fb[..., :3].astype(np.float16).astype(np.float32)), mode
            else:
                dst = be.host_frame(presented=True)
                be.download_frame(dst)
                be.wait_downloads()
                assert np.array_equal(dst, pres), mode
    for be in ranks + [full]:
        be.close()
