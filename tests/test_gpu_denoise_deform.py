"""Option "denoise_deform" (include/rfw_hip.h, DESIGN.md "Denoiser: deforming meshes"): the temporal denoiser follows skinned meshes
(csrc/denoise.inc: k_dn_tris, k_dn_pose, k_dn_motion's state 3, k_dn_temporal_deform).

Off by default and then no bit changes; without a skinned copy in the scene it changes no bit either.  The blend is held against a float64
numpy restatement fed with the device's own previous history, ids, guides, records, view, accumulator, triangle plane and the previous
image's rows of the "triangles" tap.  Small frames, so that tests/test_denoise_deform_on_cpu.py can run the file on the emulated library.

Bounds (the largest figure measured over the test's cases on the emulated library - the same float32 operations, without contraction, as the
device build - times 4, rounded up to one significant digit):
  test_the_taps: |M (w v0 + u v1 + v v2) - g1| measured 2.4e-4 over the hit pixels of the skinned scene (three poses) and of the Cornell
    box seen from behind, bound 1e-3.  The figure is the 16-bit barycentrics': the worst pixels lie on the skinned scene's room, whose
    triangles have edges of up to 16, and 16 / 65535 = 2.4e-4; on the skinned tubes the figure is 1.6e-5, on the Cornell box 6.1e-5.
  test_the_formula_restated: |x - want| / max(1, |want|) measured 4.2e-5, bound 2e-4; |h - want| measured 6.1e-5, bound 3e-4; at most 1
    pixel of a frame (of about 7500 filtered ones) had a weight sum within 1e-4 of the threshold (the condition is at most 0.5 %).  The
    worst pixel of every image is a pixel of the room (state 1), where the formula is the predecessor's; over the state 3 pixels alone the
    largest x deviation was 3.8e-5.
ISA (tests/test_denoise_deform_on_cpu.py): in the parent commit's listing k_dn_temporal takes 43 VGPRs and k_dn_temporal_motion 44."""

import ctypes as C

import numpy as np
import pytest

from rfw_rs_amd import BackendError, Scene, pod
from conftest import rel_l2
from test_gpu_denoise import ALBEDO_FLOOR, DEFAULT_COLOUR, atrous_restated, attach, bits, render
from test_gpu_denoise_temporal import MIN_WEIGHT, demodulated, sequence, temporal
from test_gpu_denoise_motion import MOTIONS, NO_ID, image, instance_list, motion_backend, motion_restated, move, spheres_scene, translation

pytestmark = pytest.mark.gpu
W = H = 64
FLIPPED = 0x80000000
TAP_BOUND, X_BOUND, H_BOUND = 1e-3, 2e-4, 3e-4


def deform_backend(scene, w=W, h=H, passes=1, hmax=8, **options):
    be = motion_backend(scene, w, h, passes, hmax, **options)
    be.set_option("denoise_deform", 1)
    return be


def skinned_ids(scene):
    """the instance ids that carry a skin"""
    return [k for k, (mesh, slot) in enumerate(instance_list(scene)) if scene.instance_matrix(mesh, slot)[1] >= 0]


def triangles(be):
    """the device triangle buffer as (rows, 11, 4) float32: static meshes, then the skinned copies"""
    return np.frombuffer(be.debug_read("triangles", 1 << 26).tobytes(), np.float32).reshape(-1, 11, 4).copy()


def taps(be):
    a, b, state = be.denoise_motion()
    return be.accumulator(), be.framebuffer(), be.denoise_history(), be.denoise_ids(), np.concatenate([a.reshape(len(a), 12), b.reshape(len(b), 9)], 1), state


def same_taps(a, b):
    return all(x.shape == y.shape and np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def posed(be, scene, view, count=3):
    """`count` images of the skinned scene, a pose each; every image's taps"""
    out = []
    for i in range(count):
        scene.pose(0.1 * i)
        image(be, scene, view)
        out.append(taps(be))
    return out


# ---------------------------------------------------------------- 1. off is untouched
def test_off_is_untouched():
    scene = Scene().build("skinned")
    view = scene.view(W, H)
    empty = lambda b: b.denoise_tris().size == 0 and b.denoise_pose()[0].size == 0 and b.denoise_pose()[1].size == 0
    want = {}
    for name, make in (("motion", lambda: motion_backend(scene)), ("temporal", lambda: temporal(scene))):
        be = make()
        want[name] = posed(be, scene, view)
        be.close()
    be = motion_backend(scene)
    be.set_option("denoise_deform", 0)
    assert all(same_taps(g, w_) for g, w_ in zip(posed(be, scene, view), want["motion"])), "the option named with 0"
    assert empty(be)
    be.close()
    be = temporal(scene)
    be.set_option("denoise_deform", 1)  # without denoise_motion: nothing
    assert all(same_taps(g, w_) for g, w_ in zip(posed(be, scene, view), want["temporal"])), "on without denoise_motion"
    assert empty(be), "nothing is allocated or written"
    be.close()
    be = deform_backend(scene)
    posed(be, scene, view, 2)
    assert not empty(be) and 3 in list(be.denoise_motion()[2])
    be.set_option("denoise_deform", 0)
    assert empty(be), "off: released"
    assert all(same_taps(g, w_) for g, w_ in zip(posed(be, scene, view), want["motion"])), "on and off again: a fresh instance's bits"
    assert empty(be)
    for value in (2, -1, 0.5, float("nan")):
        with pytest.raises(BackendError):
            be.set_option("denoise_deform", value)
    be.close()


# ---------------------------------------------------------------- 2. no skinned copy, no change
def test_no_skinned_copy_no_change():
    runs = []
    for on in (0, 1):
        scene, mesh = spheres_scene()
        views = sequence(scene.view(W, H), 4, 0.02, -0.015)
        be = motion_backend(scene, W, H, 2, 8)
        be.set_option("denoise_deform", on)
        out = []
        for i in range(4):
            if i:
                for slot in range(4):
                    move(scene, mesh, slot, MOTIONS[(slot + i) % 4])
            scene.sync(be)
            be.render(views[i])
            out.append(taps(be))
        if on:
            table, pose = be.denoise_pose()
            assert table.shape == (5, 3) and not table.any() and pose.shape[0] == 0
            assert list(out[-1][5]) == [1, 2, 2, 2, 2]
        runs.append(out)
        be.close()
    for i, (a, b) in enumerate(zip(*runs)):
        assert same_taps(a, b), i


# ---------------------------------------------------------------- 3. states
def send_instances(be, scene, mesh, skin_of):
    """set_3d_instances of `mesh` with the scene's matrices and skin ids but for the slots of `skin_of`, straight at the backend"""
    mats, skin_ids = [], []
    while True:
        try:
            m, skin = scene.instance_matrix(mesh, len(mats))
        except KeyError:
            break
        skin_ids.append(skin_of.get(len(mats), skin))
        mats.append(m)
    m = (pod.Mat4 * len(mats))(*[pod.Mat4((C.c_float * 16)(*np.asarray(a, np.float32).T.reshape(16))) for a in mats])
    s = (C.c_int32 * len(mats))(*skin_ids)
    d = pod.InstancesData3D()
    d.local_aabb = scene.mesh_data(mesh).bounds
    d.matrices, d.num_matrices = m, len(mats)
    d.skin_ids, d.num_skin_ids = s, len(mats)
    d.flags, d.num_flags = None, 0
    be.set_3d_instances(mesh, d)
    be.synchronize()


def test_states():
    scene = Scene().build("skinned")
    view = scene.view(W, H)
    il = instance_list(scene)
    sk = skinned_ids(scene)
    assert len(sk) == 2 and len(il) == 4
    expect = [3 if k in sk else 1 for k in range(len(il))]
    be = deform_backend(scene)
    scene.pose(0.0)
    image(be, scene, view)
    a, b, state = be.denoise_motion()
    assert list(state) == [0] * len(il) and not a.any() and not b.any(), "the first image after a drop has no history"
    for i in (1, 2):
        scene.pose(0.1 * i)
        image(be, scene, view)
        assert list(be.denoise_motion()[2]) == expect
    table, pose = be.denoise_pose()
    assert all((table[k, 1] > 0) == (k in sk) for k in range(len(il)))
    # a skinned instance under a new matrix: still deforming, and the record carries the previous matrix as it was
    mesh, slot = il[sk[0]]
    before = scene.instance_matrix(mesh, slot)[0].astype(np.float32)
    move(scene, mesh, slot, lambda m: translation((0.02, 0.0, -0.03)) @ m)
    scene.pose(0.3)
    image(be, scene, view)
    a, b, state = be.denoise_motion()
    assert list(state) == expect
    assert np.array_equal(bits(a[sk[0]]), bits(before[:3])), "a = the rows of the previous forward matrix"
    inv_t = np.linalg.inv(before.astype(np.float64)[:3, :3]).T
    assert np.abs(b[sk[0]] - inv_t).max() <= 1e-5 * np.abs(inv_t).max(), "b = the rows of the previous InstanceNormal"
    # the latter copy loses its skin: no history for one image, then an instance like any other; and gets it back
    mesh, slot = il[sk[1]]
    skin = scene.instance_matrix(mesh, slot)[1]
    for ids, first, then in (({slot: -1}, 0, 1), ({slot: skin}, 0, 3)):
        send_instances(be, scene, mesh, ids)
        be.reset_accumulation()
        be.render(view)
        state = list(be.denoise_motion()[2])
        assert state[sk[1]] == first and state[sk[0]] == 3 and state[0] == 1, (ids, state)
        be.reset_accumulation()
        be.render(view)
        state = list(be.denoise_motion()[2])
        assert state[sk[1]] == then and state[sk[0]] == 3, (ids, state)
    be.close()


# ---------------------------------------------------------------- 4. the taps
def rebuilt(tri, tris_tap, matrices, ids):
    """(P, n, hit) per pixel in float64 from the triangle plane: M (w v0 + u v1 + v v2) and the unit normal transpose(inverse(M)) gN, not yet faced"""
    hit = ids != NO_ID
    row = np.where(hit, tri[..., 0] & (FLIPPED - 1), 0).astype(np.int64)
    u, v = (tri[..., 1] & 65535) / 65535.0, (tri[..., 1] >> 16) / 65535.0
    t = tris_tap[row].astype(np.float64)
    p = (1.0 - u - v)[..., None] * t[..., 0, :3] + u[..., None] * t[..., 1, :3] + v[..., None] * t[..., 2, :3]
    m = np.stack(matrices)[np.where(hit, ids, 0)]
    P = np.einsum("hwrc,hwc->hwr", m[..., :3, :3], p) + m[..., :3, 3]
    n = np.einsum("hwrc,hwc->hwr", np.linalg.inv(m[..., :3, :3]).transpose(0, 1, 3, 2), t[..., 3, :3])
    return P, n / np.linalg.norm(n, axis=-1, keepdims=True), hit


def outside():
    """the Cornell box seen from behind its back wall: every primary hit is a back face"""
    scene = Scene().build("cornell")
    scene.set_camera((0.0, 0.0, 3.0), (0.0, 0.0, -1.0))
    return scene


def test_the_taps():
    worst = 0.0
    for name, build, poses in (("skinned", lambda: Scene().build("skinned"), (0.0, 0.15, 0.3)), ("from behind", outside, (None,))):
        scene = build()
        view = scene.view(W, H)
        il = instance_list(scene)
        sk = skinned_ids(scene)
        be = deform_backend(scene)
        for time in poses:
            if time is not None:
                scene.pose(time)
            image(be, scene, view)
            tri, ids, (g0, g1, _) = be.denoise_tris(), be.denoise_ids(), be.denoise_guide()
            tt = triangles(be)
            table, pose = be.denoise_pose()
            assert tri.shape == (H, W, 2) and table.shape == (len(il), 3)
            hit = ids != NO_ID
            assert np.all(tri[~hit][:, 0] == 0xFFFFFFFF) and np.all(tri[~hit][:, 1] == 0), "a miss"
            assert hit.sum() > W * H // 4 and all((ids == k).sum() > 20 for k in sk)
            row = tri[..., 0] & (FLIPPED - 1)
            assert np.all(row[hit] < len(tt))
            for k in sk:  # a skinned pixel's row lies in its copy
                m = ids == k
                assert np.all(row[m] >= table[k, 0]) and np.all(row[m] < table[k, 0] + table[k, 1])
                assert np.array_equal(bits(pose[table[k, 2]:table[k, 2] + table[k, 1]]), bits(tt[table[k, 0]:table[k, 0] + table[k, 1], :4])), "the snapshot is rows 0-3 of the copy"
            assert pose.shape[0] == table[:, 1].sum() and (len(sk) > 0) == (pose.shape[0] > 0)
            mats = [scene.instance_matrix(mesh, slot)[0].astype(np.float64) for mesh, slot in il]
            P, n, _ = rebuilt(tri, tt, mats, ids)
            dev = np.abs(P - g1[..., :3])
            worst = max(worst, float(dev[hit].max()))
            facing = (n * g0[..., :3]).sum(-1)
            flipped = tri[..., 0] >> 31 == 1
            assert np.all(np.abs(np.abs(facing[hit]) - 1.0) <= 1e-5), "the guide's normal is the triangle's, faced"
            assert np.array_equal(flipped[hit], (facing < 0.0)[hit]), "bit 31: the normal was negated"
            assert flipped[hit].any() == (name == "from behind")
            print(f"deform taps, {name} {time}: |M (w v0 + u v1 + v v2) - g1| {dev[hit].max():.3e}" + (f" (on the skinned instances {dev[np.isin(ids, sk)].max():.3e})" if sk else "")
                  + f", flipped {flipped[hit].sum()} of {hit.sum()}, largest |g1| {np.abs(g1[..., :3])[hit].max():.2f}")
        be.close()
    print(f"deform taps: worst {worst:.3e} (bound {TAP_BOUND})")
    assert worst <= TAP_BOUND


# ---------------------------------------------------------------- 5. the formula, restated in float64
def deform_restated(acc, n, guide, ids, records, tri, table, prev, hmax):
    """DESIGN.md "Denoiser: deforming meshes" in float64: a state 3 pixel gets P~ and n~ from the previous image's triangle rows, and from
    there it is a pixel that did not move.  prev = None or (history plane, g0, g1, view, ids, table, "triangles" tap) of the previous image.
    Returns motion_restated's tuple with the state of every filtered pixel's instance as the device reports it."""
    g0, g1, g2 = (g.astype(np.float64) for g in guide)
    a, b, st = records
    f = g2[..., 3] > 0.0
    if prev is None:
        return motion_restated(acc, n, (g0, g1, g2), ids, records, None, hmax)
    i = np.where(f, ids, 0).astype(np.int64)
    state = np.where(f, st[i], 0).astype(np.int64)
    s3 = state == 3
    ptable, ptris = prev[5].astype(np.int64), prev[6]
    local = (tri[..., 0] & (FLIPPED - 1)).astype(np.int64) - table.astype(np.int64)[i, 0]
    assert np.all((local >= 0)[s3]) and np.all((local < ptable[i, 1])[s3]), "every deforming pixel's triangle lies in its copy"
    t = ptris[np.where(s3, ptable[i, 0] + local, 0)].astype(np.float64)
    u, v = (tri[..., 1] & 65535) / 65535.0, (tri[..., 1] >> 16) / 65535.0
    p = (1.0 - u - v)[..., None] * t[..., 0, :3] + u[..., None] * t[..., 1, :3] + v[..., None] * t[..., 2, :3]
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    P = np.einsum("hwrc,hwc->hwr", a64[i][..., :3], p) + a64[i][..., 3]
    nn = np.einsum("hwrc,hwc->hwr", b64[i], t[..., 3, :3])
    nn = nn / np.where(s3, np.linalg.norm(nn, axis=-1), 1.0)[..., None]
    nn = np.where((tri[..., 0] >> 31 == 1)[..., None], -nn, nn)
    g1[s3, :3] = P[s3]
    g0[s3, :3] = nn[s3]
    x, h, sw, f, _ = motion_restated(acc, n, (g0, g1, g2), ids, (a, b, np.where(st == 3, 1, st)), prev[:5], hmax)
    return x, h, sw, f, state


def test_the_formula_restated():
    """Five images at 96 x 96; before each the skin takes a new pose and the camera moves sideways and turns; the third image gets a second
    sample, which rewrites its history from the same previous one.  Figures: the module's docstring."""
    w = h = 96
    scene = Scene().build("skinned")
    views = sequence(scene.view(w, h), 5, 0.02, -0.015)
    sk = skinned_ids(scene)
    passes, hmax = 1, 8
    be = deform_backend(scene, w, h, passes, hmax)
    last, worst_x, worst_h, left_out, kept = {}, 0.0, 0.0, 0, 0
    for i, n in ((0, 1), (1, 1), (2, 1), (2, 2), (3, 1), (4, 1)):
        if n == 1:
            scene.pose(0.1 * i)
            scene.sync(be)
        be.render(views[i])
        assert be.frame_stats()["sample_count"] == n
        acc, fb, guide, hist, ids, records = be.accumulator(), be.framebuffer(), be.denoise_guide(), be.denoise_history(), be.denoise_ids(), be.denoise_motion()
        tri, (table, _), tt = be.denoise_tris(), be.denoise_pose(), triangles(be)
        want_x, want_h, sw, f, state = deform_restated(acc, n, guide, ids, records, tri, table, last.get(i - 1), hmax)
        c = demodulated(acc, n, guide)
        assert f.sum() > w * h // 4 and not np.any(np.isnan(hist)) and np.all(hist[~f] == 0.0)
        assert all((f & (ids == k)).sum() > 60 for k in sk), "both skinned instances are in view"
        if i == 0:
            assert np.all(hist[f][:, 3] == n) and np.array_equal(bits(hist[f][:, :3]), bits(c[f]))
        else:
            assert [records[2][k] for k in sk] == [3, 3]
            near = f & (np.abs(sw - MIN_WEIGHT) <= 1e-4)
            left_out = max(left_out, int(near.sum()))
            assert near.sum() <= 0.005 * f.sum(), (i, n, int(near.sum()))
            m = f & ~near
            dev_x = np.abs(hist[..., :3] - want_x) / np.maximum(1.0, np.abs(want_x))
            dev_h = np.abs(hist[..., 3] - want_h)
            worst_x, worst_h = max(worst_x, float(dev_x[m].max())), max(worst_h, float(dev_h[m].max()))
            valid = f & (hist[..., 3] > n)
            kept += int((valid & (state == 3)).sum())
            at = np.unravel_index(np.argmax(np.where(m, dev_x.max(-1), -1.0)), m.shape)
            print(f"deform formula image {i} n={n}: x {dev_x[m].max():.3e} (state {state[at]}, weight sum {sw[at]:.4f}), h {dev_h[m].max():.3e}, near the threshold {near.sum()} of {f.sum()}, "
                  f"x on state 3 {dev_x[m & (state == 3)].max():.3e}, valid {valid.sum() / f.sum():.3f}, valid on the skinned {(valid & (state == 3)).sum() / max((f & (state == 3)).sum(), 1):.3f}")
            assert np.all(dev_x[m] <= X_BOUND), (i, n, float(dev_x[m].max()))
            assert np.all(dev_h[m] <= H_BOUND), (i, n, float(dev_h[m].max()))
            none = f & (sw < MIN_WEIGHT - 1e-4)
            assert none.any() and np.all(hist[none][:, 3] == n) and np.array_equal(bits(hist[none][:, :3]), bits(c[none])), "h = n and x = c, bit for bit"
        x = hist[..., :3].astype(np.float64)
        al = np.maximum(guide[2][..., :3].astype(np.float64), ALBEDO_FLOOR)
        want, _ = atrous_restated(x * al * n, n, guide, passes, DEFAULT_COLOUR)
        dev = np.abs(fb[..., :3] - want) / np.maximum(1.0, np.abs(want))
        assert np.all(dev[f] <= 1e-5), (i, n, float(dev[f].max()))
        last[i] = (hist, guide[0], guide[1], views[i], ids, table, tt)
    print(f"deform formula: worst x {worst_x:.3e} (bound {X_BOUND}), worst h {worst_h:.3e} (bound {H_BOUND}), left out at most {left_out} pixels of a frame, "
          f"{kept} state 3 pixels kept a history")
    assert kept > 200, "pixels of deforming instances keep a history"
    be.close()


# ---------------------------------------------------------------- 7. neighbours
def test_frame_slots_and_sub_streams_give_the_same_bits():
    def run(**options):
        scene = Scene().build("skinned")
        views = sequence(scene.view(W, H), 4, 0.02, 0.015)
        be = deform_backend(scene, passes=2, tile_size=16, **options)
        out = []
        for i, v in enumerate(views):
            scene.pose(0.1 * i)
            scene.sync(be)
            be.render(v)
            out.append(taps(be)[1:] + (be.denoise_tris(),))
        be.close()
        return out
    want = run()
    assert 3 in list(want[-1][4]) and (want[-1][1][..., 3] > 1.0).any()
    for options in ({"frames_in_flight": 3}, {"streams": 2}):
        got = run(**options)
        for i, (w_, g_) in enumerate(zip(want, got)):
            for what, a, b in zip(("frame", "history", "ids", "records", "states", "triangle plane"), w_, g_):
                assert np.array_equal(bits(a), bits(b)), (options, i, what)


def test_render_samples_modes_and_resize():
    scene = Scene().build("skinned")
    views = sequence(scene.view(W, H), 3)
    one, seq = deform_backend(scene, passes=2, max_batch=4), deform_backend(scene, passes=2)
    for b in (one, seq):
        b.render(views[0])
    scene.pose(0.1)
    for b in (one, seq):
        scene.mark_all_changed()
        scene.sync(b)
    one.render_samples(views[1], 3)
    render(seq, views[1], 3)
    assert one.frame_stats()["sample_count"] == 3
    assert np.array_equal(one.denoise_tris(), seq.denoise_tris()), "the plane is the LAST sample's"
    assert np.array_equal(one.denoise_ids(), seq.denoise_ids())
    assert 3 in list(one.denoise_motion()[2]) and list(one.denoise_motion()[2]) == list(seq.denoise_motion()[2])
    assert rel_l2(one.denoise_history(), seq.denoise_history()) <= 1e-6
    # modes 1-6 neither read nor write the plane, the snapshot, ids, records or history
    hist, ids, records, tri, (table, pose) = seq.denoise_history(), seq.denoise_ids(), seq.denoise_motion(), seq.denoise_tris(), seq.denoise_pose()
    for mode in range(1, 7):
        seq.render(views[2], mode=mode)
        assert np.array_equal(bits(seq.denoise_history()), bits(hist)) and np.array_equal(seq.denoise_ids(), ids), mode
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(seq.denoise_motion(), records)), mode
        assert np.array_equal(seq.denoise_tris(), tri) and np.array_equal(seq.denoise_pose()[0], table) and np.array_equal(bits(seq.denoise_pose()[1]), bits(pose)), mode
    # a resize drops everything: the next image is plain denoise
    seq.resize((W, H))
    assert seq.denoise_tris().size == 0 and seq.denoise_pose()[0].size == 0 and seq.denoise_pose()[1].size == 0
    seq.render(views[0])
    first = attach(scene, denoise=2)
    first.render(views[0])
    assert np.array_equal(bits(seq.accumulator()), bits(first.accumulator())) and np.array_equal(bits(seq.framebuffer()), bits(first.framebuffer()))
    assert list(seq.denoise_motion()[2]) == [0] * 4
    for b in (one, seq, first):
        b.close()


# ---------------------------------------------------------------- 6. what it buys (last in the file: the slowest)
def test_it_keeps_the_history():
    """8 images of one sample under a camera that stands still, `denoise` 1, Hmax 16, a new pose before each, with "denoise_motion" alone
    and with the option.  Over the skinned instances' filtered pixels of the last image: more of them have a history (h > n), the mean h is
    higher and the frame is closer to a raw frame of 256 samples of the final pose with the option on.  Over the pixels neither skinned tube
    ever covers the two histories are equal bit for bit.  Figures: DESIGN.md "Denoiser: deforming meshes"."""
    images = 8
    runs = {}
    for on in (0, 1):
        scene = Scene().build("skinned")
        sk = skinned_ids(scene)
        view = scene.view(W, H)
        be = motion_backend(scene, passes=1, hmax=16)
        be.set_option("denoise_deform", on)
        covered = np.zeros((H, W), bool)
        for i in range(images):
            scene.pose(0.1 * i)
            image(be, scene, view)
            covered |= np.isin(be.denoise_ids(), sk)
        f = be.denoise_guide()[2][..., 3] > 0.0
        if on:
            raw = attach(scene)
            runs["ref"] = render(raw, view, 256).framebuffer()[..., :3].copy()
            raw.close()
        runs[on] = (be.framebuffer()[..., :3].copy(), be.denoise_history().copy(), f, be.denoise_ids().copy(), covered)
        be.close()
    ref = runs["ref"]
    (fb0, h0, f0, ids0, cov0), (fb1, h1, f1, ids1, cov1) = runs[0], runs[1]
    assert np.array_equal(f0, f1) and np.array_equal(ids0, ids1) and np.array_equal(cov0, cov1)
    m = f1 & np.isin(ids1, sk)
    assert m.sum() > 100
    share = [float((h[..., 3][m] > 1.0).mean()) for h in (h0, h1)]
    mean_h = [float(h[..., 3][m].mean()) for h in (h0, h1)]
    err = [rel_l2(fb[m], ref[m]) for fb in (fb0, fb1)]
    room = f1 & ~cov1
    print(f"deform keeps the history: {m.sum()} pixels; share with a history off {share[0]:.3f} on {share[1]:.3f}; mean h off {mean_h[0]:.2f} on {mean_h[1]:.2f}; "
          f"rel-L2 against 256 samples off {err[0]:.4f} on {err[1]:.4f}; never covered: {room.sum()} pixels, mean h {h1[..., 3][room].mean():.2f}")
    assert share[1] > share[0] and mean_h[1] > mean_h[0]
    assert err[1] < err[0]
    assert room.sum() > W * H // 4 and np.array_equal(bits(h0[room]), bits(h1[room])), "the rest of the frame is untouched"
