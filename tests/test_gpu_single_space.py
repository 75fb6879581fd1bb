"""Single-space scenes (DESIGN.md "Single-space scenes"; option "single_space"): a scene whose instances are all exactly the identity, one per
mesh, is traced as ONE tree in one space — no TLAS step, no entry into or exit from an instance.  The yardstick is the unchanged two-level
path of the same library (single_space = 0): accumulators are compared bit for bit, at max path length 1 and 3, for every kernel family
(packets, one ray per lane, streaming), for scenes that qualify, that do not, and that change between the two over frame slots."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IDENTITY = np.eye(4, dtype=np.float32)


def make_scene(kind):
    """atrium2: a 20 000-triangle atrium and one displaced sphere, 2 meshes with one identity instance each; atrium65: the same atrium and 64
    spheres as 64 meshes (TLAS leaves with several instances, a graft of several nodes); cornell: the Cornell box."""
    from rfw_rs_amd import Scene
    if kind == "cornell":
        return Scene().build("cornell"), 64, 64, []
    scene = Scene().build("atrium", 20000, 0, 0.0, 0xC0FFEE)
    n, quality = (1, 2) if kind == "atrium2" else (64, 1)
    spheres = [scene.add_sphere_mesh(k, 7 + k, quality) for k in range(n)]
    scene.set_aspect(128 / 72)
    return scene, 128, 72, spheres


def backend(w, h, single_space, mpl, options=(), **kw):
    from rfw_rs_amd import HipBackend
    be = HipBackend.init(w, h, 1.0, max_path_length=mpl, **kw)
    be.set_option("single_space", single_space)
    for k, v in options:
        be.set_option(k, v)
    return be


def image(be, scene, view, samples=2):
    scene.mark_all_changed()
    scene.sync(be)
    for _ in range(samples):
        be.render(view)
    return be.accumulator().view(np.uint32).copy()


VARIANTS = {"default": (), "packets_off": (("packet_trace", 0),), "streaming": (("stream_run", 4), ("stream_refill", 16))}


@pytest.mark.parametrize("mpl", [1, 3])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("kind", ["atrium2", "atrium65", "cornell"])
def test_single_space_equals_two_level(kind, variant, mpl):
    scene, w, h, _ = make_scene(kind)
    view = scene.view(w, h)
    out = {}
    for ss in (1, 0):
        be = backend(w, h, ss, mpl, VARIANTS[variant])
        out[ss] = image(be, scene, view)
        assert be.scene_stats()["single_space"] == ss  # all three scenes qualify (Cornell is one mesh under the identity): which path ran is reported
        assert be.frame_stats()["primary_rays"] == w * h
        be.close()
    assert out[1].any()
    assert np.array_equal(out[1], out[0]), int((out[1] != out[0]).sum())


@pytest.mark.parametrize("variant", ["default", "packets_off"])
@pytest.mark.parametrize("kind", ["atrium2", "atrium65", "cornell"])
def test_counting_frames_count_the_single_space_walk(kind, variant):
    """Option count_traversal: a counting frame of a qualifying scene is traced by the counting single-space kernels, so the counters describe
    the kernels that are timed.  Against single_space = 0: the same image and ray counts; the same instances_entered for every kind of ray —
    the two-level walk enters an instance exactly when it visits that instance's BLAS root, and the single-space walk counts the visits of
    a mesh's root; the same triangles tested by the closest-hit kinds (camera, extension: every triangle of a visited leaf is tested);
    and, where the graft is ONE node standing for the one TLAS node (2 meshes, 1 mesh), the same nodes visited.  In the Cornell box every
    ray starts inside the one mesh's box, so each kind visits the mesh's root once per ray.
    NOT compared: the triangles tested by the shadow rays — an any-hit ray stops at the first blocking triangle of a leaf, and the order of
    the packets inside a leaf is the device builder's (its partition passes place primitives with atomics), so that figure differs between
    two builds of one scene with the option off (53849 and 53785 were measured for the 2-mesh scene); nor the nodes visited on the
    65-mesh scene, whose graft has chain nodes where the TLAS has leaves of several instances."""
    scene, w, h, _ = make_scene(kind)
    view = scene.view(w, h)
    got = {}
    for ss in (1, 0):
        be = backend(w, h, ss, 3, VARIANTS[variant] + (("count_traversal", 1),))
        got[ss] = (image(be, scene, view, 1), be.frame_stats())
        assert be.scene_stats()["single_space"] == ss
        be.close()
    one, two = got[1][1], got[0][1]
    print({k: (one[k], two[k]) for k in ("nodes_visited", "tris_tested", "instances_entered")})
    assert np.array_equal(got[1][0], got[0][0])
    for key in ("primary_rays", "shadow_rays", "extension_rays", "instances_entered"):
        assert one[key] == two[key], key
    assert min(one["instances_entered"]) > 0
    assert list(one["tris_tested"])[:2] == list(two["tris_tested"])[:2]  # [camera, extension, shadow]
    if kind != "atrium65":
        assert one["nodes_visited"] == two["nodes_visited"]
    if kind == "cornell":
        assert list(one["instances_entered"]) == [one["primary_rays"], one["extension_rays"], one["shadow_rays"]]


def test_a_translated_instance_renders_through_the_two_level_path():
    scene, w, h, spheres = make_scene("atrium2")
    m = IDENTITY.copy()
    m[0, 3] = 0.75
    scene.set_instance_matrix(spheres[0], 0, m)
    view = scene.view(w, h)
    out = {}
    for ss in (1, 0):
        be = backend(w, h, ss, 3)
        out[ss] = image(be, scene, view)
        assert be.scene_stats()["single_space"] == 0
        be.close()
    assert np.array_equal(out[1], out[0])


def test_minus_zero_translation_does_not_qualify():
    """bit for bit the identity: a -0.0f anywhere in the matrix is another matrix."""
    scene, w, h, spheres = make_scene("atrium2")
    m = IDENTITY.copy()
    m[1, 3] = -0.0
    scene.set_instance_matrix(spheres[0], 0, m)
    be = backend(w, h, 1, 1)
    ref = backend(w, h, 0, 1)
    view = scene.view(w, h)
    a, b = image(be, scene, view), image(ref, scene, view)
    assert be.scene_stats()["single_space"] == 0
    assert np.array_equal(a, b)
    be.close(); ref.close()


def test_qualify_move_restore_over_frame_slots():
    """Four frame slots, each with its own TLAS and graft: the scene qualifies, one instance moves (two-level path from the next frame on), then
    returns (single space again).  Every frame equals the single_space = 0 frame of the same state."""
    scene, w, h, spheres = make_scene("atrium65")
    view = scene.view(w, h)
    be = backend(w, h, 1, 3, frames_in_flight=4)
    ref = backend(w, h, 0, 3, frames_in_flight=4)
    scene.sync(be); scene.mark_all_changed(); scene.sync(ref)
    moved = IDENTITY.copy()
    moved[1, 3] = 0.5
    states = [None, moved, IDENTITY, moved, moved, IDENTITY, IDENTITY, IDENTITY, moved, IDENTITY]  # more frames than slots: every slot sees both kinds
    for k, state in enumerate(states):
        if state is not None:
            for b in (be, ref):
                scene.set_instance_matrix(spheres[3], 0, state)
                scene.sync(b)
        be.render(view); ref.render(view)
        a, r = be.accumulator().view(np.uint32), ref.accumulator().view(np.uint32)
        assert np.array_equal(a, r), (k, int((a != r).sum()))
        assert be.scene_stats()["single_space"] == (0 if state is moved else 1) and ref.scene_stats()["single_space"] == 0, k
    be.close(); ref.close()


@pytest.mark.parametrize("rows", [0, 2, 6])
def test_reduced_stack_agrees_or_flags_identically(rows):
    """Option spill_rows (the stack-spill test option) on the 65-mesh scene: with fewer HBM rows behind the LDS stack both walks either finish
    with the same image or both report the overflow."""
    from rfw_rs_amd.backend import BackendError
    scene, w, h, _ = make_scene("atrium65")
    view = scene.view(w, h)
    res = {}
    for ss in (1, 0):
        be = backend(w, h, ss, 3, (("spill_rows", rows),))
        try:
            res[ss] = image(be, scene, view, 1)
        except BackendError as e:
            assert "overflow" in str(e)
            res[ss] = None
        be.close()
    assert (res[1] is None) == (res[0] is None), rows
    if res[1] is not None:
        assert np.array_equal(res[1], res[0])


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_axis_parallel_and_minus_zero_directions(axis):
    """A camera looking down an axis at an odd resolution: the centre ray is exactly axis-parallel, its neighbours have components of either
    sign around zero (and -0.0 where a product with a zero component is negative)."""
    scene, w, h, _ = make_scene("atrium2")
    w, h = 65, 33
    d = [0.0, 0.0, 0.0]
    d[axis] = -1.0 if axis == 1 else 1.0
    scene.set_camera([0.0, 6.0, 0.0], d, fov=60.0, aspect=w / h)
    view = scene.view(w, h)
    out = {}
    for ss in (1, 0):
        be = backend(w, h, ss, 3)
        out[ss] = image(be, scene, view)
        assert be.scene_stats()["single_space"] == ss
        be.close()
    assert np.array_equal(out[1], out[0])
