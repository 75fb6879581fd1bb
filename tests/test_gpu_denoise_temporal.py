"""Options "sample_offset" and "denoise_temporal" (include/rfw_hip.h, DESIGN.md "Denoiser: temporal"): the first sample index of an image, and the
previous image's filtered input reprojected into this one (csrc/denoise.inc, k_dn_temporal).

Both are off by default and then change no bit.  The sample offset is held against the oracle at that sample index, the blend against a float64
numpy restatement of its formula fed with the device's own previous history, guides, view and accumulator.  Small frames, so that
tests/test_denoise_temporal_on_cpu.py can run the file on the emulated library too.

test_the_formula_restated: x is held to 1e-4 * max(1, |want|), h to 1e-4.  Largest figures measured over the cases of that test on the
emulated library (the same float32 operations, without contraction, as the device build): |x - want| / max(1, |want|) = 7.7e-5,
|h - want| = 3.8e-5; at most one pixel's weight sum lay within 1e-4 of the threshold; the fewest pixels with a valid history in any frame of
the four-view sequences after the first were 97.9 %."""
import functools

import numpy as np
import pytest

from rfw_rs_amd import BackendError, HipBackend, Scene, pod
from conftest import rel_l2
from test_gpu_denoise import ALBEDO_FLOOR, DEFAULT_COLOUR, K_PLANE, NORMAL_POWER, atrous_restated, attach, bits, cornell_70x37, render

pytestmark = pytest.mark.gpu
W = H = 64
MIN_WEIGHT = 0.25  # csrc/denoise.inc: kDnTemporalMinWeight


def vec(v):
    return np.array([v.x, v.y, v.z], np.float64)


def moved(view, shift=0.0, turn=0.0):
    """the view of the same camera `shift` image-plane distances to its right, turned by `turn` radians about its up axis"""
    v = pod.CameraView3D.from_buffer_copy(bytes(view))
    pos, p1, right, up, direction = vec(v.pos), vec(v.p1), vec(v.right), vec(v.up), vec(v.direction)
    distance = np.linalg.norm(p1 + 0.5 * right + 0.5 * up - pos)
    axis = up / np.linalg.norm(up)
    c, s = np.cos(turn), np.sin(turn)
    rot = lambda a: a * c + np.cross(axis, a) * s + axis * (axis @ a) * (1.0 - c)
    delta = shift * distance * right / np.linalg.norm(right)
    corner = rot(p1 - pos)
    for name, value in (("pos", pos + delta), ("p1", pos + delta + corner), ("right", rot(right)), ("up", up), ("direction", rot(direction))):
        setattr(v, name, pod.Vec3(*value.astype(np.float32)))
    return v


def sequence(view, count, shift=0.02, turn=0.0):
    return [moved(view, shift * i, turn * i) for i in range(count)]


def oracle_at(scene, w, h, view, first, count=1):
    """the accumulator of a fresh oracle after `count` samples of `view` with indices first, first + 1, ..."""
    from oracle.bindings import Oracle
    orc = Oracle(w, h)
    scene.mark_all_changed()
    scene.sync(orc)
    if first:
        orc.set_option("sample_count", first)
    for _ in range(count):
        orc.render(view)
    return orc.accumulator().copy()


def temporal(scene, w=W, h=H, passes=1, hmax=8, **options):
    be = attach(scene, w, h, denoise=passes, **options)
    be.set_option("denoise_temporal", hmax)
    return be


# ---------------------------------------------------------------- 1. off is untouched
def test_off_is_untouched():
    scene = Scene().build("cornell")
    view = scene.view(W, H)
    fresh = render(attach(scene), view, 2)
    acc, fb = fresh.accumulator(), fresh.framebuffer()
    same = lambda b: np.array_equal(bits(b.accumulator()), bits(acc)) and np.array_equal(bits(b.framebuffer()), bits(fb))
    be = attach(scene)
    assert same(render(be, view, 2))
    for key, value in (("sample_offset", 5), ("denoise_temporal", 8)):
        be.set_option(key, value)  # denoise_temporal without denoise: nothing
        render(be, view, 2)
        assert same(be) == (key == "denoise_temporal"), key
        be.set_option(key, 0)
        assert same(render(be, view, 2)), key
    be.set_option("denoise", 2)
    be.set_option("denoise_temporal", 8)
    for _ in range(3):  # three images with a history
        be.reset_accumulation()
        be.render(view)
    be.set_option("denoise_temporal", 0)
    be.set_option("denoise", 0)
    assert same(render(be, view, 2)), "on and off again: a fresh instance's bits"
    # denoise without the temporal option is what it was, whatever happened before
    plain = render(attach(scene, denoise=2), view, 2)
    be.set_option("denoise", 2)
    render(be, view, 2)
    assert np.array_equal(bits(be.framebuffer()), bits(plain.framebuffer())) and np.array_equal(bits(be.accumulator()), bits(acc))
    for key, value in (("sample_offset", -1), ("sample_offset", 2 ** 24 + 1), ("sample_offset", 1.5), ("sample_offset", float("nan")),
                       ("denoise_temporal", 65), ("denoise_temporal", -1), ("denoise_temporal", 2.5)):
        with pytest.raises(BackendError):
            be.set_option(key, value)
    be.set_option("sample_offset", 2 ** 24)  # the largest
    for b in (be, fresh, plain):
        b.close()


# ---------------------------------------------------------------- 2. sample_offset against the oracle
@pytest.mark.parametrize("s", [1, 7, 300])
def test_sample_offset_against_the_oracle(s):
    scene = Scene().build("cornell")
    view = scene.view(W, H)
    one, three = oracle_at(scene, W, H, view, s), oracle_at(scene, W, H, view, s, 3)
    singles = [one] + [oracle_at(scene, W, H, view, s + i) for i in (1, 2)]
    in_order = (singles[0] + singles[1]) + singles[2]
    print(f"sample_offset {s}: the oracle's own accumulation against the sum of three fresh oracles: rel-L2 {rel_l2(three, in_order):.3e}")
    assert rel_l2(three, in_order) <= 1e-6
    for options in ({}, {"streams": 2, "tile_size": 16}):
        be = attach(scene, **options)
        be.render(view)  # an image at index 0 first: the next one must not keep any of it
        be.set_option("sample_offset", s)
        be.render(view)
        assert be.frame_stats()["sample_count"] == 1
        assert np.array_equal(bits(be.accumulator()), bits(one)), options
        assert np.array_equal(bits(be.framebuffer()), bits(np.sqrt(one))), "the divisor is the sample COUNT"
        render(be, view, 2)
        assert be.frame_stats()["sample_count"] == 3
        assert np.array_equal(bits(be.accumulator()), bits(three)), options
        be.reset_accumulation()  # a new image starts at the offset again
        be.render(view)
        assert np.array_equal(bits(be.accumulator()), bits(one)), options
        be.close()
    be = attach(scene, max_batch=4)
    be.render_samples(view, 2)
    be.set_option("sample_offset", s)
    be.render_samples(view, 3)
    assert be.frame_stats()["sample_count"] == 3
    print(f"sample_offset {s}: render_samples against the oracle: rel-L2 {rel_l2(be.accumulator(), three):.3e}")
    assert rel_l2(be.accumulator(), three) <= 1e-6
    assert np.array_equal(bits(be.accumulator()), bits(in_order)), "the sum of the per-sample images in sample order"
    be.render(view)  # index s + 3, onto the same image
    assert rel_l2(be.accumulator(), oracle_at(scene, W, H, view, s, 4)) <= 1e-6
    # a batch of frames keeps index 0
    be.render_batch([view, view])
    zero = oracle_at(scene, W, H, view, 0)
    assert np.array_equal(bits(be.accumulator_at(0)), bits(zero)) and np.array_equal(bits(be.accumulator_at(1)), bits(zero))
    be.close()


def test_the_render_modes_honour_the_sample_offset():
    """Modes 5 and 6 seed their rays from the same field; modes 1-4 draw nothing but the pixel jitter."""
    scene = Scene().build("cornell")
    view = scene.view(W, H)
    be = attach(scene)
    for mode in range(1, 7):
        be.set_option("sample_offset", 0)
        be.render(view, mode=mode)
        at0 = be.accumulator()
        assert be.frame_stats()["sample_count"] == 1
        be.set_option("sample_offset", 9)
        be.render(view, mode=mode)
        assert be.frame_stats()["sample_count"] == 1
        assert not np.array_equal(bits(be.accumulator()), bits(at0)), mode
        at9 = be.accumulator()
        be.reset_accumulation()
        be.render(view, mode=mode)
        assert np.array_equal(bits(be.accumulator()), bits(at9)), mode
    be.close()


def test_the_automatic_advance():
    scene = Scene().build("cornell")
    view = scene.view(W, H)
    be = temporal(scene)
    for base in (0, 5):
        be.set_option("sample_offset", base)
        be.set_option("denoise_temporal", 4 if base else 8)  # (a different value: the history is dropped)
        for i in range(4):
            be.reset_accumulation()
            be.render(view)
            assert np.array_equal(bits(be.accumulator()), bits(oracle_at(scene, W, H, view, base + i))), (base, i)
    be.render(view)  # a second sample of image 3
    assert be.frame_stats()["sample_count"] == 2
    assert np.array_equal(bits(be.accumulator()), bits(oracle_at(scene, W, H, view, 5 + 3, 2)))
    be.close()


# ---------------------------------------------------------------- 3. the formula, restated in float64
def demodulated(acc, n, guide):
    """c as dn_load<true> forms it, in float32"""
    return (acc[..., :3] * np.float32(1.0) / np.float32(n)) / np.maximum(guide[2][..., :3], np.float32(ALBEDO_FLOOR))


def temporal_restated(acc, n, guide, prev, hmax):
    """DESIGN.md "Denoiser: temporal" in float64.  prev = None or (history plane, g0, g1, view) of the previous image.
    Returns x, h (0 where f = 0), the weight sum sw, f and whether the reprojected pixel has a tap inside the previous frame."""
    g0, g1, g2 = (g.astype(np.float64) for g in guide)
    f = g2[..., 3] > 0.0
    h_, w_ = f.shape
    c = acc[..., :3].astype(np.float64) / n / np.maximum(g2[..., :3], ALBEDO_FLOOR)
    x, hh, sw, inside_any = c.copy(), np.zeros(f.shape), np.zeros(f.shape), np.zeros(f.shape, bool)
    if prev is not None:
        xp, g0p, g1p, view = prev
        xp, g0p, g1p = xp.astype(np.float64), g0p.astype(np.float64), g1p.astype(np.float64)
        pos, p1, right, up = vec(view.pos), vec(view.p1), vec(view.right), vec(view.up)
        N, t, P = g0[..., :3], np.where(f, g0[..., 3], 1.0), g1[..., :3]
        d = P - pos
        nrm = np.cross(right, up)
        num, den = nrm @ (p1 - pos), d @ nrm
        front = f & (num * den > 0.0)
        q = pos + (num / np.where(front, den, 1.0))[..., None] * d - p1
        fx, fy = (q @ right) / (right @ right) * w_ - 0.5, (q @ up) / (up @ up) * h_ - 0.5
        i0, j0 = np.floor(fx), np.floor(fy)
        tx, ty = fx - i0, fy - j0
        sx, sh = np.zeros(x.shape), np.zeros(f.shape)
        for b in (0, 1):
            for a in (0, 1):
                qx, qy = i0 + a, j0 + b
                inside = front & (qx >= 0) & (qx < w_) & (qy >= 0) & (qy < h_)
                inside_any |= inside
                xi, yi = np.clip(qx, 0, w_ - 1).astype(int), np.clip(qy, 0, h_ - 1).astype(int)
                xq = xp[yi, xi]
                wn = np.maximum(0.0, (N * g0p[yi, xi, :3]).sum(-1)) ** NORMAL_POWER
                wp = np.maximum(0.0, 1.0 - np.abs((N * (g1p[yi, xi, :3] - P)).sum(-1)) / (K_PLANE * t))
                w = np.where(inside & (xq[..., 3] > 0.0), (tx if a else 1.0 - tx) * (ty if b else 1.0 - ty) * wn * wp, 0.0)
                sw += w
                sx += w[..., None] * xq[..., :3]
                sh += w * xq[..., 3]
        safe = np.where(sw > 0.0, sw, 1.0)
        hh = np.where(sw >= MIN_WEIGHT, np.minimum(sh / safe, max(hmax - n, 0)), 0.0)
        xh = sx / safe[..., None]
        x = np.where((hh > 0.0)[..., None], xh + (n / (hh + n))[..., None] * (c - xh), c)
    h = hh + n
    return np.where(f[..., None], x, 0.0), np.where(f, h, 0.0), sw, f, inside_any


# name: (scene, width, height, shift per image, turn per image)
FORMULA_CASES = {"cornell_sideways": (lambda: Scene().build("cornell"), W, H, 0.02, 0.0),
                 "cornell_turning": (lambda: Scene().build("cornell"), W, H, 0.02, -0.015),
                 "gallery_sideways": (lambda: Scene().build("gallery"), W, H, 0.02, 0.0),
                 "gallery_turning": (lambda: Scene().build("gallery"), W, H, 0.02, -0.015),
                 "cornell_70x37_turning": (cornell_70x37, 70, 37, 0.02, -0.015)}


@pytest.mark.parametrize("name", sorted(FORMULA_CASES))
def test_the_formula_restated(name):
    """Four views of a camera moving sideways (and turning), one sample each — the third image gets a second sample, which rewrites its
    history from the same previous one.  These move the image by less than a pixel, so a fifth view jumps a quarter of the image-plane
    distance to the side: there pixels leave the previous frame (and fewer than 90 % need keep a history).  Figures: the module's docstring."""
    build, w, h, shift, turn = FORMULA_CASES[name]
    scene = build()
    views = sequence(scene.view(w, h), 4, shift, turn) + [moved(scene.view(w, h), 3 * shift + 0.25, 3 * turn)]
    passes, hmax = 2, 8
    be, plain = temporal(scene, w, h, passes, hmax), attach(scene, w, h, denoise=passes)
    last, worst_x, worst_h, left_out, fewest_valid, no_history, outside = {}, 0.0, 0.0, 0, 1.0, 0, 0
    for i, n in ((0, 1), (1, 1), (2, 1), (2, 2), (3, 1), (4, 1)):
        be.render(views[i])
        assert be.frame_stats()["sample_count"] == n
        acc, fb, guide, hist = be.accumulator(), be.framebuffer(), be.denoise_guide(), be.denoise_history()
        prev = last.get(i - 1)  # (the second sample of image 2 starts from image 1's history again)
        want_x, want_h, sw, f, inside = temporal_restated(acc, n, guide, prev, hmax)
        c = demodulated(acc, n, guide)
        assert f.sum() > w * h // 4 and not np.any(np.isnan(hist))
        assert np.all(hist[~f] == 0.0)
        if i == 0:  # the first frame after a drop is plain denoise at the same sample offset
            plain.render(views[0])
            assert np.array_equal(bits(acc), bits(plain.accumulator())) and np.array_equal(bits(fb), bits(plain.framebuffer()))
            assert np.all(hist[f][:, 3] == n) and np.array_equal(bits(hist[f][:, :3]), bits(c[f]))
        else:
            near = f & (np.abs(sw - MIN_WEIGHT) <= 1e-4)  # a threshold decision float32 may take the other way
            left_out = max(left_out, int(near.sum()))
            assert near.sum() <= 0.005 * f.sum()
            m = f & ~near
            dev_x = np.abs(hist[..., :3] - want_x) / np.maximum(1.0, np.abs(want_x))
            dev_h = np.abs(hist[..., 3] - want_h)
            worst_x, worst_h = max(worst_x, float(dev_x[m].max())), max(worst_h, float(dev_h[m].max()))
            valid = f & (hist[..., 3] > n)
            print(f"temporal formula {name} image {i} n={n}: x {dev_x[m].max():.3e}, h {dev_h[m].max():.3e}, near the threshold {near.sum()}, "
                  f"valid {valid.sum() / f.sum():.3f}, mean h {hist[..., 3][valid].mean():.2f}")
            assert np.all(dev_x[m] <= 1e-4), (name, i, n, float(dev_x[m].max()))
            assert np.all(dev_h[m] <= 1e-4), (name, i, n, float(dev_h[m].max()))
            if i < 4:
                fewest_valid = min(fewest_valid, valid.sum() / f.sum())
                assert valid.sum() >= 0.9 * f.sum(), (name, i, valid.sum() / f.sum())
            # no history: reprojected outside the previous frame, or onto another surface (a wall at right angles, a disocclusion)
            none = f & (sw < MIN_WEIGHT - 1e-4)
            assert np.all(hist[none][:, 3] == n) and np.array_equal(bits(hist[none][:, :3]), bits(c[none])), "h = n and x = c, bit for bit"
            outside += int((f & ~inside).sum())
            no_history += int((f & inside & (sw == 0.0)).sum())
        # then the frame: the a-trous passes from the device's own x
        x = hist[..., :3].astype(np.float64)
        a = np.maximum(guide[2][..., :3].astype(np.float64), ALBEDO_FLOOR)
        want, _ = atrous_restated(x * a * n, n, guide, passes, DEFAULT_COLOUR)
        dev = np.abs(fb[..., :3] - want) / np.maximum(1.0, np.abs(want))
        assert np.all(dev[f] <= 1e-5), (name, i, n, float(dev[f].max()))
        last[i] = (hist, guide[0], guide[1], views[i])
    print(f"temporal formula {name}: worst x {worst_x:.3e}, worst h {worst_h:.3e}, left out at most {left_out}, fewest valid {fewest_valid:.3f}, "
          f"pixels outside the previous frame {outside}, inside it without any weight {no_history}")
    if w == h:  # (the wide frame sees past the box on both sides: what leaves it there is not filtered)
        assert outside > 0, "a pixel reprojected outside the previous frame is among the cases"
    if name.startswith("cornell"):
        assert no_history > 0, "a pixel reprojected onto another surface is among the cases"
    be.close()
    plain.close()


# ---------------------------------------------------------------- 4. it accumulates
@functools.lru_cache(maxsize=None)
def reference(kind):
    """(scene, view, raw frame of 256 samples)"""
    scene = Scene().build(kind)
    view = scene.view(W, H)
    raw = render(attach(scene), view, 256)
    ref = raw.framebuffer()[..., :3].copy()
    raw.close()
    return scene, view, ref


@pytest.mark.parametrize("kind", ["cornell", "gallery"])
def test_it_accumulates(kind):
    """e(img) = rel-L2 against the raw frame of 256 samples over the filtered pixels.  Static view: 8 images of one sample (reset in between),
    denoise 3, Hmax 16.  Moving camera (2 % of the image-plane distance per image, arriving at the same view): 16 images, denoise 1.  The
    spatial-only frame is the last image's, at the same sample index.  Moving with denoise 3 is printed only (DESIGN.md "Denoiser: temporal" quotes all ratios)."""
    for images, passes, shift, asserted in ((8, 3, 0.0, True), (16, 1, 0.02, True), (16, 3, 0.02, False)):
        scene, view, ref = reference(kind)
        views = [moved(view, shift * (i - (images - 1))) for i in range(images)]
        be = temporal(scene, passes=passes, hmax=16)
        for v in views:
            be.reset_accumulation()
            be.render(v)
        fb, hist = be.framebuffer()[..., :3], be.denoise_history()
        f = be.denoise_guide()[2][..., 3] > 0.0
        spatial = attach(scene, denoise=passes)
        spatial.set_option("sample_offset", images - 1)
        spatial.render(views[-1])
        assert np.array_equal(bits(spatial.accumulator()), bits(be.accumulator())), "the same sample"
        e = lambda img: rel_l2(img[f], ref[f])
        e_t, e_s = e(fb), e(spatial.framebuffer()[..., :3])
        valid = f & (hist[..., 3] > 1.0)
        print(f"temporal {kind} {'static' if shift == 0.0 else 'moving'} k={passes} {images} images: e(spatial) = {e_s:.4f}, e(temporal) = {e_t:.4f}, "
              f"ratio {e_t / e_s:.3f}, valid {valid.sum() / f.sum():.3f}, mean h {hist[..., 3][valid].mean():.2f}")
        if asserted:
            assert e_t < e_s, (kind, shift, passes, e_t, e_s)
        if shift == 0.0:
            assert hist[..., 3][valid].mean() > 7.0
        be.close()
        spatial.close()


# ---------------------------------------------------------------- 5. everywhere mode 0 runs
def test_frame_slots_and_sub_streams_give_the_same_bits():
    scene = Scene().build("cornell")
    views = sequence(scene.view(W, H), 4, 0.02, 0.015)
    plain = temporal(scene, passes=3, tile_size=16)
    want = []
    for v in views:
        plain.render(v)
        want.append((plain.framebuffer(), plain.denoise_history(), np.stack(plain.denoise_guide())))
    plain.close()
    for options in ({"frames_in_flight": 3}, {"streams": 2}, {"frames_in_flight": 3, "streams": 2}):
        be = temporal(scene, passes=3, tile_size=16, **options)
        for v, (fb, hist, guide) in zip(views, want):
            be.render(v)
            assert np.array_equal(bits(be.framebuffer()), bits(fb)), options
            assert np.array_equal(bits(be.denoise_history()), bits(hist)), options
            assert np.array_equal(bits(np.stack(be.denoise_guide())), bits(guide)), options
        be.close()
        # and without a read between the frames: the slots' filter stages are ordered on the device
        be = temporal(scene, passes=3, tile_size=16, **options)
        for v in views:
            be.render(v)
        assert np.array_equal(bits(be.framebuffer()), bits(want[-1][0])) and np.array_equal(bits(be.denoise_history()), bits(want[-1][1])), options
        be.close()


def test_render_samples_and_the_presented_frame():
    scene = Scene().build("cornell")
    views = sequence(scene.view(W, H), 2)
    one, seq = temporal(scene, passes=3, max_batch=4), temporal(scene, passes=3)
    one.render(views[0])
    seq.render(views[0])
    one.render_samples(views[1], 3)
    render(seq, views[1], 3)
    assert one.frame_stats()["sample_count"] == 3
    assert rel_l2(one.accumulator(), seq.accumulator()) <= 1e-6
    assert np.array_equal(bits(np.stack(one.denoise_guide())), bits(np.stack(seq.denoise_guide()))), "the guide is the LAST sample's"
    fb = one.framebuffer()
    print(f"temporal render_samples: rel-L2 of the histories {rel_l2(one.denoise_history(), seq.denoise_history()):.3e}, of the frames {rel_l2(fb, seq.framebuffer()):.3e}")
    assert rel_l2(one.denoise_history(), seq.denoise_history()) <= 1e-6
    assert rel_l2(fb, seq.framebuffer()) <= 1e-6
    assert (one.denoise_history()[..., 3] > 3.0).any(), "there is a history behind the three samples"
    # the presented BGRA8 image is the sRGB encoding of the float frame
    steps = one.srgb_steps()
    pres = one.host_frame(presented=True)
    one.download_frame(pres)
    one.wait_downloads()
    enc = lambda x: np.searchsorted(steps, x, side="right").astype(np.uint8)
    want = np.stack([enc(fb[..., 2]), enc(fb[..., 1]), enc(fb[..., 0]), np.full(fb.shape[:2], 255, np.uint8)], axis=-1)
    assert np.array_equal(pres.reshape(want.shape), want)
    one.close()
    seq.close()


def test_the_other_modes_leave_the_history_and_resize_drops_it():
    scene = Scene().build("cornell")
    views = sequence(scene.view(W, H), 3)
    be, other = temporal(scene, passes=2), temporal(scene, passes=2)
    for b in (be, other):
        b.render(views[0])
        b.render(views[1])
    hist = be.denoise_history()
    assert (hist[..., 3] > 1.0).any()
    for mode in range(1, 7):
        be.render(views[1], mode=mode)
        assert np.array_equal(bits(be.denoise_history()), bits(hist)), mode
    be.render(views[2])
    other.render(views[2])
    assert np.array_equal(bits(be.accumulator()), bits(other.accumulator())), "the modes' frames are no images of the sequence"
    assert np.array_equal(bits(be.framebuffer()), bits(other.framebuffer())) and np.array_equal(bits(be.denoise_history()), bits(other.denoise_history()))
    # a change of the pass count or of the colour width keeps the history; a resize drops it
    be.set_option("denoise", 3)
    be.set_option("denoise_colour", 16.0)
    be.render(views[1])
    assert (be.denoise_history()[..., 3] > 1.0).any()
    be.resize((W, H))
    be.render(views[0])
    f = be.denoise_guide()[2][..., 3] > 0.0
    assert np.all(be.denoise_history()[..., 3] == f), "h = n = 1 on every filtered pixel"
    first = attach(scene, denoise=3, colour=16.0)
    first.render(views[0])
    assert np.array_equal(bits(be.accumulator()), bits(first.accumulator())) and np.array_equal(bits(be.framebuffer()), bits(first.framebuffer()))
    for b in (be, other, first):
        b.close()
