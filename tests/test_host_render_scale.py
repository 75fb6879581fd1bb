"""The render scale in the host mirror (rfw-rs_amd/host): rfw::render_system asks the camera for its view at the backend's RENDER size, as
rfw does (rfw/src/system/mod.rs:217-223: render_width() = (width * scale_factor) as u32), the 2D camera keeps the window size, and
`example_animated --scale S` drives a scaled backend through the frame loop."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rfw_rs_amd import Scene


def raw(view):
    return bytes(C.string_at(C.addressof(view), C.sizeof(view)))


@pytest.mark.parametrize("w,h,scale", [(64, 64, 0.5), (70, 37, 0.61), (40, 24, 1.5), (3, 2, 0.4), (64, 64, 1.0)])
def test_render_system_hands_over_the_view_of_the_render_size(w, h, scale):
    scene = Scene().build("cornell")
    scene.set_aspect(w / h)
    rw, rh = max(1, int(w * scale)), max(1, int(h * scale))
    want = scene.view(rw, rh)
    got = scene.render_system(w, h, scale)
    assert got.spread_angle == want.spread_angle and raw(got) == raw(want)
    if rh != h:  # the spread angle follows the pixels that are traced, not the window's
        assert got.spread_angle != scene.view(w, h).spread_angle
    got, view_2d = scene.render_system(w, h, scale, with_2d=True)
    assert raw(got) == raw(want)
    assert np.array_equal(view_2d, Scene.camera_2d_view(w, h))  # Camera2D keeps the window size
    if (rw, rh) != (w, h):
        assert not np.array_equal(view_2d, Scene.camera_2d_view(rw, rh))


@pytest.mark.gpu
def test_example_animated_with_a_scale(tmp_path):
    exe = os.path.join(ROOT, "rfw-rs_amd", "host", "example_animated")
    assert os.path.exists(exe), "run __graft_entry__.build() (make -C rfw-rs_amd/host example_animated)"
    glb = Scene().build("atrium", 30000, 0, 0.0, 3).save_glb(str(tmp_path / "atrium.glb"))
    out = tmp_path / "last.ppm"
    r = subprocess.run([exe, "--gltf", glb, "--frames", "12", "--size", "320x200", "--scale", "0.5", "--spheres", "10x10", "--hud", "--out", str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "window 320x200, scale 0.5: traced at 160x100" in r.stdout and "12 frames of 320x200" in r.stdout
    raw_ppm = out.read_bytes()
    head = b"P6\n320 200\n255\n"  # presented at the window size
    assert raw_ppm.startswith(head) and len(raw_ppm) == len(head) + 320 * 200 * 3
    img = np.frombuffer(raw_ppm[len(head):], np.uint8).reshape(200, 320, 3)
    assert img.mean() > 8 and img.std() > 8  # a lit, structured image
    bad = subprocess.run([exe, "--gltf", glb, "--frames", "1", "--size", "320x200", "--scale", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert bad.returncode == 1 and "scale" in bad.stderr
