"""`example_animated --hud` (rfw-rs_amd/host/example_animated.cpp): the frame counter and the frame time drawn over the image with the
plumbing rfw-font uses — an atlas texture, one 2D mesh of glyph quads rewritten every frame, one 2D instance with the pixel-space matrix, the
frame's Camera2D view.  The text is read back from the presented frame against the font's own bitmaps; without the flag the program's
output is what it was."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rfw_rs_amd import Scene
from rfw_rs_amd.scene import host_lib

pytestmark = pytest.mark.gpu
def glyph(c):
    """the 8 x 8 bits of a character of the HUD font, None if the font lacks it"""
    rows = (C.c_uint8 * 8)()
    if host_lib().rfwhost_hud_glyph(c.encode(), rows) != 0:
        return None
    return np.array([[(r >> (7 - x)) & 1 for x in range(8)] for r in rows], bool)


CHARS = [chr(k) for k in range(32, 127) if glyph(chr(k)) is not None]  # the font's own list


def read_ppm(path):
    raw = open(path, "rb").read()
    m = re.match(rb"P6\n(\d+) (\d+)\n255\n", raw)
    w, h = int(m.group(1)), int(m.group(2))
    return np.frombuffer(raw[m.end():], np.uint8).reshape(h, w, 3)


def read_line(img, plain, y0):
    """the text of the 8-pixel line at row y0: every cell's white pixels must be exactly one glyph of the font; the others keep `plain`"""
    assert set("0123456789.: frames") <= set(CHARS)
    text = ""
    for k in range(img.shape[1] // 8):
        cell, back = img[y0:y0 + 8, 8 * k:8 * k + 8], plain[y0:y0 + 8, 8 * k:8 * k + 8]
        white = np.all(cell == 255, axis=2) & ~np.all(back == 255, axis=2)
        assert np.array_equal(cell[~white], back[~white]), (k, "a pixel outside the glyph changed")
        match = [c for c in CHARS if np.array_equal(glyph(c) & ~np.all(back == 255, axis=2), white)]
        assert match, (y0, k, white.astype(int))
        text += match[0]
    return text


def test_example_animated_hud(tmp_path):
    exe = os.path.join(ROOT, "rfw-rs_amd", "host", "example_animated")
    assert os.path.exists(exe), "run __graft_entry__.build() (make -C rfw-rs_amd/host example_animated)"
    glb = Scene().build("atrium", 20000, 0, 0.0, 3).save_glb(str(tmp_path / "atrium.glb"))
    outs = []
    for flags in ([], ["--hud"], []):
        out = tmp_path / f"frame{len(outs)}.ppm"
        r = subprocess.run([exe, "--gltf", glb, "--frames", "8", "--size", "64x64", "--spheres", "6x6", "--out", str(out)] + flags,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "8 frames of 64x64" in r.stdout
        outs.append(read_ppm(out))
    plain, hud, again = outs
    assert np.array_equal(plain, again), "without the flag the program's output is what it was, run after run"
    assert np.array_equal(hud[18:], plain[18:]) and np.array_equal(hud[0], plain[0]) and np.array_equal(hud[9], plain[9]), "outside the two lines of text nothing changed"
    assert read_line(hud, plain, 1) == "frame 7 "
    assert re.fullmatch(r"\d+\.\d\d ms *", read_line(hud, plain, 10)), read_line(hud, plain, 10)
