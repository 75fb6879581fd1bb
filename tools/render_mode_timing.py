#!/usr/bin/env python3
"""Frame times of render() per mode (include/rfw_hip.h RFW_HIP_RENDER_*) on the bench scene: python3 tools/render_mode_timing.py [--modes 0,5,6]

One instance, one frame at a time: every repeat renders `--frames` frames of the same view and then reads the framebuffer back (the wait),
after `--warmup` frames.  Prints one line per mode with the median, min and max of the repeats' ms per frame.  DESIGN.md "Render modes"
quotes its output.

--denoise 0,1,3,5 times mode 0 under option "denoise" instead (DESIGN.md "Denoiser"): the settings take turns, repeat by repeat, so that
they share whatever else the machine is doing; --denoise-form 1 / 2 forces the direct / tiled kernel form; --bandwidth adds what
rfw_hip_bandwidth_probe reads per second, the yardstick of a pass's 64 algorithmic bytes per pixel.  --denoise-temporal H times every
non-zero setting k a second time with option "denoise_temporal" = H (DESIGN.md "Denoiser: temporal"), in the same turns; every frame of a
timed repeat then starts a new image (reset_accumulation), for both, since that is where the history acts.  --denoise-motion 0,1 times
every temporal setting once per listed value of option "denoise_motion" (DESIGN.md "Denoiser: motion"; 0 never names the option, so that
a library without it can be timed through RFW_HIP_LIB), in the same turns.  --denoise-deform 0,1 does the same for option "denoise_deform"
(DESIGN.md "Denoiser: deforming meshes"; it needs --denoise-motion with a 1, and acts on the settings whose motion is 1); --scene skinned
takes the skinned tubes in their room in place of the atrium, and then every frame of a timed repeat takes a new pose (a synchronize() per
frame, in every setting alike), since that is where the option acts.  With --bandwidth the option's byte floor is printed next to the probe:
40 B per slab slot for the triangle plane, 128 B per triangle of a skinned copy for k_dn_pose, and 8 B plus up to 64 B of snapshot per
pixel of a deforming instance for k_dn_temporal_deform (triangles and pixels as the taps of the latest frame count them).

--overlay a,b,c times mode 0 with the 2D layer (DESIGN.md "2D layer"), the settings taking turns: a = a view_2d and no 2D data (the only
setting a library from before the layer can run: RFW_HIP_LIB), b = a HUD of 2000 textured glyph quads of 12 x 16 pixels (4000 triangles),
c = the same over one translucent panel of half the frame.  With --bandwidth it prints the layer's floor next to the probe: 32 bytes per
touched pixel, the records (160 + 48 bytes written, 160 read per primitive) and the bin words written once (primitives and words as
rfw_hip_debug_read "ov_stats" counts them).  The three kernels' own times are not gathered here: the layer runs inside the frame's existing
time slot (no new event pair: rfw_hip_frame_stats keeps its layout), so they are read from a kernel trace of this tool's run,
`rocprofv3 --kernel-trace --stats -- python3 tools/render_mode_timing.py --overlay b,c --repeats 1 --frames 20` (DESIGN.md "2D layer")."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="0,5,6")
    ap.add_argument("--denoise", default="")
    ap.add_argument("--denoise-form", type=int, default=0)
    ap.add_argument("--denoise-temporal", type=int, default=0)
    ap.add_argument("--denoise-motion", default="")
    ap.add_argument("--denoise-deform", default="")
    ap.add_argument("--scene", default="atrium", choices=("atrium", "skinned"))
    ap.add_argument("--overlay", default="")
    ap.add_argument("--max-path-length", type=int, default=None)  # 1 for the modes (DESIGN.md "Render modes"), 3 with --denoise or --overlay
    ap.add_argument("--bandwidth", action="store_true")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--triangles", type=int, default=1048576)  # bench.py's atrium1m
    ap.add_argument("--ao-samples", type=int, default=4)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if a.max_path_length is None:
        a.max_path_length = 3 if a.denoise or a.overlay else 1
    import torch  # (the order bench.py has: torch's HIP runtime first)
    torch.cuda.init()
    from rfw_rs_amd import HipBackend, RenderMode, Scene
    scene = Scene().build("atrium", a.triangles, 0, 0.0, 0xC0FFEE) if a.scene == "atrium" else Scene().build("skinned")
    scene.set_aspect(a.width / a.height)
    view = scene.view(a.width, a.height)
    be = HipBackend.init(a.width, a.height, 1.0, max_path_length=a.max_path_length)
    scene.sync(be)
    what = f"{a.repeats} x {a.frames} frames, {a.width}x{a.height}, " + (f"atrium of {a.triangles} triangles" if a.scene == "atrium" else "the skinned scene, a pose per frame") + f", max path length {a.max_path_length}"
    if a.denoise:
        passes = [int(k) for k in a.denoise.split(",")]
        motions = [int(m) for m in a.denoise_motion.split(",")] if a.denoise_motion else [0]
        if any(motions) and not a.denoise_temporal:
            ap.error("--denoise-motion needs --denoise-temporal")
        deforms = [int(d) for d in a.denoise_deform.split(",")] if a.denoise_deform else [0]
        if any(deforms) and not any(motions):
            ap.error("--denoise-deform needs --denoise-motion with a 1")
        settings = [(k, 0, 0, 0) for k in passes] + [(k, a.denoise_temporal, m, d) for k in passes if k and a.denoise_temporal for m in motions for d in (deforms if m else [0])]
        posed = 0
        if any(passes):
            be.set_option("denoise_form", a.denoise_form)
        runs = {s: [] for s in settings}
        for rep in range(-1, a.repeats):  # (-1: the warm-up round of every setting)
            for k, hmax, motion, deform in settings:
                if any(passes):  # (all zero: never name the option, so that a library without it can be timed too)
                    be.set_option("denoise", k)
                if a.denoise_temporal:
                    be.set_option("denoise_temporal", hmax)
                if any(motions):
                    be.set_option("denoise_motion", motion)
                if any(deforms):
                    be.set_option("denoise_deform", deform)
                t0 = time.perf_counter()
                for _ in range(a.warmup if rep < 0 else a.frames):
                    if a.scene == "skinned":
                        posed += 1
                        scene.pose(0.02 * posed)
                        scene.sync(be)
                    if a.denoise_temporal:
                        be.reset_accumulation()
                    be.render(view)
                be.framebuffer()
                if rep >= 0:
                    runs[(k, hmax, motion, deform)].append((time.perf_counter() - t0) * 1e3 / a.frames)
                    if deform:
                        ids, state = be.denoise_ids(), be.denoise_motion()[2]
                        floor = (int(be.denoise_pose()[1].shape[0]), int((state[ids[ids < len(state)]] == 3).sum()))
        for k, hmax, motion, deform in settings:
            r = runs[(k, hmax, motion, deform)]
            print(f"denoise {k} form {a.denoise_form}{f' temporal {hmax}' if hmax else ''}{f' motion {motion}' if hmax and any(motions) else ''}{f' deform {deform}' if hmax and any(deforms) else ''}: "
                  f"{statistics.median(r):.3f} ms/frame (min {min(r):.3f}, max {max(r):.3f}; {what})", flush=True)
        if a.bandwidth:
            px = a.width * a.height
            print(f"bandwidth probe: {be.bandwidth_probe():.0f} GB/s (read + written); a pass moves 64 B x {px} pixels = {64e-6 * px:.1f} MB"
                  + (f", k_dn_temporal at least 128 B x {px} = {128e-6 * px:.1f} MB" if a.denoise_temporal else "")
                  + (f", k_dn_temporal_motion up to 24 B x {px} = {24e-6 * px:.1f} MB more, k_dn_ids 36 B per slab slot" if any(motions) else ""), flush=True)
            if any(deforms) and any(passes):
                gbs = be.bandwidth_probe()
                tris, pixels = floor
                nbytes = 40 * px + 128 * tris + 72 * pixels
                print(f"denoise_deform floor: k_dn_tris 40 B x {px} slab slots, k_dn_pose 128 B x {tris} triangles, k_dn_temporal_deform up to 72 B x {pixels} pixels of deforming instances "
                      f"= {nbytes / 1e6:.2f} MB = {nbytes / gbs / 1e3:.2f} us at the probe's {gbs:.0f} GB/s", flush=True)
        be.close()
        return
    if a.overlay:
        import numpy as np
        from rfw_rs_amd import pod
        settings = a.overlay.split(",")
        w, h = a.width, a.height
        view_2d = Scene.camera_2d_view(w, h)
        pixel = np.eye(4, dtype=np.float32)  # scale(1, -1, 1) * translate(-w / 2, -h / 2, 0), column-major
        pixel[1, 1], pixel[3, 0], pixel[3, 1] = -1.0, -w / 2.0, h / 2.0
        pixel = pixel.reshape(16)

        def quad(x0, y0, x1, y1, c, uv=(0.0, 0.0, 1.0, 1.0)):
            p = [(x0, y0, uv[0], uv[1]), (x1, y0, uv[2], uv[1]), (x1, y1, uv[2], uv[3]), (x0, y0, uv[0], uv[1]), (x1, y1, uv[2], uv[3]), (x0, y1, uv[0], uv[3])]
            return [[x, y, 0.0, 0.0, u, v, *c] for x, y, u, v in p]

        if any(s != "a" for s in settings):
            atlas = np.full((8, 128, 4), 255, np.uint8)  # 16 glyph cells, white, random glyph bits in alpha
            atlas[..., 3] = np.random.default_rng(1).integers(0, 2, size=(8, 128), dtype=np.uint8) * 255
            be.set_textures([pod.TextureData(128, 8, 1, atlas.ctypes.data_as(pod.C.POINTER(pod.C.c_uint8)), 0)])  # (the atrium has no textures of its own)
            glyphs = []
            for k in range(2000):
                x, y, g = 40.0 + 14.0 * (k % 100), 40.0 + 18.0 * (k // 100), k % 16
                glyphs += quad(x, y, x + 12.0, y + 16.0, (1.0, 1.0, 1.0, 1.0), (g / 16.0, 0.0, (g + 1) / 16.0, 1.0))
            be.set_2d_mesh(0, quad(0.0, 0.0, w / 2.0, float(h), (0.1, 0.1, 0.3, 0.5)))
            be.set_2d_mesh(1, glyphs, 0)
            be.synchronize()
        runs = {s: [] for s in settings}
        # pixels a setting touches: its quads lie on whole pixels and do not overlap within a mesh (the panel counts again under the glyphs)
        area = lambda v: sum(int((v[k + 1][0] - v[k][0]) * (v[k + 2][1] - v[k][1])) for k in range(0, len(v), 6))
        glyph_px = area(glyphs) if any(s != "a" for s in settings) else 0
        touched = {"a": 0, "b": glyph_px, "c": glyph_px + (w // 2) * h}
        stats = {}
        for rep in range(-1, a.repeats):
            for s in settings:
                if s != "a" or len(settings) > 1:
                    be.set_2d_instances(0, [pixel] if s == "c" else None)
                    be.set_2d_instances(1, [pixel] if s in "bc" else None)
                    be.synchronize()
                    be.framebuffer()
                t0 = time.perf_counter()
                for _ in range(a.warmup if rep < 0 else a.frames):
                    be.render(view, view_2d)
                be.framebuffer()
                if rep >= 0:
                    runs[s].append((time.perf_counter() - t0) * 1e3 / a.frames)
                    if s != "a":
                        stats[s] = be.overlay_stats()
        for s in settings:
            r = runs[s]
            print(f"overlay {s}: {statistics.median(r):.3f} ms/frame (min {min(r):.3f}, max {max(r):.3f}; {what})", flush=True)
        if a.bandwidth:
            gbs = be.bandwidth_probe()
            for s in settings:
                st = stats.get(s, {"drawn": 0, "dropped": 0, "bin_words": 0})  # (the device's own counts of the setting's latest frame)
                n_prims, words = st["drawn"] + st["dropped"], st["bin_words"]
                nbytes = 32 * touched[s] + (160 + 48 + 160) * n_prims + 8 * words
                print(f"overlay {s} floor: {touched[s]} touched pixels, {n_prims} primitives, {words} bin words = {nbytes / 1e6:.2f} MB = {nbytes / gbs / 1e3:.2f} us at the probe's {gbs:.0f} GB/s", flush=True)
        be.close()
        return
    be.set_option("ao_samples", a.ao_samples)
    for mode in (RenderMode(int(m)) for m in a.modes.split(",")):
        for _ in range(a.warmup):
            be.render(view, mode=mode)
        be.framebuffer()
        runs = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            for _ in range(a.frames):
                be.render(view, mode=mode)
            be.framebuffer()
            runs.append((time.perf_counter() - t0) * 1e3 / a.frames)
        print(f"mode {int(mode)} {mode.name}: {statistics.median(runs):.3f} ms/frame (min {min(runs):.3f}, max {max(runs):.3f}; {what}, "
              f"ao_samples {a.ao_samples})", flush=True)
    be.close()


if __name__ == "__main__":
    main()
