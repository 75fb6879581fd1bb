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
a library without it can be timed through RFW_HIP_LIB), in the same turns."""
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
    ap.add_argument("--max-path-length", type=int, default=None)  # 1 for the modes (DESIGN.md "Render modes"), 3 with --denoise
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
        a.max_path_length = 3 if a.denoise else 1
    import torch  # (the order bench.py has: torch's HIP runtime first)
    torch.cuda.init()
    from rfw_rs_amd import HipBackend, RenderMode, Scene
    scene = Scene().build("atrium", a.triangles, 0, 0.0, 0xC0FFEE)
    scene.set_aspect(a.width / a.height)
    view = scene.view(a.width, a.height)
    be = HipBackend.init(a.width, a.height, 1.0, max_path_length=a.max_path_length)
    scene.sync(be)
    what = f"{a.repeats} x {a.frames} frames, {a.width}x{a.height}, atrium of {a.triangles} triangles, max path length {a.max_path_length}"
    if a.denoise:
        passes = [int(k) for k in a.denoise.split(",")]
        motions = [int(m) for m in a.denoise_motion.split(",")] if a.denoise_motion else [0]
        if any(motions) and not a.denoise_temporal:
            ap.error("--denoise-motion needs --denoise-temporal")
        settings = [(k, 0, 0) for k in passes] + [(k, a.denoise_temporal, m) for k in passes if k and a.denoise_temporal for m in motions]
        if any(passes):
            be.set_option("denoise_form", a.denoise_form)
        runs = {s: [] for s in settings}
        for rep in range(-1, a.repeats):  # (-1: the warm-up round of every setting)
            for k, hmax, motion in settings:
                if any(passes):  # (all zero: never name the option, so that a library without it can be timed too)
                    be.set_option("denoise", k)
                if a.denoise_temporal:
                    be.set_option("denoise_temporal", hmax)
                if any(motions):
                    be.set_option("denoise_motion", motion)
                t0 = time.perf_counter()
                for _ in range(a.warmup if rep < 0 else a.frames):
                    if a.denoise_temporal:
                        be.reset_accumulation()
                    be.render(view)
                be.framebuffer()
                if rep >= 0:
                    runs[(k, hmax, motion)].append((time.perf_counter() - t0) * 1e3 / a.frames)
        for k, hmax, motion in settings:
            r = runs[(k, hmax, motion)]
            print(f"denoise {k} form {a.denoise_form}{f' temporal {hmax}' if hmax else ''}{f' motion {motion}' if hmax and any(motions) else ''}: {statistics.median(r):.3f} ms/frame (min {min(r):.3f}, max {max(r):.3f}; {what})", flush=True)
        if a.bandwidth:
            px = a.width * a.height
            print(f"bandwidth probe: {be.bandwidth_probe():.0f} GB/s (read + written); a pass moves 64 B x {px} pixels = {64e-6 * px:.1f} MB"
                  + (f", k_dn_temporal at least 128 B x {px} = {128e-6 * px:.1f} MB" if a.denoise_temporal else "")
                  + (f", k_dn_temporal_motion up to 24 B x {px} = {24e-6 * px:.1f} MB more, k_dn_ids 36 B per slab slot" if any(motions) else ""), flush=True)
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
