#!/usr/bin/env python3
"""Frame times of render() under a render scale (include/rfw_hip.h rfw_hip_create) on the bench scene: python3 tools/render_scale_timing.py

One instance per setting (window, scale), one frame at a time, as tools/render_mode_timing.py times mode 0: every repeat renders `--frames`
frames of the same view — the camera's for the RENDER size — and then reads the framebuffer back (the wait), after `--warmup` frames.
Prints one line per setting with the median, min and max of the repeats' ms per frame and the mean ms_other of the timed frames
(rfw_hip_frame_stats: the finaliser, the resampling stage and the 2D layer share that event pair).  The default settings are the ones
DESIGN.md "Render scale" quotes: a 1920 x 1080 window at scale 1, 0.75 and 0.5, and a 3840 x 2160 window at 0.5.

The stage's own share: ms_other of a scaled setting minus ms_other of the scale-1 setting with the same RENDER size, where the list has
one (3840 x 2160 at 0.5 against 1920 x 1080 at 1: the same frame traced and finalised, then resampled 1080p -> 4K).  --bandwidth prints
next to it the stage's bytes, RW RH 16 read + W H 16 written, and what rfw_hip_bandwidth_probe moves per second."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default="1920x1080@1,1920x1080@0.75,1920x1080@0.5,3840x2160@0.5")
    ap.add_argument("--scale-filter", type=int, default=1)
    ap.add_argument("--max-path-length", type=int, default=1)  # as tools/render_mode_timing.py times mode 0
    ap.add_argument("--bandwidth", action="store_true")
    ap.add_argument("--triangles", type=int, default=1048576)  # bench.py's atrium1m
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch  # (the order bench.py has: torch's HIP runtime first)
    torch.cuda.init()
    from rfw_rs_amd import HipBackend, Scene
    scene = Scene().build("atrium", a.triangles, 0, 0.0, 0xC0FFEE)
    results, gbs = [], None
    for s in a.settings.split(","):
        size, scale = s.split("@")
        w, h = (int(v) for v in size.split("x"))
        scale = float(scale)
        be = HipBackend.init(w, h, scale, max_path_length=a.max_path_length)
        if scale != 1.0 or a.scale_filter != 1:  # (scale 1 never names the option, so that a library without it can be timed through RFW_HIP_LIB)
            be.set_option("scale_filter", a.scale_filter)
        rw, rh = be.render_size() if hasattr(be, "render_size") else (w, h)
        scene.set_aspect(w / h)
        view = scene.view(rw, rh)
        scene.mark_all_changed()
        scene.sync(be)
        for _ in range(a.warmup):
            be.render(view)
        be.framebuffer()
        be.drain_timing()
        runs = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            for _ in range(a.frames):
                be.render(view)
            be.framebuffer()
            runs.append((time.perf_counter() - t0) * 1e3 / a.frames)
        ms, n = be.drain_timing()
        other = ms["ms_other"] / max(n, 1)
        if a.bandwidth and gbs is None:
            gbs = be.bandwidth_probe()
        be.close()
        results.append((w, h, scale, rw, rh, other))
        print(f"window {w}x{h} scale {scale:g} -> traced at {rw}x{rh}: {statistics.median(runs):.3f} ms/frame (min {min(runs):.3f}, max {max(runs):.3f}), "
              f"ms_other {other:.4f} over {n} frames ({a.repeats} x {a.frames} frames, atrium of {a.triangles} triangles, max path length {a.max_path_length}, "
              f"scale_filter {a.scale_filter})", flush=True)
    base = {(rw, rh): other for w, h, scale, rw, rh, other in results if (rw, rh) == (w, h)}
    for w, h, scale, rw, rh, other in results:
        if (rw, rh) != (w, h) and (rw, rh) in base:
            nbytes = 16 * (rw * rh + w * h)
            line = f"resampling stage {rw}x{rh} -> {w}x{h}: {other - base[(rw, rh)]:.4f} ms (ms_other {other:.4f} - {base[(rw, rh)]:.4f} of the {rw}x{rh} window at scale 1)"
            if gbs:
                line += f"; {nbytes / 1e6:.1f} MB read + written = {nbytes / gbs / 1e6:.4f} ms at the probe's {gbs:.0f} GB/s"
            print(line, flush=True)


if __name__ == "__main__":
    main()
