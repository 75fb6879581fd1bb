#!/usr/bin/env python3
"""Frame times of render() with the display transform (include/rfw_hip.h option "tonemap") on the bench scene: python3 tools/display_timing.py

One instance per setting, one frame at a time, as tools/render_scale_timing.py: every repeat renders `--frames` frames of the same view and
then reads the framebuffer back (the wait), after `--warmup` frames.  Prints one line per setting with the median, min and max of the
repeats' ms per frame and the mean ms_other of the timed frames (rfw_hip_frame_stats: the finaliser, the display transform, the resampling
stage and the 2D layer share that event pair).  Settings: off | manual (exposure 2, `--curve`) | auto (automatic exposure).  "off" never names
an option, so that a tree without the stage can be timed with the same tool.

The stage's own share is ms_other of a setting minus ms_other of "off".  --bandwidth prints next to it what the stage's bytes would cost
at the rate rfw_hip_bandwidth_probe reports: the apply kernel reads and writes 16 B per pixel each, the histogram reads 16 B per pixel."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default="off,manual,auto")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--curve", type=int, default=3)
    ap.add_argument("--max-path-length", type=int, default=1)
    ap.add_argument("--bandwidth", action="store_true")
    ap.add_argument("--triangles", type=int, default=1048576)  # bench.py's atrium1m
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch  # (the order bench.py has: torch's HIP runtime first)
    torch.cuda.init()
    from rfw_rs_amd import HipBackend, Scene
    w, h = (int(v) for v in a.size.split("x"))
    scene = Scene().build("atrium", a.triangles, 0, 0.0, 0xC0FFEE)
    scene.set_aspect(w / h)
    view = scene.view(w, h)
    others, gbs = {}, None
    for s in a.settings.split(","):
        be = HipBackend.init(w, h, 1.0, max_path_length=a.max_path_length)
        if s == "manual":
            be.set_option("tonemap", a.curve)
            be.set_option("exposure", 2.0)
        elif s == "auto":
            be.set_option("tonemap", a.curve)
            be.set_option("auto_exposure", 1)
        elif s != "off":
            raise SystemExit(f"unknown setting {s}")
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
        others[s] = ms["ms_other"] / max(n, 1)
        state = be.display_state() if s != "off" else None
        if a.bandwidth and gbs is None:
            gbs = be.bandwidth_probe()
        be.close()
        print(f"{s}: {statistics.median(runs):.3f} ms/frame (min {min(runs):.3f}, max {max(runs):.3f}), ms_other {others[s]:.4f} over {n} frames "
              f"({a.repeats} x {a.frames} frames of {w}x{h}, atrium of {a.triangles} triangles, max path length {a.max_path_length})"
              + (f", exposure {state['exposure']:.4g}" if state else ""), flush=True)
    for s, other in others.items():
        if s == "off" or "off" not in others:
            continue
        nbytes = w * h * (32 if s == "manual" else 48)
        line = f"display transform, {s}: {other - others['off']:.4f} ms (ms_other {other:.4f} - {others['off']:.4f} with the stage off)"
        if gbs:
            line += f"; {nbytes / 1e6:.1f} MB read + written = {nbytes / gbs / 1e6:.4f} ms at the probe's {gbs:.0f} GB/s"
        print(line, flush=True)


if __name__ == "__main__":
    main()
