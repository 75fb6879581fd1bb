#!/usr/bin/env python3
"""Frame times of render() per mode (include/rfw_hip.h RFW_HIP_RENDER_*) on the bench scene: python3 tools/render_mode_timing.py [--modes 0,5,6]

One instance, one frame at a time: every repeat renders `--frames` frames of the same view and then reads the framebuffer back (the wait),
after `--warmup` frames.  Prints one line per mode with the median, min and max of the repeats' ms per frame.  DESIGN.md "Render modes"
quotes its output."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="0,5,6")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--triangles", type=int, default=1048576)  # bench.py's atrium1m
    ap.add_argument("--ao-samples", type=int, default=4)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch  # (the order bench.py has: torch's HIP runtime first)
    torch.cuda.init()
    from rfw_rs_amd import HipBackend, RenderMode, Scene
    scene = Scene().build("atrium", a.triangles, 0, 0.0, 0xC0FFEE)
    scene.set_aspect(a.width / a.height)
    view = scene.view(a.width, a.height)
    be = HipBackend.init(a.width, a.height, 1.0, max_path_length=1)
    scene.sync(be)
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
        print(f"mode {int(mode)} {mode.name}: {statistics.median(runs):.3f} ms/frame (min {min(runs):.3f}, max {max(runs):.3f}; {a.repeats} x {a.frames} "
              f"frames, {a.width}x{a.height}, atrium of {a.triangles} triangles, ao_samples {a.ao_samples}, max path length 1)", flush=True)
    be.close()


if __name__ == "__main__":
    main()
