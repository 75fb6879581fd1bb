#!/usr/bin/env python3
"""Frame times of render() with the materials' parameter maps (include/rfw_hip.h option "material_maps") on the bench scene:
python3 tools/material_maps_timing.py [--tree ROOT]

One instance per setting, one frame at a time, as tools/display_timing.py: every repeat renders `--frames` frames of the same view and then
reads the framebuffer back (the wait), after `--warmup` frames.  Prints one line per setting with the median, min and max of the repeats' ms
per frame and the mean ms_shade of the timed frames (rfw_hip_frame_stats: k_shade of every bounce).  Settings:
  off        never names the option, so that a tree without it (--tree: the root of another checkout, built) is timed with the same tool
  maps       option on, every textured material given its diffuse texture as its metallic-roughness map
  maps_all   option on, one 256 x 256 noise texture added and made the metallic-roughness map of every material no colour component of which
             exceeds 1 — the bench scene has no textured material, so this is the row in which k_shade_maps runs there
The last lines give ms_shade of each setting against "off" and the bytes a shaded hit adds: one 16-byte material load and up to four 4-byte
texels per parameter map."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time


def recorded_materials(scene, pod, BackendTable):
    """the scene's materials as its synchronize hands them to a backend (a table that keeps the materials and ignores the rest)"""
    got, keep = [], []
    vp, u32 = C.c_void_p, C.c_uint32

    def cb(fn, *argtypes):
        f = C.CFUNCTYPE(C.c_int, *argtypes)(fn)
        keep.append(f)
        return C.cast(f, C.c_void_p)

    def set_materials(_, ptr, n, changed):
        got[:] = [pod.DeviceMaterial.from_buffer_copy(ptr[k]) for k in range(n)]
        return 0

    t = BackendTable()
    t.instance = None
    t.set_3d_mesh = t.set_3d_instances = cb(lambda _, i, d: 0, vp, u32, vp)
    t.unload_3d_meshes = cb(lambda _, a, n: 0, vp, vp, u32)
    t.set_materials = cb(set_materials, vp, C.POINTER(pod.DeviceMaterial), u32, vp)
    ignore4 = cb(lambda _, a, n, c: 0, vp, vp, u32, vp)
    t.set_textures = t.set_point_lights = t.set_spot_lights = t.set_area_lights = t.set_directional_lights = t.set_skins = ignore4
    t.set_skybox = cb(lambda _, a: 0, vp, vp)
    t.synchronize = cb(lambda _: 0, vp)

    class Recorder:
        def table(self):
            return t

        def last_error(self):
            return "recorder"

    scene.mark_all_changed()
    scene.sync(Recorder())
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default="off,maps,maps_all")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--max-path-length", type=int, default=3)
    ap.add_argument("--triangles", type=int, default=1048576)  # bench.py's atrium1m
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import numpy as np
    import torch  # (the order bench.py has: torch's HIP runtime first)
    torch.cuda.init()
    from rfw_rs_amd import HipBackend, Scene, pod
    from rfw_rs_amd.scene import BackendTable
    w, h = (int(v) for v in a.size.split("x"))
    scene = Scene().build("atrium", a.triangles, 0, 0.0, 0xC0FFEE)
    scene.set_aspect(w / h)
    view = scene.view(w, h)
    materials = recorded_materials(scene, pod, BackendTable)
    shade, maps_per_hit = {}, {}
    for s in a.settings.split(","):
        if s not in ("off", "maps", "maps_all"):
            raise SystemExit(f"unknown setting {s}")
        be = HipBackend.init(w, h, 1.0, max_path_length=a.max_path_length)
        scene.mark_all_changed()
        scene.sync(be)
        mapped = 0
        if s != "off":
            be.set_option("material_maps", 1)
            ms = [pod.DeviceMaterial.from_buffer_copy(m) for m in materials]
            if s == "maps":
                for m in ms:
                    if (m.flags & 1) and m.diffuse_map >= 0:
                        m.flags |= 4 | 8
                        m.metallic_roughness_map = m.diffuse_map
                        mapped += 1
            else:
                if any(m.flags & 1 for m in ms):
                    raise SystemExit("maps_all replaces the scene's textures: it is for scenes without any")
                noise = np.random.default_rng(1).integers(0, 256, 256 * 256 * 4).astype(np.uint8)
                be.set_textures([pod.TextureData(256, 256, 1, noise.ctypes.data_as(C.POINTER(C.c_uint8)), 1)])
                for m in ms:
                    if max(m.color[:3]) <= 1.0:
                        m.flags |= 4 | 8
                        m.metallic_roughness_map = 0
                        mapped += 1
            be.set_materials(ms)
            be.synchronize()
        for _ in range(a.warmup):
            be.render(view)
        be.framebuffer()
        be.drain_timing()
        runs, shade_ms, shade_n = [], 0.0, 0
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            for _ in range(a.frames):
                be.render(view)
            be.framebuffer()
            runs.append((time.perf_counter() - t0) * 1e3 / a.frames)
            ms_, n = be.drain_timing()  # (at most 64 frames are kept between drains)
            shade_ms += ms_["ms_shade"]
            shade_n += n
        st = be.frame_stats()
        hits = st["primary_rays"] + st["extension_rays"]  # an upper bound of the hits k_shade shades per frame (sky hits included)
        be.close()
        shade[s] = shade_ms / max(shade_n, 1)
        maps_per_hit[s] = (mapped, hits)
        print(f"{s}: {statistics.median(runs):.3f} ms/frame (min {min(runs):.3f}, max {max(runs):.3f}), ms_shade {shade[s]:.4f} over {shade_n} frames, "
              f"{mapped} of {len(materials)} materials mapped ({a.repeats} x {a.frames} frames of {w}x{h}, atrium of {a.triangles} triangles, "
              f"max path length {a.max_path_length}, {hits} rays shaded per frame at most)", flush=True)
    for s, v in shade.items():
        if s == "off" or "off" not in shade:
            continue
        mapped, hits = maps_per_hit[s]
        print(f"material maps, {s}: ms_shade {v:.4f} against {shade['off']:.4f} off = {v - shade['off']:+.4f} ms per frame"
              + (f"; a hit on a mapped material adds 16 B of material and up to 16 B of texels: at most {hits * 32 / 1e6:.1f} MB per frame" if mapped else
                 "; no material is mapped: the kernels of the option off run"), flush=True)


if __name__ == "__main__":
    main()
