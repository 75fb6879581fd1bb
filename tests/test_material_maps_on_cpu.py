"""Option "material_maps" (tests/test_gpu_material_maps.py) before any device: the GPU tests run against the emulated library
(tests/emu/build_emu_lib.py, as tests/test_display_on_cpu.py) — csrc/ builds there as it stands —, the host mirror's
`example_animated --material-maps` runs on that library with a glTF file whose look lives in its metallic-roughness texture, and the gfx950
ISA listing (tools/isa_stats.py) shows that the kernels that run with the option off (k_shade) are the parent commit's, and that their
twins that read the maps (k_shade_maps) touch no scratch memory either."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def emulated(tmp_path_factory):
    import build_emu_lib
    return build_emu_lib.build(str(tmp_path_factory.mktemp("emulated_hip_material_maps")))


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang as a host compiler")
def test_material_map_tests_on_the_emulated_kernels(emulated):
    env = dict(os.environ, RFW_HIP_LIB=emulated)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_material_maps.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=3000)
    tail = r.stdout[-3000:] + r.stderr[-1500:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail


def write_metal_gltf(directory):
    """tests/gltf_util.py's lit floor with its 8 x 8 PNG as the METALLIC-ROUGHNESS texture of a white material with both factors 1: left half
    rough dielectric (G, B = 255, 0), right half smooth metal (G, B = 20, 255)"""
    from gltf_util import encode_png, write_textured_gltf
    tex = np.zeros((8, 8, 4), np.uint8)
    tex[:, :4] = (0, 255, 0, 255)
    tex[:, 4:] = (0, 20, 255, 255)
    path, _ = write_textured_gltf(directory, png=encode_png(tex))
    doc = json.loads(path.read_text())
    doc["materials"][0] = {"pbrMetallicRoughness": {"metallicRoughnessTexture": {"index": 0}, "metallicFactor": 1.0, "roughnessFactor": 1.0}}
    path.write_text(json.dumps(doc))
    return str(path)


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang as a host compiler")
def test_example_animated_with_material_maps_on_the_emulated_library(emulated, tmp_path):
    host = os.path.join(ROOT, "rfw-rs_amd", "host")
    exe = str(tmp_path / "example_animated_emu")
    sources = [os.path.join(host, f) for f in ("example_animated.cpp", "rfw_host.cpp", "gltf.cpp", "gltf_export.cpp", "jpeg.cpp", "obj.cpp")]
    r = subprocess.run([CLANG, "-O1", "-std=c++17", "-pthread", "-o", exe] + sources + [emulated, "-Wl,-rpath," + os.path.dirname(emulated), "-lz"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    gltf = write_metal_gltf(tmp_path)
    frames = {}
    for name, extra in (("off", []), ("off again", []), ("on", ["--material-maps"])):
        out = tmp_path / (name.replace(" ", "_") + ".ppm")
        r = subprocess.run([exe, "--gltf", gltf, "--frames", "3", "--size", "48x32", "--spheres", "2x2", "--path-length", "2", "--out", str(out)] + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        m = re.search(r"material maps: (\d+) of (\d+) materials have a live", r.stdout)
        assert (m is not None) == bool(extra), r.stdout
        if m:
            assert int(m.group(1)) == 1 and int(m.group(2)) >= 2, r.stdout  # the floor's; the lamp and the spheres have none
        head = b"P6\n48 32\n255\n"
        shown = out.read_bytes()
        assert shown.startswith(head) and len(shown) == len(head) + 48 * 32 * 3
        frames[name] = np.frombuffer(shown[len(head):], np.uint8)
    assert np.array_equal(frames["off"], frames["off again"])
    changed = (frames["on"].reshape(-1, 3) != frames["off"].reshape(-1, 3)).any(axis=1).mean()
    assert changed > 0.02, changed  # the floor looks different


# k_shade of the parent commit 98e110b (tools/isa_stats.py on that tree, the Makefile's flags, gfx950): <BATCH, GROUP> -> figures
PARENT_K_SHADE = {
    (True, 256): dict(vgpr=87, scratch_bytes=0, valu=5463, salu=1576, smem=39, vmem=101, lds=36, scratch=0),
    (True, 512): dict(vgpr=87, scratch_bytes=0, valu=5465, salu=1579, smem=39, vmem=101, lds=37, scratch=0),
    (False, 256): dict(vgpr=85, scratch_bytes=0, valu=5461, salu=1585, smem=27, vmem=100, lds=36, scratch=0),
    (False, 512): dict(vgpr=85, scratch_bytes=0, valu=5463, salu=1592, smem=27, vmem=100, lds=37, scratch=0),
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_isa_of_k_shade(tmp_path_factory):
    import isa_stats
    path, _ = isa_stats.build(out_dir=str(tmp_path_factory.mktemp("rfw_isa_material_maps")))
    ks = isa_stats.parse(path)
    for (batch, group), want in PARENT_K_SHADE.items():
        args = "<%s, %d>" % ("true" if batch else "false", group)
        off, on = ks.get("k_shade" + args), ks.get("k_shade_maps" + args)  # MAPS = false (the name the parent's kernel has), MAPS = true
        assert off and on, (args, sorted(k for k in ks if "k_shade" in k))
        assert {k: off[k] for k in want} == want, ("k_shade" + args, off)
        assert on["scratch_bytes"] <= off["scratch_bytes"] and on["scratch"] <= off["scratch"], ("k_shade_maps" + args, on)
        print("k_shade_maps" + args, on)
    assert sum(k.startswith("k_shade") for k in ks) == 8
