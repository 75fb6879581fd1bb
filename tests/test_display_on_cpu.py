"""The display transform (tests/test_gpu_display.py) before any device: the GPU tests run against the emulated library (tests/emu/build_emu_lib.py, as
tests/test_render_scale_on_cpu.py) — csrc/display.inc builds there as it stands, with no textual substitution —, the host mirror's
`example_animated --tonemap 3 --auto-exposure` runs on that library too, and the gfx950 ISA listing (tools/isa_stats.py) shows that the
stage's three kernels touch no scratch memory and stay inside the LDS and register figures DESIGN.md "Display transform" gives."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def emulated(tmp_path_factory):
    import build_emu_lib
    return build_emu_lib.build(str(tmp_path_factory.mktemp("emulated_hip_display")))


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang as a host compiler")
def test_display_tests_on_the_emulated_kernels(emulated):
    env = dict(os.environ, RFW_HIP_LIB=emulated)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_display.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=3000)
    tail = r.stdout[-3000:] + r.stderr[-1500:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang as a host compiler")
def test_example_animated_with_a_tonemap_on_the_emulated_library(emulated, tmp_path):
    from rfw_rs_amd import Scene
    host = os.path.join(ROOT, "rfw-rs_amd", "host")
    exe = str(tmp_path / "example_animated_emu")
    sources = [os.path.join(host, f) for f in ("example_animated.cpp", "rfw_host.cpp", "gltf.cpp", "gltf_export.cpp", "jpeg.cpp", "obj.cpp")]
    r = subprocess.run([CLANG, "-O1", "-std=c++17", "-pthread", "-o", exe] + sources + [emulated, "-Wl,-rpath," + os.path.dirname(emulated), "-lz"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    glb = Scene().build("atrium", 2000, 0, 0.0, 3).save_glb(str(tmp_path / "atrium.glb"))
    out = tmp_path / "last.ppm"
    args = [exe, "--gltf", glb, "--frames", "6", "--size", "48x32", "--spheres", "3x3", "--path-length", "1", "--out", str(out)]
    r = subprocess.run(args + ["--tonemap", "3", "--auto-exposure"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"tonemap 3, automatic exposure: the last frame was shown with exposure (\S+)", r.stdout)
    assert m, r.stdout
    assert 1.0 / 64.0 <= float(m.group(1)) <= 64.0  # exposure_min ... exposure_max
    head = b"P6\n48 32\n255\n"
    shown = out.read_bytes()
    assert shown.startswith(head) and len(shown) == len(head) + 48 * 32 * 3
    r = subprocess.run(args + ["--tonemap", "1"], capture_output=True, text=True, timeout=600)  # manual: the default exposure, 1
    assert r.returncode == 0 and "tonemap 1, manual exposure: the last frame was shown with exposure 1\n" in r.stdout, r.stdout + r.stderr[-2000:]
    r = subprocess.run(args + ["--tonemap", "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "tonemap" in r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_isa_of_the_display_kernels(tmp_path_factory):
    import isa_stats
    path, _ = isa_stats.build(out_dir=str(tmp_path_factory.mktemp("rfw_isa_display")))
    ks = isa_stats.parse(path)
    for name in ("k_display_hist", "k_display_resolve", "k_display_apply"):
        assert name in ks, (name, sorted(ks))
        assert ks[name]["scratch_bytes"] == 0 and ks[name]["scratch"] == 0, (name, ks[name])
        assert ks[name]["vgpr"] <= 128, (name, ks[name])  # at least 4 wavefronts per SIMD
    assert ks["k_display_hist"]["lds_bytes"] <= 4096, ks["k_display_hist"]
