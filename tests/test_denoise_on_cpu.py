"""Option "denoise" (tests/test_gpu_denoise.py) before any device: the GPU tests run against the emulated library (tests/emu/build_emu_lib.py,
as tests/test_render_modes_on_cpu.py), and the gfx950 ISA listing (tools/isa_stats.py) shows that the new kernels touch no scratch memory,
stay far inside the LDS, and that factoring the primary-hit block out of k_aov left it free of scratch."""
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


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang as a host compiler")
def test_denoise_tests_on_the_emulated_kernels(tmp_path_factory):
    import build_emu_lib
    lib = build_emu_lib.build(str(tmp_path_factory.mktemp("emulated_hip_denoise")))
    env = dict(os.environ, RFW_HIP_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_denoise.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=3000)
    tail = r.stdout[-3000:] + r.stderr[-1500:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_isa_of_the_denoise_kernels(tmp_path_factory):
    import isa_stats
    path, _ = isa_stats.build(out_dir=str(tmp_path_factory.mktemp("rfw_isa_denoise")))
    ks = isa_stats.parse(path)
    atrous = [n for n in ks if re.match(r"k_atrous<", n)]
    assert len(atrous) == 8, sorted(ks)  # <FIRST, LAST, TILED>
    for name in atrous + ["k_dn_guide", "k_aov"]:
        assert name in ks, (name, sorted(ks))
        assert ks[name]["scratch_bytes"] == 0 and ks[name]["scratch"] == 0, (name, ks[name])
        assert ks[name]["lds_bytes"] <= 160 * 1024, (name, ks[name])
        assert ks[name]["vgpr"] <= 128, (name, ks[name])  # at least 4 wavefronts per SIMD
    for name in atrous:
        tiled = name.endswith("true>")
        assert (ks[name]["lds_bytes"] == 3 * 20 * 32 * 16) == tiled, (name, ks[name])  # the staged 20 x 20 window at a pitch of 32
