"""Option "denoise_motion" (tests/test_gpu_denoise_motion.py) before any device: the GPU tests run against the emulated library
(tests/emu/build_emu_lib.py, as tests/test_denoise_temporal_on_cpu.py), and the gfx950 ISA listing (tools/isa_stats.py) shows that the three
new kernels touch no scratch memory, use no LDS and leave room for four wavefronts per SIMD."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang as a host compiler")
def test_motion_tests_on_the_emulated_kernels(tmp_path_factory):
    import build_emu_lib
    lib = build_emu_lib.build(str(tmp_path_factory.mktemp("emulated_hip_denoise_motion")))
    env = dict(os.environ, RFW_HIP_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_denoise_motion.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=3000)
    tail = r.stdout[-3000:] + r.stderr[-1500:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_isa_of_the_motion_kernels(tmp_path_factory):
    import isa_stats
    path, _ = isa_stats.build(out_dir=str(tmp_path_factory.mktemp("rfw_isa_denoise_motion")))
    ks = isa_stats.parse(path)
    for name in ("k_dn_temporal_motion", "k_dn_ids", "k_dn_motion"):
        assert name in ks, sorted(ks)
        k = ks[name]
        print(name + ":", k)
        assert k["scratch_bytes"] == 0 and k["scratch"] == 0, (name, k)
        assert k["vgpr"] <= 128, (name, k)  # at least 4 wavefronts per SIMD
        assert k["lds_bytes"] == 0 and k["lds"] == 0, (name, k)
    # the kernel it shares its body with keeps its resources (tests/test_denoise_temporal_on_cpu.py holds the bounds)
    assert ks["k_dn_temporal"]["vgpr"] <= ks["k_dn_temporal_motion"]["vgpr"], (ks["k_dn_temporal"], ks["k_dn_temporal_motion"])
