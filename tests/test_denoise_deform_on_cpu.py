"""Option "denoise_deform" (tests/test_gpu_denoise_deform.py) before any device: the GPU tests run against the emulated library
(tests/emu/build_emu_lib.py, as tests/test_denoise_motion_on_cpu.py), and the gfx950 ISA listing (tools/isa_stats.py) shows that the three
new kernels touch no scratch memory, use no LDS and leave room for four wavefronts per SIMD, and that the two kernels k_dn_temporal_deform
shares its body with take no more registers than in the parent commit's listing: k_dn_temporal 43 VGPRs, k_dn_temporal_motion 44."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
HIPCC = "/opt/rocm/bin/hipcc"
PARENT_VGPRS = {"k_dn_temporal": 43, "k_dn_temporal_motion": 44}


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang as a host compiler")
def test_deform_tests_on_the_emulated_kernels(tmp_path_factory):
    import build_emu_lib
    lib = build_emu_lib.build(str(tmp_path_factory.mktemp("emulated_hip_denoise_deform")))
    env = dict(os.environ, RFW_HIP_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_denoise_deform.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=3000)
    tail = r.stdout[-3000:] + r.stderr[-1500:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_isa_of_the_deform_kernels(tmp_path_factory):
    import isa_stats
    path, _ = isa_stats.build(out_dir=str(tmp_path_factory.mktemp("rfw_isa_denoise_deform")))
    ks = isa_stats.parse(path)
    for name in ("k_dn_temporal_deform", "k_dn_pose", "k_dn_tris"):
        assert name in ks, sorted(ks)
        k = ks[name]
        print(name + ":", k)
        assert k["scratch_bytes"] == 0 and k["scratch"] == 0, (name, k)
        assert k["vgpr"] <= 128, (name, k)  # at least 4 wavefronts per SIMD
        assert k["lds_bytes"] == 0 and k["lds"] == 0, (name, k)
    for name, vgprs in PARENT_VGPRS.items():
        print(name + ":", ks[name])
        assert ks[name]["vgpr"] <= vgprs, (name, ks[name])
        assert ks[name]["scratch_bytes"] == 0 and ks[name]["lds_bytes"] == 0, (name, ks[name])
