"""The render scale (tests/test_gpu_render_scale.py) before any device: the GPU tests run against the emulated library (tests/emu/build_emu_lib.py, as
tests/test_overlay_on_cpu.py) — csrc/resample.inc builds there as it stands, with no textual substitution — and the gfx950 ISA listing
(tools/isa_stats.py) shows that the stage's kernels touch neither scratch memory nor LDS: the tap loops run over registers.
Figures: DESIGN.md "Render scale"."""
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
def test_render_scale_tests_on_the_emulated_kernels(tmp_path_factory):
    import build_emu_lib
    lib = build_emu_lib.build(str(tmp_path_factory.mktemp("emulated_hip_render_scale")))
    env = dict(os.environ, RFW_HIP_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_render_scale.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=3000)
    tail = r.stdout[-3000:] + r.stderr[-1500:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_isa_of_the_resample_kernels(tmp_path_factory):
    import isa_stats
    path, _ = isa_stats.build(out_dir=str(tmp_path_factory.mktemp("rfw_isa_render_scale")))
    ks = isa_stats.parse(path)
    for name in ("k_resample", "k_resample_wide"):
        assert name in ks, (name, sorted(ks))
        assert ks[name]["scratch_bytes"] == 0 and ks[name]["scratch"] == 0, (name, ks[name])  # the weights of the unrolled tap loop live in registers
        assert ks[name]["lds_bytes"] == 0, (name, ks[name])
        assert ks[name]["vgpr"] <= 128, (name, ks[name])  # at least 4 wavefronts per SIMD
