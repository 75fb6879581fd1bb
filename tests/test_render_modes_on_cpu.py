"""Render modes (tests/test_gpu_render_modes.py) before any device: the GPU tests run against the emulated library (tests/emu/build_emu_lib.py,
as tests/test_device_source_on_cpu.py), and the gfx950 ISA listing (tools/isa_stats.py, as tests/test_isa_budget.py) shows that the new
kernels touch no scratch memory and that the path tracer's kernels are what they were before the modes existed."""
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
def test_render_mode_tests_on_the_emulated_kernels(tmp_path_factory):
    import build_emu_lib
    lib = build_emu_lib.build(str(tmp_path_factory.mktemp("emulated_hip_modes")))
    env = dict(os.environ, RFW_HIP_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_render_modes.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=2400)
    tail = r.stdout[-3000:] + r.stderr[-1500:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail


# (instructions, VGPRs) of the path tracer's kernels before the render modes (tools/isa_stats.py on the parent commit); the keys are the
# demangled names as they are now: k_assemble gained a LINEAR parameter, k_pack_f16 / k_pack_bgra8 became templates on it (false = before)
MODE0 = {
    "k_primary_packet<false>": (1202, 63),
    "k_primary<false>": (1325, 72),
    "k_primary_batch_packet<false>": (1233, 63),
    "k_primary_batch<false>": (1368, 72),
    "k_extend_stream<false>": (952, 66),
    "k_extend<false>": (809, 72),
    "k_shade<false, 256>": (7209, 85),
    "k_shade<false, 512>": (7219, 85),
    "k_shadow_packet<false, true>": (825, 55),
    "k_shadow_packet<false, false>": (825, 55),
    "k_shadow_stream<false, true>": (1198, 64),
    "k_shadow_stream<false, false>": (1198, 64),
    "k_shadow<false, true>": (1645, 62),
    "k_shadow<false, false>": (1645, 62),
    "k_assemble<true, true, false>": (181, 14),
    "k_assemble<true, false, false>": (299, 23),
    "k_assemble<false, true, false>": (179, 14),
    "k_assemble<false, false, false>": (296, 24),
    "k_pack_bgra8<false>": (283, 28),
    "_ZN6rfwhip10k_pack_f16ILb0EEEvPK15HIP_vector_typeIfLj4EEPDF16_mj": (111, 22),  # (c++filt does not demangle _Float16)
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_isa_of_the_render_mode_kernels(tmp_path_factory):
    import isa_stats
    path, _ = isa_stats.build(out_dir=str(tmp_path_factory.mktemp("rfw_isa_modes")))
    ks = isa_stats.parse(path)
    count = lambda k: sum(k[x] for x in ("valu", "salu", "smem", "vmem", "lds", "scratch"))
    for name in ("k_aov", "k_ao_filter", "k_assemble<true, false, true>", "k_assemble<false, false, true>", "k_pack_bgra8<true>"):
        assert name in ks, (name, sorted(ks))
        assert ks[name]["scratch_bytes"] == 0 and ks[name]["scratch"] == 0, (name, ks[name])
    f16 = [n for n in ks if re.match(r"_ZN6rfwhip10k_pack_f16ILb1E", n)]  # k_pack_f16<true> (c++filt does not demangle _Float16)
    assert len(f16) == 1 and ks[f16[0]]["scratch_bytes"] == 0 and ks[f16[0]]["scratch"] == 0, [(n, ks[n]) for n in f16]
    assert ks["k_ao_filter"]["lds_bytes"] <= 160 * 1024
    for name, want in MODE0.items():
        if want is None:
            continue
        assert name in ks, name
        assert (count(ks[name]), ks[name]["vgpr"]) == want, (name, count(ks[name]), ks[name]["vgpr"])
