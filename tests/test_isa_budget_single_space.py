"""The single-space twins of the trace kernels (DESIGN.md "Single-space scenes") on the gfx950 ISA listing, held to what tests/test_isa_budget.py
asks of the two-level kernels: the non-counting instantiations touch no scratch memory, every instantiation stays inside the register budget
of the occupancy it is compiled for — and, their reason to exist, each holds fewer instructions than its two-level twin."""
import os
import re
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_stats  # noqa: E402

TWINS = {  # single-space kernel -> (its two-level twin, the waves-per-SIMD constant both are compiled for)
    "k_primary_ss<false>": ("k_primary<false>", "kTraceWaves"),
    "k_primary_packet_ss<false>": ("k_primary_packet<false>", "kPacketWaves"),
    "k_primary_batch_ss<false>": ("k_primary_batch<false>", "kTraceWaves"),
    "k_primary_batch_packet_ss<false>": ("k_primary_batch_packet<false>", "kPacketWaves"),
    "k_extend_ss<false>": ("k_extend<false>", "kTraceWaves"),
    "k_extend_stream_ss<false>": ("k_extend_stream<false>", "kStreamWaves"),
    "k_shadow_ss<false>": ("k_shadow<false, false>", "kTraceWavesAny"),
    "k_shadow_packet_ss<false, true>": ("k_shadow_packet<false, true>", "kPacketWaves"),
    "k_shadow_packet_ss<false, false>": ("k_shadow_packet<false, false>", "kPacketWaves"),
    "k_shadow_stream_ss<false, true>": ("k_shadow_stream<false, true>", "kStreamWavesAny"),
    "k_shadow_stream_ss<false, false>": ("k_shadow_stream<false, false>", "kStreamWavesAny"),
}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    path, _ = isa_stats.build(out_dir=str(tmp_path_factory.mktemp("rfw_isa_ss")))
    return isa_stats.parse(path)


def waves_per_simd():
    src = open(os.path.join(ROOT, "rfw-rs_amd", "csrc", "kernels.hip")).read()
    decl = re.search(r"constexpr int (kTraceWaves = \d+(?:, k\w+Waves\w* = \d+)+);", src).group(1)
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"(k\w+) = (\d+)", decl)}


def test_single_space_kernels_touch_no_scratch(kernels):
    for name in TWINS:
        assert name in kernels, (name, sorted(k for k in kernels if "_ss<" in k))
        assert kernels[name]["scratch_bytes"] == 0 and kernels[name]["scratch"] == 0, (name, kernels[name])


def test_single_space_kernels_fit_their_occupancy(kernels):
    budget = {8: 64, 7: 72, 6: 85, 5: 102}  # VGPRs per lane at that many waves per SIMD (tests/test_isa_budget.py)
    waves = waves_per_simd()
    for name in TWINS:  # the counting instantiations exist (counting frames of a qualifying scene run them) and are held to the same budget
        assert re.sub(r"<false", "<true", name) in kernels, name
    for name, k in kernels.items():
        base = re.sub(r"<true", "<false", name)  # the counting instantiations are held to the same budget
        if base in TWINS:
            assert k["vgpr"] <= budget[waves[TWINS[base][1]]], (name, k["vgpr"])
    fit = lambda vgpr: min(8, 512 // (((vgpr + 7) // 8) * 8))  # waves per SIMD that a kernel's registers allow (granule 8, 512 per lane and SIMD)
    for name, (twin, _) in TWINS.items():
        assert fit(kernels[name]["vgpr"]) >= fit(kernels[twin]["vgpr"]), (name, kernels[name]["vgpr"], kernels[twin]["vgpr"])  # waves per SIMD do not drop


def test_single_space_kernels_are_shorter_than_their_twins(kernels):
    count = lambda k: sum(k[x] for x in ("valu", "salu", "smem", "vmem", "lds", "scratch"))
    for name, (twin, _) in TWINS.items():
        assert count(kernels[name]) < count(kernels[twin]), (name, count(kernels[name]), count(kernels[twin]))
        assert kernels[name].get("lds_bytes", 0) <= kernels[twin].get("lds_bytes", 0), name  # (no parked ray above the stack)
