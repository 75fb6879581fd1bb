"""What the compiler made of the kernels, checked on the gfx950 ISA listing (hipcc cross-compiles here: no GPU needed, ~15 s).

* No trace kernel of the product (the non-counting instantiations) touches scratch memory: VERDICT r04 found `k_shadow` reloading spilled
  register pairs inside its traversal loop at the 64-VGPR / 8-wave cap.
* Every trace kernel stays inside the register budget of the occupancy it is compiled for.
* The issue-rate probe's loops hold exactly the vector instructions per trip the host multiplies by (28 were counted as 32).
* The flat traversal loops (round 5) keep their share of scalar instructions: the nested loops they replaced spent 40-53 % of their
  instructions on exec-mask arithmetic, which takes the same issue slots as vector work; a change that brings a flag back across the loop's
  joins shows up here before it shows up in a frame rate.
* The build is free of the "inline asm clobber list contains reserved registers" warning (round 4's v_writelane asm wrote M0)."""
import os
import re
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_stats  # noqa: E402


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    path, stderr = isa_stats.build(out_dir=str(tmp_path_factory.mktemp("rfw_isa")))
    return path, stderr, isa_stats.parse(path)


TRACE = ("k_primary", "k_extend", "k_shadow", "k_query")


def test_no_trace_kernel_touches_scratch(listing):
    _, _, ks = listing
    seen = 0
    for name, k in ks.items():
        if not name.startswith(TRACE):
            continue
        counting = re.search(r"<true", name) is not None  # COUNT / DEPTH instantiations: instrumented frames outside every timed region
        if counting:
            continue
        seen += 1
        assert k["scratch_bytes"] == 0 and k["scratch"] == 0, (name, k)
    assert seen >= 12  # primary (4 flavours), extend (2), shadow (2 + 2 + 2), queries (2)


def test_trace_kernels_fit_their_occupancy(listing):
    _, _, ks = listing
    budget = {8: 64, 7: 72, 6: 85, 5: 102}  # VGPRs per lane at that many waves per SIMD (512 / waves, granule 8)
    src = open(os.path.join(ROOT, "rfw-rs_amd", "csrc", "kernels.hip")).read()
    decl = re.search(r"constexpr int (kTraceWaves = \d+(?:, k\w+Waves\w* = \d+)+);", src).group(1)  # the waves per SIMD each kind of kernel is compiled for
    waves = {m.group(1): int(m.group(2)) for m in re.finditer(r"(k\w+) = (\d+)", decl)}
    want = {"k_shadow<": waves["kTraceWavesAny"], "k_shadow_stream<": waves["kStreamWavesAny"], "k_shadow_packet<": waves["kPacketWaves"],
            "k_primary_packet<": waves["kPacketWaves"], "k_primary<": waves["kTraceWaves"], "k_extend<": waves["kTraceWaves"],
            "k_extend_stream<": waves["kStreamWaves"]}
    for name, k in ks.items():
        for prefix, w in want.items():
            if name.startswith(prefix):
                assert k["vgpr"] <= budget[w], (name, k["vgpr"], w)


def test_flat_loops_keep_their_scalar_share(listing):
    """Static scalar instruction counts of the kernels whose loops are flat (traverse_flat.inc), against bounds half way
    between what the flat and the nested forms compile to (round 5, ROCm 7.2: k_shadow 803 / 923, k_shadow_stream 646 / 876,
    k_extend_stream 423 / 549).  A tripwire for the source and for the compiler, not a performance claim."""
    _, _, ks = listing
    want = {"k_shadow<false, false>": 865, "k_shadow_stream<false, false>": 760, "k_extend_stream<false>": 485}
    for name, bound in want.items():
        assert name in ks, (name, sorted(ks)[:8])
        assert ks[name]["salu"] <= bound, (name, ks[name]["salu"], bound)


def test_block_table_of_a_kernel(listing):
    """tools/isa_blocks.py (how round 5 read the hot trip of a loop) still parses the listing: the flat any-hit kernel has a loop whose blocks
    hold a four-child node test (24 byte conversions) and no more than a handful of register copies."""
    import isa_blocks
    path, _, _ = listing
    lines = open(path).read().splitlines()
    hit = [i for i, _, d in isa_blocks.kernels_of(lines) if "k_shadow<false, false>" in d]
    assert len(hit) == 1
    blocks = isa_blocks.blocks_of(isa_blocks.body_of(lines, hit[0]))
    in_loop = [b for b in blocks if b[2]]
    assert len(in_loop) > 20
    node_tests = [b for b in in_loop if sum(1 for x in b[1] if x.startswith("v_cvt_f32_ubyte")) == 24]
    assert len(node_tests) == 2, len(node_tests)  # (one per visiting order)
    for b in node_tests:
        v, mv, s, mem = isa_blocks.count(b[1])
        assert 70 <= v <= 85 and mv <= 2 and mem == 4, (b[0], v, mv, s, mem)


def test_issue_probe_loops_hold_the_counted_instructions(listing):
    path, _, _ = listing
    src = open(os.path.join(ROOT, "rfw-rs_amd", "csrc", "kernels.hip")).read()
    m = re.search(r"issue_probe_vector_per_trip\(int mix\) \{ return mix == 0 \? (\d+)u : \(mix == 1 \? (\d+)u : (\d+)u\); \}", src)
    assert m, "issue_probe_vector_per_trip not found"
    declared = [int(x) for x in m.groups()]
    text = open(path).read()
    for mix, want in enumerate(declared):
        body = text[text.index(f"_ZN6rfwhip13k_issue_probeILi{mix}EEEvPfjf:"):]
        body = body[:body.index("s_endpgm")].splitlines()
        labels = {}
        loops = []
        for i, ln in enumerate(body):
            s = ln.strip()
            lm = re.match(r"^(\.LBB\w+):", s)
            if lm:
                labels[lm.group(1)] = i
            bm = re.match(r"^s_cbranch\w*\s+(\.LBB\w+)", s)
            if bm and bm.group(1) in labels:
                loops.append((labels[bm.group(1)], i))
        assert len(loops) == 1, (mix, loops)
        a, b = loops[0]
        ins = [ln.strip().split()[0] for ln in body[a:b] if ln.strip() and not ln.strip().startswith((";", ".", "/")) and not ln.strip().endswith(":")]
        vector = [op for op in ins if op.startswith("v_")]
        assert len(vector) == want, (mix, want, len(vector), vector)
        if mix == 2:  # the packet step's scalar companions ride along (loop control adds a few)
            assert 27 <= len([op for op in ins if op.startswith("s_") and not op.startswith(("s_cbranch", "s_waitcnt", "s_nop"))]) <= 31


def test_build_has_no_reserved_register_clobbers(listing):
    _, stderr, _ = listing
    assert "reserved registers" not in stderr, stderr[-1500:]
    assert "error" not in stderr.lower()
