"""Single-space scenes (DESIGN.md "Single-space scenes") before any device, on the emulated library (tests/emu/build_emu_lib.py, as
tests/test_device_source_on_cpu.py): what the host qualifies is what the device flags — every instance of a qualifying scene carries
kInstanceIdentity —, the graft is a tree over exactly the meshes' root nodes whose boxes contain the boxes below them, and a frame traced
through the single-space kernels equals the two-level frame bit for bit."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang as a host compiler")

STRUCTURE = r'''
import numpy as np
from rfw_rs_amd import HipBackend, Scene

scene = Scene().build("atrium", 20000, 0, 0.0, 0xC0FFEE)
spheres = [scene.add_sphere_mesh(k, 7 + k, 1) for k in range(64)]
be = HipBackend.init(64, 36, 1.0, max_path_length=1)
scene.sync(be)
st = be.scene_stats()
assert st["single_space"] == 1 and st["instances"] == 65, st
root, stride, slots = (int(x) for x in be.debug_read("single_space", 12).view(np.uint32))
assert root > 0 and root + slots <= stride

xf = be.debug_read("xforms", 65 * 64).view(np.uint32).reshape(65, 16)
assert ((xf[:, 14] & 3) == 3).all()            # valid and kInstanceIdentity: the device agrees with the host's qualification
mesh_roots = set(int(x) for x in xf[:, 12])    # InstanceXform::node_base
assert len(mesh_roots) == 65

def boxes(node):                               # octant copy 0 of a Node4Q: qlo = lower planes, qhi = upper planes
    f = node.view(np.float32)
    o, s = np.array([f[0], f[1], f[2]], np.float64), np.array([f[3], f[10], f[11]], np.float64)
    out = []
    for k in range(4):
        child = int(node[12 + k])
        if child == 0xffffffff:
            continue
        lo = np.array([(int(node[4 + a]) >> (8 * k)) & 255 for a in range(3)]) * s + o
        hi = np.array([(int(node[7 + a]) >> (8 * k)) & 255 for a in range(3)]) * s + o
        out.append((child, lo, hi))
    return out

graft = be.debug_read("blas_graft", slots * 64).view(np.uint32).reshape(-1, 16)
raw = be.debug_read("blas_raw", 1 << 30).view(np.float32).reshape(-1, 32)   # the builders' own nodes: lox hix loy hiy loz hiz (4 each), children

def mesh_bounds(index):                        # a mesh's root node: the box of the mesh as its builder saw it (before quantisation)
    n = raw[index]
    live = n[24:28].view(np.uint32) != 0xffffffff
    return (np.array([n[0:4][live].min(), n[8:12][live].min(), n[16:20][live].min()], np.float64),
            np.array([n[4:8][live].max(), n[12:16][live].max(), n[20:24][live].max()], np.float64))

# every box on the way from the graft's root down to a mesh's root contains that mesh (each level's boxes are rounded outwards on their own
# grid, so they contain what they were made from, not necessarily each other)
seen, todo = set(), [(root, [])]
while todo:
    index, above = todo.pop()
    assert root <= index < root + slots
    for child, lo, hi in boxes(graft[index - root]):
        assert not (child & 0x80000000), "a graft holds no triangles"
        if child >= root:
            todo.append((child, above + [(lo, hi)]))
            continue
        assert child not in seen
        seen.add(child)
        mlo, mhi = mesh_bounds(child)
        for blo, bhi in above + [(lo, hi)]:
            assert (blo <= mlo).all() and (bhi >= mhi).all(), (index, child, blo, mlo, bhi, mhi)
assert seen == mesh_roots, (len(seen), len(mesh_roots))

m = np.eye(4, dtype=np.float32); m[2, 3] = 0.25
scene.set_instance_matrix(spheres[5], 0, m); scene.sync(be)
assert be.scene_stats()["single_space"] == 0
assert int(be.debug_read("single_space", 4).view(np.uint32)[0]) == 0
scene.set_instance_matrix(spheres[5], 0, np.eye(4, dtype=np.float32)); scene.sync(be)
assert be.scene_stats()["single_space"] == 1
be.close()
print("structure ok")
'''


@pytest.fixture(scope="module")
def emulated_library(tmp_path_factory):
    import build_emu_lib
    return build_emu_lib.build(str(tmp_path_factory.mktemp("emulated_hip_single_space")))


def test_qualification_flags_and_graft(emulated_library):
    env = dict(os.environ, RFW_HIP_LIB=emulated_library, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", STRUCTURE], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "structure ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_a_single_space_frame_on_the_emulated_kernels(emulated_library):
    """tests/test_gpu_single_space.py's first case at max path length 1: packets for the camera rays, one ray per lane for the shadow rays."""
    env = dict(os.environ, RFW_HIP_LIB=emulated_library)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_single_space.py", "-k",
                        "test_single_space_equals_two_level and atrium2 and default and not 3"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    tail = r.stdout[-3000:] + r.stderr[-1500:]
    assert r.returncode == 0 and "1 passed" in tail, tail
