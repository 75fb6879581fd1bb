"""Bindings of the C++ host library (rfw-rs_amd/host/librfw_host.so): scene-side inputs of the
Backend boundary (Mesh3D::from, into_device_material, update_lights, Camera3D::get_view,
synchronize_system) and the synthetic scenes standing in for the assets the reference lacks."""
import ctypes as C
import os

from . import pod

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB = os.path.join(_HERE, "host", "librfw_host.so")


class BackendTable(C.Structure):
    """Table of C entry points with the rfw_hip_* signatures (see rfw_host.cpp rfwhost_backend_table)."""
    _fields_ = [("instance", C.c_void_p)] + [(n, C.c_void_p) for n in (
        "set_3d_mesh", "unload_3d_meshes", "set_3d_instances", "set_materials", "synchronize",
        "set_point_lights", "set_spot_lights", "set_area_lights", "set_directional_lights", "set_textures", "set_skybox", "set_skins",
        "set_2d_mesh", "set_2d_instances")]  # (the last two may stay null: a backend without a 2D layer)


_lib = None


def host_lib():
    global _lib
    if _lib is None:
        if not os.path.exists(HOST_LIB):
            raise RuntimeError(f"{HOST_LIB} missing: run `python -c 'import __graft_entry__ as g; g.build()'` first")
        l = C.CDLL(HOST_LIB)
        l.rfwhost_scene_create.restype = C.c_void_p
        l.rfwhost_scene_destroy.argtypes = [C.c_void_p]
        l.rfwhost_build.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32]
        l.rfwhost_animate.argtypes = [C.c_void_p, C.c_float]
        l.rfwhost_load_gltf.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        l.rfwhost_save_glb.argtypes = [C.c_void_p, C.c_char_p]
        l.rfwhost_last_error.argtypes = [C.c_void_p]
        l.rfwhost_last_error.restype = C.c_char_p
        l.rfwhost_pose.argtypes = [C.c_void_p, C.c_float]
        l.rfwhost_set_camera.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float]
        l.rfwhost_set_aspect.argtypes = [C.c_void_p, C.c_float]
        l.rfwhost_camera_view.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(pod.CameraView3D)]
        l.rfwhost_mark_all_changed.argtypes = [C.c_void_p]
        l.rfwhost_render_system.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_double, C.c_int, C.POINTER(pod.CameraView3D), C.POINTER(C.c_float)]
        l.rfwhost_synchronize.argtypes = [C.c_void_p, C.POINTER(BackendTable)]
        l.rfwhost_triangle_count.argtypes = [C.c_void_p]
        l.rfwhost_triangle_count.restype = C.c_uint64
        l.rfwhost_counts.argtypes = [C.c_void_p, C.c_uint32]
        l.rfwhost_counts.restype = C.c_uint32
        l.rfwhost_mesh_data.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(pod.MeshData3D)]
        l.rfwhost_edit.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
        l.rfwhost_into_device_material.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(pod.DeviceMaterial)]
        l.rfwhost_set_animation_time.argtypes = [C.c_void_p, C.c_double]
        l.rfwhost_camera_move.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        l.rfwhost_load_obj.argtypes = [C.c_void_p, C.c_char_p]
        l.rfwhost_add_quad.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_float, C.c_uint32]
        l.rfwhost_material.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_int32)]
        l.rfwhost_texture.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p, C.c_uint64]
        l.rfwhost_set_graph_transform.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        l.rfwhost_graph_count.argtypes = [C.c_void_p]
        l.rfwhost_instantiate_graph.argtypes = [C.c_void_p, C.c_uint32]
        l.rfwhost_animation_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
        l.rfwhost_skin_matrices.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_float), C.c_uint32]
        l.rfwhost_instance_matrix.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
        l.rfwhost_set_instance_matrix.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
        l.rfwhost_add_2d_mesh.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32]
        l.rfwhost_set_2d_mesh.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int32]
        l.rfwhost_add_2d_quad.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_int32, C.POINTER(C.c_float)]
        l.rfwhost_add_2d_instance.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_float)]
        l.rfwhost_set_2d_matrix.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
        l.rfwhost_2d_mesh.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_int32)]
        l.rfwhost_camera_2d_view.argtypes = [C.c_uint32, C.c_uint32, C.c_double, C.POINTER(C.c_float)]
        l.rfwhost_hud_glyph.argtypes = [C.c_char, C.POINTER(C.c_uint8)]
        l.rfwhost_decode_image.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p, C.c_uint64, C.POINTER(C.c_char_p)]
        _lib = l
    return _lib


def decode_image(data):
    """PNG or JPEG bytes -> (h, w, 4) uint8 RGBA through the importer's own decoders (host/gltf.cpp, host/jpeg.cpp)."""
    import numpy as np
    l = host_lib()
    w, h, err = C.c_uint32(), C.c_uint32(), C.c_char_p()
    if l.rfwhost_decode_image(data, len(data), C.byref(w), C.byref(h), None, 0, C.byref(err)) != 0:
        raise ValueError((err.value or b"").decode(errors="replace"))
    out = np.empty((h.value, w.value, 4), np.uint8)
    l.rfwhost_decode_image(data, len(data), C.byref(w), C.byref(h), out.ctypes.data, out.nbytes, C.byref(err))
    return out


class Scene:
    """A host-side scene (rfw::Scene + Camera3D).  `sync(backend)` runs rfw::synchronize_system against any
    object exposing `.table()` (the product's HipBackend, or the oracle binding used by the tests)."""

    def __init__(self):
        self._l = host_lib()
        self._h = C.c_void_p(self._l.rfwhost_scene_create())

    def __del__(self):
        try:
            self._l.rfwhost_scene_destroy(self._h)
        except Exception:
            pass

    def build(self, kind, a=0, b=0, c=0.0, seed=1):
        rc = self._l.rfwhost_build(self._h, kind.encode(), a, b, c, seed)
        if rc != 0:
            raise ValueError(f"unknown scene kind {kind}")
        return self

    def load_gltf(self, path, use_camera=True):
        """Adds a glTF 2.0 file (.gltf or .glb) to the scene: meshes, materials, instances, skins, first perspective camera."""
        if self._l.rfwhost_load_gltf(self._h, os.fsencode(path), 1 if use_camera else 0) != 0:
            raise ValueError((self._l.rfwhost_last_error(self._h) or b"").decode(errors="replace"))
        return self

    def add_quad(self, normal, position, width, height, material):
        """Quad3D::new (crates/rfw-scene/src/objects_3d/quad.rs) as a mesh with one instance; returns the mesh id."""
        mesh = self._l.rfwhost_add_quad(self._h, (C.c_float * 3)(*normal), (C.c_float * 3)(*position), width, height, material)
        if mesh < 0:
            raise ValueError("add_quad: unknown material")
        return int(mesh)

    def load(self, path):
        """Scene::load (crates/rfw-scene/src/lib.rs): the loader is picked by the file's extension — .gltf / .glb or .obj."""
        ext = os.path.splitext(str(path))[1].lower()
        if ext in (".gltf", ".glb"):
            return self.load_gltf(path)
        if ext == ".obj":
            self.load_obj(path)
            return self
        raise ValueError(f"no loader for {ext!r} files")

    def load_obj(self, path):
        """ObjLoader (crates/rfw-scene/src/loaders/obj.rs): a Wavefront OBJ file with its material libraries and textures as ONE mesh with one
        instance at the identity.  Returns the mesh id."""
        mesh = self._l.rfwhost_load_obj(self._h, os.fsencode(path))
        if mesh < 0:
            raise ValueError((self._l.rfwhost_last_error(self._h) or b"").decode(errors="replace"))
        return int(mesh)

    def material(self, index):
        v, t = (C.c_float * 20)(), (C.c_int32 * 5)()
        if self._l.rfwhost_material(self._h, index, v, t) != 0:
            raise KeyError(index)
        names = ["metallic", "subsurface", "specular_f", "roughness", "specular_tint", "anisotropic", "sheen", "sheen_tint", "clearcoat", "clearcoat_gloss", "transmission", "eta"]
        out = {"color": list(v[0:4]), "specular": list(v[4:8]), **{n: v[8 + i] for i, n in enumerate(names)}}
        out.update(dict(zip(["diffuse_tex", "normal_tex", "metallic_roughness_tex", "emissive_tex", "sheen_tex"], list(t))))
        return out

    def texture(self, index):
        """Level 0 of scene texture `index` as (h, w, 4) uint8 in B, G, R, A order (what set_textures hands the backend)."""
        import numpy as np
        w, h = C.c_uint32(), C.c_uint32()
        if self._l.rfwhost_texture(self._h, index, C.byref(w), C.byref(h), None, 0) < 0:
            raise KeyError(index)
        out = np.empty((h.value, w.value, 4), np.uint8)
        self._l.rfwhost_texture(self._h, index, C.byref(w), C.byref(h), out.ctypes.data, out.nbytes)
        return out

    def save_glb(self, path):
        """Writes the scene (static meshes, instances, materials, punctual lights, camera) as a binary glTF 2.0 file."""
        if self._l.rfwhost_save_glb(self._h, os.fsencode(path)) != 0:
            raise ValueError((self._l.rfwhost_last_error(self._h) or b"").decode(errors="replace"))
        return path

    def animate(self, time):
        if self._l.rfwhost_animate(self._h, time) != 0:
            raise RuntimeError("scene has no animated instance grid")

    def pose(self, time):
        if self._l.rfwhost_pose(self._h, time) != 0:
            raise RuntimeError("scene has no skins")

    def set_animation_time(self, time):
        """Scene::set_animations_time (crates/rfw-scene/src/lib.rs:685-687): the loaded glTF graphs' animations at `time` seconds (looping):
        node TRS -> instance matrices and joint matrices, marked changed for the next sync().  Returns the number of animations."""
        return int(self._l.rfwhost_set_animation_time(self._h, float(time)))

    def set_graph_transform(self, graph, translation=(0, 0, 0), rotation=(0, 0, 0, 1), scale=(1, 1, 1)):
        """GraphHandle::get_transform() of the graph-th loaded glTF document (rotation: quaternion x, y, z, w); -1 = the latest."""
        if graph < 0:
            graph += int(self._l.rfwhost_graph_count(self._h))
        t, q, sc = (C.c_double * 3)(*translation), (C.c_double * 4)(*rotation), (C.c_double * 3)(*scale)
        if self._l.rfwhost_set_graph_transform(self._h, graph, t, q, sc) != 0:
            raise KeyError(graph)

    def instantiate_graph(self, graph=-1):
        """Scene::add_3d(&descriptor) once more: a new graph over the same meshes (new instances, new skins); returns its index."""
        if graph < 0:
            graph += int(self._l.rfwhost_graph_count(self._h))
        g = int(self._l.rfwhost_instantiate_graph(self._h, graph))
        if g < 0:
            raise KeyError(graph)
        return g

    def animation_info(self, index=0):
        d, c = C.c_double(), C.c_uint32()
        if self._l.rfwhost_animation_info(self._h, index, C.byref(d), C.byref(c)) != 0:
            raise KeyError(index)
        return {"duration": d.value, "channels": c.value}

    def skin_matrices(self, skin):
        import numpy as np
        n = self._l.rfwhost_skin_matrices(self._h, skin, None, 0)
        if n < 0:
            raise KeyError(skin)
        out = np.zeros((n, 16), np.float32)
        self._l.rfwhost_skin_matrices(self._h, skin, out.ctypes.data_as(C.POINTER(C.c_float)), n)
        return out.reshape(n, 4, 4).transpose(0, 2, 1)   # column-major storage -> [joint, row, column]

    def instance_matrix(self, mesh, slot):
        import numpy as np
        out = np.zeros(16, np.float32)
        rc = self._l.rfwhost_instance_matrix(self._h, mesh, slot, out.ctypes.data_as(C.POINTER(C.c_float)))
        if rc < 0:
            raise KeyError((mesh, slot))
        return out.reshape(4, 4).T, rc - 1                # (matrix, skin id or -1)

    def set_instance_matrix(self, mesh, slot, matrix):
        """Scene::set_matrix: `matrix` ([row, column], as instance_matrix() returns it) becomes the matrix of instance `slot` of mesh `mesh`,
        marked changed for the next sync()."""
        import numpy as np
        m = np.ascontiguousarray(np.asarray(matrix, np.float32).reshape(4, 4).T)  # column-major storage
        if self._l.rfwhost_set_instance_matrix(self._h, mesh, slot, m.ctypes.data_as(C.POINTER(C.c_float))) != 0:
            raise KeyError((mesh, slot))

    # ---- the 2D layer (matrices: 16 column-major floats, as glam's to_cols_array gives them)
    def add_2d_mesh(self, vertices, tex_id=None):
        """Scene::add_2d with a Mesh2D: vertices as HipBackend.set_2d_mesh takes them; returns the mesh id."""
        from .backend import vertices_2d
        v = vertices_2d(vertices)
        return int(self._l.rfwhost_add_2d_mesh(self._h, v.ctypes.data if len(v) else None, len(v), -1 if tex_id is None else int(tex_id)))

    def set_2d_mesh(self, mesh, vertices, tex_id=None):
        from .backend import vertices_2d
        v = vertices_2d(vertices)
        self._l.rfwhost_set_2d_mesh(self._h, mesh, v.ctypes.data if len(v) else None, len(v), -1 if tex_id is None else int(tex_id))

    def add_2d_quad(self, bottom_left, top_right, layer=0.0, tex=None, colour=(1.0, 1.0, 1.0, 1.0)):
        """Quad2D { bottom_left, top_right, layer, texture, color }.into_mesh_2d() added to the scene; returns the mesh id."""
        return int(self._l.rfwhost_add_2d_quad(self._h, (C.c_float * 2)(*bottom_left), (C.c_float * 2)(*top_right), layer, -1 if tex is None else int(tex),
                                               (C.c_float * 4)(*colour)))

    def mesh_2d(self, mesh):
        """(vertices as (n,) VERTEX_2D records, tex_id or None)"""
        import numpy as np
        from .backend import VERTEX_2D
        tex = C.c_int32(-1)
        n = self._l.rfwhost_2d_mesh(self._h, mesh, None, 0, C.byref(tex))
        if n < 0:
            raise KeyError(mesh)
        v = np.zeros(n, VERTEX_2D)
        self._l.rfwhost_2d_mesh(self._h, mesh, v.ctypes.data, n, C.byref(tex))
        return v, (None if tex.value < 0 else tex.value)

    def add_2d_instance(self, mesh, matrix):
        return int(self._l.rfwhost_add_2d_instance(self._h, mesh, (C.c_float * 16)(*[float(x) for x in matrix])))

    def set_2d_matrix(self, mesh, slot, matrix):
        if self._l.rfwhost_set_2d_matrix(self._h, mesh, slot, (C.c_float * 16)(*[float(x) for x in matrix])) != 0:
            raise KeyError((mesh, slot))

    def remove_2d_instance(self, mesh, slot):
        """the slot keeps its place and gets a zero matrix: it draws nothing"""
        if self._l.rfwhost_set_2d_matrix(self._h, mesh, slot, None) != 0:
            raise KeyError((mesh, slot))

    @staticmethod
    def camera_2d_view(width, height, scale=1.0):
        """Camera2D::from_width_height(width, height, scale).get_view().matrix as 16 column-major float32"""
        import numpy as np
        out = np.zeros(16, np.float32)
        host_lib().rfwhost_camera_2d_view(width, height, scale, out.ctypes.data_as(C.POINTER(C.c_float)))
        return out

    def set_camera(self, pos, direction, fov=40.0, aperture=0.0, aspect=1.0):
        p = (C.c_float * 3)(*pos)
        d = (C.c_float * 3)(*direction)
        self._l.rfwhost_set_camera(self._h, p, d, fov, aperture, aspect)

    def _camera_move(self, op, a, b=None):
        out = (C.c_float * 6)()
        if self._l.rfwhost_camera_move(self._h, op, (C.c_float * 3)(*a), (C.c_float * 3)(*b) if b is not None else None, out) != 0:
            raise ValueError("camera move")
        return list(out[0:3]), list(out[3:6])

    def translate_relative(self, delta):
        """Camera3D::translate_relative (camera/mod.rs:164-170); returns (position, direction)."""
        return self._camera_move(0, delta)

    def translate_target(self, delta):
        return self._camera_move(1, delta)

    def look_at(self, origin, target):
        return self._camera_move(2, origin, target)

    def set_aspect(self, aspect):
        self._l.rfwhost_set_aspect(self._h, aspect)

    def view(self, width, height):
        v = pod.CameraView3D()
        self._l.rfwhost_camera_view(self._h, width, height, C.byref(v))
        return v

    def render_system(self, width, height, scale=1.0, with_2d=False):
        """rfw::render_system for a window of width x height under `scale`, against a backend that only records what it is handed: the 3D
        view (the camera's for the RENDER size) and, with_2d, the 16 floats of the 2D view (Camera2D::from_width_height of the window)."""
        import numpy as np
        v, m = pod.CameraView3D(), np.zeros(16, np.float32)
        if self._l.rfwhost_render_system(self._h, width, height, scale, int(with_2d), C.byref(v), m.ctypes.data_as(C.POINTER(C.c_float))) != 0:
            raise RuntimeError("rfwhost_render_system: the backend was not handed exactly one frame")
        return (v, m) if with_2d else v

    def replace_mesh_with_sphere(self, mesh_id, sphere_no, seed, quality=4):
        """Mesh `mesh_id` becomes displaced sphere number `sphere_no` of the atrium (quality 4 = 5120 triangles); marked changed."""
        if self._l.rfwhost_edit(self._h, 0, mesh_id, sphere_no, quality, seed) < 0:
            raise KeyError(mesh_id)

    def remove_mesh(self, mesh_id):
        self._l.rfwhost_edit(self._h, 1, mesh_id, 0, 0, 0)

    def add_sphere_mesh(self, sphere_no, seed, quality=4):
        return int(self._l.rfwhost_edit(self._h, 2, 0, sphere_no, quality, seed))

    def recolour_material(self, index, rgb_bytes, roughness_byte):
        """Changes ONE material and marks only it changed (set_materials then carries a `changed` bit slice)."""
        seed = rgb_bytes[0] | (rgb_bytes[1] << 8) | (rgb_bytes[2] << 16)
        if self._l.rfwhost_edit(self._h, 3, index, roughness_byte, 0, seed) < 0:
            raise KeyError(index)

    def repaint_texture(self, index, seed):
        """Changes ONE texture (same size, new texels) and marks only it changed (set_textures then carries a `changed` bit slice)."""
        if self._l.rfwhost_edit(self._h, 4, index, 0, 0, seed) < 0:
            raise KeyError(index)

    def mark_all_changed(self):
        self._l.rfwhost_mark_all_changed(self._h)

    def sync(self, backend):
        t = backend.table()
        rc = self._l.rfwhost_synchronize(self._h, C.byref(t))
        if rc != 0:
            raise RuntimeError(f"synchronize_system failed: {backend.last_error()}")

    @property
    def triangle_count(self):
        return int(self._l.rfwhost_triangle_count(self._h))

    def counts(self):
        names = ["meshes", "instances", "materials", "area_lights", "point_lights", "spot_lights", "directional_lights"]
        return {n: int(self._l.rfwhost_counts(self._h, i)) for i, n in enumerate(names)}

    def mesh_data(self, mesh_id):
        d = pod.MeshData3D()
        if self._l.rfwhost_mesh_data(self._h, mesh_id, C.byref(d)) != 0:
            raise KeyError(mesh_id)
        return d


def into_device_material(color, params16):
    out = pod.DeviceMaterial()
    host_lib().rfwhost_into_device_material((C.c_float * 4)(*color), (C.c_float * 16)(*params16), C.byref(out))
    return out
