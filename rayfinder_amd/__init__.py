"""rayfinder_amd -- MI355X-native offline path-tracing core (thin Python host over the C ABI).

The product is librayfinder_amd.so (C++20 host + hand-written gfx950 HIP kernels, see
include/rayfinder_amd.h).  This package only marshals numpy arrays across the C ABI so that tests,
bench.py and torch.distributed plumbing can drive it; it mirrors the reference's seams
(src/pt/reference_path_tracer.hpp:59-76, src/pt-format/pt_format.hpp:18-43,
src/common/bvh.hpp:33, src/common/camera.hpp:24-34) by name.  No CPU fallback exists.
"""
import ctypes as C
import os

import numpy as np

from . import _ffi
from ._ffi import RayfinderError, check, lib  # noqa: F401

NODE_DTYPE = np.dtype([("min", "<f4", 3), ("pad0", "<f4"), ("max", "<f4", 3), ("pad1", "<f4"),
                       ("trianglesOffset", "<u4"), ("secondChildOffset", "<u4"),
                       ("triangleCount", "<u4"), ("splitAxis", "<u4")])
TILE = 32


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def version():
    return lib.rf_version().decode()


# ------------------------------------------------------------------------------------- camera / sky
def camera_to_array(cam):
    return np.frombuffer(bytes(cam), dtype=np.float32).copy()


def camera_from_array(a):
    cam = _ffi.Camera()
    C.memmove(C.byref(cam), _f32(a).ctypes.data, 76)
    return cam


def create_camera(origin, look_at, aperture, focus_distance, vfov_radians, aspect_ratio):
    """createCamera (src/common/camera.cpp:7-42) -> _ffi.Camera"""
    cam = _ffi.Camera()
    check(lib.rf_create_camera(_ptr(_f32(origin)), _ptr(_f32(look_at)), aperture, focus_distance, vfov_radians, aspect_ratio, C.byref(cam)))
    return cam


def fly_camera(width, height, position=(1.22, 1.25, -1.25), yaw_degrees=129.64, pitch_degrees=-13.73, vfov_degrees=70.0,
               aperture=0.0, focus_distance=10.0):
    """The interactive app's default camera (fly_camera_controller.hpp:47-52, main.cpp:49,314)."""
    cam = _ffi.Camera()
    aspect = np.float32(np.float32(width) / np.float32(height))
    check(lib.rf_fly_camera(_ptr(_f32(position)), yaw_degrees, pitch_degrees, vfov_degrees, aperture, focus_distance, aspect, C.byref(cam)))
    return cam


def bvh_visualizer_camera(nodes, aspect_ratio):
    cam = _ffi.Camera()
    check(lib.rf_bvh_visualizer_camera(_ptr(np.ascontiguousarray(nodes[:1])), np.float32(aspect_ratio), C.byref(cam)))
    return cam


def make_sky(turbidity=1.0, albedo=(1.0, 1.0, 1.0), sun_zenith_degrees=30.0, sun_azimuth_degrees=0.0):
    return _ffi.Sky(turbidity, (C.c_float * 3)(*albedo), sun_zenith_degrees, sun_azimuth_degrees)


def sky_state_new(elevation, turbidity, albedo):
    st = np.zeros(33, np.float32)
    rc = lib.rf_sky_state_new(np.float32(elevation), np.float32(turbidity), _ptr(_f32(albedo)), _ptr(st))
    return rc, st


def sky_state_radiance(state33, theta, gamma, channel):
    return np.float32(lib.rf_sky_state_radiance(_ptr(_f32(state33)), np.float32(theta), np.float32(gamma), channel))


def aligned_sky_state(sky):
    out = np.zeros(40, np.float32)
    check(lib.rf_aligned_sky_state(C.byref(sky), _ptr(out)))
    return out


def make_render_parameters(width, height, camera, spp=128, bounces=4, sky=None, exposure=1.0):
    return _ffi.RenderParameters(width, height, camera, spp, bounces, sky if sky is not None else make_sky(), exposure)


# ------------------------------------------------------------------------------------- BVH (host)
def build_bvh(positions36):
    """buildBvh (src/common/bvh.hpp:33) -> (nodes[NODE_DTYPE], triangleIndices[u64], depth)"""
    tris = _f32(positions36).reshape(-1, 9)
    n = tris.shape[0]
    nodes = np.zeros(max(2 * n, 1), dtype=NODE_DTYPE)
    idx = np.zeros(n, np.uint64)
    cnt = C.c_uint64(0)
    depth = C.c_int32(0)
    check(lib.rf_build_bvh(_ptr(tris), n, _ptr(nodes), C.byref(cnt), _ptr(idx), C.byref(depth)))
    return nodes[:cnt.value].copy(), idx, depth.value


# ------------------------------------------------------------------------------------- BVH queries on the host
INTERSECTION_DTYPE = np.dtype([("p", "<f4", 3), ("t", "<f4"), ("triangle", "<u4"), ("u", "<f4"), ("v", "<f4")])
BVH_STATS_DTYPE = np.dtype([("nodes_visited", "<u4"), ("triangle_tests", "<u4"), ("stack_high_water", "<u4")])


def _positions(tris):
    """(N, 9) f32 Positions (36 B) or (N, 12) PositionAttribute (48 B) -> (array, stride)"""
    tris = _f32(tris)
    tris = tris.reshape(-1, 12 if tris.ndim == 2 and tris.shape[1] == 12 else 9)
    return tris, tris.shape[1] * 4


def intersect_bvh(ray6, nodes, positions, t_max):
    """rayIntersectBvh (src/common/ray_intersection.hpp:43-49) on the host -> (hit: bool, intersection record, stats record)."""
    nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
    tris, stride = _positions(positions)
    out = np.zeros(1, INTERSECTION_DTYPE); st = np.zeros(1, BVH_STATS_DTYPE)
    hit = C.c_int(0)
    check(lib.rf_intersect_bvh(_ptr(_f32(ray6)), _ptr(nodes), nodes.shape[0], _ptr(tris), stride, tris.shape[0], np.float32(t_max), _ptr(out), _ptr(st), C.byref(hit)))
    return bool(hit.value), out[0], st[0]


def intersect_bvh_batch(rays6, nodes, positions, t_max, threads=0):
    """-> dict(hit u8, tri, t, uv, p, nodesVisited, triTests, stackHigh), one entry per ray; host threads, no GPU."""
    nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
    tris, stride = _positions(positions)
    rays = _f32(rays6).reshape(-1, 6)
    n = rays.shape[0]
    hit = np.zeros(n, np.uint8); out = np.zeros(n, INTERSECTION_DTYPE); st = np.zeros(n, BVH_STATS_DTYPE)
    check(lib.rf_intersect_bvh_batch(_ptr(rays), n, _ptr(nodes), nodes.shape[0], _ptr(tris), stride, tris.shape[0], np.float32(t_max), threads, _ptr(hit), _ptr(out), _ptr(st)))
    return dict(hit=hit, tri=out["triangle"].copy(), t=out["t"].copy(), uv=np.stack([out["u"], out["v"]], axis=1), p=out["p"].copy(),
                nodesVisited=st["nodes_visited"].copy(), triTests=st["triangle_tests"].copy(), stackHigh=st["stack_high_water"].copy())


def bvh_visualizer_pass(camera, width, height, nodes, positions, threads=0, row_begin=0, row_end=None):
    """The bvh-visualizer pixel loop (src/bvh-visualizer/main.cpp:60-78) on the host; the CPU twin of
    ReferencePathTracer.trace_primary_stats -> dict(nodesVisited, hit, t, triTests), each width*height."""
    nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
    tris, stride = _positions(positions)
    n = width * height
    nv = np.zeros(n, np.uint32); hit = np.zeros(n, np.uint8); t = np.zeros(n, np.float32); tt = np.zeros(n, np.uint32)
    check(lib.rf_bvh_visualizer_pass(C.byref(camera), width, height, row_begin, height if row_end is None else row_end, _ptr(nodes), nodes.shape[0], _ptr(tris), stride,
                                     tris.shape[0], threads, _ptr(nv), _ptr(hit), _ptr(t), _ptr(tt)))
    return dict(nodesVisited=nv, hit=hit, t=t, triTests=tt)


def bvh_visualizer_grey(nodes_visited):
    """src/bvh-visualizer/main.cpp:73-76: grey level u32(min(0.01f * nodesVisited, 1) * 255) per pixel (f32 arithmetic)."""
    x = np.float32(0.01) * np.asarray(nodes_visited).astype(np.float32)
    return (np.minimum(x, np.float32(1.0)) * np.float32(255.0)).astype(np.uint32).astype(np.uint8)


def check_wide_layouts(nodes):
    """rf_check_wide_layouts: the render path's record layouts of a flattened tree decode to the same child planes (host only).
    -> {"regular": bool, "compact": bool, "hot": bool}; raises on a mismatch."""
    nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
    flags = C.c_uint32(0)
    check(lib.rf_check_wide_layouts(_ptr(nodes), nodes.shape[0], C.byref(flags)))
    return {"regular": bool(flags.value & 1), "compact": bool(flags.value & 2), "hot": bool(flags.value & 4), "quad": bool(flags.value & 8), "quad_half": bool(flags.value & 16), "quad_local": bool(flags.value & 32), "oct": bool(flags.value & 64)}


def wide_layout_stats(nodes):
    """Flags of check_wide_layouts plus the surface-area ratio of the half-precision quad boxes (the renderer uses them by default
    closest-hit: half-precision records up to 1.075, local-grid beyond; shadow: local-grid up to 1.10, exact beyond)."""
    nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
    flags = C.c_uint32(0); ratio = C.c_float(0.0)
    check(lib.rf_wide_layout_stats(_ptr(nodes), nodes.shape[0], C.byref(flags), C.byref(ratio)))
    return {"flags": flags.value, "quad_half_area_ratio": float(ratio.value)}


def texture_from_memory(data):
    """Texture::fromMemory (texture.cpp:12-54): PNG / JPEG bytes -> (BGRA u32 texels [h*w], width, height)."""
    buf = np.frombuffer(bytes(data), np.uint8)
    w, h = C.c_uint32(0), C.c_uint32(0)
    check(lib.rf_texture_from_memory(_ptr(buf), buf.size, C.byref(w), C.byref(h), None))
    px = np.zeros(w.value * h.value, np.uint32)
    check(lib.rf_texture_from_memory(_ptr(buf), buf.size, C.byref(w), C.byref(h), _ptr(px)))
    return px, w.value, h.value


def set_bake_bvh_builder(gpu_device=None):
    """BVH builder of PtFormat.from_gltf / from_triangles: None = host (default), int = GPU builder on that device."""
    check(lib.rf_pt_format_set_bvh_builder(-1 if gpu_device is None else int(gpu_device)))


def build_bvh_gpu(positions36, device_ordinal=0):
    """GPU build of the same tree (rf_bvh_gpu.hip) -> (nodes, triangleIndices, depth, build_ms)."""
    tris = _f32(positions36).reshape(-1, 9)
    n = tris.shape[0]
    nodes = np.zeros(max(2 * n, 1), dtype=NODE_DTYPE)
    idx = np.zeros(n, np.uint64)
    cnt = C.c_uint64(0)
    depth = C.c_int32(0)
    ms = C.c_float(0)
    check(lib.rf_build_bvh_gpu(_ptr(tris), n, _ptr(nodes), C.byref(cnt), _ptr(idx), C.byref(depth), device_ordinal, C.byref(ms)))
    return nodes[:cnt.value].copy(), idx, depth.value, ms.value


def tiles_for_rank(width, height, rank, world_size):
    n = C.c_uint32(0)
    check(lib.rf_tiles_for_rank(width, height, rank, world_size, None, C.byref(n)))
    tiles = np.zeros(n.value, np.uint32)
    check(lib.rf_tiles_for_rank(width, height, rank, world_size, _ptr(tiles), C.byref(n)))
    return tiles


def untile(compact, tile_ids, width, height, image=None):
    """compact: (numTiles*1024, 4) f32 tile-major -> (H, W, 4) row-major (other pixels untouched)."""
    compact = _f32(compact).reshape(-1, 4)
    tile_ids = np.ascontiguousarray(tile_ids, np.uint32)
    if image is None:
        image = np.zeros((height, width, 4), np.float32)
    check(lib.rf_untile(_ptr(compact), _ptr(tile_ids), tile_ids.size, width, height, _ptr(image)))
    return image


# ------------------------------------------------------------------------------------- .pt files
class PtFormat:
    """nlrs::PtFormat (src/pt-format/pt_format.hpp:18-43) held by the native library."""

    def __init__(self, handle):
        self._h = C.c_void_p(handle)

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.rf_pt_format_destroy(self._h)
            self._h = None

    @classmethod
    def from_gltf(cls, path):
        h = C.c_void_p()
        check(lib.rf_pt_format_from_gltf(str(path).encode(), C.byref(h)))
        return cls(h.value)

    @classmethod
    def load(cls, path):
        h = C.c_void_p()
        check(lib.rf_pt_format_load(str(path).encode(), C.byref(h)))
        return cls(h.value)

    @classmethod
    def deserialize(cls, data):
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        h = C.c_void_p()
        check(lib.rf_pt_format_deserialize(_ptr(buf), buf.size, C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_triangles(cls, positions36, normals36, tex_coords24, texture_indices, textures):
        """textures: list of (pixels u32 array, width, height)"""
        p = _f32(positions36).reshape(-1, 9)
        n = _f32(normals36).reshape(-1, 9)
        t = _f32(tex_coords24).reshape(-1, 6)
        ti = np.ascontiguousarray(texture_indices, np.uint32)
        keep = [np.ascontiguousarray(px, np.uint32) for px, _, _ in textures]
        arr = (_ffi.Texture * max(len(textures), 1))()
        for i, (px, w, h) in enumerate(textures):
            arr[i] = _ffi.Texture(keep[i].ctypes.data, w, h)
        h = C.c_void_p()
        check(lib.rf_pt_format_from_triangles(_ptr(p), _ptr(n), _ptr(t), _ptr(ti), p.shape[0], arr, len(textures), C.byref(h)))
        return cls(h.value)

    def save(self, path):
        check(lib.rf_pt_format_save(self._h, str(path).encode()))

    def serialize(self):
        size = C.c_uint64(0)
        check(lib.rf_pt_format_serialize(self._h, None, C.byref(size)))
        buf = np.zeros(size.value, np.uint8)
        check(lib.rf_pt_format_serialize(self._h, _ptr(buf), C.byref(size)))
        return buf.tobytes()

    def view(self):
        v = _ffi.PtFormatView()
        check(lib.rf_pt_format_view_get(self._h, C.byref(v)))
        return v

    def _array(self, ptr, count, dtype, cols=None):
        if count == 0:
            return np.zeros((0,) if cols is None else (0, cols), dtype)
        dt = np.dtype(dtype)
        n = count * (cols or 1)
        a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n * dt.itemsize,)).view(dt).copy()
        return a if cols is None else a.reshape(count, cols)

    def arrays(self):
        """Copies of every array as numpy (names as in the reference struct)."""
        v = self.view()
        out = dict(
            bvhNodes=self._array(v.bvh_nodes, v.num_bvh_nodes, NODE_DTYPE),
            bvhPositionAttributes=self._array(v.bvh_position_attributes, v.num_bvh_position_attributes, np.float32, 9),
            trianglePositionAttributes=self._array(v.triangle_position_attributes, v.num_triangle_position_attributes, np.float32, 12),
            triangleVertexAttributes=self._array(v.triangle_vertex_attributes, v.num_triangle_vertex_attributes, np.float32, 20),
            vertexPositions=self._array(v.vertex_positions, v.num_vertex_positions, np.float32, 4),
            vertexNormals=self._array(v.vertex_normals, v.num_vertex_normals, np.float32, 4),
            vertexTexCoords=self._array(v.vertex_tex_coords, v.num_vertex_tex_coords, np.float32, 2),
            vertexIndices=self._array(v.vertex_indices, v.num_vertex_indices, np.uint32),
            modelVertexPositions=self._array(v.model_vertex_positions, v.num_model_vertex_positions, np.uint64, 2),
            modelVertexNormals=self._array(v.model_vertex_normals, v.num_model_vertex_normals, np.uint64, 2),
            modelVertexTexCoords=self._array(v.model_vertex_tex_coords, v.num_model_vertex_tex_coords, np.uint64, 2),
            modelVertexIndices=self._array(v.model_vertex_indices, v.num_model_vertex_indices, np.uint64, 2),
            modelBaseColorTextureIndices=self._array(v.model_base_color_texture_indices, v.num_model_base_color_texture_indices, np.uint32),
        )
        out["baseColorTextures"] = [self.texture(i) for i in range(v.num_textures)]
        return out

    def texture(self, i):
        t = _ffi.Texture()
        check(lib.rf_pt_format_texture(self._h, i, C.byref(t)))
        px = self._array(t.pixels, t.width * t.height, np.uint32)
        return px, t.width, t.height

    def scene(self):
        """nlrs::Scene spans (src/pt/main.cpp:150-157); valid while this PtFormat is alive."""
        v = self.view()
        textures = (_ffi.Texture * max(int(v.num_textures), 1))()
        sc = _ffi.Scene()
        check(lib.rf_pt_format_scene(self._h, C.byref(sc), textures))
        sc._keepalive = (textures, self)
        return sc


def scene_from_arrays(nodes, positions48, attrs80, textures):
    """Build an rf_scene from numpy arrays; textures = list of (pixels u32, w, h)."""
    nodes = np.ascontiguousarray(nodes)
    pos = _f32(positions48).reshape(-1, 12)
    att = np.ascontiguousarray(attrs80, dtype=np.float32).reshape(-1, 20)
    keep = [np.ascontiguousarray(px, np.uint32) for px, _, _ in textures]
    arr = (_ffi.Texture * max(len(textures), 1))()
    for i, (px, w, h) in enumerate(textures):
        arr[i] = _ffi.Texture(keep[i].ctypes.data, w, h)
    sc = _ffi.Scene(nodes.ctypes.data, nodes.shape[0], pos.ctypes.data, att.ctypes.data, pos.shape[0], arr, len(textures))
    sc._keepalive = (nodes, pos, att, keep, arr)
    return sc


# ------------------------------------------------------------------------------------- multi-GPU frame exchange
RF_GATHER_LOOPBACK = 1
RF_GATHER_AOVS = 2      # with the image: plane 1 = {albedo.rgb, coverage}, plane 2 = {normal.xyz, depth}
RF_GATHER_MOMENTS = 4   # with the image: plane 3 = the radiance second moments
RF_GATHER_TILE_COUNTS = 8   # with the image: one sample count per tile (TileComm.render_adaptive)
RF_GATHER_ROBUST_MEAN = 16  # with the image: plane 4 = the robust mean of every rank's own pixels {M.rgb, float(trim)}, combined before the exchange
RF_GATHER_DIRECT = 32       # with the image: plane 5 = the direct radiance sums D (set_direct)


def _gather_flags(loopback=False, aovs=False, moments=False, tile_counts=False, robust_mean=False, direct=False):
    return ((RF_GATHER_LOOPBACK if loopback else 0) | (RF_GATHER_AOVS if aovs else 0) | (RF_GATHER_MOMENTS if moments else 0) | (RF_GATHER_TILE_COUNTS if tile_counts else 0)
            | (RF_GATHER_ROBUST_MEAN if robust_mean else 0) | (RF_GATHER_DIRECT if direct else 0))


class _GatheredPlanes(dict):
    """TileComm.gathered_planes()'s dict.  The flags that came later, tile_counts, robust_mean and direct, are ABSENT WHEN FALSE: they are stored only when the gather carried
    them, so a gather without them still compares equal to the dict it always gave.  Only the subscript reads an absent one as False (g["robust_mean"]); `in`, .get()
    and iteration see the keys that are stored, and dict(g) is a plain dict without this.  Prefer g.get("robust_mean", False) in new code."""

    def __missing__(self, key):
        if key in ("tile_counts", "robust_mean", "direct"):
            return False
        raise KeyError(key)


def gather_layout(width, height, world_size):
    """Staging layout of the frame-end gather: (rank_first_tile[world+1], tile_slot[tiles], tile_owner[tiles])."""
    n = ((width + 31) // 32) * ((height + 31) // 32)
    first = np.zeros(world_size + 1, np.uint32); slot = np.zeros(n, np.uint32); owner = np.zeros(n, np.uint32)
    check(lib.rf_gather_layout(width, height, world_size, _ptr(first), _ptr(slot), _ptr(owner)))
    return first, slot, owner


def gather_plan(width, height, world_size, rank, root=0, loopback=False):
    """The point-to-point operations `rank` posts for a frame-end gather to `root` (what rf_renderer_gather_frame executes):
    (n, 4) u32 rows {is_send, peer, offset_tiles, count_tiles}.  Host arithmetic, no GPU."""
    n = C.c_uint32(0)
    flags = RF_GATHER_LOOPBACK if loopback else 0
    check(lib.rf_gather_plan(width, height, world_size, rank, root, flags, None, C.byref(n)))
    ops = np.zeros((n.value, 4), np.uint32)
    check(lib.rf_gather_plan(width, height, world_size, rank, root, flags, _ptr(ops), C.byref(n)))
    return ops


def gather_plan_planes(width, height, world_size, rank, root=0, loopback=False, aovs=False, moments=False, robust_mean=False, direct=False):
    """gather_plan for a gather that also carries the AOV sums (planes 1, 2), the second moments (plane 3), the robust mean (plane 4) and / or the direct sums
    (plane 5) in the one group: (n, 5) u32 rows {is_send, peer, plane, offset_tiles, count_tiles}; offsets count from the start of the plane's own staging area /
    compact buffer.  direct=True: the list without it, followed by gather_plan's rows tagged plane 5.  Host arithmetic, no GPU."""
    n = C.c_uint32(0)
    flags = _gather_flags(loopback, aovs, moments, robust_mean=robust_mean, direct=direct)
    check(lib.rf_gather_plan_planes(width, height, world_size, rank, root, flags, None, C.byref(n)))
    ops = np.zeros((n.value, 5), np.uint32)
    check(lib.rf_gather_plan_planes(width, height, world_size, rank, root, flags, _ptr(ops), C.byref(n)))
    return ops


def gather_plan_counts(width, height, world_size, rank, root=0, loopback=False):
    """The operations a gather with tile_counts=True posts for the per-tile sample counts, behind those of its planes: (n, 4) u32 rows
    {is_send, peer, offset_words, count_words}, one u32 word per tile.  Host arithmetic, no GPU."""
    n = C.c_uint32(0)
    flags = RF_GATHER_LOOPBACK if loopback else 0
    check(lib.rf_gather_plan_counts(width, height, world_size, rank, root, flags, None, C.byref(n)))
    ops = np.zeros((n.value, 4), np.uint32)
    check(lib.rf_gather_plan_counts(width, height, world_size, rank, root, flags, _ptr(ops), C.byref(n)))
    return ops


def device_count():
    """hipGetDeviceCount as the library sees it (0 without a GPU)."""
    n = C.c_int32(0)
    check(lib.rf_device_count(C.byref(n)))
    return n.value


def comm_unique_id():
    """ncclGetUniqueId: 128 bytes that rank 0 hands to the other ranks before TileComm(...)."""
    buf = np.zeros(128, np.uint8)
    check(lib.rf_comm_unique_id(_ptr(buf)))
    return buf.tobytes()


class TileComm:
    """One RCCL communicator per rank (one process per GPU); collective constructor."""

    def __init__(self, unique_id, rank, world_size, device_ordinal=0):
        buf = np.frombuffer(bytes(unique_id), np.uint8).copy()
        assert buf.size == 128
        self._h = C.c_void_p()
        self.rank, self.world_size = rank, world_size
        check(lib.rf_comm_create(_ptr(buf), rank, world_size, device_ordinal, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.rf_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def info(self):
        """What RCCL reports for this communicator: dict(rccl_ranks, rccl_rank, device)."""
        n, r, d = C.c_uint32(0), C.c_uint32(0), C.c_int32(0)
        check(lib.rf_comm_info(self._h, C.byref(n), C.byref(r), C.byref(d)))
        return dict(rccl_ranks=n.value, rccl_rank=r.value, device=d.value)

    def local_transport(self):
        """True: this communicator runs on the local TEST transport (RF_COMM_TRANSPORT=local when its id was made), not on RCCL."""
        v = C.c_uint32(0)
        check(lib.rf_comm_transport(self._h, C.byref(v)))
        return bool(v.value)

    def last_exchange_ms(self):
        """Device time of this rank's last gather_frame (HIP events around the sends / receives + the root's un-tile); -1 before the first."""
        v = C.c_double(-1.0)
        check(lib.rf_comm_last_exchange_ms(self._h, C.byref(v)))
        return v.value

    def read_frame(self, renderer, width, height):
        """Root: the gathered row-major (H, W, 4) float image."""
        img = np.zeros((height, width, 4), np.float32)
        check(lib.rf_comm_read_frame(self._h, renderer._h, _ptr(img)))
        return img

    def all_reduce_max(self, value, renderer=None):
        v = C.c_double(value)
        check(lib.rf_comm_all_reduce_max(self._h, renderer._h if renderer is not None else None, C.byref(v)))
        return v.value

    # the root's side of a gather that carried more than the image (Renderer.gather_frame(..., aovs=True, moments=True)); every call is refused on another rank,
    # before any gather, and when the last gather did not carry the planes it needs
    def gathered_planes(self):
        """What the last gather left on this (root) rank: dict(aovs, moments, width, height, samples), and tile_counts / robust_mean = True when it carried them
        (looked up after a gather without them: False)."""
        f, w, h, n = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        check(lib.rf_comm_gathered_planes(self._h, C.byref(f), C.byref(w), C.byref(h), C.byref(n)))
        out = _GatheredPlanes(aovs=bool(f.value & RF_GATHER_AOVS), moments=bool(f.value & RF_GATHER_MOMENTS), width=w.value, height=h.value, samples=n.value)
        if f.value & RF_GATHER_TILE_COUNTS:                                   # (a key of its own, and only then: a gather without counts reports what it always did)
            out["tile_counts"] = True
        if f.value & RF_GATHER_ROBUST_MEAN:
            out["robust_mean"] = True
        if f.value & RF_GATHER_DIRECT:
            out["direct"] = True
        return out

    def read_plane(self, renderer, plane):
        """Root: the gathered row-major (H, W, 4) f32 sums of plane 0 = S, 1 = {albedo, coverage}, 2 = {normal, depth}, 3 = the second moments, 5 = the direct sums
        (plane 4, the robust mean, is read through read_robust_mean)."""
        g = self.gathered_planes()
        img = np.zeros((g["height"], g["width"], 4), np.float32)
        check(lib.rf_comm_read_plane(self._h, renderer._h, plane, _ptr(img)))
        return img

    def denoise(self, renderer, params=None):
        """Root: the a-trous denoiser over the gathered image and AOV sums, in device memory, on the renderer's stream.  params: a dict of iterations, sigma_color,
        sigma_normal, sigma_depth (the rest, or None: the defaults)."""
        check(lib.rf_comm_denoise(self._h, renderer._h, C.byref(_denoise_parameters(dict(params or {})))))

    def read_denoised(self, renderer):
        """-> (rgb (H,W,3) f32 denoised mean, bgra (H,W) u32 display texels under the renderer's exposure, the sample count of the gathered sums)"""
        g = self.gathered_planes()
        rgba = np.zeros((g["height"], g["width"], 4), np.float32)
        bgra = np.zeros((g["height"], g["width"]), np.uint32)
        n = C.c_uint32(0)
        check(lib.rf_comm_read_denoised(self._h, renderer._h, _ptr(rgba), _ptr(bgra), C.byref(n)))
        return rgba[..., :3], bgra, n.value

    def noise_estimate(self, renderer, maps=True):
        """Root: the noise estimate over the gathered image and second moments (needs >= 2 samples).  -> the dict of ReferencePathTracer.noise_estimate; maps=False:
        the scalars alone (error_map, tile_sum, tile_max are None and are not computed / copied)."""
        g = self.gathered_planes()
        est = _ffi.NoiseEstimate()
        emap = tsum = tmax = None
        if maps:
            emap = np.zeros((g["height"], g["width"]), np.float32)
            tsum = np.zeros(_noise_tiles(g["width"], g["height"]), np.float32); tmax = np.zeros_like(tsum)
        check(lib.rf_comm_noise_estimate(self._h, renderer._h, C.byref(est), _ptr(emap) if maps else None, _ptr(tsum) if maps else None, _ptr(tmax) if maps else None))
        return _noise_result(est, emap, tsum, tmax)


    # tile-adaptive sampling across the ranks of the communicator (include/rayfinder_amd.h: "TILE-ADAPTIVE SAMPLING ACROSS RANKS")
    def render_adaptive(self, renderer, target_tile_error, check_every=8, min_samples=0, max_samples=0):
        """ReferencePathTracer.render_adaptive for a frame whose tiles are dealt to the ranks: COLLECTIVE, the same parameters on every rank; renderer's tile shard is
        this communicator's (rank, world_size).  Every tile ends with the count and the sums one un-sharded handle gives it.
        -> dict(rank: render_adaptive's dict over this rank's tiles (stopped_tiles: below the frame's leading count), frame_leading_samples, frame_min_tile_samples,
        max_rank_pixel_samples).  While the two frame counts differ, gather with tile_counts=True.  Refused while the bucket sums are on, unless they were set with
        set_buckets(k, tile_counts=True, shard=True): the bucket planes of every tile are then the un-sharded handle's too."""
        p = _ffi.AdaptiveParameters(target_tile_error, check_every, min_samples, max_samples)
        res = _ffi.CommAdaptiveResult()
        check(lib.rf_comm_render_adaptive(self._h, renderer._h, C.byref(p), C.byref(res)))
        rank = {k: getattr(res.rank, k) for k, _ in res.rank._fields_ if k not in ("reserved", "last")}
        rank["last"] = {k: getattr(res.rank.last, k) for k, _ in res.rank.last._fields_} if res.rank.last.samples else None
        return dict(rank=rank, frame_leading_samples=res.frame_leading_samples, frame_min_tile_samples=res.frame_min_tile_samples,
                    max_rank_pixel_samples=res.max_rank_pixel_samples)

    def read_tile_samples(self):
        """Root, after a gather with tile_counts=True: (tiles_y, tiles_x) u32, the sample count of every 32x32 tile of the frame."""
        g = self.gathered_planes()
        counts = np.zeros(((g["height"] + TILE - 1) // TILE, (g["width"] + TILE - 1) // TILE), np.uint32)
        n = C.c_uint32(0)
        check(lib.rf_comm_read_tile_samples(self._h, _ptr(counts), C.byref(n)))
        assert n.value == counts.size
        return counts

    def read_mean(self, renderer):
        """Root, after a gather with tile_counts=True: (H, W, 4) f32 {sum.rgb / the tile's sample count, 1}."""
        g = self.gathered_planes()
        mean = np.zeros((g["height"], g["width"], 4), np.float32)
        check(lib.rf_comm_read_mean(self._h, renderer._h, _ptr(mean)))
        return mean

    # the robust mean of the sharded frame (include/rayfinder_amd.h: "ROBUST MEAN ACROSS RANKS"): every rank combined its own pixels before the exchange
    def read_robust_mean(self, renderer):
        """Root, after a gather with robust_mean=True: the dict of ReferencePathTracer.read_robust_mean (mean, bgra8 under the renderer's exposure, trim, samples: the
        N the gather recorded) plus K, as the gather left them."""
        g = self.gathered_planes()
        h, w = g["height"], g["width"]
        rgba = np.zeros((h, w, 4), np.float32)
        bgra = np.zeros((h, w), np.uint32)
        trim = np.zeros((h, w), np.uint8)
        k, n = C.c_uint32(0), C.c_uint32(0)
        check(lib.rf_comm_read_robust_mean(self._h, renderer._h, _ptr(rgba), _ptr(bgra), _ptr(trim), C.byref(k), C.byref(n)))
        return dict(mean=rgba[..., :3], bgra8=bgra, trim=trim, samples=n.value, K=k.value)

    def denoise_robust(self, renderer, params=None):
        """Root: denoise with the gathered robust mean in place of the plain mean (the gather needs aovs=True and robust_mean=True); read_denoised reads the result.
        params as for denoise."""
        check(lib.rf_comm_denoise_robust(self._h, renderer._h, C.byref(_denoise_parameters(dict(params or {})))))

    # the direct sums of the sharded frame (include/rayfinder_amd.h: "DIRECT SUMS ACROSS RANKS"): plane 5 of a gather with direct=True
    def denoise_split(self, renderer, direct=None, indirect=None):
        """Root: the split-component denoiser over the gathered S, D and AOV sums, in device memory, on the renderer's stream (the gather needs aovs=True and
        direct=True; with tile_counts=True every pixel is divided by its tile's count); read_denoised reads the result.  direct / indirect as for
        ReferencePathTracer.denoise_split."""
        pd, pi = _split_parameters(direct, indirect)
        check(lib.rf_comm_denoise_split(self._h, renderer._h, C.byref(pd), C.byref(pi)))

    def read_split(self, renderer):
        """Root, after a gather with direct=True: ((H, W, 4) f32 {D.rgb / n, 1}, (H, W, 4) f32 {(S.rgb - D.rgb) / n, 1}), the direct and the indirect light as means;
        n = the gathered sample count, or the pixel's tile's count after a gather with tile_counts=True ({0, 0, 0, 1} in a tile without a sample)."""
        g = self.gathered_planes()
        direct = np.zeros((g["height"], g["width"], 4), np.float32)
        indirect = np.zeros_like(direct)
        check(lib.rf_comm_read_split(self._h, renderer._h, _ptr(direct), _ptr(indirect)))
        return direct, indirect


    def export_features(self, renderer, channels=("color", "albedo", "normal", "depth"), layout="chw", dtype="f32", out=None):
        """Root: ReferencePathTracer.export_features over the gathered planes where they lie (the gather needs the planes the channels read: aovs, moments, direct; with
        tile_counts=True every pixel takes its tile's count) -> torch tensor on the communicator's device, bit for bit what the un-sharded handle's export gives."""
        req, count = _feature_request(channels, layout, dtype)
        g = self.gathered_planes()
        device = C.c_int32(0)
        check(lib.rf_comm_info(self._h, None, None, C.byref(device)))
        shape = (count, g["height"], g["width"]) if layout == "chw" else (g["height"], g["width"], count)
        out = _feature_tensor("TileComm.export_features", out, shape, dtype, device.value)
        check(lib.rf_comm_export_features(self._h, renderer._h, C.byref(req), C.c_void_p(out.data_ptr()), out.numel() * out.element_size(), None))
        return out


# ------------------------------------------------------------------------------------- feature export
def feature_channels(mask_or_names):
    """-> (channel names in output order, C) of a feature request: an RF_FEATURE_* mask, one group name or an iterable of group names out of color, albedo, normal,
    depth, coverage, direct, indirect, variance, error, samples.  The output order is the groups' bit order whatever the order given; a group of three gives
    name.r / .g / .b (normal: .x / .y / .z).  ValueError for an empty or unknown selection."""
    names, _, count = _feature_selection(mask_or_names)
    return names, count


def _feature_selection(mask_or_names):
    bits = {name: bit for name, bit, _ in _ffi.FEATURE_GROUPS}
    if isinstance(mask_or_names, (int, np.integer)) and not isinstance(mask_or_names, bool):
        mask = int(mask_or_names)
    else:
        groups = (mask_or_names,) if isinstance(mask_or_names, str) else tuple(mask_or_names)
        unknown = [g for g in groups if g not in bits]
        if unknown:
            raise ValueError(f"unknown feature channels {unknown}: choose from {[g for g, _, _ in _ffi.FEATURE_GROUPS]}")
        mask = 0
        for g in groups:
            mask |= bits[g]
    if mask <= 0 or mask & ~sum(bits.values()):
        raise ValueError("feature channels: the selection is empty or holds unknown RF_FEATURE_* bits")
    names = []
    for name, bit, n in _ffi.FEATURE_GROUPS:
        if mask & bit:
            names += [name] if n == 1 else [f"{name}.{c}" for c in ("xyz" if name == "normal" else "rgb")]
    count = C.c_uint32(0)
    check(lib.rf_feature_channel_count(mask, C.byref(count)))
    assert count.value == len(names)
    return tuple(names), mask, count.value


def _feature_request(channels, layout, dtype):
    _, mask, count = _feature_selection(channels)
    layouts = {"chw": _ffi.RF_FEATURES_CHW, "hwc": _ffi.RF_FEATURES_HWC}
    dtypes = {"f32": _ffi.RF_FEATURES_F32, "f16": _ffi.RF_FEATURES_F16}
    if layout not in layouts:
        raise ValueError(f"feature layout {layout!r}: 'chw' or 'hwc'")
    if dtype not in dtypes:
        raise ValueError(f"feature dtype {dtype!r}: 'f32' or 'f16'")
    return _ffi.FeatureRequest(mask, layouts[layout], dtypes[dtype], 0), count


def _feature_tensor(what, out, shape, dtype, device_ordinal):
    """The destination of an export: a new torch tensor on the device, or the caller's `out` once its device, dtype, shape and contiguity have been checked (a storage
    offset is fine: the library needs element alignment only)."""
    import torch
    tdtype = torch.float16 if dtype == "f16" else torch.float32
    if out is None:
        return torch.empty(shape, dtype=tdtype, device=torch.device("cuda", device_ordinal))
    if not isinstance(out, torch.Tensor):
        raise TypeError(f"{what}: out must be a torch.Tensor")
    if out.device.type != "cuda" or (out.device.index or 0) != device_ordinal:
        raise ValueError(f"{what}: out lies on {out.device}, the sums on cuda:{device_ordinal}")
    if out.dtype != tdtype:
        raise ValueError(f"{what}: out is {out.dtype}, the request asks for {tdtype}")
    if tuple(out.shape) != tuple(shape):
        raise ValueError(f"{what}: out has shape {tuple(out.shape)}, the request gives {tuple(shape)}")
    if not out.is_contiguous():
        raise ValueError(f"{what}: out must be contiguous")
    return out


# ------------------------------------------------------------------------------------- rays from device tensors
def _ray_tensor(what, name, t):
    """One input of cast_rays / cast_occlusion, checked before the library is called: a float32 tensor (N, 3) whose rows are 3 consecutive floats at a row stride of
    at least 3 (a contiguous (N, 3) tensor, either half of an (N, 6) one, rows with padding).  -> the row stride in floats.  (Its device: _ray_device)"""
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a torch.Tensor")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} is {t.dtype}, the rays are torch.float32")
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, the rays are (N, 3)")
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < 3):
        raise ValueError(f"{what}: {name} has strides {tuple(t.stride())}: a row is 3 consecutive floats, rows at least 3 floats apart")
    return int(t.stride(0)) if t.shape[0] > 1 else 3


def _ray_device(what, name, t, device_ordinal):
    if t.device.type != "cuda" or (t.device.index or 0) != device_ordinal:
        raise ValueError(f"{what}: {name} lies on {t.device}, the scene on cuda:{device_ordinal}")


def _ray_output(what, name, out, n):
    """The type, dtype, shape and contiguity of a caller's output tensor (as _feature_tensor checks an export's destination; a storage offset is fine), or
    None -> (dtype, shape) of the tensor to make"""
    import torch
    width, kind = {o[0]: (o[2], o[3]) for o in _ffi.RAY_OUTPUTS}[name]
    # (uint32 words travel as int32 tensors: -1 is the miss word 0xFFFFFFFF)
    tdtype, shape = (torch.float32 if kind == "f" else torch.int32), ((n,) if width == 1 else (n, width))
    if out is None:
        return tdtype, shape
    if not isinstance(out, torch.Tensor):
        raise TypeError(f"{what}: out[{name!r}] must be a torch.Tensor")
    if out.dtype != tdtype:
        raise ValueError(f"{what}: out[{name!r}] is {out.dtype}, {name} is {tdtype}")
    if tuple(out.shape) != shape:
        raise ValueError(f"{what}: out[{name!r}] has shape {tuple(out.shape)}, {name} of {n} rays is {shape}")
    if not out.is_contiguous():
        raise ValueError(f"{what}: out[{name!r}] must be contiguous")
    return tdtype, shape


def _ray_batch(what, origins, directions, t_max, kind, names, out, device_ordinal):
    """-> (the rf_ray_batch of a call, its output tensors by name); every check that needs no library call: the names, the tensors' layouts, then their devices"""
    import torch
    known = [o[0] for o in _ffi.RAY_OUTPUTS if o[1] == kind]
    names = (names,) if isinstance(names, str) else tuple(names)
    unknown = [n for n in names if n not in known]
    if unknown or not names or len(set(names)) != len(names):
        raise ValueError(f"{what}: outputs {list(names)}: choose one or more of {known}, each once")
    so, sd = _ray_tensor(what, "origins", origins), _ray_tensor(what, "directions", directions)
    if origins.shape[0] != directions.shape[0]:
        raise ValueError(f"{what}: {origins.shape[0]} origins, {directions.shape[0]} directions")
    t_max = float(t_max)
    if t_max != t_max:
        raise ValueError(f"{what}: t_max is NaN")
    if out is not None and not isinstance(out, dict):
        raise TypeError(f"{what}: out must be a dict of torch tensors by output name")
    if out is not None and set(out) - set(names):
        raise ValueError(f"{what}: out holds {sorted(set(out) - set(names), key=str)}, which outputs={list(names)} does not ask for")
    n = int(origins.shape[0])
    given = {name: None if out is None else out.get(name) for name in names}
    made = {name: _ray_output(what, name, given[name], n) for name in names}
    _ray_device(what, "origins", origins, device_ordinal)
    _ray_device(what, "directions", directions, device_ordinal)
    for name in names:
        if given[name] is not None:
            _ray_device(what, f"out[{name!r}]", given[name], device_ordinal)
    tensors = {name: given[name] if given[name] is not None else torch.empty(made[name][1], dtype=made[name][0], device=torch.device("cuda", device_ordinal)) for name in names}
    batch = _ffi.RayBatch()
    batch.origins, batch.directions, batch.origin_stride, batch.direction_stride = origins.data_ptr(), directions.data_ptr(), so, sd
    batch.num_rays, batch.t_max, batch.kind = n, t_max, kind
    for name, t in tensors.items():
        setattr(batch, name, t.data_ptr())
    return batch, tensors


def export_features_images(color_sum=None, sumsq=None, albedo_coverage=None, normal_depth=None, direct_sum=None, samples=0, tile_samples=None,
                           channels=("color", "albedo", "normal", "depth"), layout="chw", dtype="f32", device_ordinal=0):
    """rf_export_features_images: the feature export over (H, W, 4) f32 sums held on the host -- the accumulation S, the second moments Q, {albedo, coverage},
    {normal, depth} and the direct sums D; one that no selected channel reads may be None -- of `samples` samples, or with one count per 32x32 tile (tile_samples in
    tile order, as denoise_tiles takes them).  -> numpy (C, H, W) or (H, W, C) array of float32 / float16."""
    req, count = _feature_request(channels, layout, dtype)
    given = [a for a in (color_sum, sumsq, albedo_coverage, normal_depth, direct_sum) if a is not None]
    if not given:
        raise ValueError("export_features_images: no sum was given (the frame size comes from the sums; samples alone needs color_sum too)")
    planes = [None if a is None else _f32(a) for a in (color_sum, sumsq, albedo_coverage, normal_depth, direct_sum)]
    h, w = _f32(given[0]).shape[:2]
    for a in planes:
        if a is not None and a.shape != (h, w, 4):
            raise ValueError("export_features_images: the sums must be (H, W, 4) arrays of one size")
    counts = None
    if tile_samples is not None:
        counts = np.ascontiguousarray(tile_samples, np.uint32).reshape(-1)
        if counts.size != _noise_tiles(w, h):
            raise ValueError(f"export_features_images: {_noise_tiles(w, h)} tile counts expected, got {counts.size}")
    out = np.zeros((count, h, w) if layout == "chw" else (h, w, count), np.float16 if dtype == "f16" else np.float32)
    check(lib.rf_export_features_images(device_ordinal, w, h, int(samples), _ptr(counts), *(_ptr(a) for a in planes), C.byref(req), _ptr(out)))
    return out


# ------------------------------------------------------------------------------------- renderer
def denoise_defaults():
    """-> dict of the denoiser's default parameters (rf_denoise_default_parameters)."""
    d = _ffi.DenoiseParameters()
    check(lib.rf_denoise_default_parameters(C.byref(d)))
    return dict(iterations=d.iterations, sigma_color=d.sigma_color, sigma_normal=d.sigma_normal, sigma_depth=d.sigma_depth)


def _denoise_parameters(params):
    unknown = set(params) - {"iterations", "sigma_color", "sigma_normal", "sigma_depth"}
    if unknown:
        raise TypeError(f"unknown denoise parameters: {sorted(unknown)}")
    p = dict(denoise_defaults(), **params)
    return _ffi.DenoiseParameters(int(p["iterations"]), float(p["sigma_color"]), float(p["sigma_normal"]), float(p["sigma_depth"]))


def denoise_images(color_sum, albedo_coverage, normal_depth, samples, exposure=1.0, device_ordinal=0, **params):
    """rf_denoise_images: the denoiser over (H,W,4) f32 sums held on the host (accumulation, {albedo, coverage}, {normal, depth}) of `samples` samples.
    -> (rgb (H,W,3) f32 denoised mean, bgra (H,W) u32 display texels under `exposure`)."""
    color_sum, albedo_coverage, normal_depth = (_f32(a) for a in (color_sum, albedo_coverage, normal_depth))
    h, w = color_sum.shape[:2]
    for a in (color_sum, albedo_coverage, normal_depth):
        if a.shape != (h, w, 4):
            raise ValueError("denoise_images: the three sums must be (H, W, 4) arrays of one size")
    rgba = np.zeros((h, w, 4), np.float32)
    bgra = np.zeros((h, w), np.uint32)
    check(lib.rf_denoise_images(device_ordinal, w, h, samples, _ptr(color_sum), _ptr(albedo_coverage), _ptr(normal_depth), C.byref(_denoise_parameters(params)),
                                exposure, _ptr(rgba), _ptr(bgra)))
    return rgba[..., :3], bgra


def denoise_split_defaults():
    """-> (direct, indirect): the split-component denoiser's two default parameter dicts (rf_denoise_split_default_parameters)."""
    d, i = _ffi.DenoiseParameters(), _ffi.DenoiseParameters()
    check(lib.rf_denoise_split_default_parameters(C.byref(d), C.byref(i)))
    return tuple(dict(iterations=p.iterations, sigma_color=p.sigma_color, sigma_normal=p.sigma_normal, sigma_depth=p.sigma_depth) for p in (d, i))


def _split_parameters(direct, indirect):
    out = []
    for params, base in zip((direct, indirect), denoise_split_defaults()):
        params = dict(params or {})
        unknown = set(params) - set(base)
        if unknown:
            raise TypeError(f"unknown denoise parameters: {sorted(unknown)}")
        p = dict(base, **params)
        out.append(_ffi.DenoiseParameters(int(p["iterations"]), float(p["sigma_color"]), float(p["sigma_normal"]), float(p["sigma_depth"])))
    return out


def denoise_split_images(color_sum, direct_sum, albedo_coverage, normal_depth, samples, exposure=1.0, device_ordinal=0, direct=None, indirect=None):
    """rf_denoise_split_images: the split-component denoiser over (H,W,4) f32 sums held on the host (accumulation S, direct sums D, {albedo, coverage}, {normal,
    depth}) of `samples` samples; direct / indirect: dicts of iterations, sigma_color, sigma_normal, sigma_depth for that component (the rest: its defaults).
    -> (rgb (H,W,3) f32 denoised mean, bgra (H,W) u32 display texels under `exposure`)."""
    color_sum, direct_sum, albedo_coverage, normal_depth = (_f32(a) for a in (color_sum, direct_sum, albedo_coverage, normal_depth))
    h, w = color_sum.shape[:2]
    for a in (color_sum, direct_sum, albedo_coverage, normal_depth):
        if a.shape != (h, w, 4):
            raise ValueError("denoise_split_images: the four sums must be (H, W, 4) arrays of one size")
    pd, pi = _split_parameters(direct, indirect)
    rgba = np.zeros((h, w, 4), np.float32)
    bgra = np.zeros((h, w), np.uint32)
    check(lib.rf_denoise_split_images(device_ordinal, w, h, samples, _ptr(color_sum), _ptr(direct_sum), _ptr(albedo_coverage), _ptr(normal_depth), C.byref(pd), C.byref(pi),
                                      exposure, _ptr(rgba), _ptr(bgra)))
    return rgba[..., :3], bgra


def denoise_tiles(color_sum, albedo_coverage, normal_depth, tile_samples, exposure=1.0, device_ordinal=0, **params):
    """rf_denoise_tiles: denoise_images with one sample count (> 0) per 32x32 tile, tile_samples in tile order (tile_y * ceil(W / 32) + tile_x): every pixel's sums
    are divided by its own tile's count.  -> (rgb (H,W,3) f32 denoised mean, bgra (H,W) u32 display texels under `exposure`)."""
    color_sum, albedo_coverage, normal_depth = (_f32(a) for a in (color_sum, albedo_coverage, normal_depth))
    h, w = color_sum.shape[:2]
    for a in (color_sum, albedo_coverage, normal_depth):
        if a.shape != (h, w, 4):
            raise ValueError("denoise_tiles: the three sums must be (H, W, 4) arrays of one size")
    counts = np.ascontiguousarray(tile_samples, np.uint32).reshape(-1)
    if counts.size != _noise_tiles(w, h):
        raise ValueError(f"denoise_tiles: {_noise_tiles(w, h)} tile counts expected, got {counts.size}")
    rgba = np.zeros((h, w, 4), np.float32)
    bgra = np.zeros((h, w), np.uint32)
    check(lib.rf_denoise_tiles(device_ordinal, w, h, _ptr(counts), _ptr(color_sum), _ptr(albedo_coverage), _ptr(normal_depth), C.byref(_denoise_parameters(params)),
                               exposure, _ptr(rgba), _ptr(bgra)))
    return rgba[..., :3], bgra


def denoise_split_tiles(color_sum, direct_sum, albedo_coverage, normal_depth, tile_samples, exposure=1.0, device_ordinal=0, direct=None, indirect=None):
    """rf_denoise_split_tiles: denoise_split_images with one sample count (> 0) per 32x32 tile, tile_samples in tile order (tile_y * ceil(W / 32) + tile_x): every
    pixel's sums -- S, D and the AOV sums alike -- are divided by its own tile's count (a frame of render_adaptive with set_direct(True, tile_counts=True) and
    set_aovs(True, tile_counts=True), or the sum of the ranks' reads after TileComm.render_adaptive with the gathered counts).
    -> (rgb (H,W,3) f32 denoised mean, bgra (H,W) u32 display texels under `exposure`)."""
    color_sum, direct_sum, albedo_coverage, normal_depth = (_f32(a) for a in (color_sum, direct_sum, albedo_coverage, normal_depth))
    h, w = color_sum.shape[:2]
    for a in (color_sum, direct_sum, albedo_coverage, normal_depth):
        if a.shape != (h, w, 4):
            raise ValueError("denoise_split_tiles: the four sums must be (H, W, 4) arrays of one size")
    counts = np.ascontiguousarray(tile_samples, np.uint32).reshape(-1)
    if counts.size != _noise_tiles(w, h):
        raise ValueError(f"denoise_split_tiles: {_noise_tiles(w, h)} tile counts expected, got {counts.size}")
    pd, pi = _split_parameters(direct, indirect)
    rgba = np.zeros((h, w, 4), np.float32)
    bgra = np.zeros((h, w), np.uint32)
    check(lib.rf_denoise_split_tiles(device_ordinal, w, h, _ptr(counts), _ptr(color_sum), _ptr(direct_sum), _ptr(albedo_coverage), _ptr(normal_depth), C.byref(pd),
                                     C.byref(pi), exposure, _ptr(rgba), _ptr(bgra)))
    return rgba[..., :3], bgra


def robust_mean_images(buckets, samples, exposure=1.0, device_ordinal=0):
    """rf_robust_mean_images: the firefly-robust mean over (K, H, W, 4) f32 bucket sums held on the host (e.g. the sum of several ranks' read_buckets) of `samples`
    >= K samples, K odd in 3 .. 15.  -> dict(mean (H,W,3) f32, bgra8 (H,W) u32 display texels under `exposure`, trim (H,W) u8, samples)."""
    buckets = _f32(buckets)
    if buckets.ndim != 4 or buckets.shape[3] != 4:
        raise ValueError("robust_mean_images: the bucket sums must be a (K, H, W, 4) array")
    k, h, w = buckets.shape[:3]
    rgba = np.zeros((h, w, 4), np.float32)
    bgra = np.zeros((h, w), np.uint32)
    trim = np.zeros((h, w), np.uint8)
    check(lib.rf_robust_mean_images(device_ordinal, w, h, k, samples, _ptr(buckets), exposure, _ptr(rgba), _ptr(bgra), _ptr(trim)))
    return dict(mean=rgba[..., :3], bgra8=bgra, trim=trim, samples=int(samples))


def temporal_defaults():
    """-> dict of the temporal history's default parameters (rf_temporal_default_parameters)."""
    d = _ffi.TemporalParameters()
    check(lib.rf_temporal_default_parameters(C.byref(d)))
    return dict(max_history=d.max_history, depth_tolerance=d.depth_tolerance, min_normal_dot=d.min_normal_dot)


def _temporal_parameters(params):
    unknown = set(params) - {"max_history", "depth_tolerance", "min_normal_dot"}
    if unknown:
        raise TypeError(f"unknown temporal parameters: {sorted(unknown)}")
    p = dict(temporal_defaults(), **params)
    return _ffi.TemporalParameters(float(p["max_history"]), float(p["depth_tolerance"]), float(p["min_normal_dot"]), 0)


def _camera_arg(cam):
    return cam if isinstance(cam, _ffi.Camera) else camera_from_array(cam)


def temporal_images(color_sum, albedo_coverage, normal_depth, samples, camera, history=None, exposure=1.0, device_ordinal=0, **params):
    """rf_temporal_images: the temporal reprojection over (H,W,4) f32 sums held on the host (accumulation, {albedo, coverage}, {normal, depth}) of `samples` samples seen
    by `camera` (_ffi.Camera or its 19 floats).  history: None, or dict(color (H,W,4) = {mean rgb, effective sample count}, geometry (H,W,4) = {unit normal, depth},
    camera): the previous view's result as this function or read_temporal returns it, plus its camera.  Keyword arguments: max_history, depth_tolerance,
    min_normal_dot.  -> dict(color (H,W,4) f32 {T.rgb, T.w}, geometry (H,W,4) f32 {n, z}, bgra8 (H,W) u32 display texels under `exposure`, samples)."""
    color_sum, albedo_coverage, normal_depth = (_f32(a) for a in (color_sum, albedo_coverage, normal_depth))
    h, w = color_sum.shape[:2]
    planes = [color_sum, albedo_coverage, normal_depth]
    hist_color = hist_geometry = hist_camera = None
    if history is not None:
        hist_color, hist_geometry = _f32(history["color"]), _f32(history["geometry"])
        hist_camera = C.byref(_camera_arg(history["camera"]))
        planes += [hist_color, hist_geometry]
    for a in planes:
        if a.shape != (h, w, 4):
            raise ValueError("temporal_images: the sums and the history planes must be (H, W, 4) arrays of one size")
    color = np.zeros((h, w, 4), np.float32)
    geometry = np.zeros((h, w, 4), np.float32)
    bgra = np.zeros((h, w), np.uint32)
    check(lib.rf_temporal_images(device_ordinal, w, h, int(samples), _ptr(color_sum), _ptr(albedo_coverage), _ptr(normal_depth), C.byref(_camera_arg(camera)),
                                 _ptr(hist_color), _ptr(hist_geometry), hist_camera, C.byref(_temporal_parameters(params)), exposure, _ptr(color), _ptr(geometry),
                                 _ptr(bgra)))
    return dict(color=color, geometry=geometry, bgra8=bgra, samples=int(samples))


def robust_mean_tiles(buckets, tile_samples, exposure=1.0, device_ordinal=0):
    """rf_robust_mean_tiles: robust_mean_images with one sample count (>= K) per 32x32 tile, tile_samples in tile order (tile_y * ceil(W / 32) + tile_x): every
    pixel is combined with its own tile's count (read_buckets and read_tile_samples of a frame of render_adaptive).  -> dict(mean, bgra8, trim, tile_samples)."""
    buckets = _f32(buckets)
    if buckets.ndim != 4 or buckets.shape[3] != 4:
        raise ValueError("robust_mean_tiles: the bucket sums must be a (K, H, W, 4) array")
    k, h, w = buckets.shape[:3]
    counts = np.ascontiguousarray(tile_samples, np.uint32).reshape(-1)
    if counts.size != _noise_tiles(w, h):
        raise ValueError(f"robust_mean_tiles: {_noise_tiles(w, h)} tile counts expected, got {counts.size}")
    rgba = np.zeros((h, w, 4), np.float32)
    bgra = np.zeros((h, w), np.uint32)
    trim = np.zeros((h, w), np.uint8)
    check(lib.rf_robust_mean_tiles(device_ordinal, w, h, k, _ptr(counts), _ptr(buckets), exposure, _ptr(rgba), _ptr(bgra), _ptr(trim)))
    return dict(mean=rgba[..., :3], bgra8=bgra, trim=trim, tile_samples=counts)


def _noise_result(est, error_map, tile_sum, tile_max):
    out = {k: getattr(est, k) for k, _ in est._fields_}
    out.update(error_map=error_map, tile_sum=tile_sum, tile_max=tile_max)
    return out


def _noise_tiles(width, height):
    return ((width + TILE - 1) // TILE) * ((height + TILE - 1) // TILE)


def noise_estimate_images(color_sum, sumsq, samples, device_ordinal=0):
    """rf_noise_estimate_images: the noise estimate over (H,W,4) f32 sums held on the host (the accumulation and the radiance second moments) of `samples` >= 2
    samples.  -> dict(mean_error, max_error, worst_tile, samples, pixels, nonfinite_pixels, error_map (H,W), tile_sum, tile_max (one entry per 32x32 tile))."""
    color_sum, sumsq = _f32(color_sum), _f32(sumsq)
    h, w = color_sum.shape[:2]
    if color_sum.shape != (h, w, 4) or sumsq.shape != (h, w, 4):
        raise ValueError("noise_estimate_images: the two sums must be (H, W, 4) arrays of one size")
    est = _ffi.NoiseEstimate()
    emap = np.zeros((h, w), np.float32)
    tsum = np.zeros(_noise_tiles(w, h), np.float32); tmax = np.zeros_like(tsum)
    check(lib.rf_noise_estimate_images(device_ordinal, w, h, samples, _ptr(color_sum), _ptr(sumsq), C.byref(est), _ptr(emap), _ptr(tsum), _ptr(tmax)))
    return _noise_result(est, emap, tsum, tmax)


def noise_estimate_tiles(color_sum, sumsq, tile_samples, device_ordinal=0):
    """rf_noise_estimate_tiles: noise_estimate_images with one sample count (>= 2) per 32x32 tile, tile_samples in tile order (tile_y * ceil(W / 32) + tile_x).
    -> the same dict; samples = the largest count."""
    color_sum, sumsq = _f32(color_sum), _f32(sumsq)
    h, w = color_sum.shape[:2]
    if color_sum.shape != (h, w, 4) or sumsq.shape != (h, w, 4):
        raise ValueError("noise_estimate_tiles: the two sums must be (H, W, 4) arrays of one size")
    counts = np.ascontiguousarray(tile_samples, np.uint32).reshape(-1)
    if counts.size != _noise_tiles(w, h):
        raise ValueError(f"noise_estimate_tiles: {_noise_tiles(w, h)} tile counts expected, got {counts.size}")
    est = _ffi.NoiseEstimate()
    emap = np.zeros((h, w), np.float32)
    tsum = np.zeros(counts.size, np.float32); tmax = np.zeros_like(tsum)
    check(lib.rf_noise_estimate_tiles(device_ordinal, w, h, _ptr(counts), _ptr(color_sum), _ptr(sumsq), C.byref(est), _ptr(emap), _ptr(tsum), _ptr(tmax)))
    return _noise_result(est, emap, tsum, tmax)


def _checkpoint_bytes(blob_or_path):
    if isinstance(blob_or_path, (str, os.PathLike)):
        with open(blob_or_path, "rb") as f:
            return f.read()
    return bytes(blob_or_path)


def checkpoint_info(blob):
    """The header of a checkpoint blob (bytes or a path), host only: sizes, counts, the four switch words, per family (S, AOVs, Q, D, buckets) family_samples /
    family_restarted, and the camera and sky it was rendered with.  RayfinderError (RF_ERROR_INVALID_ARGUMENT) for a blob a load would refuse by its own bytes."""
    data = _checkpoint_bytes(blob)
    info = _ffi.CheckpointInfo()
    check(lib.rf_checkpoint_info(C.c_char_p(data), len(data), C.byref(info)))  # (the pointer of an empty blob is still a pointer)
    out = {k: int(getattr(info, k)) for k, _ in info._fields_ if k not in ("family_samples", "family_restarted", "camera", "sky")}
    out.update(family_samples=[int(v) for v in info.family_samples], family_restarted=[int(v) for v in info.family_restarted], camera=info.camera, sky=info.sky)
    return out


class ReferencePathTracer:
    """Host-side mirror of nlrs::ReferencePathTracer (src/pt/reference_path_tracer.hpp:59-76).

    ctor copies the scene into HBM; set_render_parameters resets accumulation on any change;
    render(n) advances n frames (one sample each) without host round trips.
    """

    def __init__(self, render_params, scene, max_width=0, max_height=0, device_ordinal=0, max_paths_in_flight=0):
        desc = _ffi.RendererDescriptor(render_params, max_width, max_height, device_ordinal, max_paths_in_flight)
        self._h = C.c_void_p()
        self._params = render_params
        self._device_ordinal = device_ordinal
        check(lib.rf_renderer_create(C.byref(desc), C.byref(scene), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and lib is not None:   # lib is None once the interpreter is shutting down
            lib.rf_renderer_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def set_render_parameters(self, params):
        check(lib.rf_renderer_set_render_parameters(self._h, C.byref(params)))
        self._params = params

    def render(self, num_frames=1):
        check(lib.rf_renderer_render(self._h, num_frames))

    def synchronize(self):
        check(lib.rf_renderer_synchronize(self._h))

    def average_renderpass_duration_ms(self):
        return lib.rf_renderer_average_renderpass_duration_ms(self._h)

    def render_progress_percentage(self):
        return lib.rf_renderer_render_progress_percentage(self._h)

    def read_accumulation(self):
        """-> ((H, W, 4) f32 sum image, accumulated sample count)"""
        img = np.zeros((self._params.height, self._params.width, 4), np.float32)
        acc = C.c_uint32(0)
        check(lib.rf_renderer_read_accumulation(self._h, _ptr(img), C.byref(acc)))
        return img, acc.value

    def read_tonemapped(self):
        img = np.zeros((self._params.height, self._params.width), np.uint32)
        check(lib.rf_renderer_read_tonemapped(self._h, _ptr(img)))
        return img

    # first-hit AOVs (rf_renderer_set_aovs / rf_renderer_read_aovs; include/rayfinder_amd.h states what they hold)
    def set_aovs(self, enabled=True, tile_counts=False):
        """Turn the first-hit AOVs (albedo, shading normal, depth) on or off; any change clears their sums.  tile_counts (RF_AOV_TILE_COUNTS): the sums follow the
        per-tile sample counts of render_adaptive, which then runs with the AOVs on, and denoise works on the frame it leaves; until render_adaptive is called,
        nothing differs.  Changing it clears the sums too; it is refused without `enabled`."""
        check(lib.rf_renderer_set_aovs(self._h, (_ffi.RF_AOV_FIRST_HIT if enabled else 0) | (_ffi.RF_AOV_TILE_COUNTS if tile_counts else 0)))

    def read_aovs(self):
        """-> dict of per-pixel SUMS in sample order: albedo (H,W,3), normal (H,W,3), depth (H,W), coverage (H,W), and samples (the AOV sample count)."""
        h, w = self._params.height, self._params.width
        ac = np.zeros((h, w, 4), np.float32); nd = np.zeros((h, w, 4), np.float32)
        n = C.c_uint32(0)
        check(lib.rf_renderer_read_aovs(self._h, _ptr(ac), _ptr(nd), C.byref(n)))
        return dict(albedo=ac[..., :3], normal=nd[..., :3], depth=nd[..., 3], coverage=ac[..., 3], samples=n.value)

    def aov_means(self):
        """-> dict albedo (H,W,3) and normal (H,W,3) divided by the sample count, depth (H,W) divided by the coverage (0 where nothing was hit), coverage (H,W) as a
        fraction, and samples.  All zeros before the first AOV sample.  After render_adaptive (the tiles hold different counts) every pixel is divided by its own
        tile's count; samples is the leading count."""
        s = self.read_aovs()
        cov = s["coverage"]
        depth = np.divide(s["depth"], cov, out=np.zeros_like(cov), where=cov > 0)
        if s["samples"] and not self.tile_samples_uniform():
            n = np.repeat(np.repeat(np.maximum(self.read_tile_samples(), 1), TILE, 0), TILE, 1)[:cov.shape[0], :cov.shape[1]].astype(np.float32)
            return dict(albedo=s["albedo"] / n[..., None], normal=s["normal"] / n[..., None], depth=depth, coverage=cov / n, samples=s["samples"])
        n = np.float32(max(s["samples"], 1))
        return dict(albedo=s["albedo"] / n, normal=s["normal"] / n, depth=depth, coverage=cov / n, samples=s["samples"])

    # edge-aware a-trous denoiser (rf_renderer_denoise / rf_renderer_read_denoised; include/rayfinder_amd.h states its arithmetic)
    def denoise(self, **params):
        """Denoise the accumulation with the first-hit AOVs as guides (needs the AOVs on from the first sample, no tile shard).  After render_adaptive, while the
        tiles hold different counts, it needs set_aovs(True, tile_counts=True) from the first sample: every pixel is then divided by its own tile's count before
        the filter, and the snapshot's sample count is the leading count.  Keyword arguments: iterations, sigma_color, sigma_normal, sigma_depth (the rest: the
        defaults)."""
        check(lib.rf_renderer_denoise(self._h, C.byref(_denoise_parameters(params))))

    def read_denoised(self):
        """-> (rgb (H,W,3) f32 denoised mean, bgra (H,W) u32 display texels, the sample count of the denoised accumulation)"""
        h, w = self._params.height, self._params.width
        rgba = np.zeros((h, w, 4), np.float32)
        bgra = np.zeros((h, w), np.uint32)
        n = C.c_uint32(0)
        check(lib.rf_renderer_read_denoised(self._h, _ptr(rgba), _ptr(bgra), C.byref(n)))
        return rgba[..., :3], bgra, n.value

    # direct radiance sums and the split-component denoiser (include/rayfinder_amd.h states what D holds and the filter's arithmetic)
    def set_direct(self, enabled=True, tile_counts=False):
        """Turn the per-pixel direct radiance sums on or off; any change clears them.  tile_counts (RF_DIRECT_TILE_COUNTS): the sums follow the per-tile counts under
        render_adaptive (and TileComm.render_adaptive), and denoise_split then runs in the non-uniform state; without it render_adaptive is refused while they are on."""
        check(lib.rf_renderer_set_direct(self._h, int(bool(enabled)) | (_ffi.RF_DIRECT_TILE_COUNTS if tile_counts else 0)))

    def read_direct(self):
        """-> ((H, W, 4) f32 sums of each sample's radiance after bounce 1 (sky on a primary miss, the first hit's sun term), in sample order; the direct sample
        count).  Indirect light is read_accumulation()[0] - this, per channel."""
        d = np.zeros((self._params.height, self._params.width, 4), np.float32)
        n = C.c_uint32(0)
        check(lib.rf_renderer_read_direct(self._h, _ptr(d), C.byref(n)))
        return d, n.value

    def denoise_split(self, direct=None, indirect=None):
        """Denoise the direct and the indirect light separately and recombine them (needs the AOVs and the direct sums on from the first sample, no tile shard; after
        render_adaptive both with tile_counts=True: every pixel is then divided by its tile's count);
        read_denoised reads the result.  direct / indirect: dicts of iterations, sigma_color, sigma_normal, sigma_depth (the rest: that component's defaults)."""
        pd, pi = _split_parameters(direct, indirect)
        check(lib.rf_renderer_denoise_split(self._h, C.byref(pd), C.byref(pi)))

    # the feature export (rf_renderer_export_features; include/rayfinder_amd.h states every channel's arithmetic)
    def export_features(self, channels=("color", "albedo", "normal", "depth"), layout="chw", dtype="f32", out=None):
        """The frame as a tensor on the GPU: the selected feature channels -- out of color, albedo, normal, depth, coverage, direct, indirect, variance, error, samples;
        always in that order -- of the handle's own sums, every pixel divided by its (tile's) sample count, written by one kernel into a torch tensor on the handle's
        device: (C, H, W) for layout "chw", (H, W, C) for "hwc"; torch.float32 for dtype "f32", torch.float16 for "f16".  out: a contiguous tensor of that shape, dtype
        and device to write into (a storage offset is fine); None: torch.empty.  The call waits for the kernel: the tensor may be used on any stream at once.  Needs the
        sums its channels read on from the first sample (set_aovs, set_direct, set_moments; after render_adaptive with tile_counts=True) and no tile shard."""
        req, count = _feature_request(channels, layout, dtype)
        h, w = self._params.height, self._params.width
        out = _feature_tensor("export_features", out, (count, h, w) if layout == "chw" else (h, w, count), dtype, self._device_ordinal)
        check(lib.rf_renderer_export_features(self._h, C.byref(req), C.c_void_p(out.data_ptr()), out.numel() * out.element_size(), None))
        return out

    # rays from device tensors (rf_renderer_cast_rays; include/rayfinder_amd.h states every output's value)
    def _cast(self, what, origins, directions, t_max, kind, names, out):
        import torch
        batch, tensors = _ray_batch(what, origins, directions, t_max, kind, names, out, self._device_ordinal)
        if batch.num_rays:
            # the inputs are complete before the library reads them on the handle's own stream
            torch.cuda.current_stream(torch.device("cuda", self._device_ordinal)).synchronize()
            check(lib.rf_renderer_cast_rays(self._h, C.byref(batch)))
        return tensors

    def cast_rays(self, origins, directions, t_max=10000.0, outputs=("triangle", "t", "position", "normal", "albedo"), out=None):
        """What do these rays hit, and what is the surface there?  origins, directions: float32 CUDA tensors (N, 3) on the handle's device, rows of 3 consecutive floats
        at a row stride >= 3 (the two halves of an (N, 6) tensor qualify).  The rays go through the renderer's production traversal in (1e-5, t_max); -> a dict of
        torch tensors on the device, one per name in `outputs`: triangle (N,) int32 (-1: a miss), t (N,), bary (N, 2), position (N, 3) the offset hit point,
        geometric_normal (N, 3), normal (N, 3) the unit shading normal, texcoord (N, 2), albedo (N, 3), texture (N,) int32; float32, +0 on a miss.  out: a dict of
        contiguous tensors of those shapes and dtypes to write into (a storage offset is fine; names it lacks are allocated).  Torch's current stream on the device is
        synchronised first, the call waits for its kernels: the tensors may be used on any stream at once.  Nothing of the render state changes."""
        return self._cast("cast_rays", origins, directions, t_max, _ffi.RF_RAYS_CLOSEST, outputs, out)

    def cast_occlusion(self, origins, directions, t_max=10000.0, out=None):
        """-> float32 tensor (N,): 1.0 where nothing is hit in (1e-5, t_max) along the ray, else 0.0 (shadowRay's answer).  Rays, stream rule and `out` (here one
        tensor) as cast_rays."""
        if out is not None:
            import torch
            if not isinstance(out, torch.Tensor):
                raise TypeError("cast_occlusion: out must be a torch.Tensor")
            out = {"visibility": out}
        return self._cast("cast_occlusion", origins, directions, t_max, _ffi.RF_RAYS_ANY, ("visibility",), out)["visibility"]

    # radiance second moments, the noise estimate and render-to-a-noise-target (include/rayfinder_amd.h states the estimate's arithmetic)
    def set_moments(self, enabled=True):
        """Turn the per-pixel radiance second moments on or off; any change clears them."""
        check(lib.rf_renderer_set_moments(self._h, int(bool(enabled))))

    def read_moments(self):
        """-> ((H, W, 4) f32 sums of the squared per-sample radiance {r*r, g*g, b*b, 0} in sample order, the moment sample count)"""
        q = np.zeros((self._params.height, self._params.width, 4), np.float32)
        n = C.c_uint32(0)
        check(lib.rf_renderer_read_moments(self._h, _ptr(q), C.byref(n)))
        return q, n.value

    # bucket sums and the firefly-robust mean (include/rayfinder_amd.h states what the buckets hold and the combine's arithmetic)
    def set_buckets(self, k, tile_counts=False, shard=False):
        """Keep k bucket sums (k odd, 3 .. 15; 0: off, the default): bucket b sums the radiance of the samples whose ordinal is b mod k.  Any change clears them.
        Without tile_counts they keep one count for the frame: render_adaptive is refused while they are on.  tile_counts (RF_BUCKETS_TILE_COUNTS, k > 0): the sums
        follow the per-tile sample counts of render_adaptive, which then runs with the buckets on, and robust_mean / denoise_robust work on the frame it leaves;
        until render_adaptive is called, nothing differs.  shard (RF_BUCKETS_SHARD_TILE_COUNTS, only with tile_counts): the per-tile-count sums are also kept under
        a tile shard -- TileComm.render_adaptive then runs with the buckets on -- and gather_frame(robust_mean=True, tile_counts=True) carries the robust mean of the
        frame it leaves; without a tile shard nothing differs from tile_counts alone."""
        check(lib.rf_renderer_set_buckets(self._h, int(k) | (_ffi.RF_BUCKETS_TILE_COUNTS if tile_counts else 0) | (_ffi.RF_BUCKETS_SHARD_TILE_COUNTS if shard else 0)))

    def read_buckets(self):
        """-> ((K, H, W, 4) f32 bucket sums {r, g, b, 0} in sample order, the bucket sample count); K = 0 while the buckets are off"""
        k, n = C.c_uint32(0), C.c_uint32(0)
        check(lib.rf_renderer_read_buckets(self._h, None, C.byref(k), C.byref(n)))
        b = np.zeros((k.value, self._params.height, self._params.width, 4), np.float32)
        if k.value:
            check(lib.rf_renderer_read_buckets(self._h, _ptr(b), C.byref(k), C.byref(n)))
        return b, n.value

    def robust_mean(self):
        """Combine the bucket sums into the robust mean (needs the buckets on from the first sample, at least K samples -- after render_adaptive: in every tile, and
        the buckets set with tile_counts --, no tile shard); read_robust_mean reads it."""
        check(lib.rf_renderer_robust_mean(self._h))

    def read_robust_mean(self):
        """-> dict(mean (H,W,3) f32, bgra8 (H,W) u32 display texels, trim (H,W) u8: the buckets cut from each end, samples: the count of the combined accumulation)"""
        h, w = self._params.height, self._params.width
        rgba = np.zeros((h, w, 4), np.float32)
        bgra = np.zeros((h, w), np.uint32)
        trim = np.zeros((h, w), np.uint8)
        n = C.c_uint32(0)
        check(lib.rf_renderer_read_robust_mean(self._h, _ptr(rgba), _ptr(bgra), _ptr(trim), C.byref(n)))
        return dict(mean=rgba[..., :3], bgra8=bgra, trim=trim, samples=n.value)

    def denoise_robust(self, **params):
        """robust_mean, then denoise with the robust mean in place of the plain mean (needs what both need); read_denoised reads the result.  Keyword arguments as
        for denoise."""
        check(lib.rf_renderer_denoise_robust(self._h, C.byref(_denoise_parameters(params))))

    # the temporal history (include/rayfinder_amd.h, "Temporal history"): the previous view's frame reprojected into the current camera
    def temporal_accumulate(self, **params):
        """Blend the current view's samples with the kept history, reprojected into the current camera (needs the AOVs on from the first sample, at least one sample,
        no tile shard, the uniform state); without a history the result is the plain mean.  Calling it again later in the same accumulation recomputes from the same
        history.  Keyword arguments: max_history, depth_tolerance, min_normal_dot (temporal_defaults()).  read_temporal reads the result."""
        check(lib.rf_renderer_temporal_accumulate(self._h, C.byref(_temporal_parameters(params))))

    def temporal_commit(self):
        """The current temporal result becomes the history of the views that follow (no copy); the result is then gone.  The history survives
        set_render_parameters; a new frame size, a tile shard and temporal_reset drop it."""
        check(lib.rf_renderer_temporal_commit(self._h))

    def temporal_reset(self):
        """Drop the temporal history and the current result (a cut: the next view shares nothing with the last)."""
        check(lib.rf_renderer_temporal_reset(self._h))

    def read_temporal(self):
        """-> dict(color (H,W,4) f32 {T.rgb, T.w = the effective sample count}, bgra8 (H,W) u32 display texels, geometry (H,W,4) f32 {unit normal, depth; zeros:
        background}, samples: the count of the current view's accumulation)"""
        h, w = self._params.height, self._params.width
        rgba = np.zeros((h, w, 4), np.float32)
        bgra = np.zeros((h, w), np.uint32)
        geometry = np.zeros((h, w, 4), np.float32)
        n = C.c_uint32(0)
        check(lib.rf_renderer_read_temporal(self._h, _ptr(rgba), _ptr(bgra), _ptr(geometry), C.byref(n)))
        return dict(color=rgba, bgra8=bgra, geometry=geometry, samples=n.value)

    def denoise_temporal(self, temporal=None, **params):
        """temporal_accumulate (temporal: its parameter dict, None = the defaults), then denoise with the temporal result in place of the plain mean; read_denoised
        reads the result.  Keyword arguments as for denoise."""
        check(lib.rf_renderer_denoise_temporal(self._h, C.byref(_temporal_parameters(dict(temporal or {}))), C.byref(_denoise_parameters(params))))

    def noise_estimate(self):
        """The noise estimate over the accumulation and the moments (needs the moments on from the first sample, >= 2 samples, no tile shard).
        -> dict(mean_error, max_error, worst_tile, samples, pixels, nonfinite_pixels, error_map (H,W), tile_sum, tile_max (one entry per 32x32 tile))."""
        h, w = self._params.height, self._params.width
        est = _ffi.NoiseEstimate()
        emap = np.zeros((h, w), np.float32)
        tsum = np.zeros(_noise_tiles(w, h), np.float32); tmax = np.zeros_like(tsum)
        check(lib.rf_renderer_noise_estimate(self._h, C.byref(est), _ptr(emap), _ptr(tsum), _ptr(tmax)))
        return _noise_result(est, emap, tsum, tmax)

    def render_until(self, target_mean_error, check_every=8, max_frames=0xFFFFFFFF):
        """Render in steps of check_every frames until the estimate's mean_error is <= target_mean_error, max_frames frames have been rendered or the accumulation
        is full.  -> (frames rendered, dict of the last estimate's scalars, or None when fewer than 2 samples were accumulated)."""
        frames = C.c_uint32(0)
        est = _ffi.NoiseEstimate()
        check(lib.rf_renderer_render_until(self._h, target_mean_error, check_every, max_frames, C.byref(frames), C.byref(est)))
        return frames.value, ({k: getattr(est, k) for k, _ in est._fields_} if est.samples else None)

    # tile-adaptive sampling (include/rayfinder_amd.h states the loop and what the reads return while the tiles hold different counts)
    def render_adaptive(self, target_tile_error, check_every=8, min_samples=0, max_samples=0):
        """Keep sampling only the 32x32 tiles whose mean error is above target_tile_error, checking every check_every samples from min_samples on, up to max_samples
        (0: the frame's samples per pixel).  Needs the moments on from the first sample, no tile shard, and the AOVs off or on with tile_counts=True from the first
        sample (their sums then hold, per tile, the tile's own first samples, as the image does).
        -> dict(estimate_passes, tiles, stopped_tiles, min_tile_samples, max_tile_samples, pixel_samples, last: the last pass's estimate scalars or None)."""
        p = _ffi.AdaptiveParameters(target_tile_error, check_every, min_samples, max_samples)
        res = _ffi.AdaptiveResult()
        check(lib.rf_renderer_render_adaptive(self._h, C.byref(p), C.byref(res)))
        out = {k: getattr(res, k) for k, _ in res._fields_ if k not in ("reserved", "last")}
        out["last"] = {k: getattr(res.last, k) for k, _ in res.last._fields_} if res.last.samples else None
        return out

    def read_tile_samples(self):
        """-> (tiles_y, tiles_x) u32: the sample count of every 32x32 tile"""
        h, w = self._params.height, self._params.width
        counts = np.zeros(((h + TILE - 1) // TILE, (w + TILE - 1) // TILE), np.uint32)
        n = C.c_uint32(0)
        check(lib.rf_renderer_read_tile_samples(self._h, _ptr(counts), C.byref(n)))
        assert n.value == counts.size
        return counts

    def tile_samples_uniform(self):
        """-> False while the tiles of this handle's shard hold different sample counts (after render_adaptive stopped some of them)"""
        counts = self.read_tile_samples()
        return np.unique(counts[counts > 0]).size <= 1                      # (0: a tile of another rank's shard)

    def read_mean(self):
        """-> (H, W, 4) f32 {sum.rgb / the tile's sample count, 1}"""
        mean = np.zeros((self._params.height, self._params.width, 4), np.float32)
        check(lib.rf_renderer_read_mean(self._h, _ptr(mean)))
        return mean

    # deferred-lighting variant (nlrs::DeferredRenderer's lighting + resolve passes over a primary-ray G-buffer)
    def render_deferred(self, num_frames=1):
        check(lib.rf_renderer_render_deferred(self._h, num_frames))

    def reset_deferred(self):
        check(lib.rf_renderer_reset_deferred(self._h))

    def read_deferred(self):
        """-> (sample buffer (H,W,3), accumulation buffer (H,W,3), BGRA8 (H,W), frames rendered)"""
        w, h = self._params.width, self._params.height
        sample = np.zeros((h, w, 3), np.float32); accum = np.zeros((h, w, 3), np.float32); bgra = np.zeros((h, w), np.uint32)
        n = C.c_uint32(0)
        check(lib.rf_renderer_read_deferred(self._h, _ptr(sample), _ptr(accum), _ptr(bgra), C.byref(n)))
        return sample, accum, bgra, n.value

    def set_counting(self, enabled):
        check(lib.rf_renderer_set_counting(self._h, int(enabled)))

    def set_timing(self, enabled):
        check(lib.rf_renderer_set_timing(self._h, int(enabled)))

    def set_option(self, name, value):
        check(lib.rf_renderer_set_option(self._h, name.encode(), int(value)))

    def reset_stats(self):
        check(lib.rf_renderer_reset_stats(self._h))

    def stats(self):
        s = _ffi.Stats()
        check(lib.rf_renderer_get_stats(self._h, C.byref(s)))
        return s.as_dict()

    LAYOUT_NAMES = ("binary", "compact", "hot", "quad", "quad_half", "quad_local", "oct", "scalar", "packet")

    def layout_info(self, bounces=8):
        """rf_renderer_layout_info: the record layout this renderer reads in the closest-hit / any-hit launch of bounce 1..n (what it picked by itself for the
        scene + any option set since), whether that any-hit launch starts at the occluder cache, and the per-scene parameters behind the choice."""
        raw = np.zeros(48 + 4 + 2 + 2, np.uint32)      # 3 x 16 words, 4 words, 2 floats, one u64
        check(lib.rf_renderer_layout_info(self._h, _ptr(raw)))
        n = min(bounces, 16)
        return dict(closest=[self.LAYOUT_NAMES[v] for v in raw[:n]], shadow=[self.LAYOUT_NAMES[v] for v in raw[16:16 + n]], shadow_cached=[bool(v) for v in raw[32:32 + n]],
                    occluder_hint_levels=int(raw[48]), shadow_first_look_from_bounce=int(raw[49]), dense_leaf_min=int(raw[50]), legacy_layouts_compiled=bool(raw[51]),
                    quad_half_area_ratio=float(raw[52:53].view(np.float32)[0]), tree_bytes=int(raw[54:56].view(np.uint64)[0]))

    # rf_launch_plan, word by word
    LAUNCH_PLAN_FIELDS = (
        "num_samples", "num_bounces", "sample_perm", "dense_raygen", "const_origin", "primary_layout", "occluder_grid", "occluder_scale_bits", "occluder_mask", "runs",
        "tile_list", "accumulate_kernel", "accumulate_pixels", "aov_pixels", "moment_pixels", "raygen_count_word",
        "closest_kernel", "closest_layout", "closest_counting", "closest_nearest", "closest_dense", "closest_refill_min", "closest_chunk", "closest_leaf_vote", "closest_flags",
        "closest_extra_lds", "closest_count_word", "closest_cursor_word",
        "shade_sorted", "shade_aov", "shade_flags", "shade_sort_scale", "shade_grid_cap",
        "shadow_kernel", "shadow_layout", "shadow_counting", "shadow_nearest", "shadow_dense", "shadow_refill_min", "shadow_chunk", "shadow_leaf_vote", "shadow_flags",
        "shadow_extra_lds", "shadow_count_word", "shadow_cursor_word", "shadow_cached", "shadow_first_look", "shadow_self", "shadow_source", "look_flags", "look_count_word",
        "look_list_word")

    def launch_plan(self, bounce, num_samples):
        """rf_renderer_launch_plan: the launches of bounce `bounce` (1-based) of this renderer's next batch of num_samples samples, as it would enqueue them in its
        present state -> dict of ints (include/rayfinder_amd.h: rf_launch_plan)."""
        raw = np.zeros(len(self.LAUNCH_PLAN_FIELDS), np.uint32)
        check(lib.rf_renderer_launch_plan(self._h, bounce, num_samples, _ptr(raw)))
        return dict(zip(self.LAUNCH_PLAN_FIELDS, (int(v) for v in raw)))

    def memory_info(self):
        """Device memory held by the handle: dict(path_state_bytes, paths_allocated, max_paths_per_batch, scene_bytes)."""
        v = [C.c_uint64(0) for _ in range(4)]
        check(lib.rf_renderer_memory_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("path_state_bytes", "paths_allocated", "max_paths_per_batch", "scene_bytes"), (x.value for x in v)))

    def bounce_stats(self):
        """Per-bounce queue occupancy (rays traced) and traversal kernel ms since the last reset."""
        cap = 32
        cr = np.zeros(cap, np.uint64); sr = np.zeros(cap, np.uint64); mc = np.zeros(cap, np.float64); ms = np.zeros(cap, np.float64)
        n = C.c_uint32(0)
        check(lib.rf_renderer_get_bounce_stats(self._h, cap, _ptr(cr), _ptr(sr), _ptr(mc), _ptr(ms), C.byref(n)))
        k = n.value
        return dict(closest_rays=cr[:k], shadow_rays=sr[:k], ms_closest=mc[:k], ms_shadow=ms[:k])

    # multi-GPU tile sharding
    def set_tile_shard(self, rank, world_size):
        check(lib.rf_renderer_set_tile_shard(self._h, rank, world_size))

    def shard_tiles(self):
        n = C.c_uint32(0)
        check(lib.rf_renderer_shard_tiles(self._h, None, C.byref(n)))
        tiles = np.zeros(n.value, np.uint32)
        check(lib.rf_renderer_shard_tiles(self._h, _ptr(tiles), C.byref(n)))
        return tiles

    def accumulation_device_buffer(self):
        p = C.c_void_p()
        n = C.c_uint64(0)
        check(lib.rf_renderer_accumulation_device_buffer(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def gather_frame(self, comm, root=0, loopback=False, aovs=False, moments=False, tile_counts=False, robust_mean=False, direct=False):
        """Frame-end RCCL exchange (collective; enqueued on the handle's stream).  Root: device pointer of the
        row-major W*H float4 image; other ranks: None.  aovs / moments: the first-hit AOV sums / the radiance second moments travel in the same group
        and are un-tiled with the image (they must be on from the first sample); the root then reads, denoises and estimates the gathered frame through
        comm.read_plane / denoise / noise_estimate.  tile_counts: the per-tile sample counts travel too (needed after comm.render_adaptive stopped some tiles):
        the root's denoise / noise_estimate then take each tile's own count, and comm.read_tile_samples / read_mean read them.  robust_mean: every rank combines
        its own bucket sums (set_buckets from the first sample, at least K samples) before the exchange and the result travels as one more plane; the root reads it
        through comm.read_robust_mean and denoises with it through comm.denoise_robust.  While the tiles hold different counts, robust_mean needs tile_counts and
        buckets set with set_buckets(k, tile_counts=True, shard=True), every tile at k samples or more: each rank then combines every tile with its own count.
        direct: the direct sums (set_direct from the first sample; after comm.render_adaptive with tile_counts=True) travel as plane 5; the root reads them through
        comm.read_plane(r, 5) and comm.read_split, and with aovs=True denoises the two components through comm.denoise_split."""
        p = C.c_void_p()
        check(lib.rf_renderer_gather_frame(self._h, comm._h, root, _gather_flags(loopback, aovs, moments, tile_counts, robust_mean, direct), C.byref(p)))
        return p.value

    def tonemap_device_image(self, device_ptr, width, height, samples):
        out = np.zeros((height, width), np.uint32)
        check(lib.rf_renderer_tonemap_device_image(self._h, C.c_void_p(device_ptr), width * height, samples, _ptr(out)))
        return out

    def bind_accumulation_buffer(self, device_ptr, nbytes):
        check(lib.rf_renderer_bind_accumulation_buffer(self._h, C.c_void_p(device_ptr), nbytes))

    # state digest and checkpoints (rf_renderer_state_digest / _save_checkpoint / _load_checkpoint; include/rayfinder_amd.h defines the digest)
    def state_digest(self, timing=False):
        """-> dict of Python ints: the plane digests (accumulation, albedo_coverage, normal_depth, moments, direct, bucket: a list of 15), the counts digest, per
        family (S, AOVs, Q, D, buckets) family_on / family_samples, frame_count, accumulated, num_tiles and the four switch words: two handles in the same state
        return equal dicts.  timing: also kernel_ms, the digest kernel's own time in this call (a float; not part of the state)."""
        d = _ffi.StateDigest()
        check(lib.rf_renderer_state_digest(self._h, C.byref(d)))
        out = {k: int(getattr(d, k)) for k, _ in d._fields_ if k not in ("bucket", "family_on", "family_samples", "kernel_ms")}
        out.update(bucket=[int(v) for v in d.bucket], family_on=[int(v) for v in d.family_on], family_samples=[int(v) for v in d.family_samples])
        if timing:
            out["kernel_ms"] = float(d.kernel_ms)
        return out

    def save_checkpoint(self, path=None):
        """-> the checkpoint blob (bytes).  With a path it is also written there: to a temporary file beside it first, then renamed over it."""
        n = C.c_uint64(0)
        check(lib.rf_renderer_save_checkpoint(self._h, None, C.byref(n)))
        buf = bytearray(n.value)
        check(lib.rf_renderer_save_checkpoint(self._h, (C.c_char * len(buf)).from_buffer(buf), C.byref(n)))
        if path is not None:
            # (the file is written from the buffer the library filled; the one copy made is the bytes object returned)
            tmp = f"{os.fspath(path)}.tmp{os.getpid()}"
            with open(tmp, "wb") as f:
                f.write(buf)
                f.flush()
                os.fsync(f.fileno())
            os.replace(tmp, path)
        return bytes(buf)

    def load_checkpoint(self, blobs):
        """One blob (bytes), a path, or a list of either: together they must hold every tile of this handle's shard exactly once (other tiles are ignored).
        RayfinderError with status RF_ERROR_INVALID_ARGUMENT: refused, the handle unchanged; RF_ERROR_CORRUPT: the accumulation was restarted."""
        if isinstance(blobs, (bytes, bytearray, memoryview, str, os.PathLike)):
            blobs = [blobs]
        arrays = [np.frombuffer(_checkpoint_bytes(b) if isinstance(b, (str, os.PathLike)) else b, np.uint8) for b in blobs]  # (a blob in memory is read where it lies)
        ptrs = (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])
        sizes = (C.c_uint64 * len(arrays))(*[a.size for a in arrays])
        check(lib.rf_renderer_load_checkpoint(self._h, ptrs, sizes, len(arrays)))

    def resume(self, path):
        """Set the four switches (AOVs, moments, direct, buckets) as the checkpoint's info says, then load it.  -> the info."""
        blob = _checkpoint_bytes(path)
        info = checkpoint_info(blob)
        check(lib.rf_renderer_set_aovs(self._h, info["aov_flags"]))
        check(lib.rf_renderer_set_moments(self._h, info["moments_on"]))
        check(lib.rf_renderer_set_direct(self._h, info["direct_word"]))
        check(lib.rf_renderer_set_buckets(self._h, info["buckets_word"]))
        self.load_checkpoint(blob)
        return info

    # BVH queries
    def trace_primary_stats(self, camera, width, height):
        n = width * height
        nv = np.zeros(n, np.uint32); hit = np.zeros(n, np.uint8); t = np.zeros(n, np.float32); tt = np.zeros(n, np.uint32)
        check(lib.rf_renderer_trace_primary_stats(self._h, C.byref(camera), width, height, _ptr(nv), _ptr(hit), _ptr(t), _ptr(tt)))
        return dict(nodesVisited=nv, hit=hit, t=t, triTests=tt)

    def intersect_rays(self, rays6, t_max):
        rays = _f32(rays6).reshape(-1, 6)
        n = rays.shape[0]
        out = dict(tri=np.zeros(n, np.uint32), t=np.zeros(n, np.float32), uv=np.zeros((n, 2), np.float32),
                   p=np.zeros((n, 3), np.float32), nodesVisited=np.zeros(n, np.uint32), triTests=np.zeros(n, np.uint32))
        check(lib.rf_renderer_intersect_rays(self._h, _ptr(rays), n, np.float32(t_max), _ptr(out["tri"]), _ptr(out["t"]), _ptr(out["uv"]),
                                             _ptr(out["p"]), _ptr(out["nodesVisited"]), _ptr(out["triTests"])))
        out["hit"] = (out["tri"] != 0xFFFFFFFF).astype(np.uint8)
        return out

    def occluded_rays(self, rays6, t_max):
        rays = _f32(rays6).reshape(-1, 6)
        vis = np.zeros(rays.shape[0], np.float32)
        check(lib.rf_renderer_occluded_rays(self._h, _ptr(rays), rays.shape[0], np.float32(t_max), _ptr(vis)))
        return vis
