"""gsm_amd -- Python mirror of the reference's GlobalRenderer operator surface over the
MI355X C ABI (include/gsm_renderer.h, include/gsm_debug.h).

Mirrors Sources/Renderer/Shared/GaussianRendererProtocol.swift (RendererConfig,
GaussianInput, CameraParams, RendererError) and GlobalRenderer.swift (init, render,
renderStereo, debugReadTotalAssignments, lastGPUTime).  Device buffers are torch
tensors on a ROCm device (PyTorch is plumbing: memory, streams, torch.distributed);
every frame runs in the hand-written gfx950 kernels of libgsm_amd.so.  There is no
CPU fallback: if the library is missing, importing a renderer raises.
"""
from __future__ import annotations

import ctypes as C
import enum
import os
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

try:  # load torch's HIP runtime first so libgsm_amd.so binds to the same one
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is always present in this image
    torch = None

from .types import PROJECTED, RENDER_DATA, WORLD16, WORLD32  # noqa: F401

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# GSM_AMD_LIB: another in-tree build of the same library (A/B experiments, tools/); default lib/
LIB_PATH = os.environ.get("GSM_AMD_LIB") or os.path.join(os.path.dirname(_PKG_DIR), "lib", "libgsm_amd.so")
INCLUDE_DIR = os.path.join(os.path.dirname(os.path.dirname(_PKG_DIR)), "include")


class Status(enum.IntEnum):
    """RendererError cases (GaussianRendererProtocol.swift:274-292) as C status codes."""
    OK = 0
    DEVICE_NOT_AVAILABLE = 1
    FAILED_TO_CREATE_LIBRARY = 2
    FAILED_TO_CREATE_PIPELINE = 3
    FAILED_TO_ALLOCATE_BUFFER = 4
    FAILED_TO_ALLOCATE_TEXTURE = 5
    INVALID_GAUSSIAN_COUNT = 6
    INVALID_DIMENSIONS = 7
    INVALID_BUFFER_SIZE = 8
    INVALID_TILE_COUNT = 9
    INVALID_ASSIGNMENT_CAPACITY = 10
    RENDER_FAILED = 11
    ENCODER_CREATION_FAILED = 12
    MISSING_REQUIRED_BUFFER = 13
    INVALID_ARGUMENT = 14
    UNSUPPORTED = 15
    PHASE_ORDER = 16


class RendererError(RuntimeError):
    def __init__(self, status: int, what: str = ""):
        self.status = Status(status)
        msg = _lib().gsm_status_string(int(status)).decode() if _LIB is not None else self.status.name
        super().__init__(f"{self.status.name}: {msg}{(' (' + what + ')') if what else ''}")


class RenderPrecision(enum.IntEnum):  # GaussianRendererProtocol.swift:4-7
    FLOAT32 = 0
    FLOAT16 = 1


class GaussianColorSpace(enum.IntEnum):  # GaussianRendererProtocol.swift:196-201
    LINEAR = 0
    SRGB = 1


class ColorFormat(enum.IntEnum):
    """Colour target pixel format (RendererConfig.colorFormat, GaussianRendererProtocol.swift:207;
    include/gsm_renderer.h gsm_color_format has the conversion rules)."""
    RGBA16F = 0
    RGBA32F = 1
    RGBA8_UNORM = 2
    RGBA8_UNORM_SRGB = 3
    BGRA8_UNORM = 4
    BGRA8_UNORM_SRGB = 5

    @property
    def bytes_per_pixel(self) -> int:
        return 8 if self == ColorFormat.RGBA16F else (16 if self == ColorFormat.RGBA32F else 4)


class BufferId(enum.IntEnum):  # include/gsm_debug.h gsm_buffer_id
    RENDER_DATA = 0
    BOUNDS = 1
    TILE_COUNTS = 2
    KEYS = 3
    VALUES = 4
    SORTED_KEYS = 5
    SORTED_VALUES = 6
    HEADERS = 7
    EXP_TABLE = 8
    BLEND_TRACE = 9


STAGES = ("project", "scan", "scatter", "sort", "headers", "blend")
# gsm_blend_kernel (include/gsm_debug.h) -> the kernel's name in rocprofv3 traces
BLEND_KERNELS = {0: None, 1: "k_blend_px", 2: "k_blend_px", 3: "k_blend_pw"}


@dataclass
class RendererConfig:
    """RendererConfig (GaussianRendererProtocol.swift:195-228) with the same defaults."""
    max_gaussians: int = 6_000_000
    max_width: int = 1920
    max_height: int = 1080
    precision: RenderPrecision = RenderPrecision.FLOAT16
    color_format: int = 0
    gaussian_color_space: GaussianColorSpace = GaussianColorSpace.SRGB
    back_to_front: bool = False


@dataclass
class GaussianInput:
    """GaussianInput (GaussianRendererProtocol.swift:9-26): device buffers + counts."""
    gaussians: "torch.Tensor"
    harmonics: "torch.Tensor"
    gaussian_count: int
    shComponents: int = 0

    @property
    def sh_components(self) -> int:
        return self.shComponents


@dataclass
class CameraParams:
    """CameraParams (GaussianRendererProtocol.swift:28-54).  view/proj are 16 floats in
    simd_float4x4 (column-major) memory order."""
    view: np.ndarray
    proj: np.ndarray
    position: np.ndarray = field(default_factory=lambda: np.zeros(3, np.float32))
    focal_x: float = 0.0
    focal_y: float = 0.0
    near: float = 0.1
    far: float = 10.0

    @staticmethod
    def from_dict(d: dict) -> "CameraParams":
        return CameraParams(np.asarray(d["view"], np.float32).reshape(16),
                            np.asarray(d["proj"], np.float32).reshape(16),
                            np.asarray(d.get("position", np.zeros(3)), np.float32).reshape(3),
                            float(d.get("focal_x", 0.0)), float(d.get("focal_y", 0.0)),
                            float(d.get("near", 0.1)), float(d.get("far", 10.0)))

    def to_dict(self) -> dict:
        return {"view": np.asarray(self.view, np.float32), "proj": np.asarray(self.proj, np.float32),
                "position": np.asarray(self.position, np.float32), "focal_x": self.focal_x,
                "focal_y": self.focal_y, "near": self.near, "far": self.far}


@dataclass
class BatchView:
    """gsm_global_view: one view of GlobalRenderer.render_batch -- its own scene, camera, frame size and targets
    (depth None: this view writes no depth; pitches None: width * bytes per pixel / width * 2)."""
    input: GaussianInput
    camera: CameraParams
    width: int
    height: int
    color: "torch.Tensor"
    depth: Optional["torch.Tensor"] = None
    color_pitch: Optional[int] = None
    depth_pitch: Optional[int] = None


@dataclass
class SceneObject:
    """gsm_global_object: one object of GlobalRenderer.render_composite -- a resident scene and the frame's camera
    as seen from that scene's own space (scenes.object_camera(camera, model) for a model matrix)."""
    input: GaussianInput
    camera: CameraParams


@dataclass
class Frame:
    """gsm_global_frame: one descriptor of GlobalRenderer.render_frames -- `render_frame`'s arguments as a value.
    objects: one (GaussianInput, CameraParams) pair (or a SceneObject list of one); pick / occluder / states /
    styles None: that option is not given; pitches None: width * bytes per pixel.  orthographic: the frame follows
    the orthographic projection rule (FRAME_ORTHOGRAPHIC is or-ed into flags)."""
    objects: object
    width: int
    height: int
    color: "torch.Tensor"
    depth: Optional["torch.Tensor"] = None
    pick: Optional["torch.Tensor"] = None
    occluder: Optional["torch.Tensor"] = None
    states: object = None
    styles: object = None
    color_pitch: Optional[int] = None
    depth_pitch: Optional[int] = None
    pick_pitch: Optional[int] = None
    occluder_pitch: Optional[int] = None
    style_count: Optional[int] = None
    flags: int = 0
    orthographic: bool = False


@dataclass
class Style:
    """gsm_global_style: one entry of a styled frame's table.  tint is (r, g, b) in the u8 colour space of the
    projected gaussians; tint_amount 0 leaves the colour, 255 replaces it; opacity_scale 255 leaves the opacity, 0
    removes the splat's tiles; hidden culls the gaussian."""
    tint: tuple = (0, 0, 0)
    tint_amount: int = 0
    opacity_scale: int = 255
    hidden: bool = False


SELECT_ALL, SELECT_BOX, SELECT_ELLIPSOID = 0, 1, 2  # include/gsm_renderer.h GSM_SELECT_*
SELECT_OUTSIDE = 1


@dataclass
class SelectQuery:
    """gsm_global_select_query: the predicate of GlobalRenderer.select_where.  The defaults are
    gsm_global_select_query_default's: no shape, identity rows, both ranges (-inf, +inf), every state.  to_shape:
    twelve floats, a row-major 3x4 from scene space to the shape's unit space (scenes.box_to_shape,
    scenes.sphere_to_shape)."""
    shape: int = SELECT_ALL
    flags: int = 0
    to_shape: tuple = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    opacity_min: float = float("-inf")
    opacity_max: float = float("inf")
    scale_min: float = float("-inf")
    scale_max: float = float("inf")
    test_mask: int = 0
    test_value: int = 0


# ---------------------------------------------------------------------------
# ctypes layer
# ---------------------------------------------------------------------------
class _Config(C.Structure):
    _fields_ = [("max_gaussians", C.c_uint32), ("max_width", C.c_uint32), ("max_height", C.c_uint32),
                ("precision", C.c_uint32), ("color_format", C.c_uint32),
                ("gaussian_color_space", C.c_uint32), ("back_to_front", C.c_uint32)]


class _Input(C.Structure):
    _fields_ = [("gaussians", C.c_void_p), ("harmonics", C.c_void_p),
                ("gaussian_count", C.c_uint32), ("sh_components", C.c_uint32)]


class _Camera(C.Structure):
    _fields_ = [("view", C.c_float * 16), ("proj", C.c_float * 16), ("position", C.c_float * 3),
                ("focal_x", C.c_float), ("focal_y", C.c_float),
                ("near_plane", C.c_float), ("far_plane", C.c_float)]


class _GlobalView(C.Structure):  # gsm_global_view
    _fields_ = [("input", _Input), ("camera", _Camera), ("width", C.c_uint32), ("height", C.c_uint32),
                ("color", C.c_void_p), ("color_pitch_bytes", C.c_size_t),
                ("depth", C.c_void_p), ("depth_pitch_bytes", C.c_size_t)]


class _GlobalObject(C.Structure):  # gsm_global_object
    _fields_ = [("input", _Input), ("camera", _Camera)]


class _Style(C.Structure):  # gsm_global_style
    _fields_ = [("tint_r", C.c_uint8), ("tint_g", C.c_uint8), ("tint_b", C.c_uint8), ("tint_amount", C.c_uint8),
                ("opacity_scale", C.c_uint8), ("hidden", C.c_uint8), ("pad", C.c_uint8 * 2)]


class _State(C.Structure):  # gsm_global_state
    _fields_ = [("state", C.c_void_p), ("default_state", C.c_uint32), ("pad", C.c_uint32)]


class _GlobalFrame(C.Structure):  # gsm_global_frame
    _fields_ = [("objects", C.POINTER(_GlobalObject)), ("object_count", C.c_uint32), ("width", C.c_uint32),
                ("height", C.c_uint32), ("color", C.c_void_p), ("color_pitch_bytes", C.c_size_t),
                ("depth_r16f", C.c_void_p), ("depth_pitch_bytes", C.c_size_t),
                ("pick_r32u", C.c_void_p), ("pick_pitch_bytes", C.c_size_t),
                ("occluder_r32f", C.c_void_p), ("occluder_pitch_bytes", C.c_size_t),
                ("states", C.POINTER(_State)), ("styles", C.POINTER(_Style)), ("style_count", C.c_uint32),
                ("flags", C.c_uint32)]


GLOBAL_FRAME_BYTES = 112  # include/gsm_renderer.h: sizeof(gsm_global_frame), asserted there
assert C.sizeof(_GlobalFrame) == GLOBAL_FRAME_BYTES


class _ExtractOut(C.Structure):  # gsm_global_extract_out
    _fields_ = [("gaussians", C.c_void_p), ("harmonics", C.c_void_p), ("state", C.c_void_p), ("ids", C.c_void_p),
                ("capacity", C.c_uint32), ("pad", C.c_uint32)]


EXTRACT_OUT_BYTES = 40  # include/gsm_renderer.h: sizeof(gsm_global_extract_out), asserted there
assert C.sizeof(_ExtractOut) == EXTRACT_OUT_BYTES


class _SelectQuery(C.Structure):  # gsm_global_select_query
    _fields_ = [("shape", C.c_uint32), ("flags", C.c_uint32), ("to_shape", C.c_float * 12),
                ("opacity_min", C.c_float), ("opacity_max", C.c_float), ("scale_min", C.c_float),
                ("scale_max", C.c_float), ("test_mask", C.c_uint32), ("test_value", C.c_uint32)]


class _Bounds(C.Structure):  # gsm_global_bounds
    _fields_ = [("min", C.c_float * 3), ("max", C.c_float * 3), ("count", C.c_uint32), ("skipped", C.c_uint32)]


SELECT_QUERY_BYTES, BOUNDS_BYTES = 80, 32  # include/gsm_renderer.h: asserted there
assert C.sizeof(_SelectQuery) == SELECT_QUERY_BYTES and C.sizeof(_Bounds) == BOUNDS_BYTES


class _Scene(C.Structure):  # gsm_global_scene
    _fields_ = [("gaussians", C.c_void_p), ("harmonics", C.c_void_p),
                ("gaussian_count", C.c_uint32), ("sh_components", C.c_uint32)]


class _TransformDesc(C.Structure):  # gsm_global_transform_desc
    _fields_ = [("matrix", C.c_float * 12), ("quaternion", C.c_float * 4), ("scale", C.c_float),
                ("sh1", C.c_float * 9), ("sh2", C.c_float * 25), ("sh3", C.c_float * 49)]


SCENE_BYTES, TRANSFORM_DESC_BYTES = 24, 400  # include/gsm_renderer.h: asserted there
assert C.sizeof(_Scene) == SCENE_BYTES and C.sizeof(_TransformDesc) == TRANSFORM_DESC_BYTES


class _FrameSortDesc(C.Structure):  # gsm_debug_frame_sort_desc (include/gsm_debug.h)
    _fields_ = [("shift", C.c_uint32), ("num_tiles", C.c_uint32), ("all_tiles", C.c_uint32),
                ("depth_sort", C.c_uint32), ("full", C.c_uint32), ("reserved", C.c_uint32)]


class _FrameSortOut(C.Structure):  # gsm_debug_frame_sort_out
    _fields_ = [("sorted_keys", C.c_void_p), ("sorted_values", C.c_void_p), ("tile_start", C.c_void_p),
                ("half0", C.c_void_p), ("half1", C.c_void_p), ("half_count", C.c_void_p),
                ("plan", C.c_uint32), ("reserved", C.c_uint32)]


class _Counters(C.Structure):
    _fields_ = [("total_assignments", C.c_uint32), ("max_capacity", C.c_uint32),
                ("padded_count", C.c_uint32), ("overflow", C.c_uint32), ("tiles_x", C.c_uint32),
                ("tiles_y", C.c_uint32), ("tile_count", C.c_uint32), ("gaussian_count", C.c_uint32)]


class _DfCounters(C.Structure):
    _fields_ = [("gaussian_count", C.c_uint32), ("visible", C.c_uint32), ("total_instances", C.c_uint32),
                ("max_instances", C.c_uint32), ("overflow", C.c_uint32), ("tiles_x", C.c_uint32),
                ("tiles_y", C.c_uint32), ("tile_count", C.c_uint32)]


class _DfOptions(C.Structure):  # gsm_depthfirst_options
    _fields_ = [("struct_bytes", C.c_uint32), ("depth_key_bits", C.c_uint32), ("tile_id_bits", C.c_uint32),
                ("reserved", C.c_uint32)]


class _LocalCounters(C.Structure):
    _fields_ = [("gaussian_count", C.c_uint32), ("visible", C.c_uint32), ("tiles_x", C.c_uint32),
                ("tiles_y", C.c_uint32), ("tile_count", C.c_uint32), ("active_tiles", C.c_uint32),
                ("total_entries", C.c_uint32), ("max_tile_count", C.c_uint32), ("max_per_tile", C.c_uint32),
                ("overflow", C.c_uint32)]


PICK_NONE = 0xFFFFFFFF  # include/gsm_renderer.h GSM_PICK_NONE
FRAME_ORTHOGRAPHIC = 2  # include/gsm_renderer.h GSM_FRAME_ORTHOGRAPHIC (gsm_global_frame.flags)

_LIB = None

# every function include/gsm_renderer.h and include/gsm_debug.h declare, with ctypes signature
_SIGNATURES = {
    "gsm_abi_version": ([], C.c_int),
    "gsm_status_string": ([C.c_int], C.c_char_p),
    "gsm_renderer_config_default": ([C.POINTER(_Config)], None),
    "gsm_camera_params_init": ([C.POINTER(_Camera), C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                C.c_float], None),
    "gsm_global_create": ([C.POINTER(_Config), C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "gsm_global_destroy": ([C.c_void_p], None),
    "gsm_global_render": ([C.c_void_p, C.c_void_p, C.POINTER(_Input), C.POINTER(_Camera), C.c_uint32,
                           C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t], C.c_int),
    "gsm_global_render_views": ([C.c_void_p, C.c_void_p, C.POINTER(_Input), C.POINTER(_Camera), C.c_uint32,
                                 C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p,
                                 C.c_size_t, C.c_size_t], C.c_int),
    "gsm_global_render_batch": ([C.c_void_p, C.c_void_p, C.POINTER(_GlobalView), C.c_uint32], C.c_int),
    "gsm_global_render_composite": ([C.c_void_p, C.c_void_p, C.POINTER(_GlobalObject), C.c_uint32, C.c_uint32,
                                     C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t], C.c_int),
    "gsm_global_render_pick": ([C.c_void_p, C.c_void_p, C.POINTER(_Input), C.POINTER(_Camera), C.c_uint32,
                                C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                C.c_size_t], C.c_int),
    "gsm_global_render_composite_pick": ([C.c_void_p, C.c_void_p, C.POINTER(_GlobalObject), C.c_uint32, C.c_uint32,
                                          C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.c_size_t], C.c_int),
    "gsm_global_render_occluded": ([C.c_void_p, C.c_void_p, C.POINTER(_Input), C.POINTER(_Camera), C.c_uint32,
                                    C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                    C.c_size_t], C.c_int),
    "gsm_global_render_composite_occluded": ([C.c_void_p, C.c_void_p, C.POINTER(_GlobalObject), C.c_uint32,
                                              C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p,
                                              C.c_size_t, C.c_void_p, C.c_size_t], C.c_int),
    "gsm_global_pick_owner": ([C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p], C.c_int),
    "gsm_global_render_styled": ([C.c_void_p, C.c_void_p, C.POINTER(_Input), C.POINTER(_Camera), C.c_uint32,
                                  C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                  C.POINTER(_State), C.POINTER(_Style), C.c_uint32], C.c_int),
    "gsm_global_render_composite_styled": ([C.c_void_p, C.c_void_p, C.POINTER(_GlobalObject), C.c_uint32, C.c_uint32,
                                            C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                            C.c_size_t, C.POINTER(_State), C.POINTER(_Style), C.c_uint32], C.c_int),
    "gsm_global_select_mask": ([C.c_void_p, C.c_void_p, C.POINTER(_Input), C.POINTER(_Camera), C.c_uint32,
                                C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(_Style), C.c_uint32,
                                C.c_uint32, C.c_uint32, C.c_void_p], C.c_int),
    "gsm_global_select_mask_ortho": ([C.c_void_p, C.c_void_p, C.POINTER(_Input), C.POINTER(_Camera), C.c_uint32,
                                      C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(_Style), C.c_uint32,
                                      C.c_uint32, C.c_uint32, C.c_void_p], C.c_int),
    "gsm_global_render_frame": ([C.c_void_p, C.c_void_p, C.POINTER(_GlobalFrame)], C.c_int),
    "gsm_global_select_pick": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p,
                                C.c_size_t, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p],
                               C.c_int),
    "gsm_global_render_frames": ([C.c_void_p, C.c_void_p, C.POINTER(_GlobalFrame), C.c_uint32], C.c_int),
    "gsm_global_select_pick_ids": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32,
                                    C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                    C.c_void_p], C.c_int),
    "gsm_global_keep_visible": ([C.POINTER(_Style), C.c_uint32, C.POINTER(C.c_uint32)], None),
    "gsm_global_keep_masked": ([C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)], None),
    "gsm_global_extract": ([C.c_void_p, C.c_void_p, C.POINTER(_Input), C.POINTER(_State), C.POINTER(C.c_uint32),
                            C.POINTER(_ExtractOut), C.c_void_p], C.c_int),
    "gsm_global_state_histogram": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p], C.c_int),
    "gsm_global_select_query_default": ([C.POINTER(_SelectQuery)], None),
    "gsm_global_select_where": ([C.c_void_p, C.c_void_p, C.POINTER(_Input), C.POINTER(_SelectQuery), C.c_void_p,
                                 C.POINTER(_Style), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p], C.c_int),
    "gsm_global_state_bounds": ([C.c_void_p, C.c_void_p, C.POINTER(_Input), C.POINTER(_State),
                                 C.POINTER(C.c_uint32), C.c_void_p], C.c_int),
    "gsm_global_transform_from_pose": ([C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_float),
                                        C.POINTER(_TransformDesc)], C.c_int),
    "gsm_global_transform": ([C.c_void_p, C.c_void_p, C.POINTER(_Scene), C.POINTER(_State), C.POINTER(C.c_uint32),
                              C.POINTER(_TransformDesc)], C.c_int),
    "gsm_global_render_stereo": ([C.c_void_p, C.c_void_p, C.POINTER(_Input), C.POINTER(_Camera),
                                  C.POINTER(_Camera), C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                                  C.c_void_p, C.c_size_t], C.c_int),
    "gsm_global_render_stereo_sbs": ([C.c_void_p, C.c_void_p, C.POINTER(_Input), C.POINTER(_Camera),
                                      C.POINTER(_Camera), C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                                      C.c_void_p, C.c_size_t], C.c_int),
    "gsm_global_debug_read_total_assignments": ([C.c_void_p], C.c_uint32),
    "gsm_global_last_gpu_time": ([C.c_void_p, C.POINTER(C.c_double)], C.c_int),
    "gsm_global_debug_counters": ([C.c_void_p, C.POINTER(_Counters)], C.c_int),
    "gsm_global_debug_blend_kernel": ([C.c_void_p, C.POINTER(C.c_int)], C.c_int),
    "gsm_debug_sort_workspace_bytes": ([C.c_uint32], C.c_size_t),
    "gsm_debug_sort_plan_fits": ([C.c_uint32, C.c_uint32, C.c_int, C.c_size_t], C.c_int),
    "gsm_global_debug_copy": ([C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)],
                              C.c_int),
    "gsm_global_set_profiling": ([C.c_void_p, C.c_int], C.c_int),
    "gsm_global_stage_times": ([C.c_void_p, C.POINTER(C.c_float), C.c_int], C.c_int),
    "gsm_global_set_tile_rows": ([C.c_void_p, C.c_uint32, C.c_uint32], C.c_int),
    "gsm_sort_pairs_u32": ([C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p], C.c_int),
    "gsm_debug_frame_sort_create": ([C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "gsm_debug_frame_sort_destroy": ([C.c_void_p], None),
    "gsm_debug_frame_sort_run": ([C.c_void_p, C.c_void_p, C.POINTER(_FrameSortDesc), C.c_void_p, C.c_void_p,
                                  C.c_uint32, C.POINTER(_FrameSortOut)], C.c_int),
    # include/gsm_multigpu.h
    "gsm_global_project_partition": ([C.c_void_p, C.c_void_p, C.POINTER(_Input), C.POINTER(_Camera),
                                      C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.POINTER(C.c_uint32), C.c_uint32, C.c_void_p, C.c_uint64,
                                      C.c_void_p], C.c_int),
    "gsm_global_render_records": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                   C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t], C.c_int),
    # include/gsm_depthfirst.h
    "gsm_depthfirst_create": ([C.POINTER(_Config), C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "gsm_depthfirst_default_options": ([C.POINTER(_DfOptions)], None),
    "gsm_depthfirst_create_with_options": ([C.POINTER(_Config), C.c_int, C.POINTER(_DfOptions),
                                            C.POINTER(C.c_void_p)], C.c_int),
    "gsm_depthfirst_get_options": ([C.c_void_p, C.POINTER(_DfOptions)], C.c_int),
    "gsm_depthfirst_destroy": ([C.c_void_p], None),
    "gsm_depthfirst_render_stereo_sbs": ([C.c_void_p, C.c_void_p, C.POINTER(_Input), C.POINTER(_Camera),
                                          C.POINTER(_Camera), C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                          C.c_size_t], C.c_int),
    "gsm_depthfirst_render": ([C.c_void_p, C.c_void_p, C.POINTER(_Input), C.POINTER(_Camera), C.c_uint32,
                               C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t], C.c_int),
    "gsm_depthfirst_debug_counters": ([C.c_void_p, C.POINTER(_DfCounters)], C.c_int),
    "gsm_depthfirst_debug_copy": ([C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)],
                                  C.c_int),
    "gsm_depthfirst_set_profiling": ([C.c_void_p, C.c_int], C.c_int),
    "gsm_depthfirst_stage_times": ([C.c_void_p, C.POINTER(C.c_float), C.c_int], C.c_int),
    "gsm_depthfirst_last_gpu_time": ([C.c_void_p, C.POINTER(C.c_double)], C.c_int),
    "gsm_debug_sort_rank_probe": ([C.c_int, C.POINTER(C.c_int)], C.c_int),
    "gsm_debug_partition_counts": ([C.c_void_p, C.c_void_p, C.POINTER(_Input), C.POINTER(_Camera), C.c_uint32,
                                    C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32,
                                    C.c_void_p], C.c_int),
    "gsm_debug_partition_push": ([C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                  C.POINTER(C.c_void_p), C.c_void_p], C.c_int),
    "gsm_debug_render_records_device_count": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                               C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p,
                                               C.c_size_t], C.c_int),
    "gsm_multigpu_create": ([C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    # (options structs passed as pointers: _MgOptions, gsm_multigpu_options)
    "gsm_multigpu_default_options": ([C.c_void_p], None),
    "gsm_multigpu_prepare_with_options": ([C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p),
                                           C.c_void_p], C.c_int),
    "gsm_multigpu_create_with_options": ([C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                          C.POINTER(C.c_void_p)], C.c_int),
    "gsm_multigpu_destroy": ([C.c_void_p], None),
    "gsm_multigpu_render": ([C.c_void_p, C.c_void_p, C.POINTER(_Input), C.POINTER(_Camera), C.c_uint32,
                             C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p], C.c_int),
    "gsm_multigpu_debug_counts": ([C.c_void_p, C.POINTER(C.c_uint32)], C.c_int),
    "gsm_multigpu_prepare": ([C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p], C.c_int),
    "gsm_multigpu_connect": ([C.c_void_p, C.c_void_p], C.c_int),
    "gsm_multigpu_render_phase": ([C.c_void_p, C.c_int, C.c_void_p, C.POINTER(_Input), C.POINTER(_Camera),
                                   C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                   C.c_void_p], C.c_int),
    "gsm_multigpu_frame": ([C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)], C.c_int),
    "gsm_multigpu_status": ([C.c_void_p, C.POINTER(C.c_uint32), C.c_int], C.c_int),
    "gsm_multigpu_set_timeout_ms": ([C.c_void_p, C.c_uint32], C.c_int),
    "gsm_multigpu_debug_copy_exchange": ([C.c_void_p, C.c_void_p, C.c_size_t], C.c_int),
    "gsm_multigpu_debug_copy_frame": ([C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32], C.c_int),
    "gsm_multigpu_debug_copy_depth": ([C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32], C.c_int),
    "gsm_multigpu_frame_depth": ([C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)], C.c_int),
    "gsm_multigpu_errors": ([C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int], C.c_int),
    "gsm_multigpu_finish_frame": ([C.c_void_p, C.c_void_p], C.c_int),
    "gsm_multigpu_wait_event": ([C.c_void_p, C.c_void_p], C.c_int),
    "gsm_multigpu_debug_set_epoch": ([C.c_void_p, C.c_uint32], C.c_int),
}

# every function include/gsm_local.h declares (the LocalRenderer frame)
_LOCAL_SIGNATURES = {
    "gsm_local_create": ([C.POINTER(_Config), C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "gsm_local_destroy": ([C.c_void_p], None),
    "gsm_local_render": ([C.c_void_p, C.c_void_p, C.POINTER(_Input), C.POINTER(_Camera), C.c_uint32,
                          C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t], C.c_int),
    "gsm_local_debug_counters": ([C.c_void_p, C.POINTER(_LocalCounters)], C.c_int),
    "gsm_local_debug_copy": ([C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)], C.c_int),
    "gsm_local_debug_sort_tiles": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                    C.c_void_p], C.c_int),
    "gsm_local_set_profiling": ([C.c_void_p, C.c_int], C.c_int),
    "gsm_local_stage_times": ([C.c_void_p, C.POINTER(C.c_float), C.c_int], C.c_int),
    "gsm_local_last_gpu_time": ([C.c_void_p, C.POINTER(C.c_double)], C.c_int),
}

SPLAT_RECORD_BYTES = 48  # include/gsm_multigpu.h GSM_SPLAT_RECORD_BYTES
MAX_SLABS = 16
MULTIGPU_HANDLE_BYTES = 256  # GSM_MULTIGPU_HANDLE_BYTES


def _lib():
    """Load libgsm_amd.so (built in-tree by __graft_entry__.build / make).  Raises if absent:
    there is deliberately no fallback path."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"libgsm_amd.so not built: {LIB_PATH} (run `make -C gsm-renderer_amd`)")
        L = C.CDLL(LIB_PATH)
        for name, (args, res) in list(_SIGNATURES.items()) + list(_LOCAL_SIGNATURES.items()):
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = res
        _LIB = L
    return _LIB


def library_path() -> str:
    return LIB_PATH


def _check(st: int, what: str = ""):
    if st != 0:
        raise RendererError(st, what)


def _ptr(t) -> Optional[int]:
    if t is None:
        return None
    if isinstance(t, int):
        return t
    return int(t.data_ptr())


def _camera_struct(cam: CameraParams) -> _Camera:
    c = _Camera()
    c.view[:] = [float(v) for v in np.asarray(cam.view, np.float32).reshape(16)]
    c.proj[:] = [float(v) for v in np.asarray(cam.proj, np.float32).reshape(16)]
    c.position[:] = [float(v) for v in np.asarray(cam.position, np.float32).reshape(3)]
    c.focal_x, c.focal_y = float(cam.focal_x), float(cam.focal_y)
    c.near_plane, c.far_plane = float(cam.near), float(cam.far)
    return c


def _stream_handle(stream) -> Optional[int]:
    if stream is None:
        if torch is not None and torch.cuda.is_available():
            return int(torch.cuda.current_stream().cuda_stream)
        return None
    if isinstance(stream, int):
        return stream
    return int(stream.cuda_stream)


class _Renderer:
    """What the single-device renderers share over their C entry points <_PREFIX>_*: the handle's
    life, the stage times, the counters and the raw two-call debug copy."""
    _PREFIX = ""       # gsm_global | gsm_depthfirst | gsm_local
    _STAGE_NAMES = ()  # stage_times_ms keys, in the C enum's order
    _COUNTERS = None   # the ctypes struct <_PREFIX>_debug_counters fills

    def _fn(self, name: str):
        return getattr(_lib(), f"{self._PREFIX}_{name}")

    def _open(self, device: Optional[int], config: RendererConfig, create: str = "create", *options):
        """<_PREFIX>_<create>(config, device, *options, &handle)"""
        self.config = config
        cfg = _Config(int(config.max_gaussians), int(config.max_width), int(config.max_height),
                      int(config.precision), int(config.color_format),
                      int(config.gaussian_color_space), int(bool(config.back_to_front)))
        h = C.c_void_p()
        dev = -1 if device is None else int(device)
        _check(self._fn(create)(C.byref(cfg), dev, *options, C.byref(h)), f"{self._PREFIX}_{create}")
        self._h = h
        self.device = dev
        self._bpp = ColorFormat(int(config.color_format)).bytes_per_pixel

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._fn("destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    @property
    def last_gpu_time(self) -> Optional[float]:
        s = C.c_double()
        st = self._fn("last_gpu_time")(self._h, C.byref(s))
        return float(s.value) if st == 0 else None

    def stage_times_ms(self) -> dict:
        arr = (C.c_float * len(self._STAGE_NAMES))()
        _check(self._fn("stage_times")(self._h, arr, len(arr)), f"{self._PREFIX}_stage_times")
        return {k: float(v) for k, v in zip(self._STAGE_NAMES, arr)}

    def counters(self) -> dict:
        c = self._COUNTERS()
        _check(self._fn("debug_counters")(self._h, C.byref(c)), f"{self._PREFIX}_debug_counters")
        return {name: int(getattr(c, name)) for name, _ in c._fields_}

    def _debug_copy(self, which) -> np.ndarray:
        """The bytes of buffer `which`: one call for the size, one for the copy."""
        copy = self._fn("debug_copy")
        need = C.c_size_t()
        _check(copy(self._h, int(which), None, 0, C.byref(need)), "debug_copy")
        n = int(need.value)
        raw = np.zeros(max(n, 1), np.uint8)
        if n:
            _check(copy(self._h, int(which), raw.ctypes.data, n, None), "debug_copy")
        return raw[:n]


def _object_array(objects):
    """(gsm_global_object array, count) of a SceneObject list, for the composite entries; (None, 1) for None (a
    NULL array, which the library refuses)."""
    if objects is None:
        return None, 1
    n = len(objects)
    arr = (_GlobalObject * max(n, 1))()
    for g, o in zip(arr, objects):
        g.input = _Input(_ptr(o.input.gaussians), _ptr(o.input.harmonics), int(o.input.gaussian_count),
                         int(o.input.sh_components))
        g.camera = _camera_struct(o.camera)
    return arr, n


def _style_array(styles):
    """(gsm_global_style array, count) of a Style list; (None, 0) for None (a NULL table, which the styled
    entries refuse and the select takes as "no styles")."""
    if styles is None:
        return None, 0
    arr = (_Style * max(len(styles), 1))()
    for d, s in zip(arr, styles):
        d.tint_r, d.tint_g, d.tint_b = (int(v) for v in s.tint)
        d.tint_amount, d.opacity_scale, d.hidden = int(s.tint_amount), int(s.opacity_scale), 1 if s.hidden else 0
    return arr, len(styles)


def _state_struct(state) -> _State:
    """gsm_global_state of a device byte tensor (its state array) or of an int (no array: that default)."""
    if isinstance(state, int):
        return _State(None, int(state), 0)
    return _State(_ptr(state), 0, 0)


def _select_query_struct(q: SelectQuery) -> _SelectQuery:
    s = _SelectQuery()
    s.shape, s.flags = int(q.shape) & 0xFFFFFFFF, int(q.flags) & 0xFFFFFFFF
    s.to_shape[:] = [float(v) for v in np.asarray(q.to_shape, np.float32).reshape(12)]
    s.opacity_min, s.opacity_max = float(q.opacity_min), float(q.opacity_max)
    s.scale_min, s.scale_max = float(q.scale_min), float(q.scale_max)
    s.test_mask, s.test_value = int(q.test_mask) & 0xFFFFFFFF, int(q.test_value) & 0xFFFFFFFF
    return s


class GlobalRenderer(_Renderer):
    """GlobalRenderer (GlobalRenderer.swift:72-572) on one HIP device."""
    _PREFIX, _STAGE_NAMES, _COUNTERS = "gsm_global", STAGES, _Counters

    def __init__(self, device: Optional[int] = None, config: RendererConfig = RendererConfig()):
        self._open(device, config)

    # -- GlobalRenderer.render (GlobalRenderer.swift:201-238) --
    def render(self, color_texture, depth_texture, input: GaussianInput, camera: CameraParams,
               width: int, height: int, stream=None, color_pitch: Optional[int] = None,
               depth_pitch: Optional[int] = None):
        inp = _Input(_ptr(input.gaussians), _ptr(input.harmonics), int(input.gaussian_count),
                     int(input.sh_components))
        cam = _camera_struct(camera)
        cp = color_pitch if color_pitch is not None else int(width) * self._bpp
        dp = depth_pitch if depth_pitch is not None else int(width) * 2
        st = _lib().gsm_global_render(self._h, _stream_handle(stream), C.byref(inp), C.byref(cam),
                                      int(width), int(height), _ptr(color_texture), cp,
                                      _ptr(depth_texture), dp)
        _check(st, "gsm_global_render")

    def render_views(self, color_texture, depth_texture, input: GaussianInput, cameras, width: int, height: int,
                     stream=None, color_pitch: Optional[int] = None, depth_pitch: Optional[int] = None,
                     color_view_stride: Optional[int] = None, depth_view_stride: Optional[int] = None):
        """gsm_global_render_views: len(cameras) views of one scene in one frame; view v's targets start v
        view strides (default: height rows) after color_texture / depth_texture.  cameras None: a NULL
        camera array with view_count 1 (the C entry's error path)."""
        inp = _Input(_ptr(input.gaussians), _ptr(input.harmonics), int(input.gaussian_count),
                     int(input.sh_components))
        n = 1 if cameras is None else len(cameras)
        cams = None if cameras is None else (_Camera * max(n, 1))(*[_camera_struct(c) for c in cameras])
        cp = color_pitch if color_pitch is not None else int(width) * self._bpp
        dp = depth_pitch if depth_pitch is not None else int(width) * 2
        cs = color_view_stride if color_view_stride is not None else int(height) * cp
        ds = depth_view_stride if depth_view_stride is not None else int(height) * dp
        st = _lib().gsm_global_render_views(self._h, _stream_handle(stream), C.byref(inp), cams, n, int(width),
                                            int(height), _ptr(color_texture), cp, cs, _ptr(depth_texture), dp, ds)
        _check(st, "gsm_global_render_views")

    def render_batch(self, views, stream=None):
        """gsm_global_render_batch: the BatchView list `views` -- different scenes, sizes and targets -- in one
        frame; every view's bytes equal those of `render` for that view alone.  views None: a NULL array with
        view_count 1 (the C entry's error path)."""
        n = 1 if views is None else len(views)
        arr = None
        if views is not None:
            arr = (_GlobalView * max(n, 1))()
            for g, v in zip(arr, views):
                g.input = _Input(_ptr(v.input.gaussians), _ptr(v.input.harmonics), int(v.input.gaussian_count),
                                 int(v.input.sh_components))
                g.camera = _camera_struct(v.camera)
                g.width, g.height = int(v.width), int(v.height)
                g.color, g.depth = _ptr(v.color), _ptr(v.depth)
                g.color_pitch_bytes = int(v.color_pitch) if v.color_pitch is not None else int(v.width) * self._bpp
                g.depth_pitch_bytes = int(v.depth_pitch) if v.depth_pitch is not None else int(v.width) * 2
        _check(_lib().gsm_global_render_batch(self._h, _stream_handle(stream), arr, n), "gsm_global_render_batch")

    def render_pick(self, color_texture, depth_texture, pick_texture, input: GaussianInput, camera: CameraParams,
                    width: int, height: int, stream=None, color_pitch: Optional[int] = None,
                    depth_pitch: Optional[int] = None, pick_pitch: Optional[int] = None):
        """gsm_global_render_pick: `render` plus a pick target -- an int32 / uint32 tensor of shape (H, W), or
        pitched -- that receives, per pixel, the gaussian id of the heaviest contribution (PICK_NONE: none)."""
        inp = _Input(_ptr(input.gaussians), _ptr(input.harmonics), int(input.gaussian_count),
                     int(input.sh_components))
        cam = _camera_struct(camera)
        cp = color_pitch if color_pitch is not None else int(width) * self._bpp
        dp = depth_pitch if depth_pitch is not None else int(width) * 2
        pp = pick_pitch if pick_pitch is not None else int(width) * 4
        st = _lib().gsm_global_render_pick(self._h, _stream_handle(stream), C.byref(inp), C.byref(cam), int(width),
                                           int(height), _ptr(color_texture), cp, _ptr(depth_texture), dp,
                                           _ptr(pick_texture), pp)
        _check(st, "gsm_global_render_pick")

    def render_composite_pick(self, color_texture, depth_texture, pick_texture, objects, width: int, height: int,
                              stream=None, color_pitch: Optional[int] = None, depth_pitch: Optional[int] = None,
                              pick_pitch: Optional[int] = None):
        """gsm_global_render_composite_pick: `render_composite` plus a pick target that receives, per pixel, the
        composite's item of the heaviest contribution (pick_owner maps items to objects and gaussian ids)."""
        arr, n = _object_array(objects)
        cp = color_pitch if color_pitch is not None else int(width) * self._bpp
        dp = depth_pitch if depth_pitch is not None else int(width) * 2
        pp = pick_pitch if pick_pitch is not None else int(width) * 4
        st = _lib().gsm_global_render_composite_pick(self._h, _stream_handle(stream), arr, n, int(width),
                                                     int(height), _ptr(color_texture), cp, _ptr(depth_texture), dp,
                                                     _ptr(pick_texture), pp)
        _check(st, "gsm_global_render_composite_pick")

    def render_occluded(self, color_texture, depth_texture, occluder, input: GaussianInput, camera: CameraParams,
                        width: int, height: int, stream=None, color_pitch: Optional[int] = None,
                        depth_pitch: Optional[int] = None, occluder_pitch: Optional[int] = None):
        """gsm_global_render_occluded: `render` cut at an opaque surface -- `occluder` is a float32 CUDA tensor of
        shape (H, W), or pitched, holding the surface's view-space depth (clip.w) per pixel; +inf occludes nothing."""
        inp = _Input(_ptr(input.gaussians), _ptr(input.harmonics), int(input.gaussian_count),
                     int(input.sh_components))
        cam = _camera_struct(camera)
        cp = color_pitch if color_pitch is not None else int(width) * self._bpp
        dp = depth_pitch if depth_pitch is not None else int(width) * 2
        op = occluder_pitch if occluder_pitch is not None else int(width) * 4
        st = _lib().gsm_global_render_occluded(self._h, _stream_handle(stream), C.byref(inp), C.byref(cam),
                                               int(width), int(height), _ptr(color_texture), cp,
                                               _ptr(depth_texture), dp, _ptr(occluder), op)
        _check(st, "gsm_global_render_occluded")

    def render_composite_occluded(self, color_texture, depth_texture, occluder, objects, width: int, height: int,
                                  stream=None, color_pitch: Optional[int] = None, depth_pitch: Optional[int] = None,
                                  occluder_pitch: Optional[int] = None):
        """gsm_global_render_composite_occluded: `render_composite` cut at the same kind of occluder, in the depth
        unit of the composite's shared projection."""
        arr, n = _object_array(objects)
        cp = color_pitch if color_pitch is not None else int(width) * self._bpp
        dp = depth_pitch if depth_pitch is not None else int(width) * 2
        op = occluder_pitch if occluder_pitch is not None else int(width) * 4
        st = _lib().gsm_global_render_composite_occluded(self._h, _stream_handle(stream), arr, n, int(width),
                                                         int(height), _ptr(color_texture), cp, _ptr(depth_texture),
                                                         dp, _ptr(occluder), op)
        _check(st, "gsm_global_render_composite_occluded")

    def render_styled(self, color_texture, depth_texture, pick_texture, input: GaussianInput, camera: CameraParams,
                      width: int, height: int, state, styles, stream=None, color_pitch: Optional[int] = None,
                      depth_pitch: Optional[int] = None, pick_pitch: Optional[int] = None,
                      style_count: Optional[int] = None):
        """gsm_global_render_styled: `render` (pick_texture None) or `render_pick` with the Style of every
        gaussian's state applied in the projection.  state: a uint8 CUDA tensor, one byte per gaussian, or an int
        (every gaussian's state); None passes a NULL gsm_global_state (the C entry's error path).  styles: a Style
        list (None: a NULL table); style_count overrides its length."""
        inp = _Input(_ptr(input.gaussians), _ptr(input.harmonics), int(input.gaussian_count),
                     int(input.sh_components))
        cam = _camera_struct(camera)
        cp = color_pitch if color_pitch is not None else int(width) * self._bpp
        dp = depth_pitch if depth_pitch is not None else int(width) * 2
        pp = pick_pitch if pick_pitch is not None else int(width) * 4
        arr, n = _style_array(styles)
        st = _lib().gsm_global_render_styled(self._h, _stream_handle(stream), C.byref(inp), C.byref(cam), int(width),
                                             int(height), _ptr(color_texture), cp, _ptr(depth_texture), dp,
                                             _ptr(pick_texture), pp,
                                             None if state is None else C.byref(_state_struct(state)), arr,
                                             n if style_count is None else int(style_count))
        _check(st, "gsm_global_render_styled")

    def render_composite_styled(self, color_texture, depth_texture, pick_texture, objects, width: int, height: int,
                                states, styles, stream=None, color_pitch: Optional[int] = None,
                                depth_pitch: Optional[int] = None, pick_pitch: Optional[int] = None,
                                style_count: Optional[int] = None):
        """gsm_global_render_composite_styled: `render_composite` (pick_texture None) or `render_composite_pick`
        with styles.  states: one entry per object, each a uint8 CUDA tensor or an int (the whole object's state);
        None passes a NULL array."""
        arr, n = _object_array(objects)
        cp = color_pitch if color_pitch is not None else int(width) * self._bpp
        dp = depth_pitch if depth_pitch is not None else int(width) * 2
        pp = pick_pitch if pick_pitch is not None else int(width) * 4
        sarr, sn = _style_array(styles)
        starr = None
        if states is not None:
            starr = (_State * max(len(states), 1))(*[_state_struct(s) for s in states])
        st = _lib().gsm_global_render_composite_styled(self._h, _stream_handle(stream), arr, n, int(width),
                                                       int(height), _ptr(color_texture), cp, _ptr(depth_texture), dp,
                                                       _ptr(pick_texture), pp, starr, sarr,
                                                       sn if style_count is None else int(style_count))
        _check(st, "gsm_global_render_composite_styled")

    def select_mask(self, input: GaussianInput, camera: CameraParams, width: int, height: int, mask, state,
                    and_mask: int, xor_mask: int, styles=None, matched=None, stream=None,
                    mask_pitch: Optional[int] = None, style_count: Optional[int] = None, orthographic: bool = False):
        """gsm_global_select_mask (orthographic: gsm_global_select_mask_ortho, the same select under the
        orthographic projection rule): the state byte of every gaussian whose projected centre lies on a nonzero byte
        of `mask` (uint8 CUDA tensor, height rows of mask_pitch bytes) becomes (old & and_mask) ^ xor_mask; with
        `styles`, gaussians whose current state is hidden are skipped.  matched: an int32 / uint32 CUDA tensor of
        one element that receives the count.  input.harmonics may be None."""
        inp = _Input(_ptr(input.gaussians), _ptr(input.harmonics), int(input.gaussian_count), 0)
        cam = _camera_struct(camera)
        mp = mask_pitch if mask_pitch is not None else int(width)
        sarr, sn = _style_array(styles)
        name = "gsm_global_select_mask_ortho" if orthographic else "gsm_global_select_mask"
        st = getattr(_lib(), name)(self._h, _stream_handle(stream), C.byref(inp), C.byref(cam), int(width),
                                   int(height), _ptr(mask), mp, _ptr(state), sarr,
                                   sn if style_count is None else int(style_count),
                                   int(and_mask) & 0xFFFFFFFF, int(xor_mask) & 0xFFFFFFFF, _ptr(matched))
        _check(st, name)

    def render_frame(self, color_texture, depth_texture, objects, width: int, height: int, pick=None, occluder=None,
                     states=None, styles=None, stream=None, color_pitch: Optional[int] = None,
                     depth_pitch: Optional[int] = None, pick_pitch: Optional[int] = None,
                     occluder_pitch: Optional[int] = None, style_count: Optional[int] = None, flags: int = 0,
                     null_frame: bool = False, orthographic: bool = False):
        """gsm_global_render_frame: one descriptor for every Single and Compose frame and every combination of a
        pick target, an occluder and styles.  objects: a SceneObject list, or one (GaussianInput, CameraParams)
        pair as a single object; None passes a NULL array with object_count 1.  pick / occluder: as for
        `render_pick` / `render_occluded`, None leaves the option out.  states: one entry per object (a uint8 CUDA
        tensor or an int), or a single such value for a single object; styles: a Style list.  null_frame passes a
        NULL descriptor (the C entry's error path).  orthographic: every object is projected by the orthographic
        rule (scenes.ortho_camera builds such a camera); FRAME_ORTHOGRAPHIC is or-ed into flags."""
        f = _GlobalFrame()
        keep = self._fill_frame(f, color_texture, depth_texture, objects, width, height, pick, occluder, states, styles,
                                color_pitch, depth_pitch, pick_pitch, occluder_pitch, style_count,
                                int(flags) | (FRAME_ORTHOGRAPHIC if orthographic else 0))
        st = _lib().gsm_global_render_frame(self._h, _stream_handle(stream), None if null_frame else C.byref(f))
        del keep
        _check(st, "gsm_global_render_frame")

    def _fill_frame(self, f, color_texture, depth_texture, objects, width, height, pick=None, occluder=None,
                    states=None, styles=None, color_pitch=None, depth_pitch=None, pick_pitch=None,
                    occluder_pitch=None, style_count=None, flags=0):
        """Fills the gsm_global_frame `f` (render_frame's arguments); returns the ctypes arrays it points to, which
        the caller keeps alive until the C call has returned."""
        single = isinstance(objects, tuple) and len(objects) == 2 and isinstance(objects[0], GaussianInput)
        if single:
            objects = [SceneObject(objects[0], objects[1])]
            if states is not None and not isinstance(states, (list, tuple)):
                states = [states]
        arr, n = _object_array(objects)
        sarr, sn = _style_array(styles)
        starr = None
        if states is not None:
            starr = (_State * max(len(states), 1))(*[_state_struct(s) for s in states])
        f.objects = arr if arr is not None else C.POINTER(_GlobalObject)()
        f.object_count, f.width, f.height = n, int(width), int(height)
        f.color, f.depth_r16f = _ptr(color_texture), _ptr(depth_texture)
        f.color_pitch_bytes = color_pitch if color_pitch is not None else int(width) * self._bpp
        f.depth_pitch_bytes = depth_pitch if depth_pitch is not None else int(width) * 2
        f.pick_r32u, f.occluder_r32f = _ptr(pick), _ptr(occluder)
        f.pick_pitch_bytes = pick_pitch if pick_pitch is not None else int(width) * 4
        f.occluder_pitch_bytes = occluder_pitch if occluder_pitch is not None else int(width) * 4
        f.states = starr if starr is not None else C.POINTER(_State)()
        f.styles = sarr if sarr is not None else C.POINTER(_Style)()
        f.style_count = sn if style_count is None else int(style_count)
        f.flags = int(flags)
        return arr, sarr, starr

    def render_frames(self, frames, stream=None):
        """gsm_global_render_frames: the Frame list `frames` -- each a scene, camera, size and targets with its own
        optional pick target, occluder and styles -- in one batch; every frame's bytes equal those of
        `render_frame` for that frame alone, and a pick pixel holds the gaussian id of its frame's scene.  frames
        None: a NULL array with frame_count 1 (the C entry's error path)."""
        n = 1 if frames is None else len(frames)
        arr, keep = None, []
        if frames is not None:
            arr = (_GlobalFrame * max(n, 1))()
            for f, d in zip(arr, frames):
                keep.append(self._fill_frame(f, d.color, d.depth, d.objects, d.width, d.height, d.pick, d.occluder,
                                             d.states, d.styles, d.color_pitch, d.depth_pitch, d.pick_pitch,
                                             d.occluder_pitch, d.style_count,
                                             int(d.flags) | (FRAME_ORTHOGRAPHIC if d.orthographic else 0)))
        st = _lib().gsm_global_render_frames(self._h, _stream_handle(stream), arr, n)
        del keep
        _check(st, "gsm_global_render_frames")

    def select_pick_ids(self, pick, width: int, height: int, state, gaussian_count: int, and_mask: int,
                        xor_mask: int, mask=None, matched=None, stream=None, pick_pitch: Optional[int] = None,
                        mask_pitch: Optional[int] = None):
        """gsm_global_select_pick_ids: `select_pick` for a pick image that holds gaussian ids (a frame of
        `render_frames`): every id below gaussian_count that the image shows on a nonzero byte of `mask` (None:
        every pixel) gets (old & and_mask) ^ xor_mask, once.  Reads no state of the handle's last frame."""
        pp = pick_pitch if pick_pitch is not None else int(width) * 4
        mp = mask_pitch if mask_pitch is not None else int(width)
        st = _lib().gsm_global_select_pick_ids(self._h, _stream_handle(stream), _ptr(pick), pp, int(width),
                                               int(height), _ptr(mask), mp, _ptr(state), int(gaussian_count),
                                               int(and_mask) & 0xFFFFFFFF, int(xor_mask) & 0xFFFFFFFF,
                                               _ptr(matched))
        _check(st, "gsm_global_select_pick_ids")

    def select_pick(self, pick, width: int, height: int, object: int, state, gaussian_count: int, and_mask: int,
                    xor_mask: int, mask=None, matched=None, stream=None, pick_pitch: Optional[int] = None,
                    mask_pitch: Optional[int] = None):
        """gsm_global_select_pick: the state byte of every gaussian of `object` that the last pick frame's image
        `pick` shows on a nonzero byte of `mask` (None: every pixel) becomes (old & and_mask) ^ xor_mask, once per
        gaussian.  matched: an int32 / uint32 CUDA tensor of one element that receives the count."""
        pp = pick_pitch if pick_pitch is not None else int(width) * 4
        mp = mask_pitch if mask_pitch is not None else int(width)
        st = _lib().gsm_global_select_pick(self._h, _stream_handle(stream), _ptr(pick), pp, int(width), int(height),
                                           _ptr(mask), mp, int(object), _ptr(state), int(gaussian_count),
                                           int(and_mask) & 0xFFFFFFFF, int(xor_mask) & 0xFFFFFFFF, _ptr(matched))
        _check(st, "gsm_global_select_pick")

    def extract(self, input: GaussianInput, state, keep, out_gaussians, out_harmonics, out_state=None, out_ids=None,
                capacity: Optional[int] = None, kept=None, stream=None):
        """gsm_global_extract: the rows of the gaussians whose state byte has its bit in `keep`, in ascending id
        order, into the first min(K, capacity) rows of the outputs; `kept` (an int32 / uint32 CUDA tensor of one
        element; None: one is allocated) receives K and is returned.  state: as the styled entries take it (a uint8
        CUDA tensor, an int for every gaussian's state, None for a NULL struct).  keep: a sequence of 8 words
        (keep_visible, keep_masked; None: NULL).  out_state (uint8) and out_ids (int32 / uint32) may be None.
        capacity defaults to the rows out_gaussians holds."""
        inp = _Input(_ptr(input.gaussians), _ptr(input.harmonics), int(input.gaussian_count),
                     int(input.sh_components))
        if capacity is None:
            record = 32 if int(self.config.precision) == RenderPrecision.FLOAT16 else 48
            capacity = 0 if out_gaussians is None else out_gaussians.numel() * out_gaussians.element_size() // record
        if kept is None:
            kept = torch.zeros(1, dtype=torch.int32, device=getattr(out_gaussians, "device", "cuda"))
        out = _ExtractOut(_ptr(out_gaussians), _ptr(out_harmonics), _ptr(out_state), _ptr(out_ids), int(capacity), 0)
        words = None if keep is None else (C.c_uint32 * 8)(*[int(w) & 0xFFFFFFFF for w in keep])
        st = _lib().gsm_global_extract(self._h, _stream_handle(stream), C.byref(inp),
                                       None if state is None else C.byref(_state_struct(state)), words, C.byref(out),
                                       _ptr(kept))
        _check(st, "gsm_global_extract")
        return kept

    def state_histogram(self, state, count: int, histogram, stream=None):
        """gsm_global_state_histogram: histogram[s] (an int32 / uint32 CUDA tensor of 256 elements) becomes the
        number of the first `count` bytes of `state` (a uint8 CUDA tensor) that equal s."""
        st = _lib().gsm_global_state_histogram(self._h, _stream_handle(stream), _ptr(state), int(count),
                                               _ptr(histogram))
        _check(st, "gsm_global_state_histogram")

    def select_where(self, input: GaussianInput, query, state, and_mask: int, xor_mask: int, styles=None,
                     matched=None, stream=None, style_count: Optional[int] = None):
        """gsm_global_select_where: the state byte of every gaussian whose record matches `query` (a SelectQuery;
        None: NULL) becomes (old & and_mask) ^ xor_mask -- inside or outside a box or an ellipsoid in scene space,
        opacity and largest scale in a range, a test on the current state; with `styles`, gaussians whose current
        state is hidden are skipped.  No camera.  matched: an int32 / uint32 CUDA tensor of one element that
        receives the count.  input.harmonics may be None."""
        inp = _Input(_ptr(input.gaussians), _ptr(input.harmonics), int(input.gaussian_count), 0)
        sarr, sn = _style_array(styles)
        st = _lib().gsm_global_select_where(self._h, _stream_handle(stream), C.byref(inp),
                                            None if query is None else C.byref(_select_query_struct(query)),
                                            _ptr(state), sarr, sn if style_count is None else int(style_count),
                                            int(and_mask) & 0xFFFFFFFF, int(xor_mask) & 0xFFFFFFFF, _ptr(matched))
        _check(st, "gsm_global_select_where")

    def state_bounds(self, input: GaussianInput, state, keep, bounds, stream=None):
        """gsm_global_state_bounds: `bounds` (a CUDA tensor of 32 bytes: min[3] and max[3] as float32, then count
        and skipped as uint32) receives the axis-aligned box and the count of the gaussians whose state byte has
        its bit in `keep`.  state and keep: as GlobalRenderer.extract takes them."""
        inp = _Input(_ptr(input.gaussians), _ptr(input.harmonics), int(input.gaussian_count), 0)
        words = None if keep is None else (C.c_uint32 * 8)(*[int(w) & 0xFFFFFFFF for w in keep])
        st = _lib().gsm_global_state_bounds(self._h, _stream_handle(stream), C.byref(inp),
                                            None if state is None else C.byref(_state_struct(state)), words,
                                            _ptr(bounds))
        _check(st, "gsm_global_state_bounds")

    def transform(self, gaussians, harmonics, count: int, sh_components: int, state, keep, transform, stream=None):
        """gsm_global_transform: the pose of `transform` (a Transform; None: NULL) baked, in place, into the records
        `gaussians` and the rows `harmonics` (CUDA tensors) of the gaussians whose state byte has its bit in `keep`:
        position, scales and rotation moved, bands 1 and up of the harmonics rotated.  state and keep: as
        GlobalRenderer.extract takes them.  harmonics may be None with sh_components 0 or 1."""
        scene = _Scene(_ptr(gaussians), _ptr(harmonics), int(count), int(sh_components))
        words = None if keep is None else (C.c_uint32 * 8)(*[int(w) & 0xFFFFFFFF for w in keep])
        st = _lib().gsm_global_transform(self._h, _stream_handle(stream), C.byref(scene),
                                         None if state is None else C.byref(_state_struct(state)), words,
                                         None if transform is None else C.byref(transform.struct()))
        _check(st, "gsm_global_transform")

    def pick_owner(self, items):
        """gsm_global_pick_owner: items of the last enqueued pick frame (any integer array, host) ->
        (objects, gaussians), uint32 arrays of its shape; PICK_NONE where an item names nothing."""
        it = np.ascontiguousarray(np.asarray(items).astype(np.uint32, copy=False))
        obj, gid = np.empty(it.shape, np.uint32), np.empty(it.shape, np.uint32)
        st = _lib().gsm_global_pick_owner(self._h, it.ctypes.data, int(it.size), obj.ctypes.data, gid.ctypes.data)
        _check(st, "gsm_global_pick_owner")
        return obj, gid

    def render_composite(self, color_texture, depth_texture, objects, width: int, height: int, stream=None,
                         color_pitch: Optional[int] = None, depth_pitch: Optional[int] = None):
        """gsm_global_render_composite: the SceneObject list `objects` -- resident scenes, each under its own
        pose given as a camera -- sorted and blended together into one width x height frame.  objects None: a
        NULL array with object_count 1 (the C entry's error path)."""
        arr, n = _object_array(objects)
        cp = color_pitch if color_pitch is not None else int(width) * self._bpp
        dp = depth_pitch if depth_pitch is not None else int(width) * 2
        st = _lib().gsm_global_render_composite(self._h, _stream_handle(stream), arr, n, int(width), int(height),
                                                _ptr(color_texture), cp, _ptr(depth_texture), dp)
        _check(st, "gsm_global_render_composite")

    def project_partition(self, input: GaussianInput, camera: CameraParams, width: int, height: int,
                          first: int, count: int, slab_rows, send, send_capacity: int, send_counts,
                          stream=None):
        """gsm_global_project_partition: records of ids [first, first+count) per tile-row slab
        (slab_rows: num_slabs + 1 boundaries) into `send` (device, send_capacity records);
        `send_counts` (device, uint32 per slab) receives the record count of every slab."""
        inp = _Input(_ptr(input.gaussians), _ptr(input.harmonics), int(input.gaussian_count),
                     int(input.sh_components))
        cam = _camera_struct(camera)
        rows = (C.c_uint32 * len(slab_rows))(*[int(x) for x in slab_rows])
        st = _lib().gsm_global_project_partition(self._h, _stream_handle(stream), C.byref(inp), C.byref(cam),
                                                 int(width), int(height), int(first), int(count), rows,
                                                 len(slab_rows) - 1, _ptr(send), int(send_capacity),
                                                 _ptr(send_counts))
        _check(st, "gsm_global_project_partition")

    def render_records(self, color_texture, depth_texture, records, count: int, width: int, height: int,
                       stream=None, color_pitch: Optional[int] = None, depth_pitch: Optional[int] = None):
        """gsm_global_render_records: this renderer's tile rows from `count` received records."""
        cp = color_pitch if color_pitch is not None else int(width) * self._bpp
        dp = depth_pitch if depth_pitch is not None else int(width) * 2
        st = _lib().gsm_global_render_records(self._h, _stream_handle(stream), _ptr(records), int(count),
                                              int(width), int(height), _ptr(color_texture), cp,
                                              _ptr(depth_texture), dp)
        _check(st, "gsm_global_render_records")

    def debug_partition_counts(self, input: GaussianInput, camera: CameraParams, width: int, height: int,
                               first: int, count: int, slab_rows, send_counts, stream=None):
        """gsm_debug_partition_counts: the native multi-GPU frame's projection of ids
        [first, first+count) with per-slab record counts into `send_counts` (device uint32)."""
        inp = _Input(_ptr(input.gaussians), _ptr(input.harmonics), int(input.gaussian_count),
                     int(input.sh_components))
        cam = _camera_struct(camera)
        rows = (C.c_uint32 * len(slab_rows))(*[int(x) for x in slab_rows])
        _check(_lib().gsm_debug_partition_counts(self._h, _stream_handle(stream), C.byref(inp), C.byref(cam),
                                                 int(width), int(height), int(first), int(count), rows,
                                                 len(slab_rows) - 1, _ptr(send_counts)),
               "gsm_debug_partition_counts")

    def debug_partition_push(self, world: int, rank: int, counts, recv_buffers, recv_count, stream=None):
        """gsm_debug_partition_push: the last partition's records written into their slab owners'
        receive buffers (device tensors, one per rank) at the offsets of the device count matrix."""
        bufs = (C.c_void_p * len(recv_buffers))(*[_ptr(b) for b in recv_buffers])
        _check(_lib().gsm_debug_partition_push(self._h, _stream_handle(stream), int(world), int(rank),
                                               _ptr(counts), bufs, _ptr(recv_count)),
               "gsm_debug_partition_push")

    def debug_render_records_device_count(self, color_texture, depth_texture, records, capacity: int, count,
                                          width: int, height: int, stream=None):
        """gsm_debug_render_records_device_count: render_records with the count read on the device."""
        _check(_lib().gsm_debug_render_records_device_count(self._h, _stream_handle(stream), _ptr(records),
                                                            int(capacity), _ptr(count), int(width), int(height),
                                                            _ptr(color_texture), int(width) * self._bpp,
                                                            _ptr(depth_texture), int(width) * 2),
               "gsm_debug_render_records_device_count")

    def render_stereo(self, color_texture, depth_texture, input: GaussianInput, left: CameraParams,
                      right: CameraParams, width: int, height: int, stream=None):
        inp = _Input(_ptr(input.gaussians), _ptr(input.harmonics), int(input.gaussian_count),
                     int(input.sh_components))
        cl, cr = _camera_struct(left), _camera_struct(right)
        st = _lib().gsm_global_render_stereo(self._h, _stream_handle(stream), C.byref(inp), C.byref(cl),
                                             C.byref(cr), int(width), int(height), _ptr(color_texture),
                                             int(width) * 16, _ptr(depth_texture), int(width) * 4)
        _check(st, "gsm_global_render_stereo")

    def render_stereo_sbs(self, color_texture, depth_texture, input: GaussianInput, left: CameraParams,
                          right: CameraParams, width_per_eye: int, height: int, stream=None,
                          color_pitch: Optional[int] = None, depth_pitch: Optional[int] = None):
        """gsm_global_render_stereo_sbs: both eyes into one side-by-side target (config 5)."""
        inp = _Input(_ptr(input.gaussians), _ptr(input.harmonics), int(input.gaussian_count),
                     int(input.sh_components))
        cl, cr = _camera_struct(left), _camera_struct(right)
        cp = color_pitch if color_pitch is not None else 2 * int(width_per_eye) * self._bpp
        dp = depth_pitch if depth_pitch is not None else 2 * int(width_per_eye) * 2
        st = _lib().gsm_global_render_stereo_sbs(self._h, _stream_handle(stream), C.byref(inp), C.byref(cl),
                                                 C.byref(cr), int(width_per_eye), int(height),
                                                 _ptr(color_texture), cp, _ptr(depth_texture), dp)
        _check(st, "gsm_global_render_stereo_sbs")

    def debug_read_total_assignments(self) -> int:
        return int(_lib().gsm_global_debug_read_total_assignments(self._h))

    # -- introspection (include/gsm_debug.h) --
    def set_profiling(self, stage_events: bool = True, keep_unsorted: bool = False,
                      blend_trace: bool = False, blend_events: bool = False, blend_event_period: int = 1,
                      capture: bool = False):
        """blend_event_period > 1: with blend_events, bracket the blend on every period-th frame only.
        capture (implied by keep_unsorted): keep the render data and the sorted keys / values for
        copy_buffer (include/gsm_debug.h); the product path writes neither."""
        flags = (1 if stage_events else 0) | (2 if keep_unsorted else 0) | (4 if blend_trace else 0) | \
            (8 if blend_events else 0) | (16 if capture else 0) | \
            ((max(1, min(255, int(blend_event_period))) & 0xFF) << 8)
        _check(_lib().gsm_global_set_profiling(self._h, flags), "gsm_global_set_profiling")

    def set_tile_rows(self, begin: int, end: int):
        _check(_lib().gsm_global_set_tile_rows(self._h, int(begin), int(end)), "gsm_global_set_tile_rows")

    def blend_kernel(self) -> str:
        """The blend kernel the last enqueued frame launched (gsm_global_debug_blend_kernel)."""
        k = C.c_int(0)
        _check(_lib().gsm_global_debug_blend_kernel(self._h, C.byref(k)), "gsm_global_debug_blend_kernel")
        return BLEND_KERNELS[k.value]

    def blend_kernel_kind(self) -> int:
        """gsm_blend_kernel (include/gsm_debug.h) of the last enqueued frame: 1 quadrant units, 2 half-tile
        units, 3 pair walk -- blend_kernel() gives the first two one name."""
        k = C.c_int(0)
        _check(_lib().gsm_global_debug_blend_kernel(self._h, C.byref(k)), "gsm_global_debug_blend_kernel")
        return k.value

    def copy_buffer(self, which: BufferId) -> np.ndarray:
        raw = self._debug_copy(which)
        if which == BufferId.RENDER_DATA:
            return raw.view(RENDER_DATA)
        if which == BufferId.BOUNDS:
            return raw.view(np.int32).reshape(-1, 4)
        if which in (BufferId.TILE_COUNTS, BufferId.KEYS, BufferId.SORTED_KEYS):
            return raw.view(np.uint32)
        if which in (BufferId.VALUES, BufferId.SORTED_VALUES):
            return raw.view(np.int32)
        if which == BufferId.HEADERS:
            return raw.view(np.uint32).reshape(-1, 2)
        if which == BufferId.BLEND_TRACE:
            return raw.view(np.uint64).reshape(-1, 4)
        if which == BufferId.EXP_TABLE:
            return raw.view(np.uint16)
        return raw


class DepthFirstBuffer(enum.IntEnum):  # include/gsm_depthfirst.h gsm_depthfirst_buffer
    RENDER_DATA = 0
    BOUNDS = 1
    TOUCHED = 2
    DEPTH_KEYS = 3
    DEPTH_ORDER = 4
    INSTANCE_TILES = 5
    INSTANCE_GAUSSIANS = 6
    HEADERS = 7
    BLEND_STATS = 8
    SORTED_DEPTH_KEYS = 9  # uint32[visible]: the compacted keys as the depth sort left them


DF_STAGES = ("project", "depth_sort", "instances", "tile_sort", "blend")  # gsm_depthfirst_stage

# StereoTiledRenderData (BridgingTypes.h:250-276), 32 B
STEREO_RENDER_DATA = np.dtype([(f, "<u2") for f in (
    "leftMeanX", "leftMeanY", "leftCxx", "leftCyy", "leftCxy2", "leftDepth",
    "rightMeanX", "rightMeanY", "rightCxx", "rightCyy", "rightCxy2", "rightDepth")] +
    [("colorR", "u1"), ("colorG", "u1"), ("colorB", "u1"), ("opacity", "u1"),
     ("centerDepth", "<u2"), ("pad0", "<u2")])


class DepthFirstRenderer(_Renderer):
    """DepthFirstRenderer (DepthFirstRenderer.swift:11-831) on one HIP device: the mono frame
    (render, :166-203, 237-465) and the stereo side-by-side path (renderStereo(target:
    .sideBySide), :205-223, 469-512).  renderStereo(.foveated) is out of scope.
    depth_key_bits (16 | 32) and tile_id_bits (16 | 32) are depthSortKeyPrecision and tileIdPrecision
    of DepthFirstRenderer.init (:45-50), fixed for the life of the renderer (include/gsm_depthfirst.h)."""
    _PREFIX, _STAGE_NAMES, _COUNTERS = "gsm_depthfirst", DF_STAGES, _DfCounters

    def __init__(self, device: Optional[int] = None, config: RendererConfig = RendererConfig(),
                 depth_key_bits: int = 32, tile_id_bits: int = 16):
        opt = _DfOptions(C.sizeof(_DfOptions), int(depth_key_bits), int(tile_id_bits), 0)
        self._open(device, config, "create_with_options", C.byref(opt))
        self._last_mono = False  # the last frame was a mono frame (copy_buffer's record dtype)

    @property
    def options(self) -> dict:
        """{"depth_key_bits", "tile_id_bits"} as the handle holds them (gsm_depthfirst_get_options)."""
        o = _DfOptions()
        _check(_lib().gsm_depthfirst_get_options(self._h, C.byref(o)), "gsm_depthfirst_get_options")
        return {"depth_key_bits": int(o.depth_key_bits), "tile_id_bits": int(o.tile_id_bits)}

    # -- DepthFirstRenderer.render (DepthFirstRenderer.swift:166-203) --
    def render(self, color_texture, depth_texture, input: GaussianInput, camera: CameraParams,
               width: int, height: int, stream=None, color_pitch: Optional[int] = None,
               depth_pitch: Optional[int] = None):
        """The mono frame into color_texture ([height, width] of the config's colour format) and
        depth_texture ([height, width] fp16, or None: no depth is written)."""
        inp = _Input(_ptr(input.gaussians), _ptr(input.harmonics), int(input.gaussian_count),
                     int(input.sh_components))
        cam = _camera_struct(camera)
        cp = color_pitch if color_pitch is not None else int(width) * self._bpp
        dp = depth_pitch if depth_pitch is not None else int(width) * 2
        st = _lib().gsm_depthfirst_render(self._h, _stream_handle(stream), C.byref(inp), C.byref(cam),
                                          int(width), int(height), _ptr(color_texture), cp,
                                          _ptr(depth_texture), dp)
        _check(st, "gsm_depthfirst_render")
        self._last_mono = True

    def render_stereo_sbs(self, color_texture, input: GaussianInput, left: CameraParams, right: CameraParams,
                          width_per_eye: int, height: int, scene_transform=None, stream=None,
                          color_pitch: Optional[int] = None):
        """Both eyes side by side into color_texture ([height, 2 * width_per_eye] of the
        config's colour format), as the reference's copy pass leaves them (rows flipped)."""
        inp = _Input(_ptr(input.gaussians), _ptr(input.harmonics), int(input.gaussian_count),
                     int(input.sh_components))
        cl, cr = _camera_struct(left), _camera_struct(right)
        st_arr = None
        if scene_transform is not None:
            st_arr = (C.c_float * 16)(*[float(v) for v in np.asarray(scene_transform, np.float32).reshape(16)])
        cp = color_pitch if color_pitch is not None else 2 * int(width_per_eye) * self._bpp
        st = _lib().gsm_depthfirst_render_stereo_sbs(self._h, _stream_handle(stream), C.byref(inp), C.byref(cl),
                                                     C.byref(cr), st_arr, int(width_per_eye), int(height),
                                                     _ptr(color_texture), cp)
        _check(st, "gsm_depthfirst_render_stereo_sbs")
        self._last_mono = False

    def set_profiling(self, stage_events: bool = True, blend_events: bool = False, blend_stats: bool = False,
                      blend_event_period: int = 1):
        flags = (1 if stage_events else 0) | (2 if blend_stats else 0) | (8 if blend_events else 0) | \
            ((max(1, min(255, int(blend_event_period))) & 0xFF) << 8)
        _check(_lib().gsm_depthfirst_set_profiling(self._h, flags), "set_profiling")

    def copy_buffer(self, which: DepthFirstBuffer) -> np.ndarray:
        raw = self._debug_copy(which)
        if which == DepthFirstBuffer.RENDER_DATA:  # 16-byte records after a mono frame
            return raw.view(RENDER_DATA if self._last_mono else STEREO_RENDER_DATA)
        if which == DepthFirstBuffer.BOUNDS:
            return raw.view(np.int32).reshape(-1, 4)
        if which == DepthFirstBuffer.HEADERS:
            return raw.view(np.uint32).reshape(-1, 2)
        if which in (DepthFirstBuffer.DEPTH_ORDER, DepthFirstBuffer.INSTANCE_GAUSSIANS):
            return raw.view(np.int32)
        if which == DepthFirstBuffer.BLEND_STATS:
            return raw.view(np.uint64)
        return raw.view(np.uint32)


class LocalBuffer(enum.IntEnum):  # include/gsm_local.h gsm_local_buffer
    PROJECTED = 0
    TILE_COUNTS = 1
    TILE_LISTS = 2


LOCAL_STAGES = ("project", "scatter", "sort", "blend")  # gsm_local_stage
LOCAL_MAX_PER_TILE = 2048  # GSM_LOCAL_MAX_PER_TILE


class LocalRenderer(_Renderer):
    """LocalRenderer (LocalRenderer.swift:6-257) on one HIP device: per-tile slot lists sorted by a 16-bit
    depth key, no global sort (include/gsm_local.h).  renderStereo is a fatalError in the reference."""
    _PREFIX, _STAGE_NAMES, _COUNTERS = "gsm_local", LOCAL_STAGES, _LocalCounters

    def __init__(self, device: Optional[int] = None, config: RendererConfig = RendererConfig()):
        self._open(device, config)

    # -- LocalRenderer.render (LocalRenderer.swift:83-106) --
    def render(self, color_texture, depth_texture, input: GaussianInput, camera: CameraParams,
               width: int, height: int, stream=None, color_pitch: Optional[int] = None,
               depth_pitch: Optional[int] = None):
        """One frame into color_texture ([height, width] of the config's colour format) and
        depth_texture ([height, width] fp16, or None: no depth is written)."""
        inp = _Input(_ptr(input.gaussians), _ptr(input.harmonics), int(input.gaussian_count),
                     int(input.sh_components))
        cam = _camera_struct(camera)
        cp = color_pitch if color_pitch is not None else int(width) * self._bpp
        dp = depth_pitch if depth_pitch is not None else int(width) * 2
        st = _lib().gsm_local_render(self._h, _stream_handle(stream), C.byref(inp), C.byref(cam),
                                     int(width), int(height), _ptr(color_texture), cp, _ptr(depth_texture), dp)
        _check(st, "gsm_local_render")

    def set_profiling(self, stage_events: bool = True):
        _check(_lib().gsm_local_set_profiling(self._h, 1 if stage_events else 0), "set_profiling")

    def copy_buffer(self, which: LocalBuffer) -> np.ndarray:
        raw = self._debug_copy(which)
        if which == LocalBuffer.PROJECTED:
            return raw.view(PROJECTED)
        if which == LocalBuffer.TILE_LISTS:
            return raw.view(np.uint32).reshape(-1, LOCAL_MAX_PER_TILE)
        return raw.view(np.uint32)

    @staticmethod
    def sort_tiles(keys16, indices, counts, max_per_tile: int, out_local_idx, stream=None):
        """The per-tile sort stage alone on device buffers (torch int16 keys and output, int32 indices and
        counts; tile t owns slots [t * max_per_tile, (t + 1) * max_per_tile)): out_local_idx receives each
        tile's slots ascending by (key, index, slot)."""
        _check(_lib().gsm_local_debug_sort_tiles(_stream_handle(stream), _ptr(keys16), _ptr(indices), _ptr(counts),
                                                 int(counts.numel()), int(max_per_tile), _ptr(out_local_idx)),
               "gsm_local_debug_sort_tiles")


def sort_pairs_u32(keys, values, key_bits: int = 32, stream=None):
    """Stable device radix sort of uint32 (key, value) pairs in place (torch int32 tensors)."""
    n = int(keys.numel())
    _check(_lib().gsm_sort_pairs_u32(_ptr(keys), _ptr(values), n, int(key_bits), _stream_handle(stream)),
           "gsm_sort_pairs_u32")


class FrameSortPlan(enum.IntEnum):  # include/gsm_debug.h gsm_frame_sort_plan
    ONE_NARROW = 1
    TWO_NARROW = 2
    ONE_WIDE = 3
    WIDE_THEN_NARROW = 4


@dataclass
class FrameSortResult:
    """What one FrameSort.run copied out (numpy uint32).  half0 / half1 / half_count: None without a depth sort;
    sorted_keys / sorted_values after a depth sort with full = False hold nothing specified."""
    plan: FrameSortPlan
    sorted_keys: np.ndarray
    sorted_values: np.ndarray
    tile_start: np.ndarray
    half0: Optional[np.ndarray] = None
    half1: Optional[np.ndarray] = None
    half_count: Optional[np.ndarray] = None


class FrameSort:
    """gsm_debug_frame_sort (include/gsm_debug.h; debug only): the production frame sort -- the tile passes that
    write the tile starts, then the per-tile depth sort with its half-tile lists -- on caller keys.  One handle
    keeps its workspace between runs, as a renderer does; GSM_SORT_RANK / GSM_SORT_WIDE / GSM_SORT_SCAN are read
    when it is created.  A context manager; close() frees the device buffers."""

    def __init__(self, capacity: int, max_tiles: int, device: Optional[int] = None):
        h = C.c_void_p()
        self.capacity, self.max_tiles = int(capacity), int(max_tiles)
        _check(_lib().gsm_debug_frame_sort_create(self.capacity, self.max_tiles, -1 if device is None else int(device),
                                                  C.byref(h)), "gsm_debug_frame_sort_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            _lib().gsm_debug_frame_sort_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()

    def run(self, keys, values, n: Optional[int] = None, *, shift: int, num_tiles: int,
            all_tiles: Optional[int] = None, depth_sort: bool = False, full: bool = False,
            stream=None) -> FrameSortResult:
        """Sort the first n (default: all) pairs of the device tensors keys / values (torch int32, the words read
        as uint32); shift 16: keys tile << 16 | depth16, shift 0: the tile alone.  Every key's tile is below
        num_tiles <= all_tiles (default num_tiles); bits 30 and 31 of a value are the half-tile skip flags."""
        n = int(keys.numel()) if n is None else int(n)
        all_tiles = int(num_tiles) if all_tiles is None else int(all_tiles)
        desc = _FrameSortDesc(int(shift), int(num_tiles), all_tiles, int(bool(depth_sort)), int(bool(full)), 0)
        sk, sv = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        ts = np.zeros(max(all_tiles, 0) + 1, np.uint32)
        h0 = h1 = hc = None
        if depth_sort:
            h0, h1 = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
            hc = np.zeros(2 * max(all_tiles, 0), np.uint32)
        host = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        out = _FrameSortOut(host(sk), host(sv), host(ts), host(h0), host(h1), host(hc), 0, 0)
        _check(_lib().gsm_debug_frame_sort_run(self._h, _stream_handle(stream), C.byref(desc),
                                               _ptr(keys) if n else None, _ptr(values) if n else None, n,
                                               C.byref(out)), "gsm_debug_frame_sort_run")
        return FrameSortResult(FrameSortPlan(out.plan), sk, sv, ts, h0, h1, hc)


class _MgOptions(C.Structure):
    _fields_ = [("struct_bytes", C.c_uint32), ("rows", C.c_int32), ("pipelined", C.c_int32),
                ("transport", C.c_int32), ("timeout_ms", C.c_uint32), ("reserved", C.c_uint32),
                ("nccl_comm", C.c_void_p)]


MG_ROWS = {"contiguous": 0, "interleaved": 1}
MG_TRANSPORT = {"peer_stores": 0, "rccl": 1}


@dataclass
class MultiGpuOptions:
    """gsm_multigpu_options (include/gsm_multigpu.h): row layout, pipelining, transport, barrier
    timeout, and the RCCL transport's communicator (ncclComm_t as an int)."""
    rows: str = "contiguous"
    pipelined: bool = False
    transport: str = "peer_stores"
    timeout_ms: int = 10000
    nccl_comm: Optional[int] = None

    def _c(self) -> "_MgOptions":
        o = _MgOptions()
        _lib().gsm_multigpu_default_options(C.byref(o))
        o.rows = MG_ROWS[self.rows]
        o.pipelined = 1 if self.pipelined else 0
        o.transport = MG_TRANSPORT[self.transport]
        o.timeout_ms = int(self.timeout_ms)
        o.nccl_comm = C.c_void_p(int(self.nccl_comm)) if self.nccl_comm else None
        return o


class MultiGpuRenderer:
    """gsm_multigpu_* (include/gsm_multigpu.h): one frame of a GlobalRenderer split by tile-row slab
    across the ranks of a node -- counts, records and slab pixels written straight into the owners'
    exchange memory (peer mappings over xGMI), ordered by device-side flag barriers, the bands
    gathered on rank 0 -- all inside libgsm_amd.so, no host round trip and no collective in a frame.

    Two ways to set up (both collective):
      MultiGpuRenderer(renderer, comm, rank, world)       handles exchanged over an RCCL
                                                          communicator (torch: _comm_ptr());
      MultiGpuRenderer.connect(renderer, rank, world, allgather)
                                                          handles exchanged by the caller:
                                                          allgather(bytes) -> list of every rank's
                                                          bytes (e.g. torch.distributed over gloo)."""

    def __init__(self, renderer: "GlobalRenderer", comm: Optional[int], rank: int, world_size: int, _handle=None,
                 options: Optional["MultiGpuOptions"] = None):
        """options None: gsm_multigpu_create (defaults + the environment's test overrides); otherwise
        gsm_multigpu_create_with_options."""
        self.renderer = renderer
        self.rank = int(rank)
        self.world_size = int(world_size)
        if _handle is not None:
            self._h = _handle
            return
        h = C.c_void_p()
        if options is None:
            _check(_lib().gsm_multigpu_create(renderer._h, C.c_void_p(int(comm)), int(rank), int(world_size),
                                              C.byref(h)), "gsm_multigpu_create")
        else:
            o = options._c()
            _check(_lib().gsm_multigpu_create_with_options(renderer._h, C.c_void_p(int(comm)), int(rank),
                                                           int(world_size), C.byref(o), C.byref(h)),
                   "gsm_multigpu_create_with_options")
        self._h = h

    @classmethod
    def prepare(cls, renderer: "GlobalRenderer", rank: int, world_size: int,
                options: Optional["MultiGpuOptions"] = None):
        """gsm_multigpu_prepare (options None) or gsm_multigpu_prepare_with_options: (unconnected
        renderer, this rank's handle bytes)."""
        h = C.c_void_p()
        buf = C.create_string_buffer(MULTIGPU_HANDLE_BYTES)
        if options is None:
            _check(_lib().gsm_multigpu_prepare(renderer._h, int(rank), int(world_size), C.byref(h), buf),
                   "gsm_multigpu_prepare")
        else:
            o = options._c()
            _check(_lib().gsm_multigpu_prepare_with_options(renderer._h, int(rank), int(world_size), C.byref(o),
                                                            C.byref(h), buf), "gsm_multigpu_prepare_with_options")
        return cls(renderer, None, rank, world_size, _handle=h), bytes(buf.raw)

    def connect_handles(self, handles):
        """gsm_multigpu_connect with every rank's handle bytes, in rank order."""
        blob = b"".join(bytes(x) for x in handles)
        if len(blob) != MULTIGPU_HANDLE_BYTES * self.world_size:
            raise ValueError("one handle per rank expected")
        _check(_lib().gsm_multigpu_connect(self._h, C.c_char_p(blob)), "gsm_multigpu_connect")
        return self

    @classmethod
    def connect(cls, renderer: "GlobalRenderer", rank: int, world_size: int, allgather,
                options: Optional["MultiGpuOptions"] = None):
        mg, mine = cls.prepare(renderer, rank, world_size, options)
        try:
            return mg.connect_handles(allgather(mine))
        except Exception:
            mg.close()
            raise

    @staticmethod
    def torch_allgather(data: bytes):
        """Every rank's bytes over torch.distributed's default group (any backend)."""
        import torch.distributed as dist
        out = [None] * dist.get_world_size()
        dist.all_gather_object(out, data)
        return out

    @staticmethod
    def torch_comm(device) -> int:
        """The ncclComm_t of torch.distributed's default NCCL process group on `device`."""
        import torch.distributed as dist
        return int(dist.group.WORLD._get_backend(torch.device("cuda", int(device)))._comm_ptr())

    def _args(self, input, camera, color_texture, depth_texture, width, color_pitch, depth_pitch):
        inp = _Input(_ptr(input.gaussians), _ptr(input.harmonics), int(input.gaussian_count),
                     int(input.sh_components))
        cam = _camera_struct(camera)
        cp = color_pitch if color_pitch is not None else int(width) * 8
        dp = depth_pitch if depth_pitch is not None else int(width) * 2
        return inp, cam, cp, dp

    def render(self, color_texture, depth_texture, input: GaussianInput, camera: CameraParams, width: int,
               height: int, gather: bool = True, stream=None, color_pitch: Optional[int] = None,
               depth_pitch: Optional[int] = None, gather_target=None, gather_depth: Optional[bool] = None):
        """One frame.  gather: rank 0 receives the whole frame -- in color_texture (a copy of the
        library frame), or, with gather_target = self.frame()[0], in the library frame itself; the
        other ranks' color_texture is then unused (may be None).  gather_depth (with gather): rank 0
        also receives the r16f depth -- in depth_texture (a copy) or, when depth_texture is None, in
        the library depth frame (self.frame_depth()); default: whether depth_texture is given (every
        rank must make the same choice: pass it explicitly when only rank 0 holds a depth texture)."""
        self.render_phases(range(4), color_texture, depth_texture, input, camera, width, height, gather, stream,
                           color_pitch, depth_pitch, gather_target, gather_depth)

    def render_phases(self, phases, color_texture, depth_texture, input: GaussianInput, camera: CameraParams,
                      width: int, height: int, gather: bool = True, stream=None, color_pitch: Optional[int] = None,
                      depth_pitch: Optional[int] = None, gather_target=None, gather_depth: Optional[bool] = None):
        """gsm_multigpu_render_phase for each phase in `phases` (virtual ranks: phase p of every rank
        before phase p + 1 of any, include/gsm_multigpu.h).  Every phase is issued even after one
        returned an error (the ranks stay in step); the first error is raised after the last.
        gather_depth as render's."""
        if gather_depth is None:
            gather_depth = depth_texture is not None
        inp, cam, cp, dp = self._args(input, camera, color_texture, depth_texture, width, color_pitch, depth_pitch)
        col = _ptr(color_texture)
        dep = _ptr(depth_texture)
        if gather:  # rank 0: the caller's target (a copy) or else the library frame; others: any non-NULL
            if gather_target is not None:
                g = _ptr(gather_target)
            elif self.rank == 0:
                g = col if col is not None else self.frame()[0]
            else:
                g = 1
            if not gather_depth:
                dep = None
            elif self.rank == 0:
                if dep is None:
                    dep, dp = self.frame_depth()
            else:
                dep = 1
        else:
            g = None
        first = None
        for p in phases:
            st = _lib().gsm_multigpu_render_phase(self._h, int(p), _stream_handle(stream), C.byref(inp), C.byref(cam),
                                                  int(width), int(height), col, cp, dep, dp, g)
            if st != 0 and first is None:
                first = (st, p)
        if first is not None:
            _check(first[0], f"gsm_multigpu_render_phase({first[1]})")

    def finish_frame(self, stream=None):
        """gsm_multigpu_finish_frame: the phases a caller left unfinished (barrier steps; the slab is
        abandoned from phase 2 on), so the ranks stay in step; a no-op when no frame is pending."""
        _check(_lib().gsm_multigpu_finish_frame(self._h, _stream_handle(stream)), "gsm_multigpu_finish_frame")

    def debug_set_epoch(self, epoch: int):
        """gsm_multigpu_debug_set_epoch (tests: reach the 2^31 epoch wrap in a few frames)."""
        _check(_lib().gsm_multigpu_debug_set_epoch(self._h, int(epoch) & 0xFFFFFFFF), "gsm_multigpu_debug_set_epoch")

    def wait_event(self, event):
        """gsm_multigpu_wait_event: the next frame's projection (phase 0) waits for `event` (a
        torch.cuda.Event recorded after the caller wrote this frame's gaussians / harmonics) -- needed
        when pipelined (GSM_MG_PIPELINE=1), where phase 0 runs on the library's own stream."""
        h = event.cuda_event if hasattr(event, "cuda_event") else int(event)
        _check(_lib().gsm_multigpu_wait_event(self._h, C.c_void_p(h)), "gsm_multigpu_wait_event")

    def frame(self):
        """(device pointer, pitch bytes) of rank 0's gathered frame; (None, 0) elsewhere."""
        p = C.c_void_p()
        pitch = C.c_size_t()
        _check(_lib().gsm_multigpu_frame(self._h, C.byref(p), C.byref(pitch)), "gsm_multigpu_frame")
        return p.value, int(pitch.value)

    def frame_depth(self):
        """(device pointer, pitch bytes) of rank 0's gathered r16f depth frame; (None, 0) elsewhere."""
        p = C.c_void_p()
        pitch = C.c_size_t()
        _check(_lib().gsm_multigpu_frame_depth(self._h, C.byref(p), C.byref(pitch)), "gsm_multigpu_frame_depth")
        return p.value, int(pitch.value)

    def copy_depth(self, width: int, height: int) -> np.ndarray:
        """Rank 0: the gathered r16f depth frame as uint16 bits [height, width] (synchronous)."""
        out = np.empty((int(height), int(width)), np.uint16)
        _check(_lib().gsm_multigpu_debug_copy_depth(self._h, out.ctypes.data_as(C.c_void_p), int(width) * 2,
                                                    int(width), int(height)), "gsm_multigpu_debug_copy_depth")
        return out

    def errors(self, clear: bool = False):
        """(barrier timeouts, failed peer arrivals) since create or the last clear."""
        t, f = C.c_uint32(0), C.c_uint32(0)
        _check(_lib().gsm_multigpu_errors(self._h, C.byref(t), C.byref(f), 1 if clear else 0), "gsm_multigpu_errors")
        return int(t.value), int(f.value)

    def copy_frame(self, width: int, height: int) -> np.ndarray:
        """Rank 0: the gathered rgba16f frame as uint16 bits [height, width, 4] (synchronous)."""
        out = np.empty((int(height), int(width), 4), np.uint16)
        _check(_lib().gsm_multigpu_debug_copy_frame(self._h, out.ctypes.data_as(C.c_void_p), int(width) * 8,
                                                    int(width), int(height)), "gsm_multigpu_debug_copy_frame")
        return out

    def copy_exchange(self, nbytes: int) -> np.ndarray:
        """The first nbytes of this rank's exchange memory (control, counts from byte 1024, records
        from byte 4096), synchronous."""
        out = np.empty(int(nbytes), np.uint8)
        _check(_lib().gsm_multigpu_debug_copy_exchange(self._h, out.ctypes.data_as(C.c_void_p), out.size),
               "gsm_multigpu_debug_copy_exchange")
        return out

    def status(self, clear: bool = False) -> int:
        """Barrier timeouts since create (0 on a healthy run)."""
        out = C.c_uint32(0)
        _check(_lib().gsm_multigpu_status(self._h, C.byref(out), 1 if clear else 0), "gsm_multigpu_status")
        return int(out.value)

    def set_timeout_ms(self, ms: int):
        _check(_lib().gsm_multigpu_set_timeout_ms(self._h, int(ms)), "gsm_multigpu_set_timeout_ms")

    def counts(self) -> np.ndarray:
        out = (C.c_uint32 * (self.world_size * self.world_size))()
        _check(_lib().gsm_multigpu_debug_counts(self._h, out), "gsm_multigpu_debug_counts")
        return np.array(out, np.uint32).reshape(self.world_size, self.world_size)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            _lib().gsm_multigpu_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def sort_rank_probe(device: int = 0) -> bool:
    """True when the device serves same-address LDS atomics of one wave in lane order (the sorts'
    default stable ranks); False -> the renderers rank by ballot matches."""
    out = C.c_int(0)
    _check(_lib().gsm_debug_sort_rank_probe(int(device), C.byref(out)), "gsm_debug_sort_rank_probe")
    return bool(out.value)


def keep_visible(styles, style_count: Optional[int] = None) -> list:
    """gsm_global_keep_visible: the keep set (8 words) of the states a styled frame with the Style list `styles`
    does not cull; None: every state.  style_count overrides the list's length."""
    arr, n = _style_array(styles)
    keep = (C.c_uint32 * 8)()
    _lib().gsm_global_keep_visible(arr, n if style_count is None else int(style_count), keep)
    return [int(w) for w in keep]


def keep_masked(test_mask: int, test_value: int) -> list:
    """gsm_global_keep_masked: the keep set (8 words) of the states s with (s & test_mask) == test_value."""
    keep = (C.c_uint32 * 8)()
    _lib().gsm_global_keep_masked(int(test_mask) & 0xFFFFFFFF, int(test_value) & 0xFFFFFFFF, keep)
    return [int(w) for w in keep]


class Transform:
    """gsm_global_transform_desc: a rotation, a uniform scale and a translation as GlobalRenderer.transform applies
    them -- matrix (12 floats, row-major 3x4, s R | t), quaternion (x, y, z, w of R), scale, and sh1, sh2, sh3, the
    row-major band matrices of R for the harmonics.  All float32 arrays; the entry applies them as they are."""

    def __init__(self, matrix, quaternion, scale, sh1, sh2, sh3):
        f = lambda v, n: np.ascontiguousarray(np.asarray(v, np.float32).reshape(n))
        self.matrix, self.quaternion, self.scale = f(matrix, 12), f(quaternion, 4), np.float32(scale)
        self.sh1, self.sh2, self.sh3 = f(sh1, 9), f(sh2, 25), f(sh3, 49)

    @classmethod
    def from_pose(cls, rotation, scale: float, translation) -> "Transform":
        """gsm_global_transform_from_pose: rotation is a 3x3 (row-major when flat), scale > 0, translation 3 values,
        each rounded to float32 on the way in.  Raises RendererError where the helper refuses."""
        R = (C.c_float * 9)(*[float(v) for v in np.asarray(rotation, np.float64).reshape(9)])
        t = (C.c_float * 3)(*[float(v) for v in np.asarray(translation, np.float64).reshape(3)])
        d = _TransformDesc()
        _check(_lib().gsm_global_transform_from_pose(R, float(scale), t, C.byref(d)), "gsm_global_transform_from_pose")
        return cls(list(d.matrix), list(d.quaternion), d.scale, list(d.sh1), list(d.sh2), list(d.sh3))

    @classmethod
    def from_matrix(cls, M) -> "Transform":
        """The Transform of a similarity M: a 4x4, column-major flat as scenes.object_camera and scenes.pose_matrix
        have it.  M is split in float64 into s = det(A)^(1/3), R = A / s and t, A its upper 3x3; ValueError when its
        last row is not (0, 0, 0, 1) or its determinant is not positive, RendererError when R is no rotation."""
        m = np.asarray(M, np.float64).reshape(4, 4).T
        if not np.array_equal(m[3], [0.0, 0.0, 0.0, 1.0]):
            raise ValueError("Transform.from_matrix: the last row is not (0, 0, 0, 1)")
        det = float(np.linalg.det(m[:3, :3]))
        if not (np.isfinite(det) and det > 0.0):
            raise ValueError("Transform.from_matrix: the determinant is not positive")
        s = det ** (1.0 / 3.0)
        return cls.from_pose(m[:3, :3] / s, s, m[:3, 3])

    def struct(self) -> _TransformDesc:
        d = _TransformDesc()
        d.matrix[:], d.quaternion[:], d.scale = self.matrix.tolist(), self.quaternion.tolist(), float(self.scale)
        d.sh1[:], d.sh2[:], d.sh3[:] = self.sh1.tolist(), self.sh2.tolist(), self.sh3.tolist()
        return d


def select_query_default() -> SelectQuery:
    """gsm_global_select_query_default, read back into a SelectQuery."""
    s = _SelectQuery()
    C.memset(C.byref(s), 0xA5, C.sizeof(s))
    _lib().gsm_global_select_query_default(C.byref(s))
    return SelectQuery(int(s.shape), int(s.flags), tuple(float(v) for v in s.to_shape), float(s.opacity_min),
                       float(s.opacity_max), float(s.scale_min), float(s.scale_max), int(s.test_mask),
                       int(s.test_value))


def abi_version() -> int:
    return int(_lib().gsm_abi_version())
