"""ctypes binding of libsmg_hip.so (include/smg_hip.h) - the only way the Python
layer reaches the GPU kernels.  There is no CPU fallback: if the library is missing
or no MI355X is visible every entry point raises."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SMG_HIP_LIB") or os.path.join(_HERE, "libsmg_hip.so")     # SMG_HIP_LIB: dev A/B of two builds


class SmgError(RuntimeError):
    pass


class SmgNet(C.Structure):
    _fields_ = [("params", C.c_void_p), ("grads", C.c_void_p), ("bufs", C.c_void_p), ("nbt", C.c_void_p)]


class SmgBatch(C.Structure):
    _fields_ = [
        ("n_images", C.c_int), ("images_nchw_dev", C.c_void_p), ("heightmaps_dev", C.c_void_p),
        ("hm_size", C.c_int), ("image_mean", C.c_double), ("image_std", C.c_double),
        ("n_streams", C.c_int), ("stream_image", C.POINTER(C.c_int)), ("stream_affine", C.POINTER(C.c_float)),
        ("stream_rotated", C.POINTER(C.c_int)),
        ("n_pairs", C.c_int), ("pair_a", C.POINTER(C.c_int)), ("pair_b", C.POINTER(C.c_int)),
        ("n_bn_seq_trunk", C.c_int), ("bn_seq_trunk", C.POINTER(C.c_int)),
        ("n_bn_seq_head", C.c_int), ("bn_seq_head", C.POINTER(C.c_int)),
        ("masks_dev", C.c_void_p), ("n_masks", C.c_int), ("stream_mask_a", C.POINTER(C.c_int)), ("stream_mask_b", C.POINTER(C.c_int)),
    ]


class SmgAdam(C.Structure):
    _fields_ = [("m", C.c_void_p), ("v", C.c_void_p), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("step_trunk", C.c_int), ("step_head", C.c_int)]


ABI_VERSION = 9     # SMG_ABI_VERSION of include/smg_hip.h this binding was written against

_lib = None


def lib():
    """Load the shared library once.  torch must already be imported so that the HIP
    runtime the library binds to (soname libamdhip64.so.7) is the one torch uses."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (loads torch's libamdhip64 first)
    if not os.path.exists(LIB_PATH):
        raise SmgError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950). There is no CPU fallback for the affordance path." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    L.smg_last_error.restype = C.c_char_p
    L.smg_version.restype = C.c_int
    if not hasattr(L, "smg_abi_struct_bytes") or L.smg_version() != ABI_VERSION:
        raise SmgError("%s is ABI version %d, this binding needs %d: rebuild it (make -C csrc)" % (LIB_PATH, L.smg_version(), ABI_VERSION))
    for added in ("smg_loss_scene_map_ce", "smg_scene_argmax_objects", "smg_scene_class_argmax_objects", "smg_scene_values",
                  "smg_scene_class_values", "smg_scene_topk_objects", "smg_scene_class_topk_objects", "smg_scene_best_maps",
                  "smg_scene_class_best_maps", "smg_scene_sample_objects", "smg_scene_class_sample_objects", "smg_scene_softmax_objects",
                  "smg_scene_class_softmax_objects", "smg_loss_scene_policy"):       # (added without a version step: a version-9 library built before them lacks the symbol)
        if not hasattr(L, added):
            raise SmgError("%s is ABI version %d but lacks %s, a stale build: rebuild it (make -C csrc)" % (LIB_PATH, ABI_VERSION, added))
    L.smg_abi_struct_bytes.argtypes = [C.c_int]
    for which, ty in ((0, SmgBatch), (1, SmgNet), (2, SmgAdam)):
        if L.smg_abi_struct_bytes(which) != C.sizeof(ty):
            raise SmgError("%s: struct %s is %d bytes in the library, %d in this binding" % (LIB_PATH, ty.__name__, L.smg_abi_struct_bytes(which), C.sizeof(ty)))
    L.smg_layout_count.argtypes = [C.c_int]
    for f in (L.smg_layout_param_floats, L.smg_layout_buffer_floats, L.smg_layout_nbt_count):
        f.argtypes = [C.c_int]
        f.restype = C.c_int64
    L.smg_layout_entry.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64),
                                   C.POINTER(C.c_int), C.POINTER(C.c_int64)]
    L.smg_layout_trunk_range.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.smg_layout_head_range.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.smg_engine_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.smg_engine_destroy.argtypes = [C.c_void_p]
    L.smg_engine_destroy.restype = None
    L.smg_engine_workspace_bytes.argtypes = [C.c_void_p]
    L.smg_engine_workspace_bytes.restype = C.c_int64
    L.smg_engine_geometry.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.smg_forward.argtypes = [C.c_void_p, C.POINTER(SmgNet), C.c_int, C.c_int, C.POINTER(SmgBatch), C.c_void_p, C.c_void_p]
    L.smg_loss.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.smg_loss_map.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.smg_loss_map_ce.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.smg_scene_maps.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_void_p]
    L.smg_scene_values.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.smg_scene_argmax.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.smg_scene_argmax_objects.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_int,
                                           C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.smg_scene_topk_objects.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_int,
                                         C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
    L.smg_scene_best_maps.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_int,
                                      C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.smg_scene_sample_objects.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_int,
                                           C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_double, C.c_uint64,
                                           C.c_void_p, C.c_void_p, C.c_void_p]
    L.smg_scene_softmax_objects.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_int,
                                            C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_double, C.c_void_p, C.c_void_p]
    L.smg_loss_scene.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p]
    L.smg_loss_scene_map.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]
    L.smg_loss_scene_policy.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p, C.c_int,
                                        C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.smg_scene_class_maps.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.smg_scene_class_values.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.smg_scene_class_argmax.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.smg_scene_class_argmax_objects.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                 C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.smg_scene_class_topk_objects.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p, C.c_int,
                                               C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int,
                                               C.c_void_p, C.c_void_p, C.c_void_p]
    L.smg_scene_class_best_maps.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p, C.c_int,
                                            C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.smg_scene_class_sample_objects.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                 C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_double, C.c_uint64,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
    L.smg_scene_class_softmax_objects.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                  C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_double, C.c_void_p, C.c_void_p]
    L.smg_loss_scene_ce.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]
    L.smg_loss_scene_map_ce.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.smg_backward.argtypes = [C.c_void_p, C.POINTER(SmgNet), C.c_void_p, C.c_void_p]
    if hasattr(L, "smg_backward_phase"):          # (absent from the dev builds tools/ab_kernels.sh compares against)
        L.smg_backward_phase.argtypes = [C.c_void_p, C.POINTER(SmgNet), C.c_void_p, C.c_void_p, C.c_int]
        L.smg_layout_trunk_split.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int64)]
    L.smg_engine_set_precision.argtypes = [C.c_void_p, C.c_int]
    L.smg_engine_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.smg_heightmap.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.smg_argmax.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.smg_adam_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int,
                                C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]
    L.smg_train_step_graph.argtypes = [C.c_void_p, C.POINTER(SmgNet), C.c_int, C.c_int, C.POINTER(SmgBatch), C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.POINTER(SmgAdam), C.c_void_p]
    L.smg_debug_read.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.smg_debug_read.restype = C.c_int64
    L.smg_profile_enable.argtypes = [C.c_void_p, C.c_int]
    L.smg_profile_kinds.restype = C.c_int
    L.smg_profile_kind_name.argtypes = [C.c_int]
    L.smg_profile_kind_name.restype = C.c_char_p
    L.smg_profile_read.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.smg_profile_read_bytes.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    _lib = L
    return L


EXPORTS = (
    "smg_last_error", "smg_version", "smg_abi_struct_bytes", "smg_engine_set_option", "smg_layout_count", "smg_layout_param_floats", "smg_layout_buffer_floats",
    "smg_layout_nbt_count", "smg_layout_entry", "smg_layout_trunk_range", "smg_layout_head_range",
    "smg_engine_create", "smg_engine_destroy", "smg_engine_workspace_bytes", "smg_engine_geometry",
    "smg_forward", "smg_loss", "smg_loss_map", "smg_loss_map_ce", "smg_scene_maps", "smg_scene_values", "smg_scene_argmax", "smg_scene_argmax_objects", "smg_scene_topk_objects", "smg_scene_sample_objects", "smg_scene_softmax_objects", "smg_scene_best_maps", "smg_loss_scene","smg_loss_scene_map", "smg_loss_scene_policy", "smg_scene_class_maps", "smg_scene_class_values", "smg_scene_class_argmax", "smg_scene_class_argmax_objects", "smg_scene_class_topk_objects", "smg_scene_class_sample_objects", "smg_scene_class_softmax_objects", "smg_scene_class_best_maps", "smg_loss_scene_ce", "smg_loss_scene_map_ce", "smg_backward", "smg_backward_phase", "smg_train_step_graph", "smg_layout_trunk_split", "smg_adam_step", "smg_argmax", "smg_heightmap", "smg_engine_set_precision", "smg_debug_read",
    "smg_profile_enable", "smg_profile_kinds", "smg_profile_kind_name", "smg_profile_read", "smg_profile_read_bytes",
)


def check(rc):
    if rc != 0:
        raise SmgError("libsmg_hip: %s (code %d)" % (lib().smg_last_error().decode(), rc))


def layout(head_out):
    """[(name, kind, offset, shape)] in the reference's state_dict order."""
    L = lib()
    out = []
    name = C.create_string_buffer(256)
    kind, ndim, off = C.c_int(), C.c_int(), C.c_int64()
    shape = (C.c_int64 * 4)()
    for i in range(L.smg_layout_count(head_out)):
        check(L.smg_layout_entry(head_out, i, name, 256, C.byref(kind), C.byref(off), C.byref(ndim), shape))
        out.append((name.value.decode(), kind.value, off.value, tuple(shape[k] for k in range(ndim.value))))
    return out


def trunk_range(head_out, trunk_id):
    o, n = C.c_int64(), C.c_int64()
    check(lib().smg_layout_trunk_range(head_out, trunk_id, C.byref(o), C.byref(n)))
    return o.value, n.value


def trunk_split(head_out, trunk_id):
    """Element offset of the first parameter behind dense block 1 (smg_layout_trunk_split)."""
    o = C.c_int64()
    check(lib().smg_layout_trunk_split(head_out, trunk_id, C.byref(o)))
    return o.value


def head_range(head_out, head_id):
    o, n = C.c_int64(), C.c_int64()
    check(lib().smg_layout_head_range(head_out, head_id, C.byref(o), C.byref(n)))
    return o.value, n.value


def _iarr(v):
    a = np.ascontiguousarray(v, dtype=np.int32)
    return a, a.ctypes.data_as(C.POINTER(C.c_int))


class Engine(object):
    """One smg_engine (workspaces for up to max_streams trunk passes / max_pairs heads)."""

    def __init__(self, device, input_size, max_streams, max_pairs, head_out):
        self.h = C.c_void_p()
        self.device, self.S, self.max_streams, self.max_pairs, self.head_out = device, input_size, max_streams, max_pairs, head_out
        check(lib().smg_engine_create(device, input_size, max_streams, max_pairs, head_out, C.byref(self.h)))
        H = (C.c_int * 6)()
        HWp = (C.c_int * 6)()
        check(lib().smg_engine_geometry(self.h, H, HWp))
        self.H, self.HWp = list(H), list(HWp)
        self.OH = self.OW = self.H[5] - 20 + 1
        self.forward_id = 0
        self.precision = "fp32"

    def close(self):
        if self.h:
            lib().smg_engine_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_precision(self, name):
        """Precision mode: 'fp32' (fp32 storage, split products on the 16-bit matrix cores: fp32-class; default), 'bf16' (bf16 storage of
        activations and gradients) or 'fp16' (fp16 activations, bf16 gradients); include/smg_hip.h."""
        code = PRECISIONS[str(name).replace("torch.", "")]
        check(lib().smg_engine_set_precision(self.h, code))
        self.precision = PRECISION_NAMES[code]          # canonical name: callers compare against 'fp32' / 'bf16' / 'fp16'

    def set_option(self, name, value):
        """Engine switches by name (smg_engine_set_option), e.g. ('deterministic', 1)."""
        check(lib().smg_engine_set_option(self.h, name.encode(), int(value)))

    @property
    def workspace_bytes(self):
        return lib().smg_engine_workspace_bytes(self.h)

    @staticmethod
    def _batch(images_nchw=None, heightmaps=None, hm_size=0, mean=0.0, std=1.0, n_images=0, stream_image=(), stream_affine=(),
               stream_rotated=(), pair_a=(), pair_b=(), bn_seq_trunk=None, bn_seq_head=None, masks=None, n_masks=0,
               stream_mask_a=None, stream_mask_b=None):
        """(smg_batch, arrays to keep alive while it is in use)"""
        b = SmgBatch()
        b.n_images = n_images
        b.images_nchw_dev = images_nchw
        b.heightmaps_dev = heightmaps
        b.hm_size = hm_size
        b.image_mean, b.image_std = mean, std
        keep = []
        a, p = _iarr(stream_image); keep.append(a); b.stream_image = p; b.n_streams = len(a)
        aff = np.ascontiguousarray(stream_affine, dtype=np.float32).reshape(-1); keep.append(aff)
        assert aff.size == 6 * b.n_streams
        b.stream_affine = aff.ctypes.data_as(C.POINTER(C.c_float))
        a, p = _iarr(stream_rotated); keep.append(a); b.stream_rotated = p
        a, p = _iarr(pair_a); keep.append(a); b.pair_a = p; b.n_pairs = len(a)
        a, p = _iarr(pair_b); keep.append(a); b.pair_b = p
        if bn_seq_trunk is not None and len(bn_seq_trunk):
            a, p = _iarr(bn_seq_trunk); keep.append(a); b.bn_seq_trunk = p; b.n_bn_seq_trunk = len(a)
        if bn_seq_head is not None and len(bn_seq_head):
            a, p = _iarr(bn_seq_head); keep.append(a); b.bn_seq_head = p; b.n_bn_seq_head = len(a)
        if masks is not None:
            b.masks_dev, b.n_masks = masks, n_masks
            a, p = _iarr(stream_mask_a); keep.append(a); b.stream_mask_a = p
            a, p = _iarr(stream_mask_b); keep.append(a); b.stream_mask_b = p
            assert len(stream_mask_a) == b.n_streams == len(stream_mask_b)
        return b, keep

    def forward(self, net, trunk_id, head_id, q_out, stream, **batch):
        b, keep = self._batch(**batch)
        check(lib().smg_forward(self.h, C.byref(net), trunk_id, head_id, C.byref(b), q_out, stream))
        self.forward_id += 1
        return self.forward_id

    def train_step_graph(self, net, trunk_id, head_id, loss_mode, labels, q_out, loss_out, dq, adam, stream, **batch):
        """smg_train_step_graph: zero grads + forward + loss + backward + Adam as one replayable hipGraph.  Returns the
        forward token (the engine holds that forward's activations afterwards)."""
        b, keep = self._batch(**batch)
        check(lib().smg_train_step_graph(self.h, C.byref(net), trunk_id, head_id, C.byref(b), loss_mode, labels, q_out, loss_out, dq,
                                         C.byref(adam), stream))
        self.forward_id += 1
        return self.forward_id

    def loss(self, mode, q, labels, n_pairs, loss_out, dq_out, stream):
        check(lib().smg_loss(self.h, mode, q, labels, n_pairs, loss_out, dq_out, stream))

    def loss_map(self, q, label_maps, weight_maps, n_pairs, loss_out, dq_out, stream):
        """smg_loss_map: the weighted whole-map Huber of a one-channel head; `weight_maps` None = all ones.  Marks the saved
        forward so that its backward runs the dense head form."""
        check(lib().smg_loss_map(self.h, q, label_maps, weight_maps, n_pairs, loss_out, dq_out, stream))

    def loss_map_ce(self, q, label_maps, n_pairs, loss_out, dq_out, stream):
        """smg_loss_map_ce: the whole-map cross entropy of a 3-class head, `label_maps` float32 class indices (0 / 1, anything else =
        class 2 = unlabelled).  Marks the saved forward so that its backward runs the dense head form."""
        check(lib().smg_loss_map_ce(self.h, q, label_maps, n_pairs, loss_out, dq_out, stream))

    @staticmethod
    def _affines(affine, n):
        a = np.ascontiguousarray(affine, dtype=np.float32).reshape(-1)
        if a.size != 6 * n:
            raise ValueError("need 6 affine numbers per map, got %d for %d maps" % (a.size, n))
        return a, a.ctypes.data_as(C.POINTER(C.c_float))

    def scene_maps(self, q, map_stride, n_maps, affine, hm_size, out, stream):
        """smg_scene_maps: the n_maps Q maps at `q` (device, `map_stride` elements apart) rotated back by their `affine`
        (host, 6 float32 each: models.rotation_theta) and upsampled to `out` [n_maps, hm_size, hm_size]; -inf where invalid."""
        a, p = self._affines(affine, n_maps)
        check(lib().smg_scene_maps(self.h, q, int(map_stride), int(n_maps), p, int(hm_size), out, stream))

    def scene_values(self, q, map_stride, n_maps, affine, hm_size, K, pixels, out, stream):
        """smg_scene_values: the value of those scene-frame maps at K listed heightmap pixels per map (`pixels` device int32
        [n_maps, K, 2] = iy, ix) to `out` [n_maps, K], the floats scene_maps stores there, without writing the maps; -inf where
        invalid or outside the heightmap."""
        a, p = self._affines(affine, n_maps)
        check(lib().smg_scene_values(self.h, q, int(map_stride), int(n_maps), p, int(hm_size), int(K), pixels, out, stream))

    def scene_argmax(self, q, map_stride, n_maps, affine, hm_size, idx_out, val_out, stream):
        """smg_scene_argmax: the best valid (map, iy, ix) of those scene-frame maps as a flattened index, without writing them."""
        a, p = self._affines(affine, n_maps)
        check(lib().smg_scene_argmax(self.h, q, int(map_stride), int(n_maps), p, int(hm_size), idx_out, val_out, stream))

    @staticmethod
    def _selects(n_maps, mask_a, mask_b, groups):
        """the per-map mask indices and group ids of the *_argmax_objects calls as int32 arrays (kept alive by the caller) and pointers"""
        sel = []
        for name, seq in (("mask_a", mask_a), ("mask_b", mask_b), ("groups", groups)):
            arr = np.ascontiguousarray(seq, dtype=np.int32).reshape(-1)
            if arr.size != n_maps:
                raise ValueError("%s: need one int per map, got %d for %d maps" % (name, arr.size, n_maps))
            sel.append(arr)
        return sel, [s.ctypes.data_as(C.POINTER(C.c_int)) for s in sel]

    def scene_argmax_objects(self, q, map_stride, n_maps, affine, hm_size, masks, n_masks, mask_a, mask_b, groups, n_groups,
                             idx_out, val_out, stream):
        """smg_scene_argmax_objects: scene_argmax per group of maps, every map on the heightmap pixels its masks select - `masks`
        the device float64 [n_masks, hm_size, hm_size] tensor of the forward, `mask_a` / `mask_b` / `groups` host sequences of
        n_maps ints (mask index or -1; group in [0, n_groups)).  idx_out int32[n_groups] = flattened index into [n_maps, hm, hm]
        or -1, val_out float32[n_groups]."""
        a, p = self._affines(affine, n_maps)
        sel, (ma, mb, gr) = self._selects(n_maps, mask_a, mask_b, groups)
        check(lib().smg_scene_argmax_objects(self.h, q, int(map_stride), int(n_maps), p, int(hm_size), masks, int(n_masks), ma, mb, gr,
                                             int(n_groups), idx_out, val_out, stream))

    def scene_topk_objects(self, q, map_stride, n_maps, affine, hm_size, masks, n_masks, mask_a, mask_b, groups, n_groups, K, radius,
                           idx_out, val_out, stream):
        """smg_scene_topk_objects: scene_argmax_objects' arguments plus `K` ranks and a suppression `radius` in heightmap pixels -
        per group the K best selected valid pixels, each farther than `radius` from every earlier pick of its group (in any of the
        group's maps).  idx_out int32 [n_groups, K] = flattened index into [n_maps, hm, hm] or -1, val_out float32 [n_groups, K];
        rank 0 is scene_argmax_objects' result, an exhausted group ends in (-1, -inf)."""
        a, p = self._affines(affine, n_maps)
        sel, (ma, mb, gr) = self._selects(n_maps, mask_a, mask_b, groups)
        check(lib().smg_scene_topk_objects(self.h, q, int(map_stride), int(n_maps), p, int(hm_size), masks, int(n_masks), ma, mb, gr,
                                           int(n_groups), int(K), int(radius), idx_out, val_out, stream))

    def scene_best_maps(self, q, map_stride, n_maps, affine, hm_size, masks, n_masks, mask_a, mask_b, groups, n_groups, val_out, arg_out, stream):
        """smg_scene_best_maps: the collapsed map - scene_argmax_objects' arguments, but per group and heightmap PIXEL: val_out
        float32 [n_groups, hm, hm] = the best value over the group's maps that select the pixel and have a window there (the float
        scene_maps stores), arg_out int32 [n_groups, hm, hm] = that map's index in the call (lowest on ties, the first NaN wins);
        (-inf, -1) where there is none.  `masks` None (or 0) with n_masks 0 and every term -1 is the sweep form."""
        a, p = self._affines(affine, n_maps)
        sel, (ma, mb, gr) = self._selects(n_maps, mask_a, mask_b, groups)
        check(lib().smg_scene_best_maps(self.h, q, int(map_stride), int(n_maps), p, int(hm_size), masks or None, int(n_masks), ma, mb, gr,
                                        int(n_groups), val_out, arg_out, stream))

    def scene_sample_objects(self, q, map_stride, n_maps, affine, hm_size, masks, n_masks, mask_a, mask_b, groups, n_groups, n_draws, beta,
                             seed, idx_out, val_out, stream):
        """smg_scene_sample_objects: scene_argmax_objects' arguments plus `n_draws` (1 .. 32), `beta` = 1 / temperature (finite,
        >= 0) and a 64-bit `seed` - per group n_draws independent draws of a selected valid (map, pixel) with probability
        proportional to exp(beta * value), by the Gumbel-max rule on counter-based noise (include/smg_hip.h states the hash).
        idx_out int32 [n_groups, n_draws] = flattened index into [n_maps, hm, hm] or -1, val_out float32 [n_groups, n_draws] = the
        map value at the pick; a group without a candidate is (-1, -inf) in every draw.  A pure function of its arguments."""
        a, p = self._affines(affine, n_maps)
        sel, (ma, mb, gr) = self._selects(n_maps, mask_a, mask_b, groups)
        check(lib().smg_scene_sample_objects(self.h, q, int(map_stride), int(n_maps), p, int(hm_size), masks, int(n_masks), ma, mb, gr,
                                             int(n_groups), int(n_draws), float(beta), int(seed), idx_out, val_out, stream))

    def scene_softmax_objects(self, q, map_stride, n_maps, affine, hm_size, masks, n_masks, mask_a, mask_b, groups, n_groups, beta,
                              stats_out, stream):
        """smg_scene_softmax_objects: the normaliser of scene_sample_objects' policy - scene_argmax_objects' arguments plus `beta`
        = 1 / temperature (finite, >= 0).  stats_out float64 [n_groups, 4] = per group {count, vmax, lse, mean} over its selected
        valid pixels: how many, the largest value, log sum exp(beta * value) and the Boltzmann mean of the value; a group without a
        candidate is (0, -inf, -inf, NaN).  log pi of a drawn pick is beta * value - lse."""
        a, p = self._affines(affine, n_maps)
        sel, (ma, mb, gr) = self._selects(n_maps, mask_a, mask_b, groups)
        check(lib().smg_scene_softmax_objects(self.h, q, int(map_stride), int(n_maps), p, int(hm_size), masks, int(n_masks), ma, mb, gr,
                                              int(n_groups), float(beta), stats_out, stream))

    def loss_scene(self, q, affine, hm_size, n_pairs, K, pixels, labels, weights, loss_out, dq_out, stream):
        """smg_loss_scene: the weighted Huber on K heightmap pixels (int32 [n_pairs, K, 2] = iy, ix) per pair, dq on the map;
        `weights` None = all ones.  Marks the saved forward so that its backward runs the dense head form."""
        a, p = self._affines(affine, n_pairs)
        check(lib().smg_loss_scene(self.h, q, p, int(hm_size), int(n_pairs), int(K), pixels, labels, weights, loss_out, dq_out, stream))

    def loss_scene_map(self, q, affine, hm_size, n_pairs, label_maps, weight_maps, loss_out, dq_out, stream):
        """smg_loss_scene_map: the weighted Huber on a whole label image per pair (`label_maps` / `weight_maps` device float32
        [n_pairs, hm_size, hm_size], `weight_maps` None = all ones), dq on the map; pixels without a window in their pair's
        rotation contribute nothing.  Marks the saved forward so that its backward runs the dense head form."""
        a, p = self._affines(affine, n_pairs)
        check(lib().smg_loss_scene_map(self.h, q, p, int(hm_size), int(n_pairs), label_maps, weight_maps, loss_out, dq_out, stream))

    def loss_scene_policy(self, q, affine, hm_size, n_pairs, masks, n_masks, mask_a, mask_b, groups, n_groups, beta, actions, weights,
                          stats_out, loss_out, dq_out, stream):
        """smg_loss_scene_policy: the log-likelihood and entropy loss of the Boltzmann policy pi = softmax(beta v) per group of pairs
        - scene_softmax_objects' selection on the pairs of q [n_pairs, 1, OH, OW] plus, on the device, `actions` int32 [n_groups]
        (the executed action as a flattened index into [n_pairs, hm, hm], -1 = none) and `weights` float64 [n_groups, 2] =
        {w_nll, w_ent}.  loss_out float32 [n_groups] = w_nll (lse - beta v_act) - w_ent (lse - beta mean), stats_out float64
        [n_groups, 4] = scene_softmax_objects' rows, dq_out its gradient on the maps, every element written.  Marks the saved
        forward so that its backward runs the dense head form."""
        a, p = self._affines(affine, n_pairs)
        sel, (ma, mb, gr) = self._selects(n_pairs, mask_a, mask_b, groups)
        check(lib().smg_loss_scene_policy(self.h, q, p, int(hm_size), int(n_pairs), masks, int(n_masks), ma, mb, gr, int(n_groups), float(beta),
                                          actions, weights, stats_out, loss_out, dq_out, stream))

    def scene_class_maps(self, q, n_maps, affine, hm_size, cls, out, stream):
        """smg_scene_class_maps: the class probabilities of the n_maps logit maps at `q` (device, [n_maps, 3, OH, OW]) in the scene
        frame - logits interpolated, softmax at the pixel - to `out` [n_maps, hm_size, hm_size] for cls 0 / 1 / 2 or
        [n_maps, 3, hm_size, hm_size] for cls -1; -inf where invalid."""
        a, p = self._affines(affine, n_maps)
        check(lib().smg_scene_class_maps(self.h, q, int(n_maps), p, int(hm_size), int(cls), out, stream))

    def scene_class_values(self, q, n_maps, affine, hm_size, cls, K, pixels, out, stream):
        """smg_scene_class_values: the class probabilities scene_class_maps stores at K listed heightmap pixels per map (`pixels`
        device int32 [n_maps, K, 2] = iy, ix) to `out` [n_maps, K] for cls 0 / 1 / 2 or [n_maps, 3, K] for cls -1, without
        writing the maps; -inf where invalid or outside the heightmap."""
        a, p = self._affines(affine, n_maps)
        check(lib().smg_scene_class_values(self.h, q, int(n_maps), p, int(hm_size), int(cls), int(K), pixels, out, stream))

    def scene_class_argmax(self, q, n_maps, affine, hm_size, cls, idx_out, val_out, stream):
        """smg_scene_class_argmax: the valid (map, iy, ix) with the largest P(class cls) as a flattened index, without writing the maps."""
        a, p = self._affines(affine, n_maps)
        check(lib().smg_scene_class_argmax(self.h, q, int(n_maps), p, int(hm_size), int(cls), idx_out, val_out, stream))

    def scene_class_argmax_objects(self, q, n_maps, affine, hm_size, cls, masks, n_masks, mask_a, mask_b, groups, n_groups,
                                   idx_out, val_out, stream):
        """smg_scene_class_argmax_objects: scene_class_argmax per group of maps, every map on the heightmap pixels its masks select
        - scene_argmax_objects' arguments on the logit maps `q` [n_maps, 3, OH, OW]; the value is P(class cls), cls 0 / 1 / 2."""
        a, p = self._affines(affine, n_maps)
        sel, (ma, mb, gr) = self._selects(n_maps, mask_a, mask_b, groups)
        check(lib().smg_scene_class_argmax_objects(self.h, q, int(n_maps), p, int(hm_size), int(cls), masks, int(n_masks), ma, mb, gr,
                                                   int(n_groups), idx_out, val_out, stream))

    def scene_class_topk_objects(self, q, n_maps, affine, hm_size, cls, masks, n_masks, mask_a, mask_b, groups, n_groups, K, radius,
                                 idx_out, val_out, stream):
        """smg_scene_class_topk_objects: scene_topk_objects on the logit maps `q` [n_maps, 3, OH, OW] - scene_class_argmax_objects'
        arguments plus `K` and `radius`; the value is P(class cls), idx_out / val_out are [n_groups, K]."""
        a, p = self._affines(affine, n_maps)
        sel, (ma, mb, gr) = self._selects(n_maps, mask_a, mask_b, groups)
        check(lib().smg_scene_class_topk_objects(self.h, q, int(n_maps), p, int(hm_size), int(cls), masks, int(n_masks), ma, mb, gr,
                                                 int(n_groups), int(K), int(radius), idx_out, val_out, stream))

    def scene_class_best_maps(self, q, n_maps, affine, hm_size, cls, masks, n_masks, mask_a, mask_b, groups, n_groups, val_out, arg_out, stream):
        """smg_scene_class_best_maps: scene_best_maps on the logit maps `q` [n_maps, 3, OH, OW]; the value is P(class cls), cls
        0 / 1 / 2, the float scene_class_maps stores."""
        a, p = self._affines(affine, n_maps)
        sel, (ma, mb, gr) = self._selects(n_maps, mask_a, mask_b, groups)
        check(lib().smg_scene_class_best_maps(self.h, q, int(n_maps), p, int(hm_size), int(cls), masks or None, int(n_masks), ma, mb, gr,
                                              int(n_groups), val_out, arg_out, stream))

    def scene_class_sample_objects(self, q, n_maps, affine, hm_size, cls, masks, n_masks, mask_a, mask_b, groups, n_groups, n_draws, beta,
                                   seed, idx_out, val_out, stream):
        """smg_scene_class_sample_objects: scene_sample_objects on the logit maps `q` [n_maps, 3, OH, OW] - scene_class_argmax_objects'
        arguments plus `n_draws`, `beta` and `seed`; the value is P(class cls), idx_out / val_out are [n_groups, n_draws]."""
        a, p = self._affines(affine, n_maps)
        sel, (ma, mb, gr) = self._selects(n_maps, mask_a, mask_b, groups)
        check(lib().smg_scene_class_sample_objects(self.h, q, int(n_maps), p, int(hm_size), int(cls), masks, int(n_masks), ma, mb, gr,
                                                   int(n_groups), int(n_draws), float(beta), int(seed), idx_out, val_out, stream))

    def scene_class_softmax_objects(self, q, n_maps, affine, hm_size, cls, masks, n_masks, mask_a, mask_b, groups, n_groups, beta,
                                    stats_out, stream):
        """smg_scene_class_softmax_objects: scene_softmax_objects on the logit maps `q` [n_maps, 3, OH, OW] - scene_class_argmax_objects'
        arguments plus `beta`; the value is P(class cls), stats_out is float64 [n_groups, 4]."""
        a, p = self._affines(affine, n_maps)
        sel, (ma, mb, gr) = self._selects(n_maps, mask_a, mask_b, groups)
        check(lib().smg_scene_class_softmax_objects(self.h, q, int(n_maps), p, int(hm_size), int(cls), masks, int(n_masks), ma, mb, gr,
                                                    int(n_groups), float(beta), stats_out, stream))

    def loss_scene_ce(self, q, affine, hm_size, n_pairs, K, pixels, labels, loss_out, dq_out, stream):
        """smg_loss_scene_ce: the cross entropy (class weights {1, 1, 0}) on K heightmap pixels (int32 [n_pairs, K, 2] = iy, ix) per
        pair, `labels` float32 class indices, dq on the three logit maps.  Marks the saved forward so that its backward runs the
        dense head form."""
        a, p = self._affines(affine, n_pairs)
        check(lib().smg_loss_scene_ce(self.h, q, p, int(hm_size), int(n_pairs), int(K), pixels, labels, loss_out, dq_out, stream))

    def loss_scene_map_ce(self, q, affine, hm_size, n_pairs, label_maps, loss_out, dq_out, stream):
        """smg_loss_scene_map_ce: the cross entropy (class weights {1, 1, 0}) on a whole class-label image per pair (`label_maps`
        device float32 [n_pairs, hm_size, hm_size]; 0 and 1 count, anything else is "no loss"), the mean over the labelled pixels
        that have a window in their pair's rotation, dq on the three logit maps.  Marks the saved forward so that its backward
        runs the dense head form."""
        a, p = self._affines(affine, n_pairs)
        check(lib().smg_loss_scene_map_ce(self.h, q, p, int(hm_size), int(n_pairs), label_maps, loss_out, dq_out, stream))

    def backward(self, net, dq, stream, phase=None):
        """phase None: the whole backward; 0 / 1: its two halves (smg_backward_phase)."""
        if phase is None:
            check(lib().smg_backward(self.h, C.byref(net), dq, stream))
        else:
            check(lib().smg_backward_phase(self.h, C.byref(net), dq, stream, int(phase)))

    def debug_read(self, name, stream=None, count=None):
        """count: read only the first `count` floats (a prefix of whole streams for the ring-slot names)."""
        n = lib().smg_debug_read(self.h, name.encode(), None, 0, stream)
        if n < 0:
            check(int(n))
        if count is not None:
            n = min(n, int(count))
        out = np.empty(n, dtype=np.float32)
        got = lib().smg_debug_read(self.h, name.encode(), out.ctypes.data_as(C.c_void_p), n, stream)
        if got < 0:
            check(int(got))
        return out[:got]

    def profile_enable(self, on):
        check(lib().smg_profile_enable(self.h, 1 if on else 0))

    def profile_read(self):
        """{kind_name: (ms, launches, flops, algorithmic HBM bytes)}"""
        L = lib()
        out = {}
        ms, n, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        for k in range(L.smg_profile_kinds()):
            check(L.smg_profile_read(self.h, k, C.byref(ms), C.byref(n), C.byref(fl)))
            check(L.smg_profile_read_bytes(self.h, k, C.byref(by)))
            out[L.smg_profile_kind_name(k).decode()] = (ms.value, n.value, fl.value, by.value)
        return out

    def profile_read_stages(self):
        """{kind_name: [(ms, launches, flops) for dense block 1..4]} -- the share of each dense block
        (kind ids kinds*(1+block) + kind of smg_profile_read)."""
        L = lib()
        out = {}
        ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
        K = L.smg_profile_kinds()
        for k in range(K):
            rows = []
            for b in range(4):
                check(L.smg_profile_read(self.h, K * (1 + b) + k, C.byref(ms), C.byref(n), C.byref(fl)))
                rows.append((ms.value, n.value, fl.value))
            out[L.smg_profile_kind_name(k).decode()] = rows
        return out


PRECISIONS = {"fp32": 0, "float32": 0, "bf16": 1, "bfloat16": 1, "fp16": 2, "float16": 2, "half": 2}
PRECISION_NAMES = {0: "fp32", 1: "bf16", 2: "fp16"}


def heightmap(depth_img, h, w, intrinsics, cam_pose, inv_homography, out_w, out_h, out, stream):
    def d(a, n):
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        assert a.size == n
        return a, a.ctypes.data_as(C.POINTER(C.c_double))
    k, kp = d(intrinsics, 9)
    t, tp = d(cam_pose, 16)
    m, mp = d(inv_homography, 9)
    check(lib().smg_heightmap(depth_img, h, w, kp, tp, mp, out_w, out_h, out, stream))


def argmax(values, n, idx_out, val_out, stream):
    check(lib().smg_argmax(values, n, idx_out, val_out, stream))


def adam_step(params, grads, m, v, offset, count, step, lr, beta1, beta2, eps, stream):
    check(lib().smg_adam_step(params, grads, m, v, offset, count, step, lr, beta1, beta2, eps, stream))
