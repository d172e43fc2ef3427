"""ctypes view of the C ABI declared in include/p264hip.h, include/p264parse.h and
include/p264_dropin.h.  No torch types cross this boundary: plain pointers and sizes.

The shared library is built in-tree by ``p264decoder_amd/build.py`` (hipcc, gfx950) as
``p264decoder_amd/libp264amd.so``.  There is no CPU fallback for the reconstruction:
if the library is missing, importing the product entry points raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libp264amd.so")

MAX_REFS = 16
NKERNELS = 4

MB_I4x4, MB_I16x16, MB_IPCM, MB_P_L0, MB_P_8x8, MB_P_SKIP, MB_B = range(7)
SLICE_P, SLICE_B, SLICE_I = 0, 1, 2
COEF_LUMA_DC = 1 << 24
COEF_CHROMA_DC = 1 << 25
AVAIL_LEFT, AVAIL_TOP, AVAIL_TOPRIGHT, AVAIL_TOPLEFT = 1, 2, 4, 8
EDGE_LEFT, EDGE_TOP, EDGE_INNER = 1, 2, 4
MB_I8X8 = 0x08          # bit of MbInfo.intra_modes: an I4x4 record predicted as Intra 8x8 (luma coded as 8x8 blocks)
SCALING_BYTES = 224     # Picture.scaling4x4 + Picture.scaling8x8: the table as it lies in an input slot and in a compact block
T8X8_INTRA = 2          # bit of Picture.transform_8x8: Intra4x4 records may carry MB_I8X8
MB_T8X8 = 0x04          # bit of MbInfo.intra_modes: the inter macroblock's luma residual is coded as 8x8 blocks


class MbInfo(C.Structure):
    """p264hip_mb_t (16 bytes)"""
    _fields_ = [
        ("mb_type", C.c_uint8), ("qp", C.c_uint8), ("cbp", C.c_uint8), ("intra_modes", C.c_uint8),
        ("coef_mask", C.c_uint32), ("coef_index", C.c_uint32),
        ("avail", C.c_uint8), ("edges", C.c_uint8), ("flags", C.c_uint16),
    ]


class Picture(C.Structure):
    """p264hip_picture_t"""
    _fields_ = [
        ("mb_w", C.c_int32), ("mb_h", C.c_int32), ("slice_type", C.c_int32),
        ("chroma_qp_offset", C.c_int32), ("deblock", C.c_int32),
        ("alpha_c0_offset", C.c_int32), ("beta_offset", C.c_int32),
        ("dst_slot", C.c_int32), ("n_ref", C.c_int32), ("ref_slot", C.c_int32 * MAX_REFS),
        ("n_coef_blocks", C.c_uint32), ("frame_num", C.c_uint32),
        ("mb", C.POINTER(MbInfo)), ("mv", C.POINTER(C.c_int16)), ("ref_idx", C.POINTER(C.c_int8)),
        ("i4modes", C.POINTER(C.c_uint8)), ("coefs", C.POINTER(C.c_int16)),
        ("mv_l1", C.POINTER(C.c_int16)), ("ref_idx_l1", C.POINTER(C.c_int8)), ("n_ref_l1", C.c_int32), ("weighted_bipred", C.c_int32),
        ("ref_slot_l1", C.c_int32 * MAX_REFS), ("bipred_weight", C.c_int16 * (MAX_REFS * MAX_REFS)),
        ("explicit_wp", C.c_int32), ("wp_log2_denom", C.c_int32 * 2), ("wp", C.c_int16 * (2 * MAX_REFS * 3 * 2)),   # wp: [list][ref_idx][Y, Cb, Cr][weight, offset], flat
        ("transform_8x8", C.c_int32),
        # scaling matrices: the eight resolved lists in scan order (4x4: Intra Y, Cb, Cr, Inter Y, Cb, Cr; 8x8: Intra Y, Inter Y), flat
        ("scaling_lists", C.c_int32), ("scaling4x4", C.c_uint8 * (6 * 16)), ("scaling8x8", C.c_uint8 * (2 * 64)),
        # second_chroma_qp_index_offset - chroma_qp_index_offset: Cr's qPI is Clip3(0, 51, QPY + chroma_qp_offset + cr_qp_offset_delta)
        ("cr_qp_offset_delta", C.c_int32),
    ]


assert C.sizeof(MbInfo) == 16


class LaunchInfo(C.Structure):
    """p264hip_launch_info_t"""
    _fields_ = [(n, C.c_int32) for n in ("pictures", "compute_units", "mc_wgs_per_picture", "intra_waves", "edge_info_fused",
                                         "deblock_pics_per_wg", "deblock_rb_log2", "deblock_waves", "deblock_wgs", "deblock_odd_single", "t8x8_wgs", "scaled_pictures", "cr_pictures")] + [("reserved", C.c_int32 * 2), ("intra_i8", C.c_int32)]


BUILD_TIMING = 1


class InputLayout(C.Structure):
    """p264hip_input_layout_t"""
    _fields_ = [(n, C.c_size_t) for n in ("off_mb", "off_mv", "off_ref", "off_i4", "off_coef", "off_mv_l1", "off_ref_l1", "off_weights", "bytes", "off_wp", "off_scaling")]


class CompactList(C.Structure):
    _fields_ = [("off_ref", C.c_uint32), ("off_shape", C.c_uint32), ("off_vec", C.c_uint32), ("n_vec", C.c_uint32)]


class _CompactTail(C.Union):
    """the last ten words of p264hip_compact_hdr_t: off_scaling is the first of what used to be reserved[10] (0 for flat pictures)"""
    _fields_ = [("reserved", C.c_uint32 * 10), ("off_scaling", C.c_uint32)]


class CompactHdr(C.Structure):
    """p264hip_compact_hdr_t (128 bytes)"""
    _anonymous_ = ("tail",)
    _fields_ = [("magic", C.c_uint32), ("n_mb", C.c_uint32), ("n_coef_blocks", C.c_uint32), ("bytes", C.c_uint32), ("n_lists", C.c_uint32),
                ("off_rec", C.c_uint32), ("off_i4flag", C.c_uint32), ("off_i4", C.c_uint32), ("off_lvflag", C.c_uint32), ("off_levels", C.c_uint32),
                ("off_weights", C.c_uint32), ("n_i4", C.c_uint32), ("level_bytes", C.c_uint32), ("list", CompactList * 2), ("off_wp", C.c_uint32), ("tail", _CompactTail)]


class PipeStats(C.Structure):
    """p264pipe_stats_t"""
    _fields_ = [("pictures", C.c_int64), ("bytes", C.c_int64), ("seconds", C.c_double), ("parse_seconds", C.c_double),
                ("submit_seconds", C.c_double), ("rounds", C.c_int), ("streams", C.c_int), ("threads", C.c_int), ("reserved", C.c_int),
                ("bytes_uploaded", C.c_int64), ("wait_parse_seconds", C.c_double), ("wait_device_seconds", C.c_double)]

class ParseOutput(C.Structure):
    """p264parse_output_t"""
    _fields_ = [("slot", C.c_int), ("poc", C.c_int), ("decode_index", C.c_int), ("flags", C.c_int)]


class PipeOutput(C.Structure):
    """p264pipe_output_t"""
    _fields_ = [("stream", C.c_int), ("poc", C.c_int), ("decode_index", C.c_int), ("flags", C.c_int)]


OUT_IDR, OUT_MMCO5 = 1, 2
MAX_OUTPUTS = MAX_REFS + 1


class Export(C.Structure):
    """p264hip_export_t"""
    _fields_ = [("format", C.c_int32), ("matrix", C.c_int32), ("full_range", C.c_int32),
                ("crop_left", C.c_int32), ("crop_top", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("pitch", C.c_int32), ("frame_stride", C.c_int64)]


FMT_I420, FMT_NV12, FMT_RGB24, FMT_RGBP = range(4)
MATRIX_BT601, MATRIX_BT709 = 0, 1
FORMATS = {"i420": FMT_I420, "nv12": FMT_NV12, "rgb24": FMT_RGB24, "rgbp": FMT_RGBP}
MATRICES = {"bt601": MATRIX_BT601, "bt709": MATRIX_BT709}
# p264pipe_sink_fn: (user, round, n, streams, dev)
SINK_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p)


def export_desc(fmt="i420", crop=None, frame=None, matrix="bt601", full_range=False, pitch=0, frame_stride=0):
    """A p264hip_export_t: fmt / matrix by name (or number), crop = (left, top, width, height) or None for the whole `frame` =
    (width, height).  Names that do not exist raise; everything else is the library's to check."""
    e = Export()
    e.format = FORMATS[fmt] if isinstance(fmt, str) else int(fmt)
    e.matrix = MATRICES[matrix] if isinstance(matrix, str) else int(matrix)
    e.full_range = int(full_range)
    e.crop_left, e.crop_top, e.width, e.height = crop if crop is not None else (0, 0, frame[0], frame[1])
    e.pitch, e.frame_stride = int(pitch), int(frame_stride)
    return e


class Resize(C.Structure):
    """p264hip_resize_t"""
    _fields_ = [("format", C.c_int32), ("matrix", C.c_int32), ("full_range", C.c_int32),
                ("crop_left", C.c_int32), ("crop_top", C.c_int32), ("crop_width", C.c_int32), ("crop_height", C.c_int32),
                ("width", C.c_int32), ("height", C.c_int32), ("dtype", C.c_int32), ("filter", C.c_int32),
                ("pitch", C.c_int32), ("frame_stride", C.c_int64), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


DTYPE_U8, DTYPE_F16, DTYPE_F32 = range(3)
FILTER_BILINEAR, FILTER_BILINEAR_AA = 0, 2
FILTERS = {"bilinear": FILTER_BILINEAR, "bilinear_aa": FILTER_BILINEAR_AA}
AA_MAX_TAPS = 64
DTYPES = {"u8": DTYPE_U8, "f16": DTYPE_F16, "f32": DTYPE_F32}
ELEM_BYTES = {DTYPE_U8: 1, DTYPE_F16: 2, DTYPE_F32: 4}


def resize_desc(fmt="rgbp", size=None, crop=None, frame=None, dtype="u8", scale=None, bias=None, matrix="bt601", full_range=False, pitch=0,
                frame_stride=0, filter=FILTER_BILINEAR):
    """A p264hip_resize_t: fmt / dtype / matrix / filter ("bilinear", "bilinear_aa") by name (or number), size = (width, height) of the output (None: the window's), crop =
    (left, top, width, height) of the source window or None for the whole `frame` = (width, height), scale / bias = one number for
    all channels or three (R, G, B; None: 0).  Names that do not exist raise; everything else is the library's to check."""
    r = Resize()
    r.format = FORMATS[fmt] if isinstance(fmt, str) else int(fmt)
    r.matrix = MATRICES[matrix] if isinstance(matrix, str) else int(matrix)
    r.full_range = int(full_range)
    r.crop_left, r.crop_top, r.crop_width, r.crop_height = crop if crop is not None else (0, 0, frame[0], frame[1])
    r.width, r.height = size if size is not None else (r.crop_width, r.crop_height)
    r.dtype = DTYPES[dtype] if isinstance(dtype, str) else int(dtype)
    r.filter = FILTERS[filter] if isinstance(filter, str) else int(filter)
    r.pitch, r.frame_stride = int(pitch), int(frame_stride)
    for name, v in (("scale", scale), ("bias", bias)):
        v = (0.0, 0.0, 0.0) if v is None else tuple(v) if hasattr(v, "__len__") else (v, v, v)
        if len(v) != 3:
            raise ValueError("%s: one number or three" % name)
        setattr(r, name, (C.c_float * 3)(*v))
    return r


class Roi(C.Structure):
    """p264hip_roi_t"""
    _fields_ = [("stream", C.c_int32), ("slot", C.c_int32),
                ("left", C.c_int32), ("top", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("dst_left", C.c_int32), ("dst_top", C.c_int32), ("dst_width", C.c_int32), ("dst_height", C.c_int32)]


ROI_SCRATCH_BYTES = 16 << 20          # P264HIP_ROI_SCRATCH_BYTES
# P264HIP_ROI_*: the status of an ROI of a list in device memory (p264hip_export_rois_device)
(ROI_OK, ROI_UNUSED, ROI_BAD_PICTURE, ROI_NO_PICTURE, ROI_WINDOW_EMPTY, ROI_WINDOW_ODD, ROI_WINDOW_OUTSIDE, ROI_RECT_SMALL, ROI_RECT_ODD,
 ROI_RECT_OUTSIDE, ROI_REDUCTION) = range(11)
ROIS_AFTER, ROIS_BEFORE = 1, 2        # P264HIP_ROIS_*


class RoisPlan(C.Structure):
    """p264hip_rois_plan_t"""
    _fields_ = [("seg_words", C.c_int32), ("rois_per_pair", C.c_int32), ("aa_tiles", C.c_int32), ("aa_lds_bytes", C.c_int32)]


class RoisDev(C.Structure):
    """p264hip_rois_dev_t"""
    _fields_ = [("rois_dev", C.c_void_p), ("count_dev", C.c_void_p), ("status_dev", C.c_void_p), ("slot_of_stream", C.POINTER(C.c_int32)),
                ("after_stream", C.c_void_p), ("before_stream", C.c_void_p), ("n", C.c_int32), ("max_reduction", C.c_int32), ("flags", C.c_int32)]


def rois_device_plan(desc, max_reduction=0, lib=None):
    """p264hip_rois_device_plan as a dict (seg_words, rois_per_pair, aa_tiles, aa_lds_bytes): what a call with an ROI list in device
    memory reserves per ROI for the output `desc` (a p264hip_resize_t) describes.  Raises where the library refuses."""
    plan = RoisPlan()
    if (lib or load()).p264hip_rois_device_plan(C.byref(desc), int(max_reduction), C.byref(plan)) != 0:
        raise ValueError("p264hip_rois_device_plan refuses the description (filter %d, max_reduction %d)" % (desc.filter, max_reduction))
    return {n: int(getattr(plan, n)) for n, _ in RoisPlan._fields_}


def roi_array(rois, head=2):
    """A (p264hip_roi_t array, n) from a sequence of rows or an (n, k) integer array.  A row is `head` leading members (stream, slot -
    or stream alone: head=1, the slot becomes -1), the window (left, top, width, height) and, optionally, the rectangle (dst_left,
    dst_top, dst_width, dst_height); without the rectangle the window fills the whole output.  A row of another length raises."""
    import numpy as np
    a = rois if isinstance(rois, np.ndarray) else None
    if a is None:
        rows = [tuple(row) for row in rois]
        for i, row in enumerate(rows):
            if len(row) not in (head + 4, head + 8):
                raise ValueError("ROI %d has %d members: %d or %d" % (i, len(row), head + 4, head + 8))
        a = np.array([row + (0, 0, 0, 0) if len(row) == head + 4 else row for row in rows], dtype=np.int64).reshape(len(rows), head + 8)
    if a.ndim != 2 or a.shape[1] not in (head + 4, head + 8) or a.dtype.kind not in "iu":
        raise ValueError("ROIs: an (n, %d) or (n, %d) integer array" % (head + 4, head + 8))
    full = np.zeros((max(len(a), 1), 10), np.int32)
    if head == 1:
        full[:len(a), 0] = a[:, 0]
        full[:len(a), 1] = -1
        full[:len(a), 2:1 + a.shape[1]] = a[:, 1:]
    else:
        full[:len(a), :a.shape[1]] = a
    arr = (Roi * len(full)).from_buffer_copy(full.tobytes())
    return arr, len(a)


def fill_word(fill):
    """fill = (Y, Cb, Cr) as p264hip_export_rois takes it: Y | Cb << 8 | Cr << 16"""
    y, cb, cr = (int(v) for v in fill)
    if not all(0 <= v <= 255 for v in (y, cb, cr)):
        raise ValueError("fill: three values 0 .. 255")
    return y | cb << 8 | cr << 16


def export_out(n, desc, per, pitch, frame_stride, out, check=None, wait=True):
    """(out, pointer, bytes): where an export call writes its n pictures of the description `desc` (p264hip_export_t /
    p264hip_resize_t), `per` bytes each.  out: a (device pointer, bytes) pair, handed through; a torch tensor on the device; or None -
    a new tensor (n, H*3//2, W) for I420 / NV12, (n, H, W, 3) for RGB24, (n, 3, H, W) for RGBP of the description's dtype at the tight
    layout, (n, bytes) uint8 where a pitch or a frame_stride is given.  check = (exception type, method name): refuse a tensor that
    is not contiguous, on the device and of the dtype (or uint8), and wait for what torch's current stream still has queued on it -
    the context has its own stream; wait=False leaves that wait out, for a call that orders the streams itself.  torch is imported
    only where a tensor is involved."""
    if isinstance(out, tuple):
        return out, out[0], out[1]
    torch = import_torch()
    dtype = getattr(desc, "dtype", None)                 # (None: a p264hip_export_t, bytes)
    want = {DTYPE_F16: torch.float16, DTYPE_F32: torch.float32}.get(dtype, torch.uint8)
    if out is None:
        W, H = desc.width, desc.height
        shape = (n, H * 3 // 2, W) if desc.format in (FMT_I420, FMT_NV12) else (n, H, W, 3) if desc.format == FMT_RGB24 else (n, 3, H, W)
        if not pitch and not frame_stride:
            out = torch.empty(shape, dtype=want, device="cuda")
        else:
            out = torch.empty((n, desc.frame_stride or per), dtype=torch.uint8, device="cuda")
    if check is not None:
        error, name = check
        if not (out.is_cuda and out.is_contiguous() and (out.element_size() == 1 if dtype is None else out.dtype in (want, torch.uint8))):
            raise error("%s: out must be a contiguous %s tensor on the device" % (name, "uint8" if dtype is None else "%s (or uint8)" % want))
        if wait:
            torch.cuda.current_stream(out.device).synchronize()
    return out, out.data_ptr(), out.numel() * out.element_size()


def letterbox(w, h, W, H):
    """(dst_left, dst_top, dst_width, dst_height): the centred even rectangle of a W x H output that a w x h window fills at its own
    aspect ratio - one side the output's, the other the nearest even number to the exact ratio, at least 2.  Integers only.
    1920 x 1080 into 640 x 640 gives (0, 140, 640, 360)."""
    w, h, W, H = int(w), int(h), int(W), int(H)
    if min(w, h) < 1 or min(W, H) < 2:
        raise ValueError("letterbox: a window of %d x %d into %d x %d" % (w, h, W, H))
    if w * H >= h * W:
        dw, dh = W, min(max(2 * ((h * W + w) // (2 * w)), 2), H)
    else:
        dw, dh = min(max(2 * ((w * H + h) // (2 * h)), 2), W), H
    return 2 * ((W - dw) // 4), 2 * ((H - dh) // 4), dw, dh


def import_torch():
    """torch, for the calls that hand frames to it (HipReconstructor.export_frames, Pipeline.export_last / set_sink).  A process must
    hold ONE HIP runtime: a torch wheel brings its own libamdhip64.so, which libp264amd.so shares when torch was imported before
    the library was loaded - the other way round the process ends up with two runtimes and the second sees no device."""
    import torch
    paths = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                name = line.rstrip("\n").rsplit(None, 1)[-1]
                if os.path.basename(name).startswith("libamdhip64.so"):
                    paths.add(os.path.realpath(name))
    except OSError:
        pass
    if len(paths) > 1:
        raise RuntimeError("two HIP runtimes in this process (%s): import torch before p264decoder_amd loads libp264amd.so" % ", ".join(sorted(paths)))
    return torch


_lib = None


def load(path=None):
    """Load libp264amd.so and declare prototypes.  Raises OSError if it is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    lib = C.CDLL(path or os.environ.get("P264AMD_LIB") or LIB_PATH)
    u8p, i64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int64)
    # ---- p264parse.h
    lib.p264parse_open.restype = C.c_void_p
    lib.p264parse_open.argtypes = [C.c_int]
    lib.p264parse_close.argtypes = [C.c_void_p]
    lib.p264parse_nal.restype = C.c_int
    lib.p264parse_nal.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.POINTER(Picture))]
    for f in ("p264parse_mb_width", "p264parse_mb_height", "p264parse_slots", "p264parse_generation"):
        getattr(lib, f).restype = C.c_int
        getattr(lib, f).argtypes = [C.c_void_p]
    ip = C.POINTER(C.c_int)
    if hasattr(lib, "p264parse_crop"):
        lib.p264parse_crop.restype = C.c_int
        lib.p264parse_crop.argtypes = [C.c_void_p, ip, ip, ip, ip]
    if hasattr(lib, "p264parse_set_output_order"):
        lib.p264parse_set_output_order.restype = C.c_int
        lib.p264parse_set_output_order.argtypes = [C.c_void_p, C.c_int, C.c_int]
        for f in ("p264parse_outputs", "p264parse_flush"):
            getattr(lib, f).restype = C.c_int
            getattr(lib, f).argtypes = [C.c_void_p, C.POINTER(ParseOutput), C.c_int]
        lib.p264parse_kat_output_order.restype = C.c_int
        lib.p264parse_kat_output_order.argtypes = [C.c_int, C.c_int, ip, ip, ip, ip]
    lib.p264_annexb_next.restype = C.c_int
    lib.p264_annexb_next.argtypes = [C.c_void_p, C.c_int64, i64p, i64p, i64p]
    # ---- p264hip.h
    if hasattr(lib, "p264hip_create"):
        lib.p264hip_create.restype = C.c_int
        lib.p264hip_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.p264hip_destroy.argtypes = [C.c_void_p]
        lib.p264hip_last_error.restype = C.c_char_p
        lib.p264hip_device_count.restype = C.c_int
        lib.p264hip_upload.restype = C.c_int
        lib.p264hip_upload.argtypes = [C.c_void_p, C.c_int, C.POINTER(Picture), C.c_int]
        lib.p264hip_clone_picture.restype = C.c_int
        lib.p264hip_clone_picture.argtypes = [C.c_void_p, C.c_int, C.c_int]
        lib.p264hip_reconstruct.restype = C.c_int
        lib.p264hip_reconstruct.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
        lib.p264hip_submit.restype = C.c_int
        lib.p264hip_submit.argtypes = [C.c_void_p, C.c_int, C.POINTER(Picture)]
        lib.p264hip_sync.restype = C.c_int
        lib.p264hip_sync.argtypes = [C.c_void_p]
        lib.p264hip_read_frame.restype = C.c_int
        lib.p264hip_read_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        lib.p264hip_write_frame.restype = C.c_int
        lib.p264hip_write_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        lib.p264hip_timing_enable.restype = C.c_int
        lib.p264hip_timing_enable.argtypes = [C.c_void_p, C.c_int]
        lib.p264hip_timing_read.restype = C.c_int
        lib.p264hip_timing_read.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        lib.p264hip_timing_reset.restype = C.c_int
        lib.p264hip_timing_reset.argtypes = [C.c_void_p]
        lib.p264hip_last_launch.restype = C.c_int
        lib.p264hip_last_launch.argtypes = [C.c_void_p, C.POINTER(LaunchInfo)]
        lib.p264hip_build_info.restype = C.c_int
        lib.p264hip_build_info.argtypes = []
        lib.p264hip_upload_copies.restype = C.c_int64
        lib.p264hip_upload_copies.argtypes = [C.c_void_p]
        lib.p264hip_upload_async.restype = C.c_int
        lib.p264hip_upload_async.argtypes = [C.c_void_p, C.c_int, C.POINTER(Picture)]
        lib.p264hip_host_alloc.restype = C.c_void_p
        lib.p264hip_host_alloc.argtypes = [C.c_size_t]
        lib.p264hip_host_free.argtypes = [C.c_void_p]
        lib.p264hip_marker.restype = C.c_int
        lib.p264hip_input_layout.argtypes = [C.POINTER(Picture), C.POINTER(InputLayout)]
        lib.p264hip_compact_bound.restype = C.c_size_t
        lib.p264hip_compact_bound.argtypes = [C.POINTER(Picture)]
        lib.p264hip_pack_compact.restype = C.c_int64
        lib.p264hip_pack_compact.argtypes = [C.POINTER(Picture), C.c_void_p, C.c_size_t]
        lib.p264hip_expand_compact.restype = C.c_int
        lib.p264hip_expand_compact.argtypes = [C.POINTER(Picture), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        lib.p264hip_compact_header_ok.restype = C.c_int
        lib.p264hip_compact_header_ok.argtypes = [C.POINTER(Picture), C.c_void_p, C.c_size_t]
        lib.p264hip_compact_check.restype = C.c_int
        lib.p264hip_compact_check.argtypes = [C.POINTER(Picture), C.c_void_p, C.c_size_t]
        lib.p264hip_upload_compact.restype = C.c_int
        lib.p264hip_upload_compact.argtypes = [C.c_void_p, C.c_int, C.POINTER(Picture), C.c_void_p, C.c_size_t]
        lib.p264hip_pack_input.restype = C.c_int64
        lib.p264hip_pack_input.argtypes = [C.POINTER(Picture), C.c_void_p, C.c_size_t]
        lib.p264hip_unpack_input.argtypes = [C.POINTER(Picture), C.c_void_p, C.c_size_t, C.POINTER(Picture)]
        lib.p264hip_upload_packed.argtypes = [C.c_void_p, C.c_int, C.POINTER(Picture), C.c_void_p, C.c_size_t]
        lib.p264hip_records_check.restype = C.c_int64
        lib.p264hip_records_check.argtypes = [C.POINTER(MbInfo), C.c_size_t, C.c_uint32]
        lib.p264hip_records_check_pic.restype = C.c_int64
        lib.p264hip_records_check_pic.argtypes = [C.POINTER(Picture), C.POINTER(MbInfo)]
        lib.p264hip_input_reserve.argtypes = [C.c_void_p, C.c_int, C.POINTER(Picture), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        lib.p264hip_input_commit.argtypes = [C.c_void_p, C.c_int]
        lib.p264hip_frame_planar_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        lib.p264hip_copy_to_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.p264hip_copy_from_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.p264hip_marker.argtypes = [C.c_void_p]
        lib.p264hip_marker_wait.restype = C.c_int
        lib.p264hip_marker_wait.argtypes = [C.c_void_p, C.c_int]
    if hasattr(lib, "p264hip_export_frames"):
        lib.p264hip_export_frame_bytes.restype = C.c_int64
        lib.p264hip_export_frame_bytes.argtypes = [C.POINTER(Export)]
        lib.p264hip_export_check.restype = C.c_int
        lib.p264hip_export_check.argtypes = [C.POINTER(Export), C.c_int, C.c_int]
        lib.p264hip_export_frames.restype = C.c_int
        lib.p264hip_export_frames.argtypes = [C.c_void_p, ip, ip, C.c_int, C.POINTER(Export), C.c_void_p, C.c_size_t]
    if hasattr(lib, "p264hip_export_resized"):
        lib.p264hip_resize_frame_bytes.restype = C.c_int64
        lib.p264hip_resize_frame_bytes.argtypes = [C.POINTER(Resize)]
        lib.p264hip_resize_check.restype = C.c_int
        lib.p264hip_resize_check.argtypes = [C.POINTER(Resize), C.c_int, C.c_int]
        lib.p264hip_resize_taps.restype = C.c_int
        lib.p264hip_resize_taps.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int32)]
        if hasattr(lib, "p264hip_resize_aa_taps"):
            lib.p264hip_resize_aa_taps.restype = C.c_int
            lib.p264hip_resize_aa_taps.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint16)]
        lib.p264hip_export_resized.restype = C.c_int
        lib.p264hip_export_resized.argtypes = [C.c_void_p, ip, ip, C.c_int, C.POINTER(Resize), C.c_void_p, C.c_size_t]
    # ---- p264pipe.h
    if hasattr(lib, "p264pipe_open"):
        lib.p264pipe_open.restype = C.c_void_p
        lib.p264pipe_open.argtypes = [C.c_int, C.c_int, C.c_int]
        lib.p264pipe_set_input.restype = C.c_int
        lib.p264pipe_set_input.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
        lib.p264pipe_run.restype = C.c_int
        lib.p264pipe_run.argtypes = [C.c_void_p, C.c_int, C.POINTER(PipeStats)]
        lib.p264pipe_frame_size.restype = C.c_int
        lib.p264pipe_frame_size.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.p264pipe_read_frame.restype = C.c_int
        lib.p264pipe_read_frame.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        lib.p264pipe_stream_pictures.restype = C.c_int64
        lib.p264pipe_stream_pictures.argtypes = [C.c_void_p, C.c_int]
        lib.p264pipe_close.argtypes = [C.c_void_p]
    if hasattr(lib, "p264pipe_set_sink"):
        lib.p264pipe_crop.restype = C.c_int
        lib.p264pipe_crop.argtypes = [C.c_void_p, ip, ip, ip, ip]
        lib.p264pipe_export_last.restype = C.c_int
        lib.p264pipe_export_last.argtypes = [C.c_void_p, C.POINTER(Export), C.c_void_p, C.c_size_t]
        lib.p264pipe_set_sink.restype = C.c_int
        lib.p264pipe_set_sink.argtypes = [C.c_void_p, C.POINTER(Export), C.POINTER(C.c_void_p), C.c_int, C.c_size_t, SINK_FN, C.c_void_p]
    if hasattr(lib, "p264hip_export_rois"):
        lib.p264hip_rois_frame_bytes.restype = C.c_int64
        lib.p264hip_rois_frame_bytes.argtypes = [C.POINTER(Resize)]
        lib.p264hip_rois_check.restype = C.c_int
        lib.p264hip_rois_check.argtypes = [C.POINTER(Roi), C.c_int, C.POINTER(Resize), C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.p264hip_export_rois.restype = C.c_int
        lib.p264hip_export_rois.argtypes = [C.c_void_p, C.POINTER(Roi), C.c_int, C.POINTER(Resize), C.c_uint32, C.c_void_p, C.c_size_t]
    if hasattr(lib, "p264hip_export_rois_aa"):
        lib.p264hip_rois_aa_frame_bytes.restype = C.c_int64
        lib.p264hip_rois_aa_frame_bytes.argtypes = lib.p264hip_rois_frame_bytes.argtypes
        lib.p264hip_rois_aa_check.restype = C.c_int
        lib.p264hip_rois_aa_check.argtypes = lib.p264hip_rois_check.argtypes
        lib.p264hip_export_rois_aa.restype = C.c_int
        lib.p264hip_export_rois_aa.argtypes = lib.p264hip_export_rois.argtypes
        lib.p264hip_roi_aa_segment_words.restype = C.c_int
        lib.p264hip_roi_aa_segment_words.argtypes = [C.POINTER(Roi), C.POINTER(Resize)]
        lib.p264hip_roi_aa_segment.restype = C.c_int
        lib.p264hip_roi_aa_segment.argtypes = [C.POINTER(Roi), C.POINTER(Resize), C.POINTER(C.c_uint32)]
        lib.p264hip_roi_aa_tile_width.restype = C.c_int
        lib.p264hip_roi_aa_tile_width.argtypes = [C.POINTER(Roi), C.POINTER(Resize), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    if hasattr(lib, "p264hip_export_rois_device"):
        lib.p264hip_roi_status.restype = C.c_int
        lib.p264hip_roi_status.argtypes = [C.POINTER(Roi), C.POINTER(Resize), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.p264hip_rois_device_plan.restype = C.c_int
        lib.p264hip_rois_device_plan.argtypes = [C.POINTER(Resize), C.c_int, C.POINTER(RoisPlan)]
        lib.p264hip_rois_device_check.restype = C.c_int
        lib.p264hip_rois_device_check.argtypes = [C.POINTER(RoisDev), C.POINTER(Resize), C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.p264hip_export_rois_device.restype = C.c_int
        lib.p264hip_export_rois_device.argtypes = [C.c_void_p, C.POINTER(RoisDev), C.POINTER(Resize), C.c_uint32, C.c_void_p, C.c_size_t]
    if hasattr(lib, "p264pipe_export_last_rois_device"):
        lib.p264pipe_export_last_rois_device.restype = C.c_int
        lib.p264pipe_export_last_rois_device.argtypes = [C.c_void_p, C.POINTER(RoisDev), C.POINTER(Resize), C.c_uint32, C.c_void_p, C.c_size_t]
    if hasattr(lib, "p264pipe_export_last_rois"):
        lib.p264pipe_export_last_rois.restype = C.c_int
        lib.p264pipe_export_last_rois.argtypes = [C.c_void_p, C.POINTER(Roi), C.c_int, C.POINTER(Resize), C.c_uint32, C.c_void_p, C.c_size_t]
    if hasattr(lib, "p264pipe_set_sink_resized"):
        lib.p264pipe_export_last_resized.restype = C.c_int
        lib.p264pipe_export_last_resized.argtypes = [C.c_void_p, C.POINTER(Resize), C.c_void_p, C.c_size_t]
        lib.p264pipe_set_sink_resized.restype = C.c_int
        lib.p264pipe_set_sink_resized.argtypes = [C.c_void_p, C.POINTER(Resize), C.POINTER(C.c_void_p), C.c_int, C.c_size_t, SINK_FN, C.c_void_p]
    if hasattr(lib, "p264pipe_set_output_order"):
        lib.p264pipe_set_output_order.restype = C.c_int
        lib.p264pipe_set_output_order.argtypes = [C.c_void_p, C.c_int, C.c_int]
        lib.p264pipe_delivery.restype = C.POINTER(PipeOutput)
        lib.p264pipe_delivery.argtypes = [C.c_void_p, ip]
    if path is None:
        _lib = lib
    return lib


def split_annexb(lib, data):
    """Yield (nal_type, nal_ref_idc, rbsp bytes) for every NAL unit of an Annex-B byte string,
    applying the reference's emulation-prevention strip (core/core.c:310-336, incl. quirk A-Q10)."""
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    pos, off, ln = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    while lib.p264_annexb_next(buf, len(data), C.byref(pos), C.byref(off), C.byref(ln)):
        if ln.value < 1:
            continue
        nal = data[off.value:off.value + ln.value]
        hdr = nal[0]
        yield hdr & 0x1F, (hdr >> 5) & 3, strip_emulation(nal)


def strip_emulation(nal):
    """Payload after the NAL header byte with 00 00 03 -> 00 00, except when the 03 is within the
    last three bytes (the reference's loop bound, core/core.c:323)."""
    src = nal
    n = len(src)
    out = bytearray()
    i = 1
    while i < n:
        if i < n - 3 and src[i] == 0 and src[i + 1] == 0 and src[i + 2] == 3:
            out += b"\x00\x00"
            i += 3
            continue
        out.append(src[i])
        i += 1
    return bytes(out)
