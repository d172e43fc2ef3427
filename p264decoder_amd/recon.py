"""Python mirrors of the two C-ABI layers: the host bitstream parser (p264parse_*) and the
MI355X reconstruction context (p264hip_*).  Thin ctypes plumbing - every pixel is produced by
the HIP kernels in libp264amd.so; nothing here computes."""
import ctypes as C

import numpy as np

from . import _native as N


class P264Error(RuntimeError):
    pass


class ParsedPicture:
    """An owned copy of one p264hip_picture_t (the parser reuses its buffers)."""

    def __init__(self, desc):
        n = desc.mb_w * desc.mb_h
        self.mb = np.ctypeslib.as_array(C.cast(desc.mb, C.POINTER(C.c_uint8)), (n * 16,)).copy()
        self.mv = np.ctypeslib.as_array(desc.mv, (n * 32,)).copy()
        self.ref_idx = np.ctypeslib.as_array(desc.ref_idx, (n * 4,)).copy()
        self.i4modes = np.ctypeslib.as_array(desc.i4modes, (n * 16,)).copy()
        nc = int(desc.n_coef_blocks)
        self.coefs = np.ctypeslib.as_array(desc.coefs, (nc * 16,)).copy() if nc else np.zeros(16, np.int16)
        d = N.Picture()
        C.memmove(C.byref(d), C.byref(desc), C.sizeof(N.Picture))
        if desc.slice_type == N.SLICE_B:                # list-1 arrays of a B picture
            self.mv_l1 = np.ctypeslib.as_array(desc.mv_l1, (n * 32,)).copy()
            self.ref_idx_l1 = np.ctypeslib.as_array(desc.ref_idx_l1, (n * 4,)).copy()
            d.mv_l1 = C.cast(self.mv_l1.ctypes.data, C.POINTER(C.c_int16))
            d.ref_idx_l1 = C.cast(self.ref_idx_l1.ctypes.data, C.POINTER(C.c_int8))
        else:
            d.mv_l1 = C.POINTER(C.c_int16)()
            d.ref_idx_l1 = C.POINTER(C.c_int8)()
        d.mb = C.cast(self.mb.ctypes.data, C.POINTER(N.MbInfo))
        d.mv = C.cast(self.mv.ctypes.data, C.POINTER(C.c_int16))
        d.ref_idx = C.cast(self.ref_idx.ctypes.data, C.POINTER(C.c_int8))
        d.i4modes = C.cast(self.i4modes.ctypes.data, C.POINTER(C.c_uint8))
        d.coefs = C.cast(self.coefs.ctypes.data, C.POINTER(C.c_int16))
        self.desc = d

    # convenience views -------------------------------------------------------------------
    @property
    def mb_w(self):
        return self.desc.mb_w

    @property
    def mb_h(self):
        return self.desc.mb_h

    @property
    def n_mb(self):
        return self.desc.mb_w * self.desc.mb_h

    def mb_records(self):
        dt = np.dtype([("mb_type", "u1"), ("qp", "u1"), ("cbp", "u1"), ("intra_modes", "u1"),
                       ("coef_mask", "<u4"), ("coef_index", "<u4"), ("avail", "u1"), ("edges", "u1"), ("flags", "<u2")])
        return self.mb.view(dt)

    def ipcm_macroblocks(self):
        """The picture's I_PCM macroblocks: a list of (macroblock index, its 384 sample bytes: 256 luma, 64 Cb, 64 Cr) -
        the twelve blocks of coefs[] at the record's coef_index (include/p264hip.h)."""
        raw = self.coefs.view(np.uint8)
        r = self.mb_records()
        return [(int(i), raw[int(r["coef_index"][i]) * 32:int(r["coef_index"][i]) * 32 + 384].copy())
                for i in np.flatnonzero(r["mb_type"] == N.MB_IPCM)]


class Parser:
    """p264parse_* : NAL units in, complete parsed pictures out (CPU, serial by nature)."""

    def __init__(self, quiet=True, strict=False, lib=None, intra8x8=False, scaling=False, cr_offset=False):
        """intra8x8: hand out Intra 8x8 macroblocks as I4x4 records with MB_I8X8 (P264PARSE_OPT_INTRA8X8) - for pictures that go to
        a backend that knows the record, as HipReconstructor does; off, such a macroblock ends its slice with an error.
        scaling: read the scaling matrices of High-profile parameter sets and hand out each picture's eight lists in its descriptor
        (P264PARSE_OPT_SCALING) - for a backend that reads the table, as HipReconstructor does; off, such a set is refused.
        cr_offset: accept a High-profile PPS whose second_chroma_qp_index_offset differs from chroma_qp_index_offset and hand out the
        difference as the descriptor's cr_qp_offset_delta (P264PARSE_OPT_CR_OFFSET) - for a backend that reads the delta, as
        HipReconstructor does; off, the slices of such a PPS are refused"""
        self.lib = lib or N.load()
        self.h = self.lib.p264parse_open((1 if quiet else 0) | (2 if strict else 0) | (4 if intra8x8 else 0) | (8 if scaling else 0) | (16 if cr_offset else 0))
        if not self.h:
            raise P264Error("p264parse_open failed")

    def close(self):
        if self.h:
            self.lib.p264parse_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def feed(self, nal_type, ref_idc, rbsp):
        """Returns a ParsedPicture when this NAL completed a picture, else None."""
        pic = C.POINTER(N.Picture)()
        buf = (C.c_uint8 * max(len(rbsp), 1)).from_buffer_copy(rbsp if len(rbsp) else b"\0")
        rc = self.lib.p264parse_nal(self.h, nal_type, ref_idc, buf, len(rbsp), C.byref(pic))
        if rc < 0:
            raise P264Error("p264parse_nal failed on NAL type %d" % nal_type)
        return ParsedPicture(pic.contents) if rc == 1 else None

    @property
    def slots(self):
        return self.lib.p264parse_slots(self.h)

    def set_output_order(self, depth=None):
        """Switch the output process on (p264parse_set_output_order; before the first slice): pictures keep their slots until they
        are due for display, slots becomes D + 1.  depth None: the stream's reorder depth; 0 .. 16 overrides it (0: decode order)."""
        if self.lib.p264parse_set_output_order(self.h, 1, -1 if depth is None else int(depth)):
            raise P264Error("p264parse_set_output_order refused (after the first slice, or a depth above 16)")

    def _outputs(self, call):
        out = (N.ParseOutput * N.MAX_OUTPUTS)()
        n = call(self.h, out, N.MAX_OUTPUTS)
        return [(o.slot, o.poc, o.decode_index, bool(o.flags & N.OUT_IDR)) for o in out[:n]]

    def outputs(self):
        """[(slot, poc, decode_index, idr)]: the pictures that became due with the picture feed() just returned, in output order"""
        return self._outputs(self.lib.p264parse_outputs)

    def flush(self):
        """[(slot, poc, decode_index, idr)]: every picture that still waits, ascending by order count (the end of a stream)"""
        return self._outputs(self.lib.p264parse_flush)

    @property
    def crop(self):
        """(left, top, width, height) of the active SPS's display window in luma samples (p264parse_crop); None before the first slice."""
        v = [C.c_int() for _ in range(4)]
        if self.lib.p264parse_crop(self.h, *[C.byref(x) for x in v]):
            return None
        return tuple(x.value for x in v)

    def parse_stream(self, data, limit=None):
        """All pictures of an Annex-B byte string."""
        out = []
        for typ, idc, rbsp in N.split_annexb(self.lib, data):
            p = self.feed(typ, idc, rbsp)
            if p is not None:
                out.append(p)
                if limit and len(out) >= limit:
                    break
        return out


class HipReconstructor:
    """p264hip_* : frame stores and resident picture inputs on one MI355X."""

    def __init__(self, mb_w, mb_h, n_streams=1, slots=2, max_pictures=1, device=0, lib=None):
        self.lib = lib or N.load()
        if not hasattr(self.lib, "p264hip_create"):
            raise P264Error("libp264amd.so was built without the HIP layer")
        self.mb_w, self.mb_h, self.n_streams, self.slots = mb_w, mb_h, n_streams, slots
        h = C.c_void_p()
        rc = self.lib.p264hip_create(C.byref(h), device, mb_w, mb_h, n_streams, slots, max_pictures)
        if rc != 0:
            raise P264Error("p264hip_create: %s" % self.lib.p264hip_last_error().decode())
        self.h = h
        # blocks given to upload_compact / upload_packed: their copies are asynchronous, so they stay referenced until sync()
        # or close() (a list, not one per slot: a second upload into a slot must not drop the first block while it travels)
        self._in_flight = []

    def _chk(self, rc, what):
        if rc != 0:
            raise P264Error("%s: %s" % (what, self.lib.p264hip_last_error().decode()))

    def close(self):
        if getattr(self, "h", None):
            self.lib.p264hip_destroy(self.h)
            self.h = None
            self._in_flight = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, first, pictures):
        arr = (N.Picture * len(pictures))(*[p.desc for p in pictures])
        self._chk(self.lib.p264hip_upload(self.h, first, arr, len(pictures)), "p264hip_upload")

    # ---- the packed form of a picture's arrays (p264hip_input_layout_t) and the roads into a slot that use it ----
    @staticmethod
    def pack(picture, lib=None):
        """The picture's arrays as one block in the layout of an input slot (numpy uint8; host side only)."""
        lib = lib or N.load()
        lay = N.InputLayout()
        if lib.p264hip_input_layout(C.byref(picture.desc), C.byref(lay)) != 0:
            raise P264Error("p264hip_input_layout failed")
        buf = np.zeros(lay.bytes, np.uint8)
        n = lib.p264hip_pack_input(C.byref(picture.desc), buf.ctypes.data, buf.size)
        if n != lay.bytes:
            raise P264Error("p264hip_pack_input: %d" % n)
        return buf

    @staticmethod
    def pack_compact(picture, lib=None):
        """The picture's arrays in the compact link format (include/p264hip.h: p264hip_compact_hdr_t); numpy uint8, host side only."""
        lib = lib or N.load()
        buf = np.zeros(lib.p264hip_compact_bound(C.byref(picture.desc)), np.uint8)
        n = lib.p264hip_pack_compact(C.byref(picture.desc), buf.ctypes.data, buf.size)
        if n < 0:
            raise P264Error("p264hip_pack_compact: %d" % n)
        return buf[:n].copy()

    @staticmethod
    def expand_compact(picture, compact, lib=None):
        """Host reference of the device expansion: the compact block back in the slot layout (what pack() gives, up to bytes no kernel reads)."""
        lib = lib or N.load()
        lay = N.InputLayout()
        if lib.p264hip_input_layout(C.byref(picture.desc), C.byref(lay)) != 0:
            raise P264Error("p264hip_input_layout failed")
        out = np.zeros(lay.bytes, np.uint8)
        rc = lib.p264hip_expand_compact(C.byref(picture.desc), compact.ctypes.data, compact.size, out.ctypes.data, out.size)
        if rc != 0:
            raise P264Error("p264hip_expand_compact: %d" % rc)
        return out

    def upload_compact(self, slot, picture, compact):
        self._in_flight.append(compact)
        self._chk(self.lib.p264hip_upload_compact(self.h, slot, C.byref(picture.desc), compact.ctypes.data, compact.size), "p264hip_upload_compact")

    def upload_packed(self, slot, picture, packed):
        self._in_flight.append(packed)
        self._chk(self.lib.p264hip_upload_packed(self.h, slot, C.byref(picture.desc), packed.ctypes.data, packed.size), "p264hip_upload_packed")

    def input_reserve(self, slot, picture):
        """(device address, bytes) of the block slot `slot` expects for this picture; fill it, then input_commit(slot)."""
        dev, n = C.c_void_p(), C.c_size_t()
        self._chk(self.lib.p264hip_input_reserve(self.h, slot, C.byref(picture.desc), C.byref(dev), C.byref(n)), "p264hip_input_reserve")
        return dev.value, n.value

    def input_commit(self, slot):
        self._chk(self.lib.p264hip_input_commit(self.h, slot), "p264hip_input_commit")

    def frame_planar_device(self, stream, slot, index=0):
        dev, n = C.c_void_p(), C.c_size_t()
        self._chk(self.lib.p264hip_frame_planar_device(self.h, stream, slot, index, C.byref(dev), C.byref(n)), "p264hip_frame_planar_device")
        return dev.value, n.value

    def export_frames(self, streams, slots, fmt="i420", crop=None, matrix="bt601", full_range=False, pitch=0, out=None, sync=True,
                      frame_stride=0):
        """Frames slots[i] of streams[i] into device memory, cropped to crop = (left, top, width, height) (None: the whole frame), as
        "i420" / "nv12" / "rgb24" / "rgbp" (p264hip_export_frames: one launch, queued behind every reconstruct before it).
        out: a torch uint8 tensor on the device (filled in place, from its first byte), a (device pointer, bytes) pair, or None -
        a new torch tensor (n, H*3//2, W) for I420 / NV12, (n, H, W, 3) for RGB24, (n, 3, H, W) for RGBP at the tight pitch, (n, bytes)
        otherwise.  Returns the tensor (the pair as given).  sync=False leaves the wait to sync() or a marker."""
        n = len(streams)
        e = N.export_desc(fmt, crop, (self.mb_w * 16, self.mb_h * 16), matrix, full_range, pitch, frame_stride)
        if len(slots) != n:
            raise P264Error("export_frames: %d streams, %d slots" % (n, len(slots)))
        per = self.lib.p264hip_export_frame_bytes(C.byref(e)) if out is None else 0      # (a given `out`: the call refuses what it cannot take)
        if per < 0:
            raise P264Error("export_frames: p264hip_export_frame_bytes refuses the description")
        out, ptr, cap = N.export_out(n, e, per, pitch, frame_stride, out, (P264Error, "export_frames"))
        a = (C.c_int * max(n, 1))(*streams)
        b = (C.c_int * max(n, 1))(*slots)
        self._chk(self.lib.p264hip_export_frames(self.h, a, b, n, C.byref(e), ptr, cap), "p264hip_export_frames")
        if sync:
            self.sync()
        return out

    def export_resized(self, streams, slots, size, fmt="rgbp", dtype="u8", crop=None, scale=None, bias=None, matrix="bt601", full_range=False,
                       pitch=0, frame_stride=0, out=None, sync=True, *, filter="bilinear"):
        """Frames slots[i] of streams[i] into device memory with the window crop = (left, top, width, height) (None: the whole frame)
        resized to size = (width, height) by the bilinear filter of include/p264hip.h (filter="bilinear_aa": its antialiased filter,
        the one for a reduction; at most 32:1), as "i420" / "nv12" / "rgb24" / "rgbp"; dtype
        "u8", or - "rgb24" / "rgbp" - "f16" / "f32": channel * scale + bias, scale and bias one number or three (R, G, B)
        (p264hip_export_resized: one launch, queued behind every reconstruct before it).
        out: a torch tensor of that dtype (or uint8) on the device (filled in place, from its first element), a (device pointer, bytes) pair, or
        None - a new torch tensor (n, H*3//2, W) for I420 / NV12, (n, H, W, 3) for RGB24, (n, 3, H, W) for RGBP at the tight layout,
        (n, bytes) uint8 otherwise.  Returns the tensor (the pair as given).  sync=False leaves the wait to sync() or a marker."""
        n = len(streams)
        r = N.resize_desc(fmt, size, crop, (self.mb_w * 16, self.mb_h * 16), dtype, scale, bias, matrix, full_range, pitch, frame_stride, filter)
        if len(slots) != n:
            raise P264Error("export_resized: %d streams, %d slots" % (n, len(slots)))
        per = self.lib.p264hip_resize_frame_bytes(C.byref(r)) if out is None else 0
        if per < 0:
            raise P264Error("export_resized: p264hip_resize_frame_bytes refuses the description")
        out, ptr, cap = N.export_out(n, r, per, pitch, frame_stride, out, (P264Error, "export_resized"))
        a = (C.c_int * max(n, 1))(*streams)
        b = (C.c_int * max(n, 1))(*slots)
        self._chk(self.lib.p264hip_export_resized(self.h, a, b, n, C.byref(r), ptr, cap), "p264hip_export_resized")
        if sync:
            self.sync()
        return out

    def export_rois(self, rois, size, fmt="rgbp", dtype="u8", fill=(16, 128, 128), scale=None, bias=None, matrix="bt601", full_range=False,
                    pitch=0, frame_stride=0, out=None, sync=True):
        """A window PER PICTURE, each resized by the bilinear filter into a rectangle of the size = (width, height) output and the
        constant fill = (Y, Cb, Cr) round it, in one call (p264hip_export_rois; include/p264hip.h has the contract).  rois: a sequence
        of rows, or an (n, 6 | 10) integer array: (stream, slot, left, top, width, height) - the window fills the whole output - or
        the same with the rectangle (dst_left, dst_top, dst_width, dst_height) behind it (_native.letterbox gives one that keeps the
        window's aspect ratio).  The other arguments, `out` and the result are those of export_resized, picture i being ROI i."""
        return self._export_rois(rois, size, fmt, dtype, fill, scale, bias, matrix, full_range, pitch, frame_stride, out, sync, "bilinear")

    def export_rois_aa(self, rois, size, fmt="rgbp", dtype="u8", fill=(16, 128, 128), scale=None, bias=None, matrix="bt601", full_range=False,
                       pitch=0, frame_stride=0, out=None, sync=True):
        """export_rois with the ANTIALIASED filter, the one for reductions - a 1920 x 1080 picture letterboxed into 640 x 640, a
        detector's boxes at 224 x 224 - (p264hip_export_rois_aa): every argument and the result as export_rois has them.  A window may
        be at most 32 times its rectangle in width and in height."""
        return self._export_rois(rois, size, fmt, dtype, fill, scale, bias, matrix, full_range, pitch, frame_stride, out, sync, "bilinear_aa")

    def _export_rois(self, rois, size, fmt, dtype, fill, scale, bias, matrix, full_range, pitch, frame_stride, out, sync, filter):
        arr, n = N.roi_array(rois)
        r = N.resize_desc(fmt, size, (0, 0, 2, 2), None, dtype, scale, bias, matrix, full_range, pitch, frame_stride, filter)
        word = N.fill_word(fill)
        aa = r.filter == N.FILTER_BILINEAR_AA                # (its own entry points; any other value is p264hip_export_rois' to refuse)
        per = (self.lib.p264hip_rois_aa_frame_bytes if aa else self.lib.p264hip_rois_frame_bytes)(C.byref(r)) if out is None else 0
        if per < 0:
            raise P264Error("export_rois: %s refuses the description" % ("p264hip_rois_aa_frame_bytes" if aa else "p264hip_rois_frame_bytes"))
        out, ptr, cap = N.export_out(n, r, per, pitch, frame_stride, out, (P264Error, "export_rois"))
        if aa:
            self._chk(self.lib.p264hip_export_rois_aa(self.h, arr, n, C.byref(r), word, ptr, cap), "p264hip_export_rois_aa")
        else:
            self._chk(self.lib.p264hip_export_rois(self.h, arr, n, C.byref(r), word, ptr, cap), "p264hip_export_rois")
        if sync:
            self.sync()
        return out

    def export_rois_device(self, rois, size, fmt="rgbp", dtype="u8", fill=(16, 128, 128), scale=None, bias=None, matrix="bt601", full_range=False,
                           pitch=0, frame_stride=0, out=None, *, count=None, status=False, filter="bilinear", max_reduction=0, stream="current",
                           sync=None):
        """export_rois / export_rois_aa (filter="bilinear_aa") from an ROI list IN DEVICE MEMORY - a detector's boxes, see
        rois.rois_from_boxes - (p264hip_export_rois_device; include/p264hip.h has the contract): the host sees no ROI, an invalid one
        refuses nothing and its picture is NOT WRITTEN.  rois: an (n, 10) contiguous int32 tensor on the device (the rows of
        p264hip_roi_t), or a (device pointer, n) pair.  count: None (all n), a one-element int32 device tensor or a pointer: the
        ROIs from it on are unused.  status: True allocates an (n,) int32 tensor and returns (out, status); a tensor or pointer
        is written and returned as given; False: no status.  max_reduction (antialiased filter): the largest reduction an ROI
        may have, 0 meaning 32 - the scratch a call reserves per ROI grows with it (_native.rois_device_plan).
        stream: "current" - the default where a tensor is involved - orders the call behind what torch's current stream has queued
        and torch's current stream behind the call: it behaves like a torch operation and never synchronises the host; None: no
        ordering; an integer: a raw stream handle to order with.  sync=None waits (sync()) only where there is no ordering.  The
        tensors stay referenced until the next sync().  The other arguments and `out` as export_rois has them."""
        l, r, word, out, ptr, cap, keep, status = rois_device_call(self.lib, P264Error, rois, size, fmt, dtype, fill, scale, bias, matrix, full_range, pitch,
                                                                   frame_stride, out, count, status, filter, max_reduction, stream)
        self._in_flight.append(keep)
        self._chk(self.lib.p264hip_export_rois_device(self.h, C.byref(l), C.byref(r), word, ptr, cap), "p264hip_export_rois_device")
        if sync if sync is not None else not l.flags:
            self.sync()
        return out if status is None else (out, status)

    def clone_picture(self, dst, src):
        self._chk(self.lib.p264hip_clone_picture(self.h, dst, src), "p264hip_clone_picture")

    def reconstruct(self, pic_ids, streams):
        n = len(pic_ids)
        a = (C.c_int * n)(*pic_ids)
        b = (C.c_int * n)(*streams)
        self._chk(self.lib.p264hip_reconstruct(self.h, a, b, n), "p264hip_reconstruct")

    def submit(self, stream, picture):
        self._chk(self.lib.p264hip_submit(self.h, stream, C.byref(picture.desc)), "p264hip_submit")

    def sync(self):
        self._chk(self.lib.p264hip_sync(self.h), "p264hip_sync")
        self._in_flight = []

    def read_frame(self, stream, slot):
        w, h = self.mb_w * 16, self.mb_h * 16
        y = np.empty((h, w), np.uint8)
        u = np.empty((h // 2, w // 2), np.uint8)
        v = np.empty((h // 2, w // 2), np.uint8)
        self._chk(self.lib.p264hip_read_frame(self.h, stream, slot, y.ctypes.data, w, u.ctypes.data, v.ctypes.data, w // 2), "p264hip_read_frame")
        return y, u, v

    def write_frame(self, stream, slot, y, u, v):
        w = self.mb_w * 16
        y, u, v = (np.ascontiguousarray(a, np.uint8) for a in (y, u, v))
        self._chk(self.lib.p264hip_write_frame(self.h, stream, slot, y.ctypes.data, w, u.ctypes.data, v.ctypes.data, w // 2), "p264hip_write_frame")

    def timing_enable(self, on=True):
        self._chk(self.lib.p264hip_timing_enable(self.h, 1 if on else 0), "p264hip_timing_enable")

    def timing_reset(self):
        self._chk(self.lib.p264hip_timing_reset(self.h), "p264hip_timing_reset")

    def timing_read(self):
        ms = (C.c_double * N.NKERNELS)()
        cnt = (C.c_int64 * N.NKERNELS)()
        self._chk(self.lib.p264hip_timing_read(self.h, ms, cnt), "p264hip_timing_read")
        names = ("inter", "intra", "deblock", "reconstruct")
        return {names[i]: (ms[i], cnt[i]) for i in range(N.NKERNELS)}


    def last_launch(self):
        """The launch shapes of the last reconstruct call (p264hip_launch_info_t as a dict; what depends on the batch's CONTENT
        rather than its size has its own accessor: last_t8x8_wgs, last_intra_i8, last_scaled_pictures, last_cr_pictures)."""
        li = N.LaunchInfo()
        self._chk(self.lib.p264hip_last_launch(self.h, C.byref(li)), "p264hip_last_launch")
        return {n: int(getattr(li, n)) for n, _ in N.LaunchInfo._fields_ if n not in ("reserved", "t8x8_wgs", "intra_i8", "scaled_pictures", "cr_pictures")}

    def last_t8x8_wgs(self):
        """Workgroups of k_t8x8 in the last reconstruct call: 0 unless a picture of the batch had transform_8x8."""
        li = N.LaunchInfo()
        self._chk(self.lib.p264hip_last_launch(self.h, C.byref(li)), "p264hip_last_launch")
        return int(li.t8x8_wgs)

    def last_intra_i8(self):
        """1 where the last reconstruct call ran the Intra 8x8 instances of the intra kernels (a picture of the batch had
        T8X8_INTRA in transform_8x8), else 0."""
        li = N.LaunchInfo()
        self._chk(self.lib.p264hip_last_launch(self.h, C.byref(li)), "p264hip_last_launch")
        return int(li.intra_i8)

    def last_scaled_pictures(self):
        """Pictures with scaling_lists or a non-zero cr_qp_offset_delta in the last reconstruct call; not 0: the batch ran the instances that read the scaling
        table (k_mc_sort_scaled / k_mc_sort_scaled_p, k_scaled_inter, k_intra_scaled / k_intra_sparse_scaled), 0: what a flat batch always ran."""
        li = N.LaunchInfo()
        self._chk(self.lib.p264hip_last_launch(self.h, C.byref(li)), "p264hip_last_launch")
        return int(li.scaled_pictures)

    def last_cr_pictures(self):
        """Pictures with a non-zero cr_qp_offset_delta in the last reconstruct call; not 0: the loop filter ran its Cr instances
        (k_deblock_bs_cr, k_deblock_cr), 0: what such a batch always ran."""
        li = N.LaunchInfo()
        self._chk(self.lib.p264hip_last_launch(self.h, C.byref(li)), "p264hip_last_launch")
        return int(li.cr_pictures)


def rois_device_call(lib, error, rois, size, fmt, dtype, fill, scale, bias, matrix, full_range, pitch, frame_stride, out, count, status, filter,
                     max_reduction, stream, head=2):
    """What HipReconstructor.export_rois_device and Pipeline.export_last_rois_device share: the arguments as (p264hip_rois_dev_t,
    p264hip_resize_t, fill word, out, its pointer, its bytes, the tensors to keep alive, the status tensor / pointer or None).
    head: the leading members of a row (2: stream, slot; 1: stream alone).  torch is imported only where a tensor is involved."""
    r = N.resize_desc(fmt, size, (0, 0, 2, 2), None, dtype, scale, bias, matrix, full_range, pitch, frame_stride, filter)
    keep = []

    def pointer(v, what, numel=None):
        if v is None or isinstance(v, int):
            return v
        torch = N.import_torch()
        if not (v.is_cuda and v.is_contiguous() and v.dtype == torch.int32 and (numel is None or v.numel() == numel)):
            raise error("export_rois_device: %s must be a contiguous int32 tensor on the device%s" % (what, "" if numel is None else " of %d elements" % numel))
        keep.append(v)
        return v.data_ptr()
    if isinstance(rois, tuple):
        rois_ptr, n = int(rois[0]), int(rois[1])
    else:
        if rois.dim() != 2 or rois.shape[1] != head + 8:
            raise error("export_rois_device: rois must be an (n, %d) tensor or a (pointer, n) pair" % (head + 8))
        if head == 1:                                        # (stream, window, rectangle) -> the rows of p264hip_roi_t with slot -1
            torch = N.import_torch()
            rois = torch.cat([rois[:, :1], torch.full_like(rois[:, :1], -1), rois[:, 1:]], dim=1).contiguous()
        n = int(rois.shape[0])
        rois_ptr = pointer(rois, "rois")
    count_ptr = pointer(count, "count", 1)
    if status is True:
        torch = N.import_torch()
        status = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    elif status is False:
        status = None
    status_ptr = pointer(status, "status", None if isinstance(status, int) else n)
    if stream == "current":                                  # (the default where a tensor is involved; pointers alone: no ordering)
        stream = N.import_torch().cuda.current_stream().cuda_stream if keep or not isinstance(out, tuple) else None
    aa = r.filter == N.FILTER_BILINEAR_AA
    per = (lib.p264hip_rois_aa_frame_bytes if aa else lib.p264hip_rois_frame_bytes)(C.byref(r)) if out is None else 0
    if per < 0:
        raise error("export_rois_device: %s refuses the description" % ("p264hip_rois_aa_frame_bytes" if aa else "p264hip_rois_frame_bytes"))
    out, ptr, cap = N.export_out(max(n, 1), r, per, pitch, frame_stride, out, (error, "export_rois_device"), wait=stream is None)
    if not isinstance(out, tuple):
        keep.append(out)
    l = N.RoisDev(rois_ptr, count_ptr, status_ptr, None, None, None, n, int(max_reduction), 0)
    if stream is not None:
        l.after_stream = l.before_stream = int(stream) or None
        l.flags = N.ROIS_AFTER | N.ROIS_BEFORE
    return l, r, N.fill_word(fill), out, ptr, cap, keep, status


def device_count(lib=None):
    lib = lib or N.load()
    return lib.p264hip_device_count() if hasattr(lib, "p264hip_device_count") else 0
