"""Multi-stream decode pipeline (include/p264pipe.h): threaded host parse feeding batched MI355X reconstruction."""
import ctypes as C

import numpy as np

from . import _native as N


class Pipeline:
    """N Annex-B streams decoded side by side.  device=-1 runs the parsers only (no GPU)."""

    def __init__(self, streams, threads=8, device=0, lib=None):
        self.lib = lib or N.load()
        self._bufs = [(C.c_uint8 * len(s)).from_buffer_copy(s) for s in streams]      # borrowed by the C side
        self.h = self.lib.p264pipe_open(device, len(streams), threads)
        if not self.h:
            raise RuntimeError("p264pipe_open failed (no HIP device? the reconstruction has no CPU fallback; device=-1 parses only)")
        self._sink, self._sink_error = None, None
        self.device = device
        for i, b in enumerate(self._bufs):
            if self.lib.p264pipe_set_input(self.h, i, b, len(b)):
                raise RuntimeError("p264pipe_set_input(%d) failed" % i)

    def run(self, max_pictures=0):
        st = N.PipeStats()
        self._sink_error = None
        rc = self.lib.p264pipe_run(self.h, max_pictures, C.byref(st))
        if self._sink_error is not None:
            raise self._sink_error
        if rc:
            raise RuntimeError("p264pipe_run failed")
        return {f: getattr(st, f) for f, _ in st._fields_}

    def set_output_order(self, depth=None):
        """Deliver pictures in display order (p264pipe_set_output_order; before the first run()): the sink's callback then gets
        deliveries of the pictures that became due instead of rounds, and delivery() says which they are.  depth None: every
        stream's own reorder depth; 0 .. 16 overrides it (0: decode order, one picture per picture)."""
        if self.lib.p264pipe_set_output_order(self.h, 1, -1 if depth is None else int(depth)):
            raise RuntimeError("p264pipe_set_output_order refused (after run(), or a depth above 16)")

    def delivery(self):
        """Inside a sink's callback with output order on: [(stream, poc, decode_index, idr)] of the delivery's pictures."""
        n = C.c_int()
        d = self.lib.p264pipe_delivery(self.h, C.byref(n))
        return [(d[i].stream, d[i].poc, d[i].decode_index, bool(d[i].flags & N.OUT_IDR)) for i in range(n.value)]

    def pictures(self, stream):
        return self.lib.p264pipe_stream_pictures(self.h, stream)

    def read_frame(self, stream):
        w, h = C.c_int(), C.c_int()
        if self.lib.p264pipe_frame_size(self.h, C.byref(w), C.byref(h)):
            raise RuntimeError("no picture decoded yet")
        y = np.empty((h.value, w.value), np.uint8); u = np.empty((h.value // 2, w.value // 2), np.uint8); v = np.empty_like(u)
        if self.lib.p264pipe_read_frame(self.h, stream, y.ctypes.data, w.value, u.ctypes.data, v.ctypes.data, w.value // 2):
            raise RuntimeError("p264pipe_read_frame(%d) failed" % stream)
        return y, u, v

    def crop(self):
        """(left, top, width, height): the display window of stream 0's SPS (p264pipe_crop); None before its first slice is parsed."""
        v = [C.c_int() for _ in range(4)]
        if self.lib.p264pipe_crop(self.h, *[C.byref(x) for x in v]):
            return None
        return tuple(x.value for x in v)

    def _window(self, crop):
        """crop, or the display window: the pipeline's once it has parsed a slice, else read from stream 0's headers here"""
        if crop is None:
            crop = self.crop()
        if crop is None:
            from .recon import Parser
            ps = Parser(lib=self.lib)
            try:
                ps.parse_stream(bytes(self._bufs[0]), limit=1)
                crop = ps.crop
            finally:
                ps.close()
        if crop is None:
            raise RuntimeError("stream 0 has no picture: no display window")
        return crop

    def _sink_fn(self, callback, per):
        """the C callback of a sink: callback(round, streams, dev, per), whose exception run() raises"""
        def trampoline(user, rnd, k, streams, dev):
            try:                                          # (an exception cannot cross the C frames: run() raises it)
                if self._sink_error is None:
                    callback(rnd, [streams[i] for i in range(k)], dev, per)
            except BaseException as exc:
                self._sink_error = exc
        return N.SINK_FN(trampoline)

    def export_last(self, fmt="i420", crop=None, matrix="bt601", full_range=False, pitch=0, out=None):
        """The last picture of every stream in device memory, stream i first to last (p264pipe_export_last); `out` and the result as
        HipReconstructor.export_frames has them."""
        n = len(self._bufs)
        crop = self._window(crop)
        e = N.export_desc(fmt, crop, None, matrix, full_range, pitch)
        per = self.lib.p264hip_export_frame_bytes(C.byref(e))
        if per < 0:
            raise RuntimeError("export_last: p264hip_export_frame_bytes refuses the description")
        out, ptr, cap = N.export_out(n, e, per, pitch, 0, out)
        if self.lib.p264pipe_export_last(self.h, C.byref(e), ptr, cap):
            raise RuntimeError("p264pipe_export_last failed: %s" % self.lib.p264hip_last_error().decode())
        return out

    def set_sink(self, fmt, callback, depth=2, crop=None, matrix="bt601", full_range=False, pitch=0, buffers=None):
        """callback(round, streams, dev, bytes) for every round of run(): `streams` lists the round's streams, picture k of the round
        lies at dev + k * bytes in device memory, in format `fmt`, cropped to `crop` (None: the display window of stream 0).  `depth`
        buffers take turns: one is written again `depth` rounds later.  Pictures arrive in decode order - after set_output_order() in
        display order: callback(delivery, streams, dev, bytes) for every delivery, `streams` may then name a stream several times and
        delivery() tells the pictures.  buffers: (pointer, bytes)
        pairs of the caller's device memory; None allocates torch tensors.  The wrapper keeps callback and buffers alive.
        On a pipeline without a device (device=-1) a sink is taken only after set_output_order(): nothing is exported, dev is None,
        and of `buffers` only the bytes count (how many pictures a delivery holds; None: one per stream)."""
        n = len(self._bufs)
        e = N.export_desc(fmt, self._window(crop), None, matrix, full_range, pitch)
        per = self.lib.p264hip_export_frame_bytes(C.byref(e))
        if per < 0:
            raise RuntimeError("set_sink: p264hip_export_frame_bytes refuses the description")
        keep = None
        if self.device < 0:                               # parsers only: no memory, the bytes alone say what a delivery holds
            cap = min(b[1] for b in buffers) if buffers else n * per
            buffers, ptrs = [], None
        elif buffers is None:
            torch = N.import_torch()
            keep = [torch.empty(n * per, dtype=torch.uint8, device="cuda") for _ in range(depth)]
            buffers = [(t.data_ptr(), t.numel()) for t in keep]
        if self.device >= 0:
            ptrs = (C.c_void_p * len(buffers))(*[b[0] for b in buffers])
            cap = min(b[1] for b in buffers)
        fn = self._sink_fn(callback, per)
        if self.lib.p264pipe_set_sink(self.h, C.byref(e), ptrs, len(buffers), cap, fn, None):
            raise RuntimeError("p264pipe_set_sink refused (a buffer too small for %d pictures of %d bytes?)" % (n, per))
        self._sink = (fn, keep, ptrs, callback)
        return per

    def export_last_resized(self, size, fmt="rgbp", dtype="u8", crop=None, scale=None, bias=None, matrix="bt601", full_range=False, pitch=0, out=None, *,
                            filter="bilinear"):
        """The last picture of every stream in device memory, the window `crop` (None: the display window) resized to size = (width,
        height) (p264pipe_export_last_resized); the arguments, `filter` among them, `out` and the result as HipReconstructor.export_resized has them."""
        n = len(self._bufs)
        r = N.resize_desc(fmt, size, self._window(crop), None, dtype, scale, bias, matrix, full_range, pitch, filter=filter)
        per = self.lib.p264hip_resize_frame_bytes(C.byref(r))
        if per < 0:
            raise RuntimeError("export_last_resized: p264hip_resize_frame_bytes refuses the description")
        out, ptr, cap = N.export_out(n, r, per, pitch, 0, out)
        if self.lib.p264pipe_export_last_resized(self.h, C.byref(r), ptr, cap):
            raise RuntimeError("p264pipe_export_last_resized failed: %s" % self.lib.p264hip_last_error().decode())
        return out

    def export_last_rois(self, rois, size, fmt="rgbp", dtype="u8", fill=(16, 128, 128), scale=None, bias=None, matrix="bt601", full_range=False,
                         pitch=0, frame_stride=0, out=None, *, filter="bilinear"):
        """Windows of the streams' last DECODED pictures, each resized into a rectangle of the size = (width, height) output with the
        constant `fill` round it (p264pipe_export_last_rois); complete on return.  rois: rows (stream, left, top, width, height) or
        the same with the rectangle (dst_left, dst_top, dst_width, dst_height) behind it, or an (n, 5 | 9) integer array; the other
        arguments, `out` and the result as HipReconstructor.export_rois has them; filter="bilinear_aa" is the antialiased filter
        (HipReconstructor.export_rois_aa: at most 32:1 per ROI).  It may be called from inside a sink's callback:
        with a decode-order sink the round's pictures are the last decoded ones - detect on the sink's buffer, crop here."""
        arr, n = N.roi_array(rois, head=1)
        r = N.resize_desc(fmt, size, (0, 0, 2, 2), None, dtype, scale, bias, matrix, full_range, pitch, frame_stride, filter)
        aa = r.filter == N.FILTER_BILINEAR_AA
        per = (self.lib.p264hip_rois_aa_frame_bytes if aa else self.lib.p264hip_rois_frame_bytes)(C.byref(r))
        if per < 0:
            raise RuntimeError("export_last_rois: %s refuses the description" % ("p264hip_rois_aa_frame_bytes" if aa else "p264hip_rois_frame_bytes"))
        out, ptr, cap = N.export_out(n, r, per, pitch, frame_stride, out)
        if self.lib.p264pipe_export_last_rois(self.h, arr, n, C.byref(r), N.fill_word(fill), ptr, cap):
            raise RuntimeError("p264pipe_export_last_rois failed: %s" % self.lib.p264hip_last_error().decode())
        return out

    def export_last_rois_device(self, rois, size, fmt="rgbp", dtype="u8", fill=(16, 128, 128), scale=None, bias=None, matrix="bt601", full_range=False,
                                pitch=0, frame_stride=0, out=None, *, count=None, status=False, filter="bilinear", max_reduction=0, stream="current"):
        """export_last_rois from an ROI list IN DEVICE MEMORY (p264pipe_export_last_rois_device): HipReconstructor.export_rois_device
        with (n, 9) rows (stream, left, top, width, height, dst_left, dst_top, dst_width, dst_height), the picture being the
        stream's last decoded one; a (pointer, n) pair names full p264hip_roi_t rows whose slot is -1.  A stream without a picture
        yet gives the status ROI_NO_PICTURE.  With an ordering stream the call is queued only (the tensors stay referenced until
        close() or the next call without one); without, it is complete on return.  Callable from inside a sink's callback."""
        from .recon import rois_device_call
        l, r, word, out, ptr, cap, keep, status = rois_device_call(self.lib, RuntimeError, rois, size, fmt, dtype, fill, scale, bias, matrix, full_range, pitch,
                                                                   frame_stride, out, count, status, filter, max_reduction, stream, head=1)
        self._rois_in_flight = (getattr(self, "_rois_in_flight", []) if l.flags else []) + [keep]
        if self.lib.p264pipe_export_last_rois_device(self.h, C.byref(l), C.byref(r), word, ptr, cap):
            raise RuntimeError("p264pipe_export_last_rois_device failed: %s" % self.lib.p264hip_last_error().decode())
        return out if status is None else (out, status)

    def set_sink_resized(self, size, callback, fmt="rgbp", dtype="u8", depth=2, crop=None, scale=None, bias=None, matrix="bt601", full_range=False,
                         pitch=0, buffers=None, *, filter="bilinear"):
        """set_sink with a resize on it (p264pipe_set_sink_resized): callback(round, streams, dev, bytes) for every round of run(),
        picture k of the round at dev + k * bytes, the window `crop` (None: the display window of stream 0) resized to size = (width,
        height), as `fmt` / `dtype` with scale, bias and `filter` as HipReconstructor.export_resized has them.  It replaces a sink set before.
        After set_output_order() the callback gets deliveries in display order, as set_sink's does."""
        n = len(self._bufs)
        r = N.resize_desc(fmt, size, self._window(crop), None, dtype, scale, bias, matrix, full_range, pitch, filter=filter)
        per = self.lib.p264hip_resize_frame_bytes(C.byref(r))
        if per < 0:
            raise RuntimeError("set_sink_resized: p264hip_resize_frame_bytes refuses the description")
        keep = None
        if buffers is None:
            torch = N.import_torch()
            keep = [torch.empty(n * per, dtype=torch.uint8, device="cuda") for _ in range(depth)]
            buffers = [(t.data_ptr(), t.numel()) for t in keep]
        ptrs = (C.c_void_p * len(buffers))(*[b[0] for b in buffers])
        cap = min(b[1] for b in buffers)
        fn = self._sink_fn(callback, per)
        if self.lib.p264pipe_set_sink_resized(self.h, C.byref(r), ptrs, len(buffers), cap, fn, None):
            raise RuntimeError("p264pipe_set_sink_resized refused (a buffer too small for %d pictures of %d bytes?)" % (n, per))
        self._sink = (fn, keep, ptrs, callback)
        return per

    def close(self):
        if self.h:
            self.lib.p264pipe_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
