"""A detector's boxes as the ROI list p264hip_export_rois_device reads (include/p264hip.h: p264hip_roi_t), made where the boxes are:
torch operations only, on the device of `boxes`, nothing read back to the host - so that detector -> rois_from_boxes ->
HipReconstructor.export_rois_device -> second model stay on one torch stream without a host wait between them."""


def rois_from_boxes(boxes, streams, slots, frame_size, letterbox_to=None):
    """(n, 10) int32 rows (stream, slot, left, top, width, height, dst_left, dst_top, dst_width, dst_height) on the device of `boxes`.

    boxes: an (n, 4) tensor x1, y1, x2, y2 in luma samples, float or integer, the box being [x1, x2) x [y1, y2).  streams, slots:
    one integer for all boxes or an (n,) integer tensor each (slot -1: the stream's picture of the call's slot table).  frame_size =
    (width, height) of the frame, both even.

    The box is clamped into the frame and the window is the smallest even rectangle that holds what is left of it: at least 2 x 2.
    A box with a member that is not finite, and a box of which nothing is left - outside the frame, reversed, without samples -
    becomes the window (0, 0, 0, 0), which the device reports as P264HIP_ROI_WINDOW_EMPTY and whose picture is not written.  The
    rectangle is all 0, the whole output - or, with letterbox_to = (W, H) of the output, what _native.letterbox gives for the
    window, in integer tensor arithmetic."""
    import torch
    if boxes.dim() != 2 or boxes.shape[1] != 4:
        raise ValueError("rois_from_boxes: boxes must be an (n, 4) tensor")
    fw, fh = int(frame_size[0]), int(frame_size[1])
    if fw < 2 or fh < 2 or (fw | fh) & 1:
        raise ValueError("rois_from_boxes: a frame of %d x %d" % (fw, fh))
    n, dev = boxes.shape[0], boxes.device
    b = boxes.to(torch.float64)
    finite = torch.isfinite(b).all(dim=1)
    b = torch.nan_to_num(b, nan=0.0, posinf=0.0, neginf=0.0)
    x1, x2 = b[:, 0].clamp(0, fw), b[:, 2].clamp(0, fw)
    y1, y2 = b[:, 1].clamp(0, fh), b[:, 3].clamp(0, fh)
    keep = (finite & (x2 > x1) & (y2 > y1)).to(torch.int64)
    left, top = 2 * torch.floor(x1 / 2).to(torch.int64), 2 * torch.floor(y1 / 2).to(torch.int64)
    width, height = 2 * torch.ceil(x2 / 2).to(torch.int64) - left, 2 * torch.ceil(y2 / 2).to(torch.int64) - top
    out = torch.zeros((n, 10), dtype=torch.int64, device=dev)
    out[:, 0] = streams if isinstance(streams, int) else streams.to(device=dev, dtype=torch.int64)
    out[:, 1] = slots if isinstance(slots, int) else slots.to(device=dev, dtype=torch.int64)
    out[:, 2], out[:, 3], out[:, 4], out[:, 5] = left * keep, top * keep, width * keep, height * keep
    if letterbox_to is not None:
        W, H = int(letterbox_to[0]), int(letterbox_to[1])
        if W < 2 or H < 2:
            raise ValueError("rois_from_boxes: a letterbox in %d x %d" % (W, H))
        w, h = width.clamp(min=1), height.clamp(min=1)          # (an empty window divides by 1 and is masked below)
        wide = w * H >= h * W
        dh_wide = (2 * ((h * W + w) // (2 * w))).clamp(min=2, max=H)
        dw_tall = (2 * ((w * H + h) // (2 * h))).clamp(min=2, max=W)
        dw = torch.where(wide, torch.full_like(w, W), dw_tall)
        dh = torch.where(wide, dh_wide, torch.full_like(h, H))
        out[:, 6], out[:, 7], out[:, 8], out[:, 9] = 2 * ((W - dw) // 4) * keep, 2 * ((H - dh) // 4) * keep, dw * keep, dh * keep
    return out.to(torch.int32)
