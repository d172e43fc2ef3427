"""A whole picture from the text of H.264 alone (TEST INFRASTRUCTURE): no call into the oracle, no oracle library loaded.

* inter macroblocks: the prediction of tests/inter_checker.py (8.4.2.2, 8.4.2.3), then the residual of tests/residual_checker.py
  (8.5) on top;
* intra macroblocks, in raster order behind them: tests/intra_checker.py's IntraChecker with ITS residual hooks and inter-sample
  source replaced by the two above (its pure functions pred4x4 / pred16x16 / pred_chroma / block_availability do 8.3; I_PCM is a
  copy);
* the loop filter: tests/slice_filter_checker.py (8.7; with every `flags` zero that is tests/deblock_checker.py).

Nothing is borrowed: the expected output of a picture at the CPU -> GPU seam is computed from the standard.  A macroblock whose
residual leaves the range H.264 bounds (8.5.10 - 8.5.12) has no defined result: reconstruct raises residual_checker.OutOfRange
(residual_checker.make_conformant brings a drawn picture into range first)."""
import numpy as np

from p264decoder_amd import _native as N
from tests import inter_checker, intra_checker, residual_checker, slice_filter_checker


class Frames:
    """a frame store: frames[slot] = [y, u, v], uint8, unpadded"""

    def __init__(self, mb_w, mb_h, slots):
        w, h = mb_w * 16, mb_h * 16
        self.frames = [[np.zeros((h, w), np.uint8), np.zeros((h // 2, w // 2), np.uint8), np.zeros((h // 2, w // 2), np.uint8)] for _ in range(slots)]

    def __getitem__(self, slot):
        return self.frames[slot]

    def write(self, slot, planes):
        for dst, src in zip(self.frames[slot], planes):
            dst[:] = src


class _Residual:
    """IntraChecker's three hooks, by residual_checker"""

    def __init__(self):
        self.cache = (None, None)

    def _of(self, pic, r, x_mb, y_mb):
        m = y_mb * pic.desc.mb_w + x_mb
        if self.cache[0] != (id(pic), m):
            self.cache = ((id(pic), m), residual_checker.residual_of(pic, m)[0])
        return self.cache[1]

    def _luma4x4_residual(self, pic, r, Y, x, y, i):
        res = self._of(pic, r, x // 16, y // 16)
        residual_checker.construct(Y, x, y, res[(0, x % 16, y % 16)])

    def _luma16x16_residual(self, pic, r, Y, x0, y0):
        for (plane, x, y), rr in self._of(pic, r, x0 // 16, y0 // 16).items():
            if plane == 0:
                residual_checker.construct(Y, x0 + x, y0 + y, rr)

    def _chroma_residual(self, pic, r, planes, x0, y0):
        for (plane, x, y), rr in self._of(pic, r, x0 // 8, y0 // 8).items():
            if plane:
                residual_checker.construct(planes[plane], x0 + x, y0 + y, rr)


class SpecRecon:
    """a frame store of `slots` frames; reconstruct() decodes one picture at the seam into it"""

    def __init__(self, mb_w, mb_h, slots):
        self.store = Frames(mb_w, mb_h, slots)
        self.census = inter_checker.Census()
        self.intra = intra_checker.IntraChecker(None, mb_w, mb_h, slots, residual=_Residual(), inter=self._inter, store=self.store)

    def _inter(self, pic):
        F = inter_checker.predict(pic, self.store, self.census)
        for m in np.flatnonzero(pic.mb_records()["mb_type"] > N.MB_IPCM):
            residual_checker.add_residual(pic, int(m), F)

    def nodeblock(self, pic):
        self.intra.residual.cache = (None, None)
        return self.intra.nodeblock(pic)

    def reconstruct(self, pic):
        """the decoded picture: [y, u, v], views into the store"""
        F = self.nodeblock(pic)
        if pic.desc.deblock:
            slice_filter_checker.deblock(pic, F)
        return F
