"""The output process of H.264 C.4.5.3 ("bumping") as include/p264parse.h states it, restated in Python from the standard's text:
which decoded pictures are due for display with every completed picture.  It imports nothing from the library; the tests compare the
parser and the pipeline with it.

A picture is (poc, idr, mmco5, ref): its picture order count, whether it is an IDR picture, whether it carried
memory_management_control_operation 5, whether it is a reference picture.  Pictures are named by their decode index.

    1. an IDR picture or one with operation 5: everything that waits is due first, ascending by order count
    2. the picture joins the waiting set W (with order count 0 after operation 5)
    3. while |W| > R the member with the smallest order count is due
    4. the next picture needs a frame buffer that holds neither a reference nor a member of W; there are `frames` + 1 of them (the
       decoded picture buffer and the picture being decoded).  While none is empty and W is not, the smallest order count is due
Of equal order counts (a stream that does not conform) the picture decoded first goes first.

References are marked by the sliding window alone (8.2.5.3: at most num_ref_frames, the oldest goes) - the marking of the streams the
tests write.  frames=None leaves out step 4 (buffers without bound), which is what p264parse_kat_output_order runs."""


class OutputOrder:
    def __init__(self, depth, frames=None, num_ref_frames=1):
        self.depth, self.frames, self.num_ref_frames = depth, frames, max(num_ref_frames, 1)
        self.waiting = {}                  # decode index -> order count
        self.refs = []                     # decode indices of the reference pictures, oldest first
        self.count = 0
        self.bumped_for_room = 0           # pictures that step 4 made due

    def _first(self):
        return min(self.waiting, key=lambda i: (self.waiting[i], i))

    def _pop(self, due):
        i = self._first()
        del self.waiting[i]
        due.append(i)

    def picture(self, poc, idr=False, mmco5=False, ref=True):
        """the decode indices that are due with this picture, in output order"""
        me, due = self.count, []
        self.count += 1
        # marking (8.2.5): an IDR picture and operation 5 empty the references, the sliding window drops the oldest
        if idr or mmco5:
            self.refs = []
        elif ref and len(self.refs) >= self.num_ref_frames:
            self.refs.pop(0)
        if ref:
            self.refs.append(me)
        if idr or mmco5:                                       # 1
            while self.waiting:
                self._pop(due)
        self.waiting[me] = 0 if mmco5 else poc                 # 2
        while len(self.waiting) > self.depth:                  # 3
            self._pop(due)
        if self.frames is not None:                            # 4
            while self.waiting and len(set(self.refs) | set(self.waiting)) >= self.frames + 1:
                self._pop(due)
                self.bumped_for_room += 1
        return due

    def flush(self):
        due = []
        while self.waiting:
            self._pop(due)
        return due


def run(pictures, depth, frames=None, num_ref_frames=1):
    """([due with picture 0, due with picture 1, ...], due at the flush, the model)"""
    m = OutputOrder(depth, frames, num_ref_frames)
    per = [m.picture(*p) for p in pictures]
    return per, m.flush(), m


# ---- the writer's B streams (p264decoder_amd/tools/synth264.c, --bframes N): decode order is the IDR picture, then groups of one P
# picture followed by the N B pictures that are shown in front of it; order count = 2 x display position; B pictures are no references
def bframes_pictures(n_pictures, bframes):
    out = []
    for n in range(n_pictures):
        if n == 0:
            out.append((0, True, False, True))
            continue
        pos, group = (n - 1) % (bframes + 1), (n - 1) // (bframes + 1) + 1
        is_b = pos > 0
        out.append((2 * ((group - 1) * (bframes + 1) + pos if is_b else group * (bframes + 1)), False, False, not is_b))
    return out


def baseline_pictures(n_pictures, gop):
    """the writer's Baseline streams (pic_order_cnt_type 2, every picture a reference): order count 2 x pictures since the IDR picture"""
    out, since = [], 0
    for n in range(n_pictures):
        idr = n == 0 or (gop > 0 and n % gop == 0)
        since = 0 if idr else since + 1
        out.append((2 * since, idr, False, True))
    return out


# Table A-1: MaxDpbMbs by level_idc
MAX_DPB_MBS = {9: 396, 10: 396, 11: 900, 12: 2376, 13: 2376, 20: 2376, 21: 4752, 22: 8100, 30: 8100, 31: 18000, 32: 20480, 40: 32768,
               41: 32768, 42: 34816, 50: 110400, 51: 184320, 52: 184320}


def dpb_frames(level_idc, mb_w, mb_h, num_ref_frames, max_dec_frame_buffering=None):
    """D of include/p264parse.h"""
    d = max_dec_frame_buffering if max_dec_frame_buffering is not None else MAX_DPB_MBS[level_idc] // (mb_w * mb_h) if level_idc in MAX_DPB_MBS else 16
    return min(max(d, num_ref_frames, 1), 16)


def deliveries(rounds, flushes, capacity):
    """The pipeline's deliveries: rounds[r][stream] = the decode indices due in round r (None: the stream has ended), flushes[stream]
    the ones due at the end; by stream ascending, a round's pictures cut into pieces of `capacity`.  [[(stream, decode index)]]"""
    out = []
    for per_stream in list(rounds) + [flushes]:
        due = [(s, i) for s, d in enumerate(per_stream) if d for i in d]
        out += [due[at:at + capacity] for at in range(0, len(due), capacity)]
    return out
