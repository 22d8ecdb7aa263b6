"""numpy restatement of the reference's scene-change detection, for the tests
of rav1e_amd's frame_deltas / SceneChangeDetector / KeyframeDetector:
PixelIter (src/frame/mod.rs:126-172), SceneChangeDetector (src/scenechange/
mod.rs) and the part of the lookahead that drives it (src/api/internal.rs:
280-330, 767-810; src/api/mod.rs:304-321, 490-492).  Shares no code with
rav1e_amd; tests/golden/ref_scenecut.npz (the reference's own text, run by
tools/refeval/gen_scenecut_ref.py) pins it.

A frame is a list of planes (visible pixels as a 2-D array, xdec, ydec): one
plane for luma only, three for Y, U, V."""
import numpy as np


def chroma_size(w, h, xdec, ydec):
    """ChromaSampling::get_chroma_dimensions"""
    return (w + xdec) >> xdec, (h + ydec) >> ydec


def make_frame(planes, xdec=0, ydec=0):
    """[(Y, 0, 0), (U, xdec, ydec), (V, xdec, ydec)] of 1 or 3 arrays."""
    return [(np.asarray(p), xdec if k else 0, ydec if k else 0) for k, p in enumerate(planes)]


def pixel_iter(frame):
    """What PixelIter yields: an (w * h - 1, n_planes) array -- the iterator
    returns None when it stands on the last position, before yielding it."""
    y_plane = frame[0][0]
    h, w = y_plane.shape
    ys, xs = np.divmod(np.arange(w * h - 1), w)
    return np.stack([p[ys >> yd, xs >> xd].astype(np.int64) for p, xd, yd in frame], axis=1)


def plane_sums(frame1, frame2):
    """The per-plane sums of has_scenecut's map / sum (fold), as Python ints."""
    d = np.abs(pixel_iter(frame1) - pixel_iter(frame2))
    return [int(v) for v in d.sum(axis=0)]


def chroma_weights(w, h, xdec, ydec):
    """How many luma positions PixelIter maps to each pixel of a plane."""
    cw, ch = chroma_size(w, h, xdec, ydec)
    wx = np.minimum(1 << xdec, w - (np.arange(cw) << xdec))
    wy = np.minimum(1 << ydec, h - (np.arange(ch) << ydec))
    wt = np.outer(wy, wx)
    wt[(h - 1) >> ydec, (w - 1) >> xdec] -= 1
    return wt


def delta_avg(sums, length, fast_mode):
    if fast_mode:
        return sums[0] // length
    d = [np.uint16((s // length) & 0xffff) for s in sums]
    return int(np.uint16(d[0] + d[1] + d[2])) // 3


class Detector:
    def __init__(self, bit_depth, fast_mode):
        # BASE_THRESHOLD * bit_depth / 8 in u8: 12 * 12 = 144 still fits
        self.threshold = (12 * bit_depth) // 8
        self.fast_mode = fast_mode
        self.excluded_frames = set()
        self.comparisons = []  # (sums, delta_avg, bool) of every has_scenecut

    def has_scenecut(self, frame1, frame2):
        h, w = frame2[0][0].shape
        n = 1 if self.fast_mode else 3
        sums = plane_sums(frame1[:n], frame2[:n])
        avg = delta_avg(sums, w * h, self.fast_mode)
        self.comparisons.append((sums, avg, avg >= self.threshold))
        return avg >= self.threshold

    def exclude_scene_flashes(self, frame_subset, frameno, keyframe_lookahead_distance):
        lookahead_distance = min(keyframe_lookahead_distance, len(frame_subset) - 1)
        if lookahead_distance > 1:
            for j in range(1, lookahead_distance + 1):
                if not self.has_scenecut(frame_subset[0], frame_subset[j]):
                    self.excluded_frames.update(frameno + i - 1 for i in range(j + 1))
        for i in range(1, lookahead_distance + 1):
            if i < lookahead_distance and \
                    self.has_scenecut(frame_subset[i], frame_subset[lookahead_distance]):
                self.excluded_frames.add(frameno + i - 1)

    def is_key_frame(self, previous_frame, current_frame, current_frameno, min_kf, max_kf,
                     no_scene_detection, keyframes, keyframes_forced):
        if current_frameno in keyframes_forced:
            return True
        distance = current_frameno - sorted(keyframes)[-1]
        if distance < min_kf:
            return False
        if distance >= max_kf:
            return True
        if no_scene_detection:
            return False
        if current_frameno in self.excluded_frames:
            return False
        return self.has_scenecut(previous_frame, current_frame)

    def analyze_next_frame(self, previous_frame, frame_set, input_frameno, min_kf, max_kf,
                           no_scene_detection, lookahead_distance, keyframes, keyframes_forced):
        if previous_frame is None:
            keyframes.add(0)
            return
        frame_set = [previous_frame] + list(frame_set)
        self.exclude_scene_flashes(frame_set, input_frameno, lookahead_distance)
        if self.is_key_frame(frame_set[0], frame_set[1], input_frameno, min_kf, max_kf,
                             no_scene_detection, keyframes, keyframes_forced):
            keyframes.add(input_frameno)


class Stream:
    """send_frame / flush over an unbounded frame queue (nothing is ever
    encoded here, so nothing leaves it)."""

    def __init__(self, bit_depth, fast_mode, min_kf, max_kf, distance=5,
                 no_scene_detection=False):
        self.detector = Detector(bit_depth, fast_mode)
        self.min_kf, self.max_kf, self.distance = min_kf, max_kf, distance
        self.no_scene_detection = no_scene_detection
        self.frame_count, self.limit, self.is_flushing = 0, None, False
        self.frame_q = {}
        self.keyframes, self.keyframes_forced = set(), set()
        self.next_lookahead_frame = 0
        self.analysed_at = []  # (input_frameno, last queue key, len(frame_set)) per analysis

    def send_frame(self, frame, force_key=False):
        if frame is None:
            if self.is_flushing:
                return
            self.limit = self.frame_count
            self.is_flushing = True
        else:
            assert not self.is_flushing
        input_frameno = self.frame_count
        if frame is not None:
            self.frame_count += 1
        self.frame_q[input_frameno] = frame
        if force_key:
            self.keyframes_forced.add(input_frameno)
        self.compute_lookahead_data()

    def flush(self):
        self.send_frame(None)

    def needs_more_frame_q_lookahead(self, input_frameno):
        lookahead_end = max(self.frame_q) if self.frame_q else 0
        frames_needed = input_frameno + self.distance + 1
        more = self.limit is None or lookahead_end < self.limit
        return lookahead_end < frames_needed and more

    def compute_lookahead_data(self):
        frames = [self.frame_q[n] for n in sorted(self.frame_q)
                  if n >= self.next_lookahead_frame and self.frame_q[n] is not None]
        idx = 0
        while not self.needs_more_frame_q_lookahead(self.next_lookahead_frame):
            current = frames[idx:]
            if not current:
                break
            n = self.next_lookahead_frame
            self.analysed_at.append((n, max(self.frame_q), len(current)))
            self.detector.analyze_next_frame(
                None if n == 0 else self.frame_q[n - 1], current, n, self.min_kf, self.max_kf,
                self.no_scene_detection, self.distance, self.keyframes, self.keyframes_forced)
            self.next_lookahead_frame += 1
            idx += 1


def run_stream(frames, bit_depth, fast_mode, min_kf, max_kf, distance=5):
    s = Stream(bit_depth, fast_mode, min_kf, max_kf, distance)
    for f in frames:
        s.send_frame(f)
    s.flush()
    return s
