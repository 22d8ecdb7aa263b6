"""Scene-change detection: frame_deltas (rv_frame_delta_batch),
SceneChangeDetector and KeyframeDetector against tests/scenecut_ref.py (a
numpy restatement of PixelIter, src/frame/mod.rs:126-172, of src/scenechange/
mod.rs and of the lookahead's gating, src/api/internal.rs:280-330, 767-810),
which itself is pinned to the vectors the reference's own text produced
(tests/golden/ref_scenecut.npz, written by tools/refeval/gen_scenecut_ref.py)
and to the known answers of the reference's src/api/test.rs.  CPU tests
first, GPU tests (exact equality) after."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rav1e_amd as R
from tests import scenecut_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_scenecut.npz")


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


def shapes_of(w, h, xdec, ydec):
    cw, ch = SR.chroma_size(w, h, xdec, ydec)
    return [(h, w), (ch, cw), (ch, cw)]


def take_frames(px, off, k0, n, w, h, xdec, ydec):
    """n frames of three planes each from a flat pixel store, plane k0 on."""
    frames, k = [], k0
    for _ in range(n):
        pl = []
        for s in shapes_of(w, h, xdec, ydec):
            pl.append(px[off[k]:off[k + 1]].reshape(s))
            k += 1
        frames.append(SR.make_frame(pl, xdec, ydec))
    return frames


# ---------------------------------------------------------------- restatement
def test_restatement_has_scenecut_equals_reference_vectors():
    g = golden()
    meta = g["pair_meta"]
    assert {(int(m[0]), int(m[1])) for m in meta} == {(16, 10), (17, 9), (9, 7), (4, 4)}
    assert {(int(m[2]), int(m[3])) for m in meta} == {(1, 1), (1, 0), (0, 0)}
    assert {int(m[4]) for m in meta} == {8, 10, 12}
    assert len({tuple(m) for m in meta.tolist()}) == 36
    for k, (w, h, xdec, ydec, bd) in enumerate(meta.tolist()):
        f1, f2 = take_frames(g["pair_px"], g["pair_off"], 6 * k, 2, w, h, xdec, ydec)
        sums = SR.plane_sums(f1, f2)
        assert sums == [int(v) for v in g["pair_sums"][k]], (k, w, h, xdec, ydec, bd)
        assert sums[0] == int(g["pair_fast_sum"][k])
        for mode, fast in enumerate((False, True)):
            det = SR.Detector(bd, fast)
            assert det.has_scenecut(f1, f2) == bool(g["pair_cut"][k][mode])
            assert det.comparisons[-1][1] == int(g["pair_avg"][k][mode])
        # the same sums as a weighted sum over each plane's own pixels: what
        # the kernel computes
        for p in range(3):
            wt = SR.chroma_weights(w, h, f1[p][1], f1[p][2])
            d = np.abs(f1[p][0].astype(np.int64) - f2[p][0].astype(np.int64))
            assert int((wt * d).sum()) == sums[p]
            assert wt.sum() == w * h - 1 and wt.min() >= 0
    assert g["pair_cut"].any(axis=0).all() and not g["pair_cut"].all(axis=0).any()


def test_restatement_analyze_next_frame_equals_reference_vectors():
    g = golden()
    meta, calls = g["seq_meta"], g["seq_calls"]
    assert len(meta) >= 6
    assert {int(m[5]) for m in meta} == {0, 1}  # both modes
    assert {(int(m[2]), int(m[3])) for m in meta} == {(1, 1), (1, 0), (0, 0)}
    assert {int(m[4]) for m in meta} == {8, 10, 12}
    k0 = 0
    for si, (w, h, xdec, ydec, bd, fast, min_kf, max_kf, forced, n) in enumerate(meta.tolist()):
        frames = take_frames(g["seq_px"], g["seq_off"], k0, n, w, h, xdec, ydec)
        k0 += 3 * n
        mine = calls[calls[:, 0] == si]
        assert len(mine) == n
        det = SR.Detector(bd, bool(fast))
        keyframes, forced_set = set(), ({forced} if forced >= 0 else set())
        for (_, N, set_len, compared, kf_mask, ex_mask) in mine.tolist():
            before = len(det.comparisons)
            det.analyze_next_frame(frames[N - 1] if N else None, frames[N:N + set_len], N, min_kf,
                                   max_kf, False, 5, keyframes, forced_set)
            assert len(det.comparisons) - before == compared, (si, N)
            assert sum(1 << v for v in keyframes) == kf_mask, (si, N)
            assert sum(1 << v for v in det.excluded_frames) == ex_mask, (si, N)
        # the streaming driver hands over the same frame sets
        s = SR.Stream(bd, bool(fast), min_kf, max_kf)
        for i, f in enumerate(frames):
            s.send_frame(f, force_key=(i == forced))
        s.flush()
        assert [(a[0], a[2]) for a in s.analysed_at] == [(c[1], c[2]) for c in mine.tolist()]
        assert sum(1 << v for v in s.keyframes) == int(mine[-1][4])
        assert sum(1 << v for v in s.detector.excluded_frames) == int(mine[-1][5])


# ---------------------------------------------------------------- known answers
# src/api/test.rs: 64 x 80, speed 10 (fast mode), 8-bit 4:2:0, constant frames,
# min interval 0; every new GOP of the expected frame list is a key frame.
def known_answers():
    t = []
    for s in range(5):  # output_frameno_reorder_scene_change_at, :542
        t.append(([0] * s + [255] * (5 - s), 5, {0} if s == 0 else {0, s}))
    for f in (1, 2, 3):  # ..._no_scene_change_at_short_flash, :1144
        t.append(([255 if i != f else 0 for i in range(5)], 5, {0}))
    t.append(([0, 0, 255, 255, 255, 255, 0, 0], 10, {0}))  # ..._at_max_len_flash, :1195
    t.append(([0, 0, 255, 255, 255, 255, 255, 0], 10, {0, 2, 7}))  # ..._past_max_len_flash, :1253
    t.append(([0, 0, 40, 100, 160, 240, 240, 240], 10, {0, 5}))  # ..._at_multiple_flashes, :1313
    # the dropped pixel: 12 * 5119 / 5120 floors to 11, below the threshold 12
    t.append(([0, 12, 12, 12, 12, 12, 12, 12], 10, {0}))
    t.append(([0, 13, 13, 13, 13, 13, 13, 13], 10, {0, 1}))
    return t


def constant_frame(v, w=64, h=80, xdec=1, ydec=1, dtype=np.uint8):
    return [np.full(s, v if k == 0 else 128, dtype) for k, s in enumerate(shapes_of(w, h, xdec, ydec))]


def test_restatement_gives_the_reference_tests_key_frames():
    for luma, max_kf, want in known_answers():
        s = SR.run_stream([SR.make_frame(constant_frame(v), 1, 1) for v in luma], 8, True, 0, max_kf)
        assert s.keyframes == want, (luma, s.keyframes)
    # constant 0 against 12: the sum is 12 * (w * h - 1)
    f0, f12 = (SR.make_frame(constant_frame(v), 1, 1) for v in (0, 12))
    assert SR.plane_sums(f0, f12) == [12 * 5119, 0, 0]
    assert SR.delta_avg([12 * 5119], 5120, True) == 11


def test_yuv_mode_divides_the_truncated_sum_by_three():
    n = 64 * 80
    for det in (SR.Detector(8, False), R.SceneChangeDetector(8, False)):
        assert det.threshold == 12
    assert SR.delta_avg([35 * n, 0, 0], n, False) == 11
    assert SR.delta_avg([36 * n, 0, 0], n, False) == 12
    d = R.SceneChangeDetector(8, False)
    assert not d.scenecut_from_sums([35 * n, 0, 0], n)
    assert d.scenecut_from_sums([36 * n, 0, 0], n)
    assert d.scenecut_from_sums([36 * n + n - 1, n - 1, n - 1], n)
    assert not d.scenecut_from_sums([12 * n, 12 * n, 11 * n], n)
    f = R.SceneChangeDetector(8, True)
    assert f.scenecut_from_sums([12 * n], n) and not f.scenecut_from_sums([12 * n - 1], n)
    assert [R.scenecut_threshold(bd) for bd in (8, 10, 12)] == [12, 15, 18]
    assert [R.fast_scene_detection(s) for s in (10, 9, 6, 2)] == [True, False, False, False]
    assert R.keyframe_lookahead_distance() == 5 and R.keyframe_lookahead_distance(True) == 2


# ---------------------------------------------------------------- validation
class FakePlane:
    """A plane descriptor without device memory: enough for the checks that
    come before any launch."""

    def __init__(self, w, h, xdec=0, ydec=0, hbd=0, pad=16):
        self.desc = R.RvPlane()
        R.lib().rv_plane_geometry(C.byref(self.desc), w, h, xdec, ydec, pad, pad, hbd)


def fake_frame(w=64, h=80, xdec=1, ydec=1, hbd=0, n_planes=3):
    cw, ch = SR.chroma_size(w, h, xdec, ydec)
    return tuple([FakePlane(w, h, 0, 0, hbd)] +
                 [FakePlane(cw, ch, xdec, ydec, hbd) for _ in range(n_planes - 1)])


def bad_calls():
    """(what the message names, frames, pairs) of every call that must be
    rejected before a launch."""
    ok = [fake_frame() for _ in range(3)]
    small = fake_frame(62, 80)
    bad_chroma = (FakePlane(64, 80), FakePlane(31, 40, 1, 1), FakePlane(31, 40, 1, 1))
    return [
        ("size", ok[:2] + [small], [(0, 2)]),
        ("hbd", ok[:2] + [fake_frame(hbd=1)], [(0, 1)]),
        ("chroma plane's size", [bad_chroma, bad_chroma], [(0, 1)]),
        ("frames", [fake_frame() for _ in range(9)], [(0, 1)]),
        ("frames", ok[:1], [(0, 0)]),
        ("pairs", ok, [(0, 1)] * 17),
        ("pairs", ok, []),
        ("out of range", ok, [(0, 3)]),
        ("out of range", ok, [(-1, 0)]),
        ("4:4:4, 4:2:2 or 4:2:0", [(FakePlane(64, 80), FakePlane(64, 40, 0, 1), FakePlane(64, 40, 0, 1))] * 2,
         [(0, 1)]),
    ]


def test_python_validation_rejects_without_launch():
    for what, frames, pairs in bad_calls():
        with pytest.raises(R.Rav1eHipError, match=what):
            R.frame_deltas(frames, pairs)
    with pytest.raises(R.Rav1eHipError, match="1 plane"):
        R.frame_deltas([fake_frame()[:2]] * 2, [(0, 1)])
    with pytest.raises(R.Rav1eHipError, match="1 plane"):
        R.frame_deltas([fake_frame(), fake_frame(n_planes=1)], [(0, 1)])


def test_c_abi_validation_rejects_without_launch():
    """Every rejected call returns RV_EINVAL and names its reason; the data
    pointers are null or never dereferenced, d_sums is null."""
    L = R.lib()

    def call(frames, pairs, n_planes=None):
        n_planes = len(frames[0]) if n_planes is None else n_planes
        descs = (R.RvPlane * (len(frames) * len(frames[0])))(*(p.desc for f in frames for p in f))
        pa = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        rc = L.rv_frame_delta_batch(descs, len(frames), n_planes, pa.ctypes.data, len(pa), None,
                                    None)
        return rc, L.rv_last_error().decode()

    want = {"size": "differ", "hbd": "differ", "chroma plane's size": "chroma plane's size",
            "frames": "n_frames", "pairs": "n_pairs", "out of range": "out of range",
            "4:4:4, 4:2:2 or 4:2:0": "4:4:4, 4:2:2 or 4:2:0"}
    for what, frames, pairs in bad_calls():
        for f in frames:
            for p in f:
                p.desc.data = 4096  # never dereferenced
        rc, msg = call(frames, pairs if len(pairs) else np.zeros((0, 2), np.int32))
        assert rc == R.RV_EINVAL and want[what] in msg, (what, rc, msg)
    ok = [fake_frame() for _ in range(2)]
    rc, msg = call(ok, [(0, 1)], n_planes=2)
    assert rc == R.RV_EINVAL and "n_planes" in msg
    # a plane without data is refused too, after the geometry
    rc, msg = call(ok, [(0, 1)])
    assert rc == R.RV_EINVAL and "no data" in msg
    for f in ok:
        for p in f:
            p.desc.data = 4096
    # a well-formed call gets as far as the missing result buffer
    rc, msg = call(ok, [(0, 1), (1, 1)])
    assert rc == R.RV_EINVAL and "null d_sums" in msg
    assert R.DELTA_MAX_FRAMES == 8 and R.DELTA_MAX_PAIRS == 16


def test_kernels_use_no_scratch(tmp_path):
    """Every kernel of rv_scenecut.hip keeps its runs and its 28 accumulators
    in registers: the compiler reports 0 bytes of scratch per lane."""
    mk = open(os.path.join(ROOT, "rav1e_amd", "csrc", "Makefile")).read()
    hipcc = os.environ.get("HIPCC", re.search(r"^HIPCC \?= (\S+)", mk, re.M).group(1))
    if shutil.which(hipcc) is None:
        pytest.skip("hipcc absent")
    arch = re.search(r"^ARCH \?= (\S+)", mk, re.M).group(1)
    flags = re.search(r"^HIPFLAGS \?= ((?:.*\\\n)*.*)$", mk, re.M).group(1)
    flags = flags.replace("\\\n", " ").replace("$(ARCH)", arch).split()
    r = subprocess.run([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                          "rv_scenecut.hip", "-o", str(tmp_path / "rv_scenecut.o")],
                       cwd=os.path.join(ROOT, "rav1e_amd", "csrc"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)
    assert len(names) == len(scratch) >= 7
    assert sum("frame_delta_kernel" in n for n in names) == 6
    assert any("frame_delta_finish_kernel" in n for n in names)
    spilled = [(n, s) for n, s in zip(names, scratch) if s != "0"]
    assert not spilled, spilled


# ---------------------------------------------------------------- the detector's logic, no GPU
class HostPlane(FakePlane):
    """A descriptor plus the visible pixels on the host, for the stand-in of
    frame_deltas below."""

    def __init__(self, a, xdec=0, ydec=0):
        super().__init__(a.shape[1], a.shape[0], xdec, ydec, int(a.dtype == np.uint16))
        self.px = a


def host_frame(planes, xdec, ydec):
    return tuple(HostPlane(np.asarray(p), xdec if k else 0, ydec if k else 0)
                 for k, p in enumerate(planes))


def host_frame_deltas(frames, pairs):
    R._delta_geometry(frames, pairs)
    ref = [SR.make_frame([p.px for p in f], f[-1].desc.xdec, f[-1].desc.ydec) for f in frames]
    return np.array([SR.plane_sums(ref[a], ref[b]) for a, b in pairs], np.uint64)


def planted_sequence(rng, bd, xdec, ydec, w=32, h=16):
    """24 frames: cuts at 5, 15 and 20, a two-frame flash at 10 and 11."""
    scenes = "AAAAABBBBBffBBBDDDDDEEEE"
    assert len(scenes) == 24
    maxv = (1 << bd) - 1
    dtype = np.uint8 if bd == 8 else np.uint16
    level = {"A": 1, "B": 5, "f": 3, "D": 7, "E": 2}
    frames = []
    for ch in scenes:
        frames.append([np.clip(level[ch] * (maxv // 8) + rng.integers(-3, 4, s), 0, maxv).astype(dtype)
                       for s in shapes_of(w, h, xdec, ydec)])
    return frames


def run_detector(make_frame, frames, bd, fast, min_kf, max_kf, xdec=1, ydec=1):
    kd = R.KeyframeDetector(bd, fast, min_kf, max_kf)
    alive = []
    for f in frames:
        kd.send_frame(make_frame(f, xdec, ydec))
        alive.append(sum(1 for v in kd.frame_q.values() if v is not None))
    kd.flush()
    return kd, alive


def check_detector_against_restatement(make_frame):
    for luma, max_kf, want in known_answers():
        kd, _ = run_detector(make_frame, [constant_frame(v) for v in luma], 8, True, 0, max_kf)
        assert kd.keyframes == want, (luma, kd.keyframes)
        kd.flush()  # a second flush changes nothing
        assert kd.keyframes == want
    rng = np.random.default_rng(5)
    for fast, bd, (xdec, ydec) in ((True, 8, (1, 1)), (False, 10, (1, 0))):
        frames = planted_sequence(rng, bd, xdec, ydec)
        ref = SR.run_stream([SR.make_frame(f, xdec, ydec) for f in frames], bd, fast, 0, 240)
        kd, alive = run_detector(make_frame, frames, bd, fast, 0, 240, xdec, ydec)
        assert ref.keyframes == {0, 5, 15, 20}  # the flash is no cut
        assert kd.keyframes == ref.keyframes
        assert kd.excluded_frames == ref.detector.excluded_frames
        assert max(alive) == kd.distance + 2 == 7
        with pytest.raises(R.Rav1eHipError, match="after flush"):
            kd.send_frame(make_frame(frames[0], xdec, ydec))


def check_launch_economy(make_frame):
    """A 20-frame stream: frames 1 .. 4 fill the memo (9, 8, 7, 6 pairs), every
    frame from 5 on whose window is full needs the newest frame against the
    five before it, and the shrinking windows of the flush need nothing."""
    rng = np.random.default_rng(11)
    frames = [[rng.integers(0, 256, s).astype(np.uint8) for s in shapes_of(32, 16, 1, 1)]
              for _ in range(20)]
    kd = R.KeyframeDetector(8, True, 0, 240)
    analysed = []
    for f in frames:
        kd.send_frame(make_frame(f, 1, 1))
        analysed.append(kd.next_lookahead_frame)
    # frame N is analysed once frame N + 6 is in: the gating
    assert analysed == [0] * 6 + list(range(1, 15))
    assert kd.launches <= kd.next_lookahead_frame
    kd.flush()
    assert kd.next_lookahead_frame == 20
    assert kd.launch_pairs == [9, 8, 7, 6] + [5] * 11
    assert kd.launches == len(kd.launch_pairs) <= 19
    ref = SR.run_stream([SR.make_frame(f, 1, 1) for f in frames], 8, True, 0, 240)
    assert kd.keyframes == ref.keyframes and kd.excluded_frames == ref.detector.excluded_frames
    # what the memo saves: the restatement compares 9 pairs per full window
    assert len(ref.detector.comparisons) > sum(kd.launch_pairs) == 85


def test_detector_logic_on_host_planes(monkeypatch):
    """SceneChangeDetector / KeyframeDetector with frame_deltas replaced by the
    restatement's sums: the decisions, the memo and the gating, without a GPU."""
    monkeypatch.setattr(R, "frame_deltas", host_frame_deltas)
    check_detector_against_restatement(host_frame)
    check_launch_economy(host_frame)
    # analyze_next_frame on the reference's recorded calls, forced keys and
    # intervals included
    g = golden()
    k0 = 0
    for si, (w, h, xdec, ydec, bd, fast, min_kf, max_kf, forced, n) in enumerate(g["seq_meta"].tolist()):
        frames = take_frames(g["seq_px"], g["seq_off"], k0, n, w, h, xdec, ydec)
        k0 += 3 * n
        dev = [host_frame([p[0] for p in f], xdec, ydec) for f in frames]
        det = R.SceneChangeDetector(bd, bool(fast))
        keyframes, forced_set = set(), ({forced} if forced >= 0 else set())
        for (_, N, set_len, _, kf_mask, ex_mask) in g["seq_calls"][g["seq_calls"][:, 0] == si].tolist():
            launches = det.launches
            det.analyze_next_frame(dev[N - 1] if N else None, dev[N:N + set_len], N, min_kf, max_kf,
                                   False, 5, keyframes, forced_set)
            assert det.launches - launches <= 1
            assert sum(1 << v for v in keyframes) == kf_mask, (si, N)
            assert sum(1 << v for v in det.excluded_frames) == ex_mask, (si, N)


# ---------------------------------------------------------------- GPU
def device_frame(planes, xdec, ydec, bd=None):
    return tuple(R.DevicePlane.from_array(np.ascontiguousarray(p), xpad=16, ypad=16,
                                          xdec=xdec if k else 0, ydec=ydec if k else 0,
                                          bit_depth=bd)
                 for k, p in enumerate(planes))


NINE_PAIRS = [(0, j) for j in range(1, 6)] + [(i, 5) for i in range(1, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,xdec,ydec,bd", [
    (17, 9, 1, 1, 8), (9, 7, 1, 1, 8), (64, 80, 1, 1, 8), (64, 80, 1, 0, 8), (64, 80, 0, 0, 8),
    (130, 66, 1, 1, 10), (320, 180, 1, 1, 12), (17, 9, 1, 0, 12)])
def test_frame_deltas_equal_restatement(w, h, xdec, ydec, bd):
    R.require_device(0)
    rng = np.random.default_rng(w * 1000 + h + bd)
    dtype = np.uint8 if bd == 8 else np.uint16
    host = [[rng.integers(0, 1 << bd, s).astype(dtype) for s in shapes_of(w, h, xdec, ydec)]
            for _ in range(6)]
    ref = [SR.make_frame(f, xdec, ydec) for f in host]
    want = np.array([SR.plane_sums(ref[a], ref[b]) for a, b in NINE_PAIRS], np.uint64)
    dev = [device_frame(f, xdec, ydec, bd) for f in host]
    got = R.frame_deltas(dev, NINE_PAIRS)
    assert got.dtype == np.uint64 and got.shape == (9, 3)
    assert (got == want).all(), (got, want)
    # luma only, and the pairs the other way round
    got1 = R.frame_deltas([f[:1] for f in dev], [(b, a) for a, b in NINE_PAIRS])
    assert (got1 == want[:, :1]).all()


@pytest.mark.gpu
def test_dropped_pixel():
    """Two frames that differ only at luma (w - 1, h - 1) and at the chroma
    pixel that holds it."""
    R.require_device(0)
    rng = np.random.default_rng(3)
    for (w, h, xdec, ydec, weight) in ((64, 80, 1, 1, 4), (64, 80, 1, 0, 2), (64, 80, 0, 0, 1),
                                       (17, 9, 1, 1, 1), (18, 9, 1, 1, 2), (17, 10, 1, 1, 2)):
        a = [rng.integers(0, 200, s).astype(np.uint8) for s in shapes_of(w, h, xdec, ydec)]
        b = [p.copy() for p in a]
        for p, d in zip(b, (50, 7, 9)):
            p[-1, -1] += d
        assert SR.chroma_weights(w, h, xdec, ydec)[-1, -1] == weight - 1
        got = R.frame_deltas([device_frame(a, xdec, ydec), device_frame(b, xdec, ydec)], [(0, 1)])
        assert got.tolist() == [[0, (weight - 1) * 7, (weight - 1) * 9]], (w, h, xdec, ydec)


@pytest.mark.gpu
def test_sum_carries_past_32_bits():
    R.require_device(0)
    w, h = 1056, 1024
    a = R.DevicePlane.from_array(np.zeros((h, w), np.uint16), xpad=16, ypad=16, bit_depth=12)
    b = R.DevicePlane.from_array(np.full((h, w), 4095, np.uint16), xpad=16, ypad=16, bit_depth=12)
    got = R.frame_deltas([(a,), (b,)], [(0, 1)])
    assert got.tolist() == [[4428099585]] and 4428099585 == (w * h - 1) * 4095 > 1 << 32


@pytest.mark.gpu
@pytest.mark.parametrize("bd", [8, 10])
def test_padding_is_not_read(bd):
    """Equal visible areas inside random, differing padding, at origins and
    strides that are no multiple of anything: every sum is 0."""
    R.require_device(0)
    rng = np.random.default_rng(bd)
    dtype = np.uint8 if bd == 8 else np.uint16
    w, h, xdec, ydec = 45, 21, 1, 1
    vis = [rng.integers(0, 1 << bd, s).astype(dtype) for s in shapes_of(w, h, xdec, ydec)]
    frames = []
    for f in range(3):
        planes = []
        for k, v in enumerate(vis):
            xo, yo = 3 + 2 * f + k, 1 + f
            full = rng.integers(0, 1 << bd, (v.shape[0] + yo + 2 + k, v.shape[1] + xo + 5 + f)).astype(dtype)
            full[yo:yo + v.shape[0], xo:xo + v.shape[1]] = v
            p = R.DevicePlane.from_full(full, xo, yo, v.shape[1], v.shape[0], bit_depth=bd)
            p.desc.xdec, p.desc.ydec = (xdec, ydec) if k else (0, 0)
            planes.append(p)
        frames.append(tuple(planes))
    got = R.frame_deltas(frames, [(0, 1), (0, 2), (1, 2)])
    assert not got.any(), got
    # and a visible difference is still seen through the same planes
    other = [v.copy() for v in vis]
    other[0][0, 0] ^= 1
    u = int(other[1][-1, 0])
    other[1][-1, 0] = u + 3 if u < 100 else u - 3
    got = R.frame_deltas([frames[0], device_frame(other, xdec, ydec, bd)], [(0, 1)])
    assert got.tolist() == [[1, 3 * 2, 0]]  # chroma row 10 of 11 holds one luma row: 2 x 1


@pytest.mark.gpu
def test_equal_indices_and_repeated_pairs():
    R.require_device(0)
    rng = np.random.default_rng(9)
    host = [[rng.integers(0, 256, s).astype(np.uint8) for s in shapes_of(40, 24, 1, 1)]
            for _ in range(3)]
    ref = [SR.make_frame(f, 1, 1) for f in host]
    dev = [device_frame(f, 1, 1) for f in host]
    pairs = [(1, 1), (0, 2), (2, 0), (0, 2), (0, 0), (1, 2)]
    got = R.frame_deltas(dev, pairs)
    want = np.array([SR.plane_sums(ref[a], ref[b]) for a, b in pairs], np.uint64)
    assert (got == want).all() and not got[0].any() and not got[4].any()
    assert (got[1] == got[2]).all() and (got[1] == got[3]).all() and got[1].all()
    assert not R.frame_deltas(dev, [(2, 2), (0, 0)]).any()


@pytest.mark.gpu
def test_keyframe_detector_on_device_frames():
    """The reference tests' key frames, the two boundary facts and one random
    sequence per mode, through KeyframeDetector on device frames."""
    R.require_device(0)
    check_detector_against_restatement(device_frame)
    d = R.SceneChangeDetector(8, False)
    f0, f12, f13 = (device_frame(constant_frame(v), 1, 1) for v in (0, 12, 13))
    assert not d.has_scenecut(f0, f12) and not d.has_scenecut(f0, f13)  # (13 + 0 + 0) / 3
    d = R.SceneChangeDetector(8, True)
    assert not d.has_scenecut(f0, f12) and d.has_scenecut(f0, f13) and d.launches == 2


@pytest.mark.gpu
def test_launch_economy():
    R.require_device(0)
    check_launch_economy(device_frame)
