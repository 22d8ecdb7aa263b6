"""Layer 1 of include/rav1e_hip.h (rav1e_amd/csrc/rv_shims.hip): every
drop-in asm-shaped entry point, the dispatch tables and the per-thread
staging contexts, bit for bit against the CPU oracle.

The CPU tests compare addresses only (no launch): rv_sad_fn / rv_satd_fn /
rv_put_fn_get against the exported symbols, with the names built from the
reference's own tables (BlockSize order of src/partition.rs, FilterMode order
of src/mc.rs, get_2d_mode_idx of src/asm/x86/mc.rs), and check on the oracle
alone that the inputs of the GPU tests cannot hide a wrong binding: the 22
sizes' SADs / SATDs and the 16 filter pairs' outputs are pairwise distinct.

The GPU tests call all 88 + 64 + 2 + 2 functions by name on host arrays with
byte strides: u8, and u16 holding 10-bit and 12-bit values.  Destinations are
wider than the block and pre-filled with a sentinel; whatever lies outside the
w x h block must come back unchanged.
"""
import ctypes as C
import functools
import threading
import time

import numpy as np
import pytest

import rav1e_amd as R
from tests import oracle_lib as O

HIP = int(R.CpuFeatureLevel.HIP)
FILTERS = ["regular", "smooth", "sharp", "bilinear"]  # FilterMode order (src/mc.rs:58-66)
SIZES = [(R.BlockSize(i).width(), R.BlockSize(i).height()) for i in range(22)]
PAIRS = [(mx, my) for my in range(4) for mx in range(4)]
KINDS = ["u8", "hbd10", "hbd12"]  # pixel type and the depth of the values it holds
BD = {"u8": 8, "hbd10": 10, "hbd12": 12}

_vp, _sz, _i32 = C.c_void_p, C.c_ssize_t, C.c_int32
DIST = C.CFUNCTYPE(C.c_uint32, _vp, _sz, _vp, _sz)
PUT = {0: C.CFUNCTYPE(None, _vp, _sz, _vp, _sz, _i32, _i32, _i32, _i32),
       1: C.CFUNCTYPE(None, _vp, _sz, _vp, _sz, _i32, _i32, _i32, _i32, _i32)}
PREP = {0: C.CFUNCTYPE(None, _vp, _vp, _sz, _i32, _i32, _i32, _i32),
        1: C.CFUNCTYPE(None, _vp, _vp, _sz, _i32, _i32, _i32, _i32, _i32)}
AVG = {0: C.CFUNCTYPE(None, _vp, _sz, _vp, _vp, _i32, _i32),
       1: C.CFUNCTYPE(None, _vp, _sz, _vp, _vp, _i32, _i32, _i32)}
FWD = C.CFUNCTYPE(_i32, _vp, _vp, _i32, _i32, _i32)
INV = C.CFUNCTYPE(_i32, _vp, _vp, _sz, _i32, _i32, _i32)
VOID = C.CFUNCTYPE(None)


def addr(name):
    """Address of the exported symbol `name`."""
    return C.cast(getattr(R.lib(), name), C.c_void_p).value


@functools.lru_cache(maxsize=None)
def fn(name, proto):
    """The exported function `name` behind a prototype of this module's own
    (the library object's cached attributes stay as the package declared them)."""
    return proto(addr(name))


def dist_name(metric, w, h, hbd):
    return f"rav1e_{'satd_' if metric else 'sad'}{w}x{h}{'_hbd' if hbd else ''}_hip"


def mc_name(op, mx, my, hbd):
    return f"rav1e_{op}_8tap_{FILTERS[mx]}_{FILTERS[my]}{'_16bpc' if hbd else ''}_hip"


# ---- inputs, shared by the CPU distinctness test and the GPU tests ----------
def _dtype(kind):
    return np.uint8 if kind == "u8" else np.uint16


DIST_AT = ((5, 7), (9, 3))  # (y, x) of the block in plane a / plane b


@functools.lru_cache(maxsize=None)
def dist_planes(kind, seed=0):
    """Two planes of different row lengths; read only."""
    rng = np.random.default_rng(7100 + 10 * seed + KINDS.index(kind))
    a = rng.integers(0, 1 << BD[kind], (140, 160)).astype(_dtype(kind))
    b = rng.integers(0, 1 << BD[kind], (144, 176)).astype(_dtype(kind))
    a.flags.writeable = b.flags.writeable = False
    return a, b


def dist_want(metric, kind, w, h, seed=0):
    a, b = dist_planes(kind, seed)
    (ay, ax), (by, bx) = DIST_AT
    return (O.get_satd if metric else O.get_sad)(a, ay, ax, b, by, bx, w, h)


MC_AT = (20, 36)        # (y, x): the 8-tap window crosses both saturated stripes
MC_AT_128 = (12, 20)
MC_FRACS = [(0, 0), (0, 9), (15, 0), (1, 15), (8, 8)]  # (mx, my) = (col, row) 1/16 pel
MC_FRAC_128 = (5, 11)


def mc_blocks(mx, my):
    """(w, h) per filter pair: 8-tap both ways, the 4-tap sets, mixed, w = 2."""
    return [(8, 8), (4, 4), (16, 4)] + ([(2, 4)] if (mx, my) == (0, 0) else [])


@functools.lru_cache(maxsize=None)
def mc_src(kind, seed=0):
    """Source with a saturated column and row stripe (clamps, u8 overshoot,
    src/mc.rs:244-245); blocks sit >= 3 from its top / left, >= 4 from its
    bottom / right.  Read only."""
    rng = np.random.default_rng(7200 + 10 * seed + KINDS.index(kind))
    bd = BD[kind]
    s = rng.integers(0, 1 << bd, (160, 168)).astype(_dtype(kind))
    stripe = np.array([0, 1, 0, 1, 1, 0, 1, 0]) * ((1 << bd) - 1)
    s[:, 40:48] = stripe
    s[24:32, :90] = stripe[:, None]
    s.flags.writeable = False
    return s


def mc_want(op, kind, w, h, at, frac, mx, my, seed=0):
    f = O.put_8tap if op == "put" else O.prep_8tap
    return f(mc_src(kind, seed), at[0], at[1], w, h, frac[0], frac[1], mx, my, bd=BD[kind])


def sentinel(shape, dtype):
    """A pattern no kernel output reproduces by accident: every byte non-zero."""
    dt = np.dtype(dtype)
    n = int(np.prod(shape))
    v = (np.arange(n, dtype=np.int64) * 37 + 11) % 251 + 1
    for k in range(1, dt.itemsize):
        v += 0x5A << (8 * k)
    return v.astype(dt).reshape(shape)


# ---- the calls: each returns what the shim wrote and whether it kept out of
# everything else ------------------------------------------------------------
def call_dist(metric, w, h, a, ay, ax, b, by, bx):
    hbd = O.hbd_of(a)
    f = fn(dist_name(metric, w, h, hbd), DIST)
    return f(O.ptr(a, ay * a.shape[1] + ax), a.shape[1] * a.itemsize,
             O.ptr(b, by * b.shape[1] + bx), b.shape[1] * b.itemsize)


def _strided_dst(w, h, dtype):
    ds = w + 9  # elements; never a source's row length (160, 168 or 176)
    d = sentinel((h + 5, ds), dtype)
    return d, d.copy(), ds


def _split(d, keep, w, h):
    """(block, outside untouched) of a destination made by _strided_dst."""
    blk = d[2:2 + h, 3:3 + w].copy()
    d[2:2 + h, 3:3 + w] = keep[2:2 + h, 3:3 + w]
    return blk, bool(np.array_equal(d, keep))


def call_put(f, src, at, w, h, frac, bd):
    """f: a put entry (by name or from rv_put_fn_get)."""
    d, keep, ds = _strided_dst(w, h, src.dtype)
    args = [O.ptr(d, 2 * ds + 3), ds * d.itemsize, O.ptr(src, at[0] * src.shape[1] + at[1]),
            src.shape[1] * src.itemsize, w, h, frac[0], frac[1]]
    f(*(args + [bd] if O.hbd_of(src) else args))
    return _split(d, keep, w, h)


def call_prep(f, src, at, w, h, frac, bd):
    t = sentinel(w * h + 16, np.int16)  # tmp is packed: guards before and after
    keep = t.copy()
    args = [O.ptr(t, 8), O.ptr(src, at[0] * src.shape[1] + at[1]), src.shape[1] * src.itemsize,
            w, h, frac[0], frac[1]]
    f(*(args + [bd] if O.hbd_of(src) else args))
    blk = t[8:8 + w * h].reshape(h, w).copy()
    t[8:8 + w * h] = keep[8:8 + w * h]
    return blk, bool(np.array_equal(t, keep))


def call_mc(op, kind, mx, my, w, h, at, frac, seed=0):
    hbd = kind != "u8"
    f = fn(mc_name(op, mx, my, hbd), (PUT if op == "put" else PREP)[hbd])
    return (call_put if op == "put" else call_prep)(f, mc_src(kind, seed), at, w, h, frac,
                                                    BD[kind])


def call_avg(kind, t1, t2):
    h, w = t1.shape
    hbd = kind != "u8"
    d, keep, ds = _strided_dst(w, h, _dtype(kind))
    args = [O.ptr(d, 2 * ds + 3), ds * d.itemsize, O.ptr(t1), O.ptr(t2), w, h]
    fn("rav1e_avg_16bpc_hip" if hbd else "rav1e_avg_hip", AVG[hbd])(
        *(args + [BD[kind]] if hbd else args))
    return _split(d, keep, w, h)


def tx_wh(s):
    return 1 << O.TX_W_LOG2[s], 1 << O.TX_H_LOG2[s]


def call_fwd(res, s, t, bd):
    """(return code, coefficients, guards and -- on an error -- output untouched)"""
    w, h = tx_wh(s)
    co = sentinel(w * h + 16, np.int32)
    keep = co.copy()
    res = np.ascontiguousarray(res, dtype=np.int16)
    rc = fn("rav1e_fwd_txfm_hip", FWD)(O.ptr(res), O.ptr(co, 8), s, t, bd)
    out = co[8:8 + w * h].copy()
    if rc == R.RV_OK:
        co[8:8 + w * h] = keep[8:8 + w * h]
    return rc, out, bool(np.array_equal(co, keep))


def call_inv(co, blk, s, t, bd):
    """Adds into a copy of blk placed in a wider sentinel array: (return code,
    block afterwards, outside untouched)."""
    w, h = tx_wh(s)
    d, keep, ds = _strided_dst(w, h, blk.dtype)
    d[2:2 + h, 3:3 + w] = keep[2:2 + h, 3:3 + w] = blk
    co = np.ascontiguousarray(co, dtype=np.int32)
    rc = fn("rav1e_inv_txfm_add_hip", INV)(O.ptr(co), O.ptr(d, 2 * ds + 3), ds * d.itemsize,
                                           s, t, bd)
    out, clean = _split(d, keep, w, h)
    return rc, out, clean


def release():
    fn("rv_shims_release", VOID)()


# =========================== CPU: addresses only =============================
def test_dist_dispatch_binds_every_size_to_its_symbol():
    L = R.lib()
    for get, metric in ((L.rv_sad_fn, 0), (L.rv_satd_fn, 1)):
        for hbd in (0, 1):
            for idx in range(22):
                w, h = R.BlockSize(idx).width(), R.BlockSize(idx).height()
                want = addr(dist_name(metric, w, h, hbd))
                assert want and get(HIP, idx, hbd) == want, (metric, hbd, idx)
                assert get(HIP, idx + 32, hbd) == want, (metric, hbd, idx)  # to_index: & 31
            for idx in range(22, 32):
                assert get(HIP, idx, hbd) is None, (metric, hbd, idx)
            for level in range(-1, 7):
                if level != HIP:
                    for idx in range(64):
                        assert get(level, idx, hbd) is None, (metric, level, idx)
    # 88 different functions
    assert len({addr(dist_name(m, w, h, b)) for m in (0, 1) for b in (0, 1)
                for w, h in SIZES}) == 88


def test_put_dispatch_binds_every_filter_pair_to_its_symbol():
    L = R.lib()
    for mx, my in PAIRS:
        want = addr(mc_name("put", mx, my, 0))
        assert want and L.rv_put_fn_get(HIP, mx, my) == want, (mx, my)
        for level in range(-1, 7):
            if level != HIP:
                assert L.rv_put_fn_get(level, mx, my) is None
    assert len({addr(mc_name(op, mx, my, b)) for op in ("put", "prep") for b in (0, 1)
                for mx, my in PAIRS}) == 64


@pytest.mark.parametrize("kind", KINDS)
def test_inputs_cannot_hide_a_wrong_binding(kind):
    """Oracle only, on the GPU tests' own arrays, positions and fractions."""
    for metric in (0, 1):
        vals = [dist_want(metric, kind, w, h) for w, h in SIZES]
        assert len(set(vals)) == 22, (metric, vals)
    cases = [(8, 8, MC_AT, fr) for fr in MC_FRACS if fr[0] and fr[1]]
    cases.append((128, 128, MC_AT_128, MC_FRAC_128))
    for op in ("put", "prep"):
        for w, h, at, fr in cases:
            outs = {mc_want(op, kind, w, h, at, fr, mx, my).tobytes() for mx, my in PAIRS}
            assert len(outs) == 16, (op, w, h, fr)


# ================================ GPU ========================================
@pytest.fixture
def shims():
    """Device 0 and a calling thread without a staging context: the first call
    starts at the initial 64 KiB and grows from there."""
    R.require_device(0)
    release()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_all_distortion_entries_vs_oracle(shims, kind):
    """22 sizes x SAD / SATD by name; u16 planes with byte strides hold 10-bit
    and 12-bit values.  128x128 comes after fifteen smaller sizes and before six
    more: for u16 its 2 x 32 KiB outgrow the context in mid-sequence."""
    a, b = dist_planes(kind)
    (ay, ax), (by, bx) = DIST_AT
    for w, h in SIZES:
        for metric in (0, 1):
            got = call_dist(metric, w, h, a, ay, ax, b, by, bx)
            assert got == dist_want(metric, kind, w, h), (metric, w, h)


@pytest.mark.gpu
def test_hbd_distortion_max_residual_12bit():
    """|diff| = 4095 over a whole 64x64: the 8x8 Hadamard reaches 64 * 4095
    (> i16); the declared ground truth (emulate_gen = 0) does not wrap."""
    R.require_device(0)
    a = np.zeros((70, 80), np.uint16)
    b = np.zeros((72, 96), np.uint16)
    a[3:67, 5:69] = 4095
    b[:, :] = 4095
    b[4:68, 9:73] = 0
    assert call_dist(0, 64, 64, a, 3, 5, b, 4, 9) == 64 * 64 * 4095
    got = call_dist(1, 64, 64, a, 3, 5, b, 4, 9)
    assert got == O.get_satd(a, 3, 5, b, 4, 9, 64, 64, 0)
    assert got != O.get_satd(a, 3, 5, b, 4, 9, 64, 64, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_all_mc_entries_vs_oracle(shims, kind):
    """16 filter pairs x put / prep by name, over the block sizes that select
    the 8-tap and the 4-tap sets and the five fraction classes."""
    for mx, my in PAIRS:
        for op in ("put", "prep"):
            for w, h in mc_blocks(mx, my):
                for fr in MC_FRACS:
                    got, clean = call_mc(op, kind, mx, my, w, h, MC_AT, fr)
                    np.testing.assert_array_equal(
                        got, mc_want(op, kind, w, h, MC_AT, fr, mx, my),
                        err_msg=str((op, mx, my, w, h, fr)))
                    assert clean, (op, mx, my, w, h, fr)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_mc_context_growth_between_small_calls(shims, kind):
    """4x4, 128x128, 4x4 back to back on a fresh context.  A u16 128x128 call
    stages 135 x 135 x 2 + 128 x 128 x 2 bytes, more than the initial 64 KiB,
    so the context frees and reallocates its buffers between the calls (the u8
    calls fit and run the same sequence without growing)."""
    for op, (mx, my) in (("put", (2, 1)), ("prep", (1, 2))):
        release()
        for w, h, at, fr in ((4, 4, MC_AT, (3, 7)), (128, 128, MC_AT_128, MC_FRAC_128),
                             (4, 4, MC_AT, (12, 5))):
            got, clean = call_mc(op, kind, mx, my, w, h, at, fr)
            np.testing.assert_array_equal(got, mc_want(op, kind, w, h, at, fr, mx, my),
                                          err_msg=str((op, w, h)))
            assert clean, (op, w, h)


def avg_inputs(kind, w, h):
    """Two different prep outputs, and a pair that reaches both clamp ends."""
    t1 = mc_want("prep", kind, w, h, MC_AT, (6, 10), 0, 0)
    t2 = mc_want("prep", kind, w, h, (MC_AT[0] + 7, MC_AT[1] + 5), (0, 12), 2, 1)
    rng = np.random.default_rng(7300 + w + h)
    c1 = rng.integers(-32768, 32768, (h, w)).astype(np.int16)
    c2 = rng.integers(-32768, 32768, (h, w)).astype(np.int16)
    c1[0], c2[0] = 32767, 32767
    c1[1], c2[1] = -32768, -32768
    return (t1, t2), (c1, c2)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_avg_entries_vs_oracle(shims, kind):
    bd = BD[kind]
    for w, h in ((4, 4), (8, 16), (64, 64)):
        prep, clamp = avg_inputs(kind, w, h)
        assert not np.array_equal(prep[0], prep[1])
        for t1, t2 in (prep, clamp):
            want = O.mc_avg(t1, t2, bd=bd, hbd=int(kind != "u8"))
            got, clean = call_avg(kind, t1, t2)
            np.testing.assert_array_equal(got, want, err_msg=str((w, h)))
            assert clean, (w, h)
        assert want.min() == 0 and want.max() == (1 << bd) - 1  # both clamp ends reached


@pytest.mark.gpu
def test_put_table_pointers_compute_what_their_names_do(shims):
    src = mc_src("u8")
    for mx, my in PAIRS:
        f = PUT[0](R.lib().rv_put_fn_get(HIP, mx, my))
        for w, h, fr in ((8, 8, (1, 15)), (16, 4, (8, 8))):
            got, clean = call_put(f, src, MC_AT, w, h, fr, 8)
            np.testing.assert_array_equal(got, mc_want("put", "u8", w, h, MC_AT, fr, mx, my),
                                          err_msg=str((mx, my, w, h)))
            assert clean


# ---- transforms -------------------------------------------------------------
def _oracle_fwd_ok(s, t):
    w, h = tx_wh(s)
    return O.fwd_txfm2d(np.zeros(w * h, np.int16), s, t, 8) is not None


def _oracle_inv_ok(s, t):
    w, h = tx_wh(s)
    return O.inv_txfm2d_add(np.zeros(min(w, 32) * min(h, 32), np.int32),
                            np.zeros((h, w), np.uint8), s, t, 8) is not None


def tx_grid(bd, ok):
    """bd 8: all 19 x 16 pairs.  bd 10 / 12: per size DCT_DCT and one type of
    the ADST family (types 1..8), a supported one where the size has any, a
    different one from size to size."""
    if bd == 8:
        return [(s, t) for s in range(19) for t in range(16)]
    grid = []
    for s in range(19):
        fam = [1 + (s + k) % 8 for k in range(8)]
        grid += [(s, 0), (s, next((t for t in fam if ok(s, t)), fam[0]))]
    return grid


@pytest.mark.gpu
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_fwd_txfm_entry_vs_oracle(shims, bd):
    rng = np.random.default_rng(7400 + bd)
    m = (1 << bd) - 1
    for s, t in tx_grid(bd, _oracle_fwd_ok):
        w, h = tx_wh(s)
        blocks = [np.full((h, w), m, np.int16), np.full((h, w), -m, np.int16),
                  rng.integers(-m, m + 1, (h, w)).astype(np.int16)]
        if not _oracle_fwd_ok(s, t):
            rc, _, untouched = call_fwd(blocks[2], s, t, bd)
            assert rc == R.RV_ENOTSUP and untouched, (s, t)
            continue
        for k, res in enumerate(blocks):
            rc, got, clean = call_fwd(res, s, t, bd)
            assert rc == R.RV_OK and clean, (s, t, k)
            np.testing.assert_array_equal(got, O.fwd_txfm2d(res, s, t, bd),
                                          err_msg=str((s, t, bd, k)))


@pytest.mark.gpu
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_inv_txfm_add_entry_vs_oracle(shims, bd):
    rng = np.random.default_rng(7500 + bd)
    dt = np.uint8 if bd == 8 else np.uint16
    for s, t in tx_grid(bd, _oracle_inv_ok):
        w, h = tx_wh(s)
        area = min(w, 32) * min(h, 32)
        coeffs = [rng.integers(-(1 << 20), 1 << 20, area).astype(np.int32),  # the clamps
                  rng.integers(-3000, 3000, area).astype(np.int32)]
        blk = rng.integers(0, 1 << bd, (h, w)).astype(dt)
        if not _oracle_inv_ok(s, t):
            rc, got, clean = call_inv(coeffs[1], blk, s, t, bd)
            assert rc == R.RV_ENOTSUP and clean, (s, t)
            np.testing.assert_array_equal(got, blk)
            continue
        for k, co in enumerate(coeffs):
            rc, got, clean = call_inv(co, blk, s, t, bd)
            assert rc == R.RV_OK and clean, (s, t, k)
            np.testing.assert_array_equal(got, O.inv_txfm2d_add(co, blk, s, t, bd),
                                          err_msg=str((s, t, bd, k)))


@pytest.mark.gpu
def test_txfm_entries_reject_and_recover(shims):
    """tx_size -1 / 19: RV_EINVAL.  An unsupported pair returns RV_ENOTSUP with
    its staging copy still in flight on the context's stream: the very next
    call, of either entry, must still be right."""
    rng = np.random.default_rng(7600)
    res = rng.integers(-255, 256, (8, 8)).astype(np.int16)
    blk = rng.integers(0, 256, (8, 8)).astype(np.uint8)
    co = rng.integers(-3000, 3000, 64).astype(np.int32)
    for s in (-1, 19):
        out, d = sentinel(64, np.int32), blk.copy()
        assert fn("rav1e_fwd_txfm_hip", FWD)(O.ptr(res), O.ptr(out), s, 0, 8) == R.RV_EINVAL
        assert fn("rav1e_inv_txfm_add_hip", INV)(O.ptr(co), O.ptr(d), 8, s, 0, 8) == R.RV_EINVAL
        assert np.array_equal(out, sentinel(64, np.int32)) and np.array_equal(d, blk)
    bad_fwd = next((s, t) for s in (4, 3) for t in range(16) if not _oracle_fwd_ok(s, t))
    bad_inv = next((s, t) for s in (4, 3) for t in range(16) if not _oracle_inv_ok(s, t))
    big = rng.integers(-255, 256, tx_wh(bad_fwd[0])[::-1]).astype(np.int16)
    for _ in range(2):
        assert call_fwd(big, *bad_fwd, 8)[0] == R.RV_ENOTSUP
        rc, got, clean = call_fwd(res, 1, 0, 8)
        assert rc == R.RV_OK and clean
        np.testing.assert_array_equal(got, O.fwd_txfm2d(res, 1, 0, 8))
        w, h = tx_wh(bad_inv[0])
        assert call_inv(np.ones(min(w, 32) * min(h, 32), np.int32), np.zeros((h, w), np.uint8),
                        *bad_inv, 8)[0] == R.RV_ENOTSUP
        rc, got, clean = call_inv(co, blk, 1, 0, 8)
        assert rc == R.RV_OK and clean
        np.testing.assert_array_equal(got, O.inv_txfm2d_add(co, blk, 1, 0, 8))
    # ... also when that next call outgrows a fresh context, which then frees the
    # buffers the abandoned copy uses
    a, b = dist_planes("hbd12")
    (ay, ax), (by, bx) = DIST_AT
    release()
    assert call_fwd(big, *bad_fwd, 8)[0] == R.RV_ENOTSUP
    assert call_dist(1, 128, 128, a, ay, ax, b, by, bx) == dist_want(1, "hbd12", 128, 128)


# ---- lifecycle --------------------------------------------------------------
def _probe():
    """One call of each family; None when all are right."""
    a, b = dist_planes("hbd10")
    (ay, ax), (by, bx) = DIST_AT
    if call_dist(1, 16, 8, a, ay, ax, b, by, bx) != dist_want(1, "hbd10", 16, 8):
        return "satd"
    got, clean = call_mc("put", "u8", 2, 0, 8, 8, MC_AT, (8, 8))
    if not clean or not np.array_equal(got, mc_want("put", "u8", 8, 8, MC_AT, (8, 8), 2, 0)):
        return "put"
    return None


@pytest.mark.gpu
def test_release_and_shutdown_then_call_again(shims):
    assert _probe() is None
    release()
    assert _probe() is None  # a new context, made on demand
    release()
    release()                # nothing to release: a no-op
    assert _probe() is None
    # no other thread holds a context here (the workers of the thread test
    # release theirs before they return): shutdown frees this thread's only
    fn("rv_shims_shutdown", VOID)()
    assert _probe() is None
    fn("rv_shims_shutdown", VOID)()
    release()
    assert _probe() is None


# ---- threads ----------------------------------------------------------------
N_THREADS = 8
_TH_SIZES = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (128, 128), (16, 64), (64, 16)]
_TH_TX = [(0, 0), (1, 3), (2, 0), (3, 0), (4, 0), (7, 2), (13, 1), (16, 0)]


def thread_ops(t):
    """About 40 (call, expected) pairs for worker t, on arrays of its own, with
    the sizes rotated by t so every worker's context grows at another moment.
    Runs on the main thread: the oracle is consulted before the workers start."""
    kind = KINDS[t % 3]
    bd = BD[kind]
    a, b = dist_planes(kind, seed=1 + t)
    (ay, ax), (by, bx) = DIST_AT
    rng = np.random.default_rng(7700 + t)
    ops = []
    for k in range(8):
        w, h = _TH_SIZES[(k + t) % 8]
        for metric in (0, 1):
            ops.append((f"dist{metric} {w}x{h}",
                        lambda metric=metric, w=w, h=h: (call_dist(metric, w, h, a, ay, ax, b,
                                                                   by, bx), True),
                        (O.get_satd if metric else O.get_sad)(a, ay, ax, b, by, bx, w, h)))
        mx, my = PAIRS[(3 * k + t) % 16]
        at = MC_AT_128 if max(w, h) == 128 else MC_AT
        fr = MC_FRACS[1 + (k + t) % 4] if (w, h) != (128, 128) else MC_FRAC_128
        op = ("put", "prep")[(k + t) % 2]
        ops.append((f"{op} {w}x{h}",
                    lambda op=op, mx=mx, my=my, w=w, h=h, at=at, fr=fr:
                    call_mc(op, kind, mx, my, w, h, at, fr, seed=1 + t),
                    mc_want(op, kind, w, h, at, fr, mx, my, seed=1 + t)))
        s, ty = _TH_TX[(k + 2 * t) % 8]
        tw, th = tx_wh(s)
        res = rng.integers(-(1 << bd) + 1, 1 << bd, (th, tw)).astype(np.int16)
        ops.append((f"fwd {s}", lambda res=res, s=s, ty=ty: call_fwd(res, s, ty, bd)[1:],
                    O.fwd_txfm2d(res, s, ty, bd)))
        co = rng.integers(-3000, 3000, min(tw, 32) * min(th, 32)).astype(np.int32)
        blk = rng.integers(0, 1 << bd, (th, tw)).astype(_dtype(kind))
        ops.append((f"inv {s}", lambda co=co, blk=blk, s=s, ty=ty: call_inv(co, blk, s, ty, bd)[1:],
                    O.inv_txfm2d_add(co, blk, s, ty, bd)))
    for w, h in ((4, 4), (64, 64)):
        t1 = rng.integers(-2000, 20000, (h, w)).astype(np.int16)
        t2 = rng.integers(-2000, 20000, (h, w)).astype(np.int16)
        ops.append((f"avg {w}x{h}", lambda t1=t1, t2=t2: call_avg(kind, t1, t2),
                    O.mc_avg(t1, t2, bd=bd, hbd=int(kind != "u8"))))
    order = np.random.default_rng(7800 + t).permutation(len(ops))
    return [ops[i] for i in order]


@pytest.mark.gpu
def test_eight_threads_call_the_shims_at_once(shims):
    """The header's contract: thread-local contexts keep the calls reentrant
    across worker threads.  One pass, in one process; ctypes drops the GIL
    around every call."""
    plans = [thread_ops(t) for t in range(N_THREADS)]
    assert all(36 <= len(p) <= 48 for p in plans)
    for t, p in enumerate(plans):
        for name, _, want in p:
            assert want is not None, (t, name)
    start = threading.Barrier(N_THREADS)
    bad, done = [], []

    def worker(t):
        try:
            start.wait(timeout=60)
            for name, call, want in plans[t]:
                got, clean = call()
                if not clean or not np.array_equal(got, want):
                    bad.append((t, name))
        except Exception as e:  # noqa: BLE001 -- reported by the main thread
            bad.append((t, repr(e)))
        finally:
            release()
            done.append(t)

    threads = [threading.Thread(target=worker, args=(t,), daemon=True) for t in range(N_THREADS)]
    for th in threads:
        th.start()
    deadline = time.monotonic() + 60  # reached only by a hang
    for th in threads:
        th.join(timeout=max(0.0, deadline - time.monotonic()))
    assert sorted(done) == list(range(N_THREADS)), f"workers still running: {done}"
    assert bad == []
    assert _probe() is None  # the main thread's own context is unaffected
