"""Reference-evaluated vectors for the coefficient bit counter
(tests/golden/ref_ec_rate.npz).

    python tools/refeval/gen_ec_rate_ref.py        (in the build container)

Runs the reference's own text through tools/refeval/rsinterp.py.  Beside what
gen_ec_ref.py binds (the Writer trait methods, lr_compute, update_cdf,
write_coeffs_lv_map and the context functions it calls), this binds

  src/ec.rs:187-222   impl StorageBackend for WriterBase<WriterCounter>
                      (store, stream_bytes), replacing the encoder's store
  src/ec.rs:366-388   frac_compute
  src/ec.rs:765-780   tell, tell_frac

Vectors:
  wr_ops / wr_state / wr_index: random operation streams (symbol_with_update
      on the default CDFs of random coefficient families of one of the four
      q contexts, bit, literal) into a fresh WriterBase<WriterCounter>;
      wr_state holds (rng, cnt, tell(), tell_frac()) of the fresh writer and
      after every operation (n_ops + 1 rows per stream);
      wr_ops rows: (0, q, cdf offset, cdf length, symbol), (2, bit, 0, 0, 0),
      (3, bits, value, 0, 0); wr_index rows: (first op, ops, first state row).
  blk_groups: for each of ref_ec.npz's five lv_cases (its lv_jobs / lv_coeffs
      are loaded, not stored again), one group per non-skip leaf -- the
      leaf's transform blocks of all planes in coding order -- priced from
      two CDF snapshots: write_coeffs_lv_map of the group's blocks into a
      fresh WriterCounter, the block contexts as the tile's sequential coding
      has them at that point, the CDFs a copy of the snapshot.  Rows: (case,
      first job, jobs, snapshot id, tell_frac delta), job indices relative
      to the case's first job; snapshot 0 = the case's lv_init_cdf, 1 = its
      last tile's lv_final_cdf (an adapted state).
"""
import io
import os
import sys
import time
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import gen_ec_ref as E  # noqa: E402
import gen_ec_tables as T  # noqa: E402
import gen_golden_ref as G  # noqa: E402
import rshost as H  # noqa: E402
import rsinterp as RI  # noqa: E402

OUT = os.path.join(E.ROOT, "tests", "golden", "ref_ec_rate.npz")
EC_REF = os.path.join(E.ROOT, "tests", "golden", "ref_ec.npz")


def make():
    I = E.make()
    ec = G.src_of(I, "ec.rs")
    # the counter's store / stream_bytes replace the encoder's
    I.define_impl("WriterBase", ec.impl("WriterBase",
                                        "impl StorageBackend for WriterBase<WriterCounter>"))
    I.globals.vars["WriterCounter"] = RI.StructType("WriterCounter")
    return I


def new_counter():
    return RI.Struct("WriterBase", {"rng": RI.TInt(0x8000, "u16"), "cnt": RI.TInt(-9, "i16"),
                                    "fake_bits_frac": RI.TInt(0, "u32"),
                                    "s": RI.Struct("WriterCounter",
                                                   {"bytes": RI.TInt(0, "usize")})})


def state_of(I, w):
    return (int(w.rng), int(w.cnt), int(E.call(I, w, "tell")), int(E.call(I, w, "tell_frac")))


# ------------------------------------------------------------- writer vectors
def gen_writer(I, rng, out, nstreams=24):
    fams = [(n, e) for n, _, shape, e in T.FAMILIES]
    offs = dict(zip([f[0] for f in T.FAMILIES], E._fam_offsets()))
    tables = {}
    ops_all, states, idx = [], [], []
    for si in range(nstreams):
        q = si % 4
        if q not in tables:
            tables[q] = E.flatten_cdfs(E.cdf_fields(q))
        state = list(tables[q])
        w = new_counter()
        n = int(rng.integers(300, 420))
        idx.append((len(ops_all), n, len(states)))
        states.append(state_of(I, w))
        for _ in range(n):
            k = int(rng.integers(0, 10))
            if k < 6:
                nm, e = fams[int(rng.integers(0, len(fams)))]
                o = offs[nm] + int(rng.integers(0, E._fam_count(nm))) * e
                s = int(min(e - 2, rng.geometric(0.45) - 1))
                cdf = [RI.TInt(v, "u16") for v in state[o:o + e]]
                E.call(I, w, "symbol_with_update", RI.TInt(s, "u32"), cdf)
                state[o:o + e] = [int(v) for v in cdf]
                ops_all.append((0, q, o, e, s))
            elif k < 8:
                b = int(rng.integers(0, 2))
                E.call(I, w, "bit", RI.TInt(b, "u16"))
                ops_all.append((2, b, 0, 0, 0))
            else:
                nb = int(rng.integers(1, 17))
                v = int(rng.integers(0, 1 << nb))
                E.call(I, w, "literal", RI.TInt(nb, "u8"), RI.TInt(v, "u32"))
                ops_all.append((3, nb, v, 0, 0))
            states.append(state_of(I, w))
        print("writer stream %d: %d ops, %d bytes" % (si, n, int(w.s.bytes)), flush=True)
    out["wr_ops"] = np.array(ops_all, np.int32)
    out["wr_state"] = np.array(states, np.int64)
    out["wr_index"] = np.array(idx, np.int64)


# -------------------------------------------------------------- block vectors
def cdf_struct(template, flat):
    """A CDFContext whose fields have template's shapes and flat's values
    (gen_ec_ref.FLAT_ORDER)."""
    it = iter(int(v) for v in flat)

    def fill(v):
        return [fill(x) for x in v] if isinstance(v, list) else E.u16(next(it))
    f = {n: fill(template[n]) for n in E.FLAT_ORDER}
    assert next(it, None) is None
    return RI.Struct("CDFContext", f)


def new_bc():
    return RI.Struct("BlockContext", {
        "above_coeff_context": [[RI.TInt(0, "u8")] * 1024 for _ in range(3)],
        "left_coeff_context": [[RI.TInt(0, "u8")] * 16 for _ in range(3)],
        "left_partition_context": [RI.TInt(0, "u8")] * 8,
        "left_tx_context": [RI.TInt(0, "u8")] * 16})


def bc_save(bc):
    return ([list(x) for x in bc.above_coeff_context], [list(x) for x in bc.left_coeff_context])


def bc_restore(bc, s):
    bc.above_coeff_context = [list(x) for x in s[0]]
    bc.left_coeff_context = [list(x) for x in s[1]]


def gen_blocks(I, out):
    ref = np.load(EC_REF)
    jobs_all, co = ref["lv_jobs"], ref["lv_coeffs"]
    init, fin = ref["lv_init_cdf"], ref["lv_final_cdf"]
    templates = {}
    rows = []
    t0 = 0
    for ci, (cid, j0, nj, xdec, ydec, q, ntiles) in enumerate(ref["lv_cases"].tolist()):
        if q not in templates:
            templates[q] = E.cdf_fields(q)
        snaps = [init[ci], fin[t0 + ntiles - 1]]
        t0 += ntiles
        jobs = jobs_all[j0:j0 + nj].tolist()
        bc = None
        j = 0
        while j < nj:
            kind, p, bx, by, tx, txt, inter, bwl, bhl, off = jobs[j]
            if kind == 3:
                bc = new_bc()
            elif kind == 2:
                E.call(I, bc, "reset_left_contexts")
            elif kind == 1:
                E.call(I, bc, "reset_skip_context", E.tile_bo(bx, by),
                       H.BlockSizeV(E.BLOCK_OF_TX[bwl - 2]), RI.TInt(xdec, "usize"),
                       RI.TInt(ydec, "usize"))
            if kind != 0:
                j += 1
                continue
            assert p == 0
            e = j + 1
            while e < nj and jobs[e][0] == 0 and jobs[e][1] != 0:
                e += 1
            saved = bc_save(bc)
            for sid, snap in enumerate(snaps):
                bc_restore(bc, saved)
                cw_obj = RI.Struct("ContextWriter", {"bc": bc,
                                                     "fc": cdf_struct(templates[q], snap)})
                w = new_counter()
                before = int(E.call(I, w, "tell_frac"))
                for k in range(j, e):
                    _, p, bx, by, tx, txt, inter, bwl, bhl, off = jobs[k]
                    xd, yd = (xdec, ydec) if p else (0, 0)
                    cwid = min(4 << tx, 32)
                    cin = [RI.TInt(int(v), "i32") for v in co[off:off + cwid * cwid]]
                    mode = RI.TInt(E.NEARESTMV if inter else 0, "usize")
                    E.call(I, cw_obj, "write_coeffs_lv_map", w, RI.TInt(p, "usize"),
                           E.tile_bo(bx, by), RI.Slice(cin), mode, E.TxSq(tx),
                           RI.TInt(txt, "usize"), H.BlockSizeV(E.BLOCK_OF_TX[bwl - 2]),
                           RI.TInt(xd, "usize"), RI.TInt(yd, "usize"), True)
                rows.append((ci, j, e - j, sid, int(E.call(I, w, "tell_frac")) - before))
            j = e
        print("case %d: %d groups so far" % (ci, len(rows) // 2), flush=True)
    out["blk_groups"] = np.array(rows, np.int64)


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps, so that the same
    vectors give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", (1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue())


def main():
    t0 = time.time()
    rng = np.random.default_rng(0xEC7A)
    out = {}
    gen_writer(make(), rng, out)
    gen_blocks(make(), out)
    save_npz(OUT, out)
    print("wrote %s (%d bytes) in %.0f s" % (OUT, os.path.getsize(OUT), time.time() - t0))


if __name__ == "__main__":
    main()
