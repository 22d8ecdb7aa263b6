"""bench.py --dump-outputs: the arrays are float32 / float64, carry the
integers they hold exactly, and a reconstruction above the sample cap is
cut to the same seeded sample on every run.  Host code: no GPU."""
import os

import numpy as np


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_is_exact_and_repeatable(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_RECON_SAMPLES", 1000)
    rng = np.random.default_rng(3)
    words = rng.integers(0, 2 ** 64, 77, dtype=np.uint64)
    words[:2] = (0, 2 ** 64 - 1)
    ent = [123456, 8, 0xDEADBEEFCAFEF00D, 101, 2 ** 40 + 1]
    small = rng.integers(0, 256, 1000).astype(np.uint8)  # at the cap: whole
    big = rng.integers(0, 1024, 4001).astype(np.uint16)  # above: sampled
    a, b, c = (str(tmp_path / n) for n in "abc")
    bench.dump_outputs(a, words, ent, small)
    bench.dump_outputs(b, words, ent, big)
    bench.dump_outputs(c, words, None, big)
    A, B, Cc = _load(a), _load(b), _load(c)
    assert sorted(A) == sorted(B) == ["entropy", "recon", "result_words"]
    assert sorted(Cc) == ["recon", "result_words"]  # no F8: no entropy array
    w = A["result_words"]
    assert w.dtype == np.float64 and w.shape == (77, 2)
    back = w[:, 0].astype(np.uint64) | (w[:, 1].astype(np.uint64) << np.uint64(32))
    assert (back == words).all()
    e = A["entropy"]
    assert e.dtype == np.float64
    assert [int(v) for v in e] == [ent[0], ent[1], ent[2] & 0xFFFFFFFF, ent[2] >> 32, ent[3], ent[4]]
    assert A["recon"].dtype == np.float32 and (A["recon"] == small).all()
    r = B["recon"]
    assert r.dtype == np.float32 and r.shape == (1000,)
    assert (r == Cc["recon"]).all()  # the same sample every time
    idx = np.sort(np.random.default_rng(0).choice(big.size, 1000, replace=False))
    assert (r == big[idx]).all()
    # the result words above their cap: the same rule
    monkeypatch.setattr(bench, "DUMP_WORD_SAMPLES", 50)
    d = str(tmp_path / "d")
    bench.dump_outputs(d, words, None, small)
    w = _load(d)["result_words"]
    idx = np.sort(np.random.default_rng(0).choice(words.size, 50, replace=False))
    assert w.shape == (50, 2)
    assert ((w[:, 0].astype(np.uint64) | (w[:, 1].astype(np.uint64) << np.uint64(32))) == words[idx]).all()
    # the caps as shipped keep a dump under 64 MB
    monkeypatch.undo()
    assert 16 * bench.DUMP_WORD_SAMPLES + 4 * bench.DUMP_RECON_SAMPLES + 48 + 3 * 128 < 64e6
