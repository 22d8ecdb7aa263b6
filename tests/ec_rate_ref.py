"""A plain-Python restatement of the reference's counting writer,
WriterBase<WriterCounter> (src/ec.rs): store (:187-205) over lr_compute
(:339-355), symbol_with_update with update_cdf (:540-551, 891-905), bit /
literal (:501-516), tell / tell_frac / frac_compute (:366-388, 765-780).
No ctypes: tests/test_ec_rate.py pins it to the reference-evaluated writer
vectors and uses it to read them."""

EC_PROB_SHIFT = 6
EC_MIN_PROB = 4
OD_BITRES = 3


class Counter:
    def __init__(self, rng=0x8000, cnt=-9, nbytes=0):
        self.rng, self.cnt, self.bytes = rng, cnt, nbytes

    def store(self, fl, fh, nms):
        r = self.rng
        if fl < 32768:
            u = (((r >> 8) * (fl >> EC_PROB_SHIFT)) >> (7 - EC_PROB_SHIFT)) + EC_MIN_PROB * nms
            v = (((r >> 8) * (fh >> EC_PROB_SHIFT)) >> (7 - EC_PROB_SHIFT)) + \
                EC_MIN_PROB * (nms - 1)
            r = (u - v) & 0xFFFF
        else:
            r = (r - ((((r >> 8) * (fh >> EC_PROB_SHIFT)) >> (7 - EC_PROB_SHIFT)) +
                      EC_MIN_PROB * (nms - 1))) & 0xFFFF
        d = 16 - r.bit_length()
        c = self.cnt
        s = c + d
        if s >= 0:
            c += 16
            if s >= 8:
                self.bytes += 1
                c -= 8
            self.bytes += 1
            s = c + d - 24
        self.rng = (r << d) & 0xFFFF
        self.cnt = s

    def symbol(self, s, cdf):
        """cdf: the nsymbs entries without the counter."""
        self.store(cdf[s - 1] if s > 0 else 32768, cdf[s], len(cdf) - s)

    def symbol_with_update(self, s, cdf):
        """cdf: a mutable sequence of nsymbs + 1 entries, adapted in place."""
        nsymbs = len(cdf) - 1
        self.symbol(s, cdf[:nsymbs])
        update_cdf(cdf, s)

    def bit(self, b):
        self.symbol(1 if b == 1 else 0, [16384, 0])

    def literal(self, bits, s):
        for k in reversed(range(bits)):
            self.bit((s >> k) & 1)

    def tell(self):
        return (self.bytes * 8 + self.cnt + 10) & 0xFFFFFFFF

    def tell_frac(self):
        return frac_compute(self.tell(), self.rng)


def update_cdf(cdf, val):
    nsymbs = len(cdf) - 1
    rate = 3 + min(nsymbs >> 1, 2) + (int(cdf[nsymbs]) >> 4)
    cdf[nsymbs] += 1 - (int(cdf[nsymbs]) >> 5)
    for i in range(nsymbs - 1):
        v = int(cdf[i])
        cdf[i] = v - (v >> rate) if i >= val else v + ((32768 - v) >> rate)


def frac_compute(nbits_total, rng):
    nbits = nbits_total << OD_BITRES
    l = 0
    for _ in range(OD_BITRES):
        rng = (rng * rng) >> 15
        b = rng >> 16
        l = (l << 1) | b
        rng >>= b
    return (nbits - l) & 0xFFFFFFFF


def ops_to_tokens(ops):
    """Writer-vector ops as rv_ec tokens (literal: its raw bits, MSB first);
    also the token index at which every op starts (n_ops + 1 entries)."""
    tok, start = [], []
    for kind, a, b, c, d in ops:
        start.append(len(tok))
        if kind == 0:
            tok.append(int(b) | int(c) << 13 | int(d) << 18)
        elif kind == 2:
            tok.append(0x80000000 | int(a))
        else:
            tok += [0x80000000 | ((int(b) >> k) & 1) for k in reversed(range(int(a)))]
    start.append(len(tok))
    return tok, start
