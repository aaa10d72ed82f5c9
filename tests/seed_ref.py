"""The seeding kernel's scheme (chiron_seed_reads, csrc/seed.hip) restated in numpy, pass by pass, and the hand cases the CPU
and the GPU tests share.

chiron_amd.map.vote is the definition: it sorts the hits.  The kernel sorts nothing.  It counts: a dense counter per bin and
strand, the winner and the far maximum by replaying the hits against the counters, the median by a 512-counter histogram of
delta over the winning two bins and a prefix sum, and the hit within that delta by counting read positions, 256 to a counter,
then one flag a position.  `Workgroup` is that scheme with the kernel's arithmetic (the offset that makes bin indices
non-negative, the packed (score, -bin) key, the pairwise prefix sum of rank_find) and, like a workgroup of the kernel, it keeps
ONE counter array over all the reads it takes and clears it by replaying the hits.  test_seed_cpu.py checks it against `vote`.

`lookup` and `roll` are the kernel's index search and rolling k-mer loop in plain Python, checked there against numpy.

long_read_cases() is the kernel at the read lengths it is made for, up to the 131072 bases it accepts.  Out of scope: genomes near
SEED_MAX_GENOME.  An index of 2^31 positions is not a test-sized input.
"""
import numpy as np

import assess_ref
import map_ref

K = 15
BIN = 256
SHIFT = 8
THREADS = 256
TOP = 0x7FFFFFFF


def lookup(val, v):
    """(first entry, count) of the run of v in sorted val: a lower bound, a gallop to the end of the run, a bisection."""
    n = len(val)
    lo, hi = 0, n
    while lo < hi:
        mid = lo + ((hi - lo) >> 1)
        if val[mid] < v:
            lo = mid + 1
        else:
            hi = mid
    if lo >= n or val[lo] != v:
        return lo, 0
    e = 1
    while lo + e < n and val[lo + e] == v:
        e <<= 1
    a, b = lo + (e >> 1) + 1, min(lo + e, n)
    while a < b:
        mid = a + ((b - a) >> 1)
        if val[mid] == v:
            a = mid + 1
        else:
            b = mid
    return lo, a - lo


def roll(codes, p0, p1):
    """The k-mers at read positions p0 .. p1 - 1 as one thread of the kernel rolls them: [(p, forward value, value of the reverse
    complement, valid)]."""
    out = []
    fwd = rev = run = 0
    for i in range(p0, p1 + K - 1 if p0 < p1 else p0):
        c = int(codes[i])
        run = 0 if c > 3 else run + 1
        fwd = ((fwd << 2) | (c & 3)) & 0x3FFFFFFF
        rev = (rev >> 2) | ((3 - (c & 3)) << 28)
        if i >= p0 + K - 1:
            out.append((i - (K - 1), fwd, rev, run >= K))
    return out


def kmer_values(codes):
    """(forward value, reverse-complement value, valid) of every k-mer position, vectorised."""
    nk = max(len(codes) - K + 1, 0)
    c = codes.astype(np.int64)
    fwd, rev, bad = np.zeros(nk, np.int64), np.zeros(nk, np.int64), np.zeros(nk, bool)
    for t in range(K):
        piece = c[t:t + nk]
        bad |= piece > 3
        fwd |= (piece & 3) << (2 * (K - 1 - t))
        rev |= (3 - (piece & 3)) << (2 * t)
    return fwd, rev, ~bad


def rank_find(h, rank):
    """The kernel's rank_find over 512 counters, two a thread: (i, rest) with sum(h[:i]) <= rank < sum(h[:i + 1]), or (-1, 0)."""
    h = np.asarray(h, np.int64)
    assert len(h) == 2 * THREADS
    a, b = h[0::2], h[1::2]
    incl = np.cumsum(a + b)
    excl = incl - (a + b)
    t = np.nonzero((excl <= rank) & (rank < incl))[0]
    if len(t) == 0:
        return -1, 0
    t = int(t[0])
    if rank < excl[t] + a[t]:
        return 2 * t, int(rank - excl[t])
    return 2 * t + 1, int(rank - excl[t] - a[t])


class Workgroup:
    """One workgroup of the kernel: its counters live as long as it does."""

    def __init__(self, index, max_read):
        self.val, self.pos = np.asarray(index[0], np.int64), np.asarray(index[1], np.int64)
        genome_len = int(self.pos.max()) + K if len(self.pos) else 0
        self.off = -(-max_read // BIN) * BIN
        self.nbins = (genome_len + self.off) // BIN + 2
        self.cnt = np.zeros((2, self.nbins), np.int32)

    def hits(self, codes):
        """Per strand, (read position, genome position) of every hit, from one lookup a k-mer."""
        fwd, rev, ok = kmer_values(codes)
        nk = len(fwd)
        out = []
        for strand, values in enumerate((fwd, rev)):
            lo = np.searchsorted(self.val, values, side="left")
            cnt = np.where(ok, np.searchsorted(self.val, values, side="right") - lo, 0)
            p = np.repeat(np.arange(nk), cnt)
            within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            g = self.pos[lo[p] + within] if len(p) else np.zeros(0, np.int64)
            out.append((p if strand == 0 else nk - 1 - p, g))
        return out

    def seed(self, codes, clear=True):
        n = len(codes)
        per = self.hits(codes)
        bins = [(g - r + self.off) >> SHIFT for r, g in per]
        for s in range(2):                                                    # 1: count
            assert len(bins[s]) == 0 or (bins[s].min() >= 0 and bins[s].max() + 1 < self.nbins)
            np.add.at(self.cnt[s], bins[s], 1)
        best = []
        for s in range(2):                                                    # 2: the winner, by replay
            score = self.cnt[s][bins[s]].astype(np.int64) + self.cnt[s][bins[s] + 1]
            best.append(int(((score << 32) | (TOP - bins[s])).max()) if len(score) else 0)
        w = 1 if (best[1] >> 32) > (best[0] >> 32) else 0
        votes, second = best[w] >> 32, best[1 - w] >> 32
        out = {"votes": votes, "votes_second": second, "strand": ("forward", "reverse")[w], "delta": None, "g": None}
        if votes == 0:
            return out
        beta = TOP - (best[w] & 0xFFFFFFFF)
        (r, g), b = per[w], bins[w]
        score = self.cnt[w][b].astype(np.int64) + self.cnt[w][b + 1]
        far = np.abs(b - beta) > (n >> SHIFT) + 2                            # 3: the far maximum, the deltas of the two bins
        if far.any():
            out["votes_second"] = max(second, int(score[far].max()))
        two = (b == beta) | (b == beta + 1)
        dh = np.zeros(2 * BIN, np.int64)
        np.add.at(dh, (g - r + self.off)[two] - (beta << SHIFT), 1)
        dl, j = rank_find(dh, (votes - 1) // 2)
        assert dl >= 0, "the counters of the two bins do not reach the rank: a stale counter"
        delta = (beta << SHIFT) + dl - self.off
        on = r[g - r == delta]                                                # 4: the j-th read position on that diagonal
        blocks = np.zeros(2 * THREADS, np.int64)
        np.add.at(blocks, on >> SHIFT, 1)
        block, j2 = rank_find(blocks, j)
        flags = np.zeros(2 * THREADS, np.int64)
        np.add.at(flags, on[(on >> SHIFT) == block] - block * THREADS, 1)
        assert flags.max() <= 1                                               # a read position hits distinct genome positions
        at, rest = rank_find(flags, j2)
        assert block >= 0 and at >= 0 and rest == 0
        out["delta"], out["g"] = int(delta), int(delta + block * THREADS + at)
        if clear:                                                             # 5: clear by replay
            for s in range(2):
                self.cnt[s][bins[s]] = 0
        return out


def seed_all(index, reads):
    """Every read through ONE workgroup, in order; its counters are all zero at the end."""
    wg = Workgroup(index, max([len(r) for r in reads] + [0]))
    out = [wg.seed(r) for r in reads]
    assert not wg.cnt.any()
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the hand cases: name -> (index, [uint8 code arrays]); `extra` carries what a test asserts beyond equality with vote
# ------------------------------------------------------------------------------------------------------------------------------
def _both(seqs):
    return [s for seq in seqs for s in (seq, map_ref.revcomp(seq))]


def hand_cases():
    from chiron_amd import assess, map as cmap
    enc = assess.encode
    rs = assess_ref.random_seq
    rng = np.random.default_rng(4141)
    cases, extra = {}, {}

    def add(name, text, reads, max_occ=cmap.MAX_OCC):
        genome = cmap.Genome(text if isinstance(text, list) else [("g", text)])
        cases[name] = (cmap.build_index(genome.codes, cmap.K, max_occ), [enc(r) for r in reads])
        return genome

    g = rs(20000, rng)
    piece = g[1000:1300]
    holes = "".join("N" if i % 15 == 14 else ch for i, ch in enumerate(piece))
    add("degenerate_reads", g, [g[1000:1000 + n] for n in (0, 1, 14, 15, 16)] +
        ["N" * 300, holes, piece[:150] + "N" + piece[151:], piece.lower().replace("t", "u"), map_ref.revcomp(piece).lower()])
    add("empty_index", "ACGTACGTACGTAC", [piece, "ACGTACGTACGTAC", ""])
    add("nothing_matches", g, [rs(300, rng), rs(2000, rng), piece])

    g = rs(30000, rng)
    reads = []
    for k, n in enumerate((255, 256, 257, 270, 271, 511, 512, 513, 2000)):
        at = 700 + 2900 * k
        reads += _both([g[at:at + n], assess_ref.mutate(g[at:at + n + n // 10 + 10], 0.12, rng)[:n], rs(n, rng)])
    assert sorted(set(len(r) for r in reads)) == [255, 256, 257, 270, 271, 511, 512, 513, 2000]
    add("lengths", g, reads)

    plant = rs(300, rng)
    flank = [rs(n, rng) for n in (8000, 9000, 5000)]
    text = flank[0] + plant + flank[1] + plant + flank[2]
    add("ties", text, [plant, map_ref.revcomp(flank[1][1000:1400]), rs(300, rng) + text[:400], text[-400:] + rs(300, rng)])
    extra["ties"] = {"two_copies_delta": 8000, "reverse_delta": 8300 + 1000, "overhang_start_delta": -300,
                     "overhang_end_delta": len(text) - 400}
    half = rs(150, rng)
    pal = half + map_ref.revcomp(half)
    add("palindrome", flank[0] + pal + flank[2], [pal])

    g = rs(30000, rng)
    s = 256 * 30 + 100
    t = 256 * 40 + 10
    reads = [g[p:p + 300] for p in (256 * 20 - 1, 256 * 20, 256 * 20 + 1)]
    reads.append(g[s:s + 300] + g[s + 500:s + 800])                                        # a 200-base deletion: bins 30 and 31
    reads.append(g[t:t + 200] + "N" + g[t + 456:t + 656] + "N" + g[t + 912:t + 1112])      # bins 40, 41, 42 hold 186 hits each: 40 wins
    add("bin_boundaries", g, _both(reads))
    extra["bin_boundaries"] = {"deletion": (s, s + 200), "tie_delta": t}

    for name, bins_apart in (("second_copy_near", 3), ("second_copy_far", 4)):             # n = 300: n // 256 + 2 = 3
        lead = rs(256 * 20, rng)
        gap = rs(256 * bins_apart - 300, rng)
        add(name, lead + plant + gap + plant + rs(20000, rng), _both([plant]))

    unit = rs(40, rng)
    g = rs(9000, rng) + unit * 20 + rs(6000, rng) + "A" * 20 + rs(5000, rng) + "T" * 20 + rs(4000, rng)
    a_at, t_at = 9000 + 800 + 6000, 9000 + 800 + 6000 + 20 + 5000
    reads = _both([unit * 10, g[8900:8900 + 500], g[a_at - 50:a_at + 70], g[t_at - 50:t_at + 70], "A" * 20, "T" * 20,
                   g[a_at - 30:a_at + 20] + g[t_at:t_at + 50]])
    add("repeats_occ64", g, reads)
    add("repeats_occ8", g, reads, max_occ=8)

    ca, cb = rs(12000, rng), rs(10000, rng)
    genome = add("two_contigs", [("ctgA", ca), ("ctgB", cb)],
                 [ca[3000:3400], map_ref.revcomp(cb[5000:5600]), ca[-8:] + cb[:7], assess_ref.mutate(cb[100:900], 0.1, rng)])
    extra["two_contigs"] = {"genome": genome, "contigs": [0, 1, None, 1]}
    return cases, extra


HYGIENE_GENOME = 30000


def hygiene_case(reads=2500):
    """More reads than workgroups against one 30 kb genome: 150 .. 400 bases, every third read its predecessor again, every seventh
    unrelated, the others cut from the genome at 5 % divergence, every other of those reverse-complemented."""
    from chiron_amd import assess, map as cmap
    rng = np.random.default_rng(4242)
    g = assess_ref.random_seq(HYGIENE_GENOME, rng)
    out = []
    for k in range(reads):
        n = int(rng.integers(150, 401))
        if k % 3 == 2:
            out.append(out[-1])
        elif k % 7 == 3:
            out.append(assess_ref.random_seq(n, rng))
        else:
            at = int(rng.integers(0, len(g) - n))
            seq = assess_ref.mutate(g[at:at + n], 0.05, rng)
            out.append(map_ref.revcomp(seq) if k % 2 else seq)
    return cmap.build_index(cmap.Genome([("g", g)]).codes), [assess.encode(r) for r in out]


def random_case(rng):
    """A genome of 2 .. 20 kb with planted repeats and N's, and reads of 0 .. 600 bases on both strands: cut from it (exact or
    mutated, some across a repeat or an N), unrelated, or hanging over an end."""
    from chiron_amd import assess, map as cmap
    size = int(rng.integers(2000, 20001))
    g = list(assess_ref.random_seq(size, rng))
    rep = assess_ref.random_seq(int(rng.integers(20, 400)), rng)
    for _ in range(int(rng.integers(0, 5))):
        at = int(rng.integers(0, size - len(rep)))
        g[at:at + len(rep)] = rep
    for _ in range(int(rng.integers(0, 4))):
        g[int(rng.integers(0, size))] = "N"
    g = "".join(g)
    n = int(rng.integers(0, 601))
    kind = int(rng.integers(0, 5))
    at = int(rng.integers(0, size - n))
    if kind == 0:
        read = assess_ref.random_seq(n, rng)
    elif kind == 1:
        read = g[at:at + n]
    elif kind == 2:
        read = assess_ref.mutate(g[at:at + n], float(rng.choice([0.03, 0.12, 0.25])), rng)
    elif kind == 3:
        read = assess_ref.random_seq(n // 3, rng) + g[:n - n // 3]
    else:
        read = rep * int(rng.integers(1, 4)) + g[at:at + n // 2]
        read = read[:600]
    if rng.integers(2):
        read = map_ref.revcomp(read)
    max_occ = int(rng.choice([2, 8, 64]))
    return cmap.build_index(cmap.Genome([("g", g)]).codes, cmap.K, max_occ), assess.encode(read)


LONG_LENGTHS = (4095, 4096, 4097, 65535, 65536, 65537, 131072)
_LONG = []


def long_read_cases():
    """One genome of 400 kb with one index, and reads of 4 k to 131072 bases (the longest the kernel takes), each on both strands:
      cut<n>     cut from the genome at 8 % divergence, n bases, n around 2^12, around 2^16 and 2^17
      tail_hit   70000 unrelated bases, then 3000 exact genome bases: every hit at read position >= 70000, so the candidate's
                 256-position counter is number 273 or above, in the upper half of the 512
      head_hit   the mirror image: counter 0 of a 73000-base read
      unrelated  131072 bases that match nothing but by chance
    The genome holds hygiene_case's 30 kb genome from position 185000 on, so that hygiene_case's short reads hit this index too
    (mixed_batch).  -> (index, {name: codes}), built once: nobody changes them."""
    if not _LONG:
        from chiron_amd import assess, map as cmap
        rng = np.random.default_rng(4343)
        rs = assess_ref.random_seq
        g = rs(185000, rng) + rs(HYGIENE_GENOME, np.random.default_rng(4242)) + rs(185000, rng)
        seqs = {}
        for k, n in enumerate(LONG_LENGTHS):
            at = (15000 * k, 110000, 230000)[0 if n < 65000 else 1 if n < 131072 else 2]
            piece = ""
            while len(piece) < n:                                            # the mutation shortens or lengthens: cut generously, trim
                piece = assess_ref.mutate(g[at:at + n + n // 20 + 400], 0.08, rng)
            seqs["cut%d" % n] = piece[:n]
        seqs["tail_hit"] = rs(70000, rng) + g[200000:203000]
        seqs["head_hit"] = g[300000:303000] + rs(70000, rng)
        seqs["unrelated"] = rs(131072, rng)
        reads = {}
        for name, seq in seqs.items():
            reads[name] = assess.encode(seq)
            reads[name + "_rc"] = assess.encode(map_ref.revcomp(seq))
        _LONG.append((cmap.build_index(cmap.Genome([("g", g)]).codes), reads))
    return _LONG[0]


def mixed_batch(short=300):
    """The 131072-base read cut from long_read_cases' genome and `short` of hygiene_case's reads, against that genome's index:
    kc_stride, off and nbins of the call are sized by the long read.  -> (index, long read, [short reads])."""
    index, reads = long_read_cases()
    return index, reads["cut131072"], hygiene_case(short)[1]
