"""Batches in which every workgroup of an alignment kernel takes a second item and forty take a third, built once and seeded.
tests/test_reuse_cases_cpu.py checks that the designed items are what their names say, by the references alone;
tests/test_gpu_reuse.py runs the batches on the GPU.

The kernels of csrc/assess.hip, map.hip, trace.hip, ctc_align.hip and pileup.hip run item q on workgroup q mod G.  A batch holds
2 G + EXTRA items, so items k, k + G and k + 2 G are the successive tenants of workgroup k < EXTRA.  `sequences` places the
designed tenants of workgroups 0, 1, ...; every other item is filler.  A builder returns a dict:
    G         the kernel's group count, from chiron_amd._lib
    items     the batch
    names     {"<sequence>.<role>": index into items} of every designed item
    triplets  [(i, i + G, i + 2 G)]: one ordinary item as all three tenants of a workgroup
    want      the reference's answer for the whole batch
plus the call's own arguments where it has some (band0, max_band, the tile).

The designed sequences (first tenant -> second -> third), where the kernel has the notion:
    a  a band in the workspace row -> a tiny band in LDS -> the same tiny item again
    b  a tiny band in LDS -> a band in the workspace row
    c  an empty item -> an ordinary item -> an empty item
    d  an item whose band doubles at least three times -> an item accepted at band0
    e  label: a status-1 read -> an ordinary read; a status-2 read -> an ordinary read; a wide read as first tenant
    f  pileup: 3 * 1024 + 1 columns -> a short alignment whose first column is an insertion; an alignment that leaves the tile
       early -> a short alignment inside it
    g  trace: the longest walk of the batch -> a pair whose band has an odd number of slots
    h  one ordinary item as first, second and third tenant
At most two items of a batch have a band past LDS (they are what a batch costs).  In assess.hip three doublings end at w = 2048,
whose certificate 2 w + 1 + |m - n| is passed only by a pair with n, m > 2049: its band is never clipped by the table and has
at least 4097 diagonals, so there the second wide item is also d's doubling item (b and d share a workgroup: tiny -> wide, three
doublings -> accepted at band0).  In ctc_align.hip a read ends with status 2 under max_band = 2048 only after its pass at
w = 2048, 4097 states wide, so there the second wide item is also e's status-2 read.
"""
import numpy as np

from chiron_amd import _lib

import assess_ref
import ctc_align_ref
import map_ref
import pileup_cases
import pileup_ref
import trace_ref
from test_gpu_label import _planted_exact as planted     # a planted path of exactly F frames over L random bases

EXTRA = 40                      # workgroups that take a third item


def place(G, sequences, filler):
    """-> (items, names): 2 G + EXTRA items, tenant t of sequence k at k + t G, filler() everywhere else."""
    assert len(sequences) <= EXTRA
    items = [None] * (2 * G + EXTRA)
    names = {}
    for k, (seq, tenants) in enumerate(sequences):
        assert len(tenants) <= 3
        for t, (role, item) in enumerate(tenants):
            items[k + t * G] = item
            assert seq + "." + role not in names
            names[seq + "." + role] = k + t * G
    for i in range(len(items)):
        if items[i] is None:
            items[i] = filler()
    return items, names


def band_slots(n, m, w):
    """Diagonals of the band of half-width w around [min(0, m-n), max(0, m-n)], clipped to the table's -n .. m."""
    return min(max(0, m - n) + w, m) - max(min(0, m - n) - w, -n) + 1


def assess_band(n, m, E, band0=_lib.ALIGN_BAND0):
    """The half-width csrc/assess.hip stops at, from the true E: the first band0 * 2^k that certifies E or covers the table."""
    w = band0
    while not (E <= 2 * w + 1 + abs(m - n) or band_slots(n, m, w) == n + m + 1):
        w *= 2
    return w


def doublings(band, band0):
    k = 0
    while band0 << k < band:
        k += 1
    assert band0 << k == band
    return k


def label_width(L, band):
    """States of the pass of half-width `band` over a read of L bases (band 0: the full table)."""
    S = 2 * L + 1
    return S if band == 0 or band >= S - 1 else min(2 * band + 1, S)


def _pair_filler(rng):
    """A related or an unrelated pair of 8 .. 48 bases each."""
    def one():
        a = assess_ref.random_seq(int(rng.integers(8, 45)), rng)
        if rng.random() < 0.7:
            b = assess_ref.mutate(a, (0.05, 0.15, 0.4)[int(rng.integers(3))], rng)[:48]
            b = b if len(b) >= 8 else a
        else:
            b = assess_ref.random_seq(int(rng.integers(8, 49)), rng)
        return a, b
    return one


def _empties(ordinary):
    """Sequence c: n = 0, m = 0 and both, each empty -> ordinary -> empty."""
    out = []
    for tag, pair in (("n0", ("", "ACGTTGCAAC")), ("m0", ("GATTACAGATTACA", "")), ("both", ("", ""))):
        out.append(("c_" + tag, [("empty1", pair), ("ordinary", ordinary()), ("empty2", pair)]))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# assess.hip: align_kernel
# ------------------------------------------------------------------------------------------------------------------------------
def assess_case():
    G = _lib.ALIGN_MAX_GROUPS
    rng = np.random.default_rng(9001)
    filler = _pair_filler(rng)
    # a's wide item: test_gpu_assess.py's test_lds_to_workspace_threshold at LDS_SLOTS + 1 (an all-N read of m + gap bases)
    L, m = _lib.ALIGN_LDS_SLOTS, 2000
    gap = (L + 1) - 2049
    wide = ("N" * (m + gap), assess_ref.random_seq(m, rng))
    tiny = filler()
    # b and d: 300 shared bases and 2100 that match nothing, so E = 2100 > 2 * 1024 + 1: accepted at w = 2048, 4097 diagonals
    core = assess_ref.random_seq(300, rng)
    wide3 = (core + "N" * 2100, core + assess_ref.random_seq(2100, rng))
    same = filler()
    sequences = [("a", [("wide", wide), ("tiny1", tiny), ("tiny2", tiny)]),
                 ("bd", [("tiny", filler()), ("wide_doubling", wide3), ("band0", filler())])]
    sequences += _empties(filler)
    sequences.append(("h", [("first", same), ("second", same), ("third", same)]))
    items, names = place(G, sequences, filler)
    big = {names["a.wide"], names["bd.wide_doubling"]}
    small = [i for i in range(len(items)) if i not in big]
    want = [None] * len(items)
    for i, em in zip(small, assess_ref.full_table_batch([items[i][0] for i in small], [items[i][1] for i in small])):
        want[i] = em
    for i in big:
        want[i] = assess_ref.full_table(*items[i])
    return {"G": G, "items": items, "names": names, "triplets": [tuple(names["h." + r] for r in ("first", "second", "third"))], "want": want}


# ------------------------------------------------------------------------------------------------------------------------------
# map.hip: infix_kernel
# ------------------------------------------------------------------------------------------------------------------------------
def map_case():
    G = _lib.INFIX_MAX_GROUPS
    band0 = _lib.INFIX_BAND0
    rng = np.random.default_rng(9002)

    def filler():
        core = assess_ref.random_seq(int(rng.integers(8, 37)), rng)
        left, right = (assess_ref.random_seq(int(rng.integers(0, 7)), rng) for _ in range(2))
        read = assess_ref.mutate(core, (0.05, 0.15, 0.4)[int(rng.integers(3))], rng)[:48] if rng.random() < 0.7 else \
            assess_ref.random_seq(int(rng.integers(8, 49)), rng)
        return (read if len(read) >= 8 else core), left + core + right

    # the wide items: test_gpu_map.py's test_lds_to_workspace_threshold at LDS_SLOTS + 1 (its first and its second form)
    L = _lib.INFIX_LDS_SLOTS
    core = assess_ref.random_seq(1000, rng)
    n = 1600
    m = n + (L + 1) - 2049
    wide_a = (core + "N" * 600, core + assess_ref.random_seq(m - 1000, rng))
    wide_b = ("N" * 300 + core + "N" * 300, assess_ref.random_seq(m - 1000, rng) + core)
    # d: 300 bases found in the window and 1100 that match nothing: E = 1100 passes 256, 512 and 1024; the band of 2048 is the
    # whole table of 2901 diagonals, in LDS
    c300 = assess_ref.random_seq(300, rng)
    doubling = (c300 + "N" * 1100, assess_ref.random_seq(100, rng) + c300 + assess_ref.random_seq(1100, rng))
    tiny, same = filler(), filler()
    sequences = [("a", [("wide", wide_a), ("tiny1", tiny), ("tiny2", tiny)]),
                 ("b", [("tiny", filler()), ("wide", wide_b)]),
                 ("d", [("doubling", doubling), ("band0", filler())])]
    sequences += _empties(filler)
    sequences.append(("h", [("first", same), ("second", same), ("third", same)]))
    items, names = place(G, sequences, filler)
    from chiron_amd import map as cmap
    want = map_ref.infix_rows([a for a, _ in items], [b for _, b in items], band0, cmap.INFIX_DTYPE)
    return {"G": G, "band0": band0, "items": items, "names": names,
            "triplets": [tuple(names["h." + r] for r in ("first", "second", "third"))], "want": want}


# ------------------------------------------------------------------------------------------------------------------------------
# trace.hip: trace_kernel
# ------------------------------------------------------------------------------------------------------------------------------
def trace_case():
    G = _lib.ALIGN_MAX_GROUPS
    rng = np.random.default_rng(9003)
    filler = _pair_filler(rng)
    # the wide items: test_gpu_trace.py's test_lds_to_workspace_threshold at LDS_SLOTS + 1, the longer side as the read and as
    # the reference
    L = _lib.ALIGN_LDS_SLOTS
    longest = L
    short = (longest - 37) & ~1
    wide_a = ("N" * longest, assess_ref.random_seq(short, rng))
    wide_b = ("N" * short, assess_ref.random_seq(longest, rng))
    # g: a walk longer than the wide items' 4096 columns, then w* = 0 with a gap of two: three slots
    base = assess_ref.random_seq(4300, rng)
    walk = (base, assess_ref.mutate(base, 0.06, rng))
    stem = assess_ref.random_seq(30, rng)
    odd = (stem + "NN", stem)
    tiny, same = filler(), filler()
    sequences = [("a", [("wide", wide_a), ("tiny1", tiny), ("tiny2", tiny)]),
                 ("b", [("tiny", filler()), ("wide", wide_b)]),
                 ("g", [("longest", walk), ("odd", odd)])]
    sequences += _empties(filler)
    sequences.append(("h", [("first", same), ("second", same), ("third", same)]))
    items, names = place(G, sequences, filler)
    want = [trace_ref.full_trace(a, b) for a, b in items]
    return {"G": G, "items": items, "names": names, "triplets": [tuple(names["h." + r] for r in ("first", "second", "third"))], "want": want}


# ------------------------------------------------------------------------------------------------------------------------------
# ctc_align.hip: ctc_align_kernel
# ------------------------------------------------------------------------------------------------------------------------------
LABEL_BAND0, LABEL_MAX_BAND = 2, 2048


def label_case():
    G = _lib.LABEL_MAX_GROUPS
    band0, max_band = LABEL_BAND0, LABEL_MAX_BAND
    rng = np.random.default_rng(9004)

    def filler():
        """L in 0 .. 12, F up to 6 L: a planted path, integer scores where ties decide, or too few frames."""
        L = int(rng.integers(0, 13))
        if L == 0:
            return np.zeros((0, 5), np.float32), np.zeros(0, np.uint8)
        lab = rng.integers(0, 4, size=L).astype(np.uint8)
        rep = int(np.count_nonzero(lab[1:] == lab[:-1]))
        kind = int(rng.integers(10))
        if kind == 0:
            return rng.integers(-3, 4, size=(int(rng.integers(0, L + rep)), 5)).astype(np.float32), lab
        if kind < 3 and L + rep <= 6 * L:
            return rng.integers(-3, 4, size=(int(rng.integers(L + rep, 6 * L + 1)), 5)).astype(np.float32), lab
        return planted(rng, L, int(rng.integers(2, 5)) * L)

    def ordinary():
        L = int(rng.integers(36, 45))
        return planted(rng, L, 3 * L)

    def found(make, band_ok):
        """The first make() whose reference band satisfies band_ok and whose status is 0."""
        for _ in range(2000):
            x, lab = make()
            _, _, band, status = ctc_align_ref.align_one(x, lab, band0, max_band)
            if status == 0 and band_ok(band):
                return x, lab
        raise AssertionError("no such read in 2000 draws")

    # The wide reads.  test_gpu_label.py reaches 4097 states by passing band0 = 2048 (test_lds_to_workspace_rows) or 1024
    # (test_doubling_across_the_lds_threshold); a batch that also holds reads accepted at band0 = 2 cannot, and from 2 a planted
    # path far off the centre line does not get there: some narrower band accepts another path that stays clear of its edges.
    # So these reads have ONE valid path, F = L + repeats: `slow` equal bases take two frames each (a blank between them), then
    # 2 * slow distinct neighbours take one.  The path is 2 * slow * (2 * slow) / (4 * slow) = slow states below the centre line
    # where the two parts meet, so every band narrower than that is rejected (the end is not reachable), whatever the scores.
    # slow = 1150: accepted at w = 2048, 4097 states.  slow = 2150: rejected at 2048 too, and 4096 is past max_band and short of
    # S - 1: status 2.
    def single_path(slow):
        lab = np.concatenate([np.zeros(slow, np.int64), np.cumsum(rng.integers(1, 4, size=2 * slow)) % 4]).astype(np.uint8)
        return rng.standard_normal((len(lab) + slow - 1, 5)).astype(np.float32), lab

    wide, exhausted = single_path(1150), single_path(2150)
    tiny, same = filler(), ordinary()
    while len(tiny[1]) < 3:
        tiny = filler()
    doubling = found(lambda: planted(rng, 60, 900, np.where(np.arange(60) < 30, 0.02, 1.0)), lambda b: b >= 8 * band0)
    at_band0 = found(lambda: planted(rng, 8, 24), lambda b: b == band0)
    lab1 = np.array([0, 0, 1, 1, 2, 3], np.uint8)                        # two repeats: 8 frames at least
    status1 = (rng.integers(-3, 4, size=(7, 5)).astype(np.float32), lab1)
    empty00 = (np.zeros((0, 5), np.float32), np.zeros(0, np.uint8))
    empty10 = (rng.integers(-3, 4, size=(1, 5)).astype(np.float32), np.zeros(0, np.uint8))
    sequences = [("a", [("wide", wide), ("tiny1", tiny), ("tiny2", tiny)]),
                 ("b", [("tiny", filler()), ("wide_status2", exhausted), ("ordinary", ordinary())]),
                 ("c_f0", [("empty1", empty00), ("ordinary", ordinary()), ("empty2", empty00)]),
                 ("c_f1", [("empty1", empty10), ("ordinary", ordinary()), ("empty2", empty10)]),
                 ("d", [("doubling", doubling), ("band0", at_band0)]),
                 ("e", [("status1", status1), ("ordinary", ordinary())]),
                 ("h", [("first", same), ("second", same), ("third", same)])]
    items, names = place(G, sequences, filler)
    want = ctc_align_ref.align([x for x, _ in items], [lab for _, lab in items], band0, max_band)
    return {"G": G, "band0": band0, "max_band": max_band, "items": items, "names": names,
            "triplets": [tuple(names["h." + r] for r in ("first", "second", "third"))], "want": want}


# ------------------------------------------------------------------------------------------------------------------------------
# pileup.hip: pileup_count_kernel
# ------------------------------------------------------------------------------------------------------------------------------
def pileup_case():
    G = _lib.PILEUP_MAX_GROUPS
    chunk = _lib.PILEUP_CHUNK
    rng = np.random.default_rng(9005)
    g0, g1 = 100, 3700
    tile = g1 - g0
    pool = [(pos + g0, read, ops) for pos, read, ops in pileup_cases.random_set(rng, 2 * G + EXTRA, tile, max_columns=60, n_rate=0.03)]

    def filler():
        return pool.pop()

    def inside(columns):
        return pileup_cases.random_alignment(rng, columns, g0 + int(rng.integers(50, 2000)))

    def of(pos, ops):
        ops = np.asarray(ops, dtype=np.uint8)
        return int(pos), rng.integers(0, 4, int((ops != 3).sum())).astype(np.uint8), ops

    before = pileup_cases.random_alignment(rng, 40, g0 - 70, p_ins=0.1, p_del=0.1)      # at most 40 positions: ends before g0
    after = pileup_cases.random_alignment(rng, 40, g1 + 3)
    no_ref = of(g0 + 500, [2] * 9)                                                    # no reference column: clipping alone
    long_one = pileup_cases.random_alignment(rng, 3 * chunk + 1, g0 + 10)              # four chunks, the last of one column
    leading_ins = of(g0 + 700, [2, 0, 0, 2, 2, 0, 3, 0, 1, 2, 0, 0])
    leaves = pileup_cases.random_alignment(rng, 2 * chunk + 500, g1 - 100, p_ins=0.1, p_del=0.1)   # its second chunk starts past g1
    same = inside(50)
    sequences = [("c_before", [("ncols0_1", before), ("ordinary", inside(55)), ("ncols0_2", before)]),
                 ("c_after", [("ncols0_1", after), ("ordinary", inside(55)), ("ncols0_2", after)]),
                 ("c_noref", [("ncols0_1", no_ref), ("ordinary", inside(55)), ("ncols0_2", no_ref)]),
                 ("f_long", [("columns3073", long_one), ("leading_insertion", leading_ins)]),
                 ("f_break", [("leaves_early", leaves), ("inside", inside(40))]),
                 ("h", [("first", same), ("second", same), ("third", same)])]
    items, names = place(G, sequences, filler)
    ref = rng.integers(0, 4, tile).astype(np.uint8)
    ref[rng.random(tile) < 0.05] = 4
    min_depth = 3
    want = pileup_ref.counter(items, g0, g1, ref, min_depth)
    alone = {name: pileup_ref.count_columns([items[i]], g0, g1) for name, i in names.items()}
    return {"G": G, "g0": g0, "g1": g1, "ref": ref, "min_depth": min_depth, "items": items, "names": names,
            "triplets": [tuple(names["h." + r] for r in ("first", "second", "third"))], "want": want, "alone": alone}


BUILDERS = {"assess": assess_case, "map": map_case, "trace": trace_case, "label": label_case, "pileup": pileup_case}
_BUILT = {}


def case(kernel):
    """The kernel's batch, built on first use and shared by every test of the process; nobody changes it."""
    if kernel not in _BUILT:
        _BUILT[kernel] = BUILDERS[kernel]()
    return _BUILT[kernel]
