"""Reference for the pileup (chiron_pileup / chiron_amd.pileup): the definition of DESIGN section 16, transcribed column by column
in plain Python.  Shares no code with the package.

An alignment is (pos, read, ops): pos a genome position, read codes 0..4, ops one byte per column (0 '=', 1 'X', 2 'I', 3 'D').
count_columns   the counts of one tile [g0, g1), planar int32 [PLANES][g1 - g0] (planes 0..4 base, 5 del, 6 + 5k + c ins, last
                over), and the clipped total of ALL the alignments given (it does not depend on the tile).
padded_counts   the same counts a second way: every alignment replayed into one padded row over (position, slot) cells, the rows
                counted column-wise with numpy.
call_position   the call rule on one position's counts; call_tile applies it to a tile.
counter         count_columns + call_tile with the signature chiron_amd.pileup.count(counter=) wants.
consensus, variants   restated from their definitions.
"""
import numpy as np

S = 4
PLANES = 6 + 5 * S + 1
DEL, INS, OVER = 5, 6, PLANES - 1


def count_columns(alignments, g0, g1):
    tile = max(g1 - g0, 0)
    planes = [[0] * tile for _ in range(PLANES)]
    clipped = 0

    def add(plane, g):
        if g0 <= g < g1:
            planes[plane][g - g0] += 1

    for pos, read, ops in alignments:
        ops = [int(o) for o in ops]
        m = sum(1 for o in ops if o in (0, 1, 3))
        assert sum(1 for o in ops if o in (0, 1, 2)) == len(read)
        q = i = k = 0
        for o in ops:
            if o in (0, 1):
                add(int(read[i]), pos + q)
                q, i, k = q + 1, i + 1, 0
            elif o == 3:
                add(DEL, pos + q)
                q, k = q + 1, 0
            else:
                assert o == 2
                if q == 0 or q == m:
                    clipped += 1
                else:
                    if k < S:
                        add(INS + 5 * k + int(read[i]), pos + q - 1)
                    elif k == S:
                        add(OVER, pos + q - 1)
                    k += 1
                i += 1
    return np.array(planes, dtype=np.int32).reshape(PLANES, tile), clipped


def padded_counts(alignments, g0, g1):
    """Row p, cell (g, 0) holds what alignment p shows at position g (0..4 a base, 5 a deletion, 9 nothing), cell (g, 1 + k) its
    (k+1)-th inserted base after g (9: none), cell (g, 1 + S) whether its insertion after g went past S bases."""
    tile = max(g1 - g0, 0)
    width = 2 + S
    rows = np.full((len(alignments), tile, width), 9, dtype=np.int64)
    clipped = 0
    for p, (pos, read, ops) in enumerate(alignments):
        ops = np.asarray(ops, dtype=np.int64)
        on_ref = ops != 2
        m = int(on_ref.sum())
        if m == 0:
            clipped += len(ops)
            continue
        ref_cols = np.nonzero(on_ref)[0]
        clipped += int(ref_cols[0]) + (len(ops) - 1 - int(ref_cols[-1]))
        read_idx = np.cumsum(ops != 3) - 1                 # the read base of each read-consuming column
        for t, col in enumerate(ref_cols):
            g = pos + t
            if not (g0 <= g < g1):
                continue
            rows[p, g - g0, 0] = 5 if ops[col] == 3 else int(read[read_idx[col]])
            if t + 1 < m:
                run = range(col + 1, ref_cols[t + 1])
                for k, c in enumerate(run):
                    if k < S:
                        rows[p, g - g0, 1 + k] = int(read[read_idx[c]])
                if len(run) > S:
                    rows[p, g - g0, 1 + S] = 1
    planes = np.zeros((PLANES, tile), dtype=np.int32)
    for c in range(5):
        planes[c] = (rows[:, :, 0] == c).sum(axis=0)
    planes[DEL] = (rows[:, :, 0] == 5).sum(axis=0)
    for k in range(S):
        for c in range(5):
            planes[INS + 5 * k + c] = (rows[:, :, 1 + k] == c).sum(axis=0)
    planes[OVER] = (rows[:, :, 1 + S] == 1).sum(axis=0)
    return planes, clipped


def call_position(base, dele, ins, r, min_depth):
    """base [5], dele, ins [S][5], the reference code r -> (depth, the 8-byte record as a list, the clause that decided the base)."""
    depth = sum(base) + dele
    if depth < min_depth:
        return depth, [r, 0, 0, 0, 0, 0, 1, 0], "low"
    keys = [((base[c], 1 if c == r else 0, -c), c) for c in range(4)] + [((dele, 0, -9), 5)]
    key, code = max(keys)
    clause = "base"
    if code == 5:
        clause = "deletion"
    elif key[0] == 0:
        code, clause = r, "only_n"
    else:
        tied = [c for c in range(4) if base[c] == key[0]]
        if len(tied) > 1:
            clause = "tie_ref" if r in tied else "tie_code"
        elif dele == key[0]:
            clause = "tie_deletion"
    emitted = []
    for k in range(S):
        if 2 * sum(ins[k]) > depth:
            best = max(range(4), key=lambda c: (ins[k][c], -c))
            emitted.append(best if ins[k][best] > 0 else 4)
        else:
            break
    return depth, [code, len(emitted)] + (emitted + [0] * S)[:S] + [0, 0], clause


def call_tile(planes, ref_codes, min_depth, clauses=None):
    """-> (depth int32 [tile], call uint8 [tile, 8]).  clauses: a dict that collects how often each clause of the rule decided."""
    tile = planes.shape[1]
    depth = np.zeros(tile, dtype=np.int32)
    call = np.zeros((tile, 8), dtype=np.uint8)
    for g in range(tile):
        ins = [[int(planes[INS + 5 * k + c, g]) for c in range(5)] for k in range(S)]
        d, rec, clause = call_position([int(planes[c, g]) for c in range(5)], int(planes[DEL, g]), ins, int(ref_codes[g]), min_depth)
        depth[g], call[g] = d, rec
        if clauses is not None:
            clauses[clause] = clauses.get(clause, 0) + 1
            if rec[1]:
                clauses["insertion"] = clauses.get("insertion", 0) + 1
                if rec[1] > 1:
                    clauses["insertion_chain"] = clauses.get("insertion_chain", 0) + 1
                if 4 in rec[2:2 + rec[1]]:
                    clauses["insertion_n"] = clauses.get("insertion_n", 0) + 1
            if clause != "low" and rec[1] < S and any(2 * sum(ins[k]) > d for k in range(rec[1] + 1, S)):
                clauses["chain_stopped"] = clauses.get("chain_stopped", 0) + 1
    return depth, call


def counter(alignments, g0, g1, ref_codes, min_depth):
    """What chiron_amd.pileup.count(counter=) calls: one tile of the given alignments, honouring the tile."""
    planes, clipped = count_columns(alignments, g0, g1)
    depth, call = call_tile(planes, ref_codes, min_depth)
    return planes, depth, call, clipped


def consensus(call, names, starts, lengths):
    out = {}
    for name, g0, L in zip(names, starts, lengths):
        seq = []
        for g in range(int(g0), int(g0) + int(L)):
            if call[g][0] != 5:
                seq.append("ACGTN"[call[g][0]])
            for k in range(call[g][1]):
                seq.append("ACGTN"[call[g][2 + k]])
        out[name] = "".join(seq)
    return out


def variants(call, depth, planes, codes, names, starts, lengths):
    out = []
    for name, g0, L in zip(names, starts, lengths):
        for t in range(int(L)):
            g = int(g0) + t
            code, r = int(call[g][0]), int(codes[g])
            rec = {"contig": name, "pos": t + 1, "depth": int(depth[g])}
            if code == 5:
                out.append(dict(rec, type="DEL", ref="ACGTN"[r], alt="-", count=-1 if planes is None else int(planes[DEL][g])))
            elif code != r:
                out.append(dict(rec, type="SUB", ref="ACGTN"[r], alt="ACGTN"[code], count=-1 if planes is None else int(planes[code][g])))
            if call[g][1]:
                alt = "".join("ACGTN"[int(call[g][2 + k])] for k in range(int(call[g][1])))
                out.append(dict(rec, type="INS", ref="-", alt=alt, count=-1 if planes is None else sum(int(planes[INS + c][g]) for c in range(5))))
    return out
