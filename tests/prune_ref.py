"""Numpy model of k_p1k_lean's pruned grid scan (csrc/tdoa_phat1024.hip,
P1K_GRID_PRUNE; the row table is tdoa_p1k_prune_section, csrc/tdoa_tables.cpp).

Everything is float32 and in the kernel's order:

  * the row table: the distinct lag tuples stably sorted by the lag slot of
    one pair (ties keep first-cell order), rows of 64, per row the range
    [lo, hi] of that pair's slots; the sort pair has the smallest widest row,
    then the smallest sum of widths, then the lowest index;
  * per wave (two frames): bound(row) = (t0 + t1) + t2 with t_p =
    max w_p[lo..hi] for the sort pair and t_q = M_q for the others;
    pass 1 scans the rows that have either frame's largest bound, pass 2 the
    rows whose bound is not below either frame's best of pass 1; a compare is
    "larger L, or equal L and smaller first cell"; no L above -inf: tuple 0;
    where pass 2 would scan more than half of the rows, the exhaustive scan in
    first-cell order runs instead.
"""
import numpy as np

F32 = np.float32
INT_MAX = 2**31 - 1
KPAD = 128  # lag slots per pair in the wave's score table; slot 127 is -inf


def distinct_tuples(lut):
    """[3][U] lag slots of the distinct tuples in first-cell order, and [U] first cells."""
    l3 = np.asarray(lut).reshape(3, -1).astype(np.int64)
    keys = (l3[0] << 16) | (l3[1] << 8) | l3[2]
    _, first = np.unique(keys, return_index=True)
    first.sort()
    return l3[:, first], first.astype(np.int64)


def row_table(T, cells):
    """The documented rule, from the tuples alone."""
    U = T.shape[1]
    rows = -(-U // 64)
    if U <= 0 or rows > 64:
        return None
    best = None
    for p in range(3):
        order = np.argsort(T[p], kind="stable")
        s = T[p, order]
        lo = s[0::64]
        hi = np.array([s[min(U, 64 * r + 64) - 1] for r in range(rows)])
        key = (int((hi - lo + 1).max()), int((hi - lo + 1).sum()), p)
        if best is None or key < best[0]:
            best = (key, order, lo, hi)
    (width, _, pair), order, lo, hi = best
    n = rows * 64
    tup = np.full((3, n), KPAD - 1, np.int64)
    tup[:, :U] = T[:, order]
    cl = np.full(n, INT_MAX, np.int64)
    cl[:U] = cells[order]
    return dict(rows=rows, pair=pair, width=width, cell0=int(cells[0]), lo=lo.astype(np.int64),
                hi=hi.astype(np.int64), tuples=tup, cells=cl, U=U)


def parse_section(words):
    """The table as the library builds it (tools/tables_dump: p1k_prune.bin, uint32 words)."""
    w = np.asarray(words, np.uint32).astype(np.int64)
    if w.size == 0:
        return None
    rows = int(w[0])
    assert w.size == 4 + 64 + 2 * 64 * rows
    rec = w[4:68]
    tw = w[68:68 + 64 * rows]
    assert (rec[rows:] == (127 | 127 << 8)).all() and (tw >> 30 == 0).all() and (tw & 0x701C07 == 0).all()
    tup = np.stack([(tw >> 3) & 0x7F, (tw >> 13) & 0x7F, (tw >> 23) & 0x7F])
    return dict(rows=rows, pair=int(w[1]), width=int(w[2]), cell0=int(w[3]), lo=rec[:rows] & 0xFF,
                hi=rec[:rows] >> 8, tuples=tup, cells=w[68 + 64 * rows:], U=int((w[68 + 64 * rows:] != INT_MAX).sum()))


def fkey(v):
    """A float32 as a signed key of the same order, -0.0 folded to +0.0 (tdoa_fft32.h)."""
    b = (np.asarray(v, F32) + F32(0)).view(np.int32).astype(np.int64)
    return np.where(b < 0, b ^ 0x7FFFFFFF, b)


def _table128(w):
    """[F][3][K] weighted scores -> the wave's [F][3][128] table: slot 127 is
    -inf; the slots from K to 126 are never read (NaN here, so a read would show)."""
    w = np.asarray(w, F32)
    t = np.full(w.shape[:2] + (KPAD,), np.nan, F32)
    t[..., :w.shape[2]] = w
    t[..., KPAD - 1] = -np.inf
    return t


def _L(t, tup):
    with np.errstate(invalid="ignore"):
        return ((t[:, 0][:, tup[0]] + t[:, 1][:, tup[1]]).astype(F32) + t[:, 2][:, tup[2]]).astype(F32)


def exhaustive(w, T, cells):
    """The exhaustive scan of [F][3][K] scores in first-cell order: a strict '>'
    from -inf keeps the first maximum; none (NaN or -inf everywhere): tuple 0."""
    L = _L(_table128(w), T)
    ok = L > -np.inf  # NaN: False
    Lm = np.where(ok, L, -np.inf).astype(F32)
    mx = (Lm.max(-1) + F32(0)).astype(F32)
    first = (Lm == mx[:, None]).argmax(-1)
    cell = np.where(ok.any(-1), cells[first], cells[0])
    return cell.astype(np.int64), mx


def bound_terms(w):
    """M_q = max(maximum, 0): what the kernel takes from the raw maximum
    (scores weighted by a prior in [0, 1] that is 1 at the maximum)."""
    with np.errstate(invalid="ignore"):
        return np.fmax(np.fmax.reduce(np.asarray(w, F32), axis=-1), F32(0))


def row_bounds(w, tab, M=None):
    """[F][rows] float32 bounds of [F][3][K] scores."""
    t = _table128(w)
    M = bound_terms(w) if M is None else np.asarray(M, F32)
    p = tab["pair"]
    wm = np.stack([np.fmax.reduce(t[:, p, lo:hi + 1], axis=-1, initial=-np.inf)
                   for lo, hi in zip(tab["lo"], tab["hi"])], 1).astype(F32)
    term = [wm if q == p else np.broadcast_to(M[:, q, None], wm.shape) for q in range(3)]
    with np.errstate(invalid="ignore"):
        return ((term[0] + term[1]).astype(F32) + term[2]).astype(F32)


def pruned_wave(w2, tab, M=None):
    """The as-built search on one wave's frames ([2][3][K]).  Returns cells [2],
    max L [2] and the number of rows scanned."""
    t = _table128(w2)
    bnd = row_bounds(w2, tab, M)
    rows = tab["rows"]
    bv = np.full((2, 64), -np.inf, F32)
    bc = np.full((2, 64), INT_MAX, np.int64)

    def scan(r):
        sl = slice(64 * r, 64 * r + 64)
        L = _L(t, tab["tuples"][:, sl])
        c = tab["cells"][sl]
        take = (L > bv) | ((L == bv) & (c[None] < bc))
        bv[take] = L[take]
        bc[take] = np.broadcast_to(c[None], bc.shape)[take]

    k = fkey(bnd)
    first = [r for r in range(rows) if k[0][r] == k[0].max() or k[1][r] == k[1].max()]
    for r in first:
        scan(r)
    V = bv.max(-1)
    with np.errstate(invalid="ignore"):
        keep = ~(bnd[0] < V[0]) | ~(bnd[1] < V[1])
    todo = [r for r in range(rows) if keep[r] and r not in first]
    if 2 * len(todo) > rows:  # flat scores: the exhaustive scan in first-cell order instead
        U = tab["U"]
        order = np.argsort(tab["cells"][:U], kind="stable")
        cell, mx = exhaustive(w2, tab["tuples"][:, :U][:, order], tab["cells"][:U][order])
        return cell, mx, rows
    for r in todo:
        scan(r)
    cell, mx = np.zeros(2, np.int64), np.zeros(2, F32)
    for f in range(2):
        kk = fkey(bv[f])
        top = kk == kk.max()
        mx[f] = bv[f][top][0] + F32(0)
        cell[f] = bc[f][top].min() if mx[f] > -np.inf else tab["cell0"]
    return cell, mx, len(first) + len(todo)
