"""Full-matrix restatement of the canonical alignment (include/msw.h, "Traceback").

TEST INFRASTRUCTURE ONLY.  A second implementation of the rule, independent of
the GPU kernel: it keeps the whole H (and E, F) matrices as integers and the
walk compares cell VALUES exactly as the rule's tables read (the kernel keeps
direction bits instead).  The fill applies the textbook recurrence of
oracle/sw_oracle.c cell by cell; the only concession to speed is that the
cells of one anti-diagonal, which do not depend on each other, are computed
in one numpy expression.

    align(read, win, match, mismatch, gap_open, gap_extend, affine)
        -> (score, (end_i, end_j), (start_i, start_j), ops)

ops: the CIGAR in forward order, run-length merged, BAM-encoded ints
(len << 4 | op, M = 0, I = 1, D = 2).
"""
import numpy as np

NEG = -(1 << 28)  # -inf for E / F: far below any reachable value, no overflow
M, I, D = 0, 1, 2


def _bytes(x):
    if isinstance(x, str):
        x = x.encode()
    return np.frombuffer(bytes(x), np.uint8) if isinstance(x, (bytes, bytearray)) else np.asarray(x, np.uint8)


def fill(read, win, match, mismatch, gap_open, gap_extend, affine):
    """H, E, F with a border: X[i + 1][j + 1] is the cell (i, j); row 0 and
    column 0 are the boundary (H = 0, E = F = -inf).  S[i][j] = s(i, j).
    Linear: E and F are None and `gap_extend` is the gap penalty."""
    r, w = _bytes(read), _bytes(win)
    m, n = len(r), len(w)
    S = np.where(r[:, None] == w[None, :], match, mismatch).astype(np.int64).reshape(m, n)
    H = np.zeros((m + 1, n + 1), np.int64)
    E = np.full((m + 1, n + 1), NEG, np.int64) if affine else None
    F = np.full((m + 1, n + 1), NEG, np.int64) if affine else None
    goe = gap_open + gap_extend
    for d in range(m + n - 1):  # anti-diagonal i + j == d
        i = np.arange(max(0, d - n + 1), min(m, d + 1))
        j = d - i
        a, b = i + 1, j + 1  # bordered indices of (i, j)
        diag = H[a - 1, b - 1] + S[i, j]
        if affine:
            e = np.maximum(E[a, b - 1] - gap_extend, H[a, b - 1] - goe)
            f = np.maximum(F[a - 1, b] - gap_extend, H[a - 1, b] - goe)
            E[a, b] = e
            F[a, b] = f
            H[a, b] = np.maximum(np.maximum(diag, e), np.maximum(f, 0))
        else:
            up = H[a - 1, b] - gap_extend
            left = H[a, b - 1] - gap_extend
            H[a, b] = np.maximum(np.maximum(diag, up), np.maximum(left, 0))
    return H, E, F, S


def best_cell(H):
    """(score, end_i, end_j): max score, then smallest i, then smallest j."""
    inner = H[1:, 1:]
    if inner.size == 0 or inner.max() <= 0:
        return 0, -1, -1
    k = int(np.argmax(inner))  # first maximum in row-major order
    i, j = divmod(k, inner.shape[1])
    return int(inner[i, j]), i, j


def walk(H, E, F, S, end_i, end_j, gap_open, gap_extend, affine):
    """The rule's tables, from (end_i, end_j) in state H.  Returns
    ((start_i, start_j), ops in walk order as a list of op codes)."""
    goe = gap_open + gap_extend
    h = lambda i, j: int(H[i + 1, j + 1])
    i, j, state = end_i, end_j, "H"
    start = (-1, -1)
    out = []
    while i >= 0 and j >= 0:
        if state == "H":
            if h(i, j) == 0:
                break
            if h(i, j) == h(i - 1, j - 1) + int(S[i, j]):
                out.append(M)
                start = (i, j)
                i, j = i - 1, j - 1
            elif not affine:
                if h(i, j) == h(i - 1, j) - gap_extend:
                    out.append(I)
                    i -= 1
                else:
                    out.append(D)
                    j -= 1
            elif h(i, j) == int(F[i + 1, j + 1]):
                state = "F"
            else:
                state = "E"
        elif state == "F":
            out.append(I)
            state = "H" if int(F[i + 1, j + 1]) == h(i - 1, j) - goe else "F"
            i -= 1
        else:
            out.append(D)
            state = "H" if int(E[i + 1, j + 1]) == h(i, j - 1) - goe else "E"
            j -= 1
    return start, out


def run_length(ops_forward):
    enc = []
    for op in ops_forward:
        if enc and enc[-1][1] == op:
            enc[-1][0] += 1
        else:
            enc.append([1, op])
    return [n << 4 | op for n, op in enc]


def align(read, win, match=2, mismatch=-1, gap_open=0, gap_extend=2, affine=False):
    H, E, F, S = fill(read, win, match, mismatch, gap_open, gap_extend, affine)
    score, ei, ej = best_cell(H)
    if score == 0:
        return 0, (-1, -1), (-1, -1), []
    start, rev = walk(H, E, F, S, ei, ej, gap_open, gap_extend, affine)
    return score, (ei, ej), start, run_length(rev[::-1])


def cigar_text(ops):
    return "".join(f"{o >> 4}{'MID'[o & 15]}" for o in ops) if len(ops) else "*"


def consumed(ops):
    """(read bases, window bases) an op list consumes."""
    r = sum(o >> 4 for o in ops if (o & 15) in (M, I))
    w = sum(o >> 4 for o in ops if (o & 15) in (M, D))
    return r, w


def rescore(ops, read, win, start, match, mismatch, gap_open, gap_extend, affine):
    """Score of the alignment the ops describe from `start` under the scheme."""
    r, w = _bytes(read), _bytes(win)
    i, j = start
    total = 0
    for o in ops:
        n, op = o >> 4, o & 15
        if op == M:
            for _ in range(n):
                total += match if r[i] == w[j] else mismatch
                i, j = i + 1, j + 1
        else:
            total -= (gap_open + n * gap_extend) if affine else n * gap_extend
            if op == I:
                i += n
            else:
                j += n
    return total, (i - 1, j - 1)
