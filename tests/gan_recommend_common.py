"""Host restatement of rg_gan_recommend's selection (include/rg_hip.h), shared by the CPU and GPU
tests: a plain NumPy loop over rows and heads on a given block of head outputs."""
import numpy as np

FLAGS = [(False, False), (True, False), (False, True), (True, True)]     # (exclude_history, distinct)


def flag_bits(exclude_history, distinct):
    return (1 if exclude_history else 0) | (2 if distinct else 0)


def replay(fake, hist, N, S, exclude_history, distinct):
    """slates (rows, S) int64 from ``fake`` (rows, >= S * N) head outputs and ``hist`` (rows, L) ids:
    heads in order, each the allowed item with the largest value (NaN below every number), equal
    values to the lower id, no allowed item left: N.  History ids outside [0, N) are ignored."""
    fake, hist = np.asarray(fake), np.asarray(hist)
    rows = fake.shape[0]
    out = np.full((rows, S), N, dtype=np.int64)
    for r in range(rows):
        allowed = np.ones(N, dtype=bool)
        if exclude_history:
            h = hist[r]
            allowed[h[(h >= 0) & (h < N)]] = False
        for s in range(S):
            ids = np.flatnonzero(allowed)
            if not len(ids):
                continue
            v = fake[r, s * N:(s + 1) * N][ids]
            v = np.where(np.isnan(v), -np.inf, v)
            best = int(ids[np.argmax(v)])             # the first maximum: the lower id
            out[r, s] = best
            if distinct:
                allowed[best] = False
    return out


def histories(rs, rows, N, L):
    """(rows, L) int32 histories with repeated ids and padding: row 0 is all padding, every other
    row holds a random number of random ids (repeats allowed) and padding after them, and one
    padding id sits in the middle of row 1's items when the row is long enough."""
    hist = np.full((rows, L), N, dtype=np.int32)
    for r in range(1, rows):
        n = rs.randint(1, L + 1)
        hist[r, :n] = rs.randint(0, N, n)
    if rows > 1 and L > 2:
        hist[1, :3] = [hist[1, 0], N, hist[1, 0]]
    return hist
