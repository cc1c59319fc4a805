"""The numpy statement of SnpLinAlg.counts and SnpLinAlg.filter (SnpArrays.filter's keywords and defaults, without the
Hardy-Weinberg test) over an n x p array of allele counts with -1 for a missing genotype.  It is the yardstick of the device
path: the device supplies integer counts, so every comparison with it is exact."""
import numpy as np


def as_mask(sel, length):
    """A boolean mask or an index array (None: everything) as a boolean mask."""
    if sel is None:
        return np.ones(length, dtype=bool)
    sel = np.asarray(sel)
    if sel.dtype == bool:
        return sel.copy()
    m = np.zeros(length, dtype=bool)
    m[sel] = True
    return m


def counts(codes, rows=None, cols=None):
    """(col_counts (p, 4) int32: n0, n1, n2, nmiss of the kept columns over the kept rows, zeros elsewhere;
    row_missing (n,) int32: missing genotypes of the kept rows among the kept columns, 0 elsewhere)."""
    n, p = codes.shape
    r, c = as_mask(rows, n), as_mask(cols, p)
    sub = codes[r]
    cc = np.stack([(sub == v).sum(axis=0) for v in (0, 1, 2, -1)], axis=1).astype(np.int32)
    cc[~c] = 0
    rm = (codes[:, c] == -1).sum(axis=1).astype(np.int32)
    rm[~r] = 0
    return cc, rm


def maf(col_counts):
    n0, n1, n2 = (col_counts[:, k].astype(np.float64) for k in range(3))
    with np.errstate(invalid="ignore", divide="ignore"):
        f = (n1 + 2.0 * n2) / (2.0 * (n0 + n1 + n2))
    return np.minimum(f, 1.0 - f)


def filter(codes, min_success_rate_per_row=0.98, min_success_rate_per_col=0.98, min_maf=0.01, maxiters=5):
    """(rmask, cmask, rounds, converged)."""
    n, p = codes.shape
    rmask, cmask = np.ones(n, dtype=bool), np.ones(p, dtype=bool)
    rmiss, cmiss = 1.0 - min_success_rate_per_row, 1.0 - min_success_rate_per_col
    rounds = 0
    for _ in range(maxiters):
        rounds += 1
        cc, rm = counts(codes, rmask, cmask)                # both counts before either mask changes
        rows, cols = int(rmask.sum()), int(cmask.sum())
        ckeep = cmask & (cc[:, 3] < cmiss * rows)
        if min_maf > 0:
            with np.errstate(invalid="ignore"):
                ckeep &= maf(cc) >= min_maf                 # NaN fails
        rkeep = rmask & (rm < rmiss * cols)
        changed = int(rkeep.sum()) != rows or int(ckeep.sum()) != cols
        rmask, cmask = rkeep, ckeep
        if not changed:
            return rmask, cmask, rounds, True
    return rmask, cmask, rounds, False


def crafted_codes():
    """1000 x 200: a block of missing genotypes, and a row and a column that survive the first round by the float64 value of
    1 - 0.98 alone and fall in the second."""
    rng = np.random.default_rng(7)
    n, p = 1000, 200
    codes = rng.integers(0, 3, (n, p))
    codes[:100, :20] = -1
    codes[100:119, 50] = -1
    codes[500, [50, 60, 70, 80]] = -1
    codes[:, 90] = 0
    codes[3:, 91] = 0
    codes[:3, 91] = 1
    return codes
