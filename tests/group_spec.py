"""project_group_sparse!(y, group, J, k) (src/utilities.jl:613-679) stated as sets, in numpy, independent of oracle/iht_oracle.c
(which walks a sort permutation twice, as the reference does):

  1. within each group keep the k_g entries of largest |y|; among equal |y| the lower index goes first;
  2. a group's norm is the sum of the squares of what it kept, taken in that order (largest first), the square rounded, then the
     add rounded: ((0 + y1^2) + y2^2) + ... in float64 -- a sequential sum, no pairwise blocks (np.sum from 8 terms on), no fma;
  3. the groups 1..G, G = max(group), are ranked by norm, descending; among equal norms the lower label goes first.  A label that
     no entry carries is a group of norm 0 and takes its place in that ranking;
  4. the entries kept in (1) whose group is among the first J stay as they are (a kept -0.0 stays -0.0); every other entry
     becomes +0.0.

k is one integer or a vector with an entry per label (entries beyond G are ignored).  NaN is not covered: |y| has no order there.
No loop runs over the labels 1..G, only over what is present, so G may be far larger than len(y)."""
import numpy as np


def abs_bits(y):
    """The bit pattern of |y|: for anything but NaN its unsigned order is the order of |y|."""
    return np.ascontiguousarray(y, dtype=np.float64).view(np.uint64) & np.uint64(0x7FFFFFFFFFFFFFFF)


def sequential_norms(sq, owner, place, count):
    """norm[o] = ((0 + s_0) + s_1) + ... over the squares s of owner o in the order of `place` (0, 1, 2, ... within each owner):
    one float64 add at a time.  Vectorised ACROSS the owners (each takes part in a step at most once), never along the sum."""
    norm = np.zeros(count, dtype=np.float64)
    if sq.size == 0:
        return norm
    by_place = np.argsort(place, kind="stable")
    edge = np.searchsorted(place[by_place], np.arange(int(place.max()) + 2))
    for t in range(edge.size - 1):
        step = by_place[edge[t]:edge[t + 1]]
        norm[owner[step]] = norm[owner[step]] + sq[step]
    return norm


def group_parts(y, group, k):
    """(present labels ascending, their norms, kept_in_group per entry) -- steps 1 and 2."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    group = np.ascontiguousarray(group, dtype=np.int64)
    assert y.ndim == 1 and group.shape == y.shape and y.size >= 1 and group.min() >= 1 and not np.isnan(y).any()
    n = y.size
    kv = np.asarray(k, dtype=np.int64)
    kg = kv[group - 1] if kv.ndim else np.full(n, int(kv), dtype=np.int64)
    assert kg.min() >= 0
    # the members of each group from the largest |y| down, equal |y| by ascending index
    order = np.lexsort((np.arange(n), ~abs_bits(y), group))
    present, first, owner = np.unique(group[order], return_index=True, return_inverse=True)
    place = np.arange(n, dtype=np.int64) - first[owner]
    kept_sorted = place < kg[order]
    kept = np.zeros(n, dtype=bool)
    kept[order] = kept_sorted
    v = y[order][kept_sorted]
    with np.errstate(over="ignore", under="ignore"):
        norms = sequential_norms(v * v, owner[kept_sorted], place[kept_sorted], present.size)
    return present, norms, kept


def group_ranks(present, norms):
    """The 1-based rank of every PRESENT label among all labels 1..G by (norm descending, label ascending), the absent ones
    counted as norm 0: a group of positive norm is behind the groups of larger norm and those of equal norm and lower label; a
    group of norm 0 is behind every group of positive norm and every label below it that has norm 0, present or not."""
    pos = norms > 0.0
    rank = np.empty(present.size, dtype=np.int64)
    by = np.lexsort((present[pos], -norms[pos]))
    r = np.empty(by.size, dtype=np.int64)
    r[by] = np.arange(1, by.size + 1)
    rank[pos] = r
    below_pos = np.cumsum(pos) - pos                      # labels below this one with a positive norm
    rank[~pos] = (int(pos.sum()) + (present - 1) - below_pos + 1)[~pos]
    return rank


def project_group_sparse(y, group, J, k):
    y = np.ascontiguousarray(y, dtype=np.float64)
    group = np.ascontiguousarray(group, dtype=np.int64)
    present, norms, kept = group_parts(y, group, k)
    rank = group_ranks(present, norms)
    alive = rank[np.searchsorted(present, group)] <= int(J)
    return np.where(kept & alive, y, 0.0)


def group_norms(y, group, k):
    """{label: norm} of the present labels, by the sequential sum of step 2."""
    present, norms, _ = group_parts(y, group, k)
    return {int(g): float(v) for g, v in zip(present, norms)}
