"""X beta over a small support (csrc/xv.hip) on the paths a FIT takes: the LRU column cache (xv_cache_lookup, k_xv_fill,
k_xv_snp_cached), the pinned ring that hands over slot and fill lists (HostStage), the coefficients gathered on the way, clamp20
behind the fix-up of imputed entries, the fallback of a support that outgrows the cache with the regrowth of the coefficient
buffers, both multi-trait kernels (k_xv_snp_cached_mt<4|6|8|10|12>, k_xv_snp_cached_multi<4>) and k_xv_coef_groups with its
padded records.  mih_xv_sparse -- the product's one public entry -- runs none of them (fresh workspace, k_xv_snp), so the
measurement build's mih_probe_xv_sequence drives sequences of calls on ONE workspace in a process of its own, and this process
holds every result against three independent references:

  (a) the exact rational X beta with an a-priori forward bound (gpu_helpers.xv_exact_misses), nothing of it measured;
  (b) the product's direct path, bit for bit: x.xv_sparse(idx, val) on a fresh workspace in THIS process (np.clip of it under
      clamp20); every trait row of a multi-trait call against the single-vector result of that trait's coefficients, under all
      three settings of MENDELIHT_XV_MULTI (unset: k_xv_snp_cached_mt, "2": k_xv_snp_cached_multi, "0": one cached pass per trait);
  (c) a numpy restatement of the summation order the kernels' comments document (gpu_helpers.xv_documented_order), bit for bit,
      where no imputed entry needs the fix-up (its `out += mu a` may or may not be contracted; (a) and (b) cover it).

The bit-equality of resident, host-driven, lock-step and column-sharded fits rests on (b); (c) pins WHAT order that is."""
import numpy as np
import pytest

from conftest import make_bed
from gpu_helpers import _dosages, _run_probe_snippet, rel, xv_documented_order, xv_exact_misses

pytestmark = pytest.mark.gpu

_ENVS = {"mt": {}, "multi": {"MENDELIHT_XV_MULTI": "2"}, "per_trait": {"MENDELIHT_XV_MULTI": "0"}}

# jobs from <out>.in.npz: job j = one matrix (its own columns, a seeded synthetic one, or the previous job's) and ONE call of
# mih_probe_xv_sequence, i.e. one workspace
_SNIPPET = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import mendeliht_amd as m
from mendeliht_amd import api
assert m.using_probes()
inp = np.load(sys.argv[2] + ".in.npz")
out, x = {}, None
for j in range(int(inp["njobs"])):
    n, c, s, i, max_nnz, cache_nnz = (int(v) for v in inp[f"j{j}_meta"])
    if f"j{j}_cols" in inp.files:
        x = m.SnpLinAlg(inp[f"j{j}_cols"], n, center=c, scale=s, impute=i)
    elif f"j{j}_syn" in inp.files:
        x = m.SnpLinAlg.synthetic(n, int(inp[f"j{j}_syn"][0]), seed=int(inp[f"j{j}_syn"][1]), center=c, scale=s, impute=i)
    nnz = np.ascontiguousarray(inp[f"j{j}_nnz"], dtype=np.int64)
    mm = np.ascontiguousarray(inp[f"j{j}_m"], dtype=np.int32)
    fl = np.ascontiguousarray(inp[f"j{j}_flags"], dtype=np.int32)
    idx = np.ascontiguousarray(inp[f"j{j}_idx"], dtype=np.int64)
    val = np.ascontiguousarray(inp[f"j{j}_val"], dtype=np.float64)
    res = np.full(int(mm.astype(np.int64).sum()) * x.n, np.nan)
    gat = np.full(max(val.size, 1), np.nan)
    api._check(api.lib().mih_probe_xv_sequence(x._h, max_nnz, cache_nnz, nnz.size, api._p(nnz), api._p(mm), api._p(fl),
                                               api._p(idx), api._p(val), api._p(res), api._p(gat)))
    out[f"j{j}_out"], out[f"j{j}_gat"] = res, gat
np.savez(sys.argv[2], **out)
"""

_LUT = np.array([[(0, 0, 1, 2)[(b >> (2 * t)) & 3] for t in range(4)] for b in range(256)], dtype=np.int8)     # PLINK code -> stored dosage
_LUT_MISS = np.array([[((b >> (2 * t)) & 3) == 1 for t in range(4)] for b in range(256)], dtype=bool)


def _decode(cols, n):
    """PLINK column bytes (k, ceil(n / 4)) -> the stored dosages (n x k, int8; 0 where missing) and the missing mask (n x k)."""
    k = cols.shape[0]
    return _LUT[cols].reshape(k, -1)[:, :n].T, _LUT_MISS[cols].reshape(k, -1)[:, :n].T


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _rows_for_exact(n):
    """(a) runs on every row up to n = 1100; beyond: rows 0..63, the last 64 and every 17th (the bitwise checks cover every row)."""
    if n <= 1100:
        return np.arange(n)
    return np.unique(np.concatenate([np.arange(64), np.arange(n - 64, n), np.arange(0, n, 17)]))


class _Job:
    """One workspace: a matrix and a sequence of calls (idx, val (m x nnz), flags)."""

    def __init__(self, n, flags, max_nnz, cache_nnz, cols=None, syn=None):
        self.n, self.csi, self.max_nnz, self.cache_nnz, self.cols, self.syn = n, tuple(int(f) for f in flags), max_nnz, cache_nnz, cols, syn
        self.calls = []

    def call(self, idx, val, flags=0):
        idx = np.asarray(idx, dtype=np.int64)
        val = np.atleast_2d(np.asarray(val, dtype=np.float64))
        assert val.shape[1] == idx.size and (val.shape[0] == 1 or flags == 0)
        self.calls.append((idx, val, int(flags)))
        return self


def _run_jobs(jobs, out_file, extra_env=None):
    """The jobs in ONE process of the measurement build; returns per job the list of (out (m x n), gathered (nnz) or None)."""
    inp = {"njobs": np.int64(len(jobs))}
    for j, jb in enumerate(jobs):
        inp[f"j{j}_meta"] = np.array([jb.n, *jb.csi, jb.max_nnz, jb.cache_nnz], dtype=np.int64)
        if jb.cols is not None:
            inp[f"j{j}_cols"] = jb.cols
        elif jb.syn is not None:
            inp[f"j{j}_syn"] = np.array(jb.syn, dtype=np.int64)
        inp[f"j{j}_nnz"] = np.array([c[0].size for c in jb.calls], dtype=np.int64)
        inp[f"j{j}_m"] = np.array([c[1].shape[0] for c in jb.calls], dtype=np.int32)
        inp[f"j{j}_flags"] = np.array([c[2] for c in jb.calls], dtype=np.int32)
        inp[f"j{j}_idx"] = np.concatenate([c[0] for c in jb.calls] + [np.zeros(0, np.int64)])
        inp[f"j{j}_val"] = np.concatenate([c[1].ravel() for c in jb.calls] + [np.zeros(0)])
    np.savez(str(out_file) + ".in.npz", **inp)
    got = _run_probe_snippet(_SNIPPET, out_file, extra_env=extra_env, timeout=1500)
    res = []
    for j, jb in enumerate(jobs):
        out, gat, oo, vo, per_call = got[f"j{j}_out"], got[f"j{j}_gat"], 0, 0, []
        for idx, val, fl in jb.calls:
            m = val.shape[0]
            per_call.append((out[oo:oo + m * jb.n].reshape(m, jb.n), gat[vo:vo + idx.size] if fl & 2 else None))
            oo += m * jb.n; vo += m * idx.size
        res.append(per_call)
    return res


class _Ref:
    """The references of one matrix in this process: the product library's handle (direct path, its mu and sinv), the decoded
    dosages, and a memo of the direct results (the same coefficients come back under the three multi-trait settings)."""

    def __init__(self, mih, n, csi, cols=None, syn=None):
        c, s, i = csi
        if cols is not None:
            self.x = mih.SnpLinAlg(cols, n, center=c, scale=s, impute=i)
        else:
            self.x = mih.SnpLinAlg.synthetic(n, syn[0], seed=syn[1], center=c, scale=s, impute=i)
        self.cols = cols
        self.n, self.csi = n, (int(c), int(s), int(i))
        self.mu, self.sinv = self.x.mu_sigma()
        self.memo, self.dec = {}, {}

    def decoded(self, idx):
        key = idx.tobytes()
        if key not in self.dec:
            if self.cols is None:
                self.cols = self.x.export_bed()
            self.dec = {key: _decode(self.cols[idx], self.n)}          # (one support at a time: the big shape's is 400 MB)
        return self.dec[key]

    def direct(self, idx, v):
        key = (idx.tobytes(), v.tobytes())
        if key not in self.memo:
            self.memo[key] = self.x.xv_sparse(idx, v)
        return self.memo[key]


def _check_call(ref, idx, val, fl, out, gat, tag, exact_traits=None, restate=True):
    """(a), (b), (c) for one call; exact_traits: the trait rows (a) runs on (None = all)."""
    c, s, i = ref.csi
    m, nnz = val.shape
    assert out.shape == (m, ref.n) and not np.isnan(out).any(), tag
    G, miss = ref.decoded(idx) if nnz else (np.zeros((ref.n, 0), np.int8), np.zeros((ref.n, 0), bool))
    if gat is not None:
        assert _same_bits(gat, val[0]), tag                          # gather_out: the coefficients, bit for bit (-0.0 included)
    for v in range(m):
        direct = ref.direct(idx, val[v])
        want = np.clip(direct, -20.0, 20.0) if fl & 4 else direct
        if not _same_bits(out[v], want):                             # (b)
            bad = np.flatnonzero(_bits(out[v]) != _bits(want))
            raise AssertionError(f"{tag} trait {v}: {bad.size} of {ref.n} rows differ from the direct path, first row {bad[0]}: "
                                 f"{out[v][bad[0]]!r} against {want[bad[0]]!r} (rel {rel(out[v], want):.3g})")
        if restate and nnz and (i == 0 or not miss.any()):           # (c)
            a = (ref.sinv[idx] if s else 1.0) * val[v]
            b = -ref.mu[idx] * a if c else np.zeros(nnz)
            doc = xv_documented_order(G, a, b)
            if not _same_bits(direct, doc):
                bad = np.flatnonzero(_bits(direct) != _bits(doc))
                raise AssertionError(f"{tag} trait {v}: {bad.size} rows differ from the documented order, first row {bad[0]}: "
                                     f"{direct[bad[0]]!r} against {doc[bad[0]]!r}")
        if exact_traits is None or v in exact_traits:                # (a)
            bad = xv_exact_misses(out[v], G, miss, ref.mu[idx], ref.sinv[idx], val[v], c, s, i, _rows_for_exact(ref.n), clamp20=bool(fl & 4))
            assert not bad, (tag, v, len(bad), bad[:3])


def _check_job(ref, job, got, tag, exact_traits=None, restate=True):
    for k, ((idx, val, fl), (out, gat)) in enumerate(zip(job.calls, got)):
        _check_call(ref, idx, val, fl, out, gat, f"{tag} call {k} (nnz {idx.size}, m {val.shape[0]}, flags {fl})",
                    exact_traits=exact_traits(val.shape[0]) if callable(exact_traits) else exact_traits, restate=restate)


class _LruModel:
    """xv_cache_lookup restated, to PROVE what the walk below exercises (evictions, returns of evicted columns)."""

    def __init__(self, slots):
        self.slots, self.col_of, self.stamp, self.slot_of, self.tick = slots, [-1] * slots, [0] * slots, {}, 0
        self.evicted, self.returns, self.fills = set(), 0, 0

    def lookup(self, idx):
        if len(idx) > self.slots:
            return False
        self.tick += 1
        miss = []
        for j in idx:
            if j in self.slot_of:
                self.stamp[self.slot_of[j]] = self.tick
            else:
                miss.append(j)
        order = sorted((sl for sl in range(self.slots) if self.stamp[sl] != self.tick), key=lambda sl: (self.stamp[sl], sl))
        if len(order) < len(miss):
            return False
        for j, sl in zip(miss, order):
            if self.col_of[sl] >= 0:
                self.slot_of.pop(self.col_of[sl], None)
                self.evicted.add(self.col_of[sl])
            self.returns += j in self.evicted
            self.evicted.discard(j)
            self.col_of[sl] = j; self.slot_of[j] = sl; self.stamp[sl] = self.tick
            self.fills += 1
        return True


def test_lru_walk_eviction_fallback_and_ring_wrap(mih, tmp_path):
    """A fit's drift of the support on a cache of 80 slots (max_nnz 64, cache_nnz 8): 60 supports of 20 - 40 columns with 1 - 3
    replaced per call, more than 80 distinct columns, so slots are evicted and evicted columns come back; one support with a
    duplicated index (mih_xv_sparse accepts it); then 80 entirely new columns (every slot replaced), 81 columns (direct fallback,
    nnz > cap: the coefficient buffers regrow), an earlier support again (the cache is still coherent), the empty support.
    flags alternate 0 .. 3 with a run of 15 staged calls (the pinned ring of 8 slots wraps)."""
    n, p = 1003, 700
    rng = np.random.default_rng(20260)
    cols = make_bed(rng, n, p)
    job = _Job(n, (1, 1, 1), 64, 8, cols=cols)
    supp = [int(j) for j in rng.choice(p, 30, replace=False)]
    dropped_early = []
    walk = []
    for k in range(60):
        if k:
            for _ in range(int(rng.integers(1, 4))):
                out_pos = int(rng.integers(len(supp)))
                if k < 6:
                    dropped_early.append(supp[out_pos])
                fresh = [j for j in (dropped_early if k in (50, 55) else rng.permutation(p)) if j not in supp]
                supp[out_pos] = int(fresh[0])                        # calls 50 and 55 bring back columns dropped in the first steps
            if len(supp) < 40 and rng.random() < 0.4:
                supp.append(int([j for j in rng.permutation(p) if j not in supp][0]))
            elif len(supp) > 20 and rng.random() < 0.3:
                supp.pop(int(rng.integers(len(supp))))
        fl = (1 if k % 2 else 3) if 20 <= k < 35 else k % 4
        lst = list(supp)
        if k == 10:                                                  # a column that is not cached yet, twice in one list
            lst += [int([j for j in range(p) if j not in supp][0])] * 2
            fl = 1
        walk.append(np.array(lst, dtype=np.int64))
        job.call(walk[-1], rng.standard_normal(len(lst)) * 0.3, fl)
    seen = set(np.concatenate(walk).tolist())
    assert len(seen) > 80 and all(20 <= w.size <= 42 for w in walk)
    new80 = np.array([j for j in rng.permutation(p) if j not in seen][:80], dtype=np.int64)
    job.call(new80, rng.standard_normal(80) * 0.2, 1)
    new81 = rng.choice(p, 81, replace=False)
    job.call(new81, rng.standard_normal(81) * 0.2, 3)
    job.call(walk[57], rng.standard_normal(walk[57].size) * 0.3, 2)
    job.call(walk[3], rng.standard_normal(walk[3].size) * 0.3, 1)
    job.call(np.zeros(0, np.int64), np.zeros(0), 0)
    job.call(np.zeros(0, np.int64), np.zeros(0), 3)
    job.call(walk[30], rng.standard_normal(walk[30].size) * 0.3, 0)
    # what the sequence does to the cache, by the rule of xv_cache_lookup
    lru, cached = _LruModel(80), []
    for k, (idx, _, _) in enumerate(job.calls):
        before = lru.fills
        cached.append(bool(idx.size) and lru.lookup(idx.tolist()))
        if k == 59:
            assert all(cached) and lru.returns >= 2 and len(lru.evicted) > 20      # within the walk: evictions, and evicted columns back
        if k == 60:
            assert lru.fills - before == 80                          # every slot replaced
    assert cached[60] and not cached[61] and cached[62] and cached[63]
    staged = [bool(fl & 1) and ok for (_, _, fl), ok in zip(job.calls, cached)]
    assert max(len(run) for run in "".join("x" if s_ else " " for s_ in staged).split()) > 8

    ref = _Ref(mih, n, (1, 1, 1), cols=cols)
    G_all, miss_all = _decode(cols, n)
    assert np.array_equal(G_all.T, _dosages(cols, n)) and not miss_all.any()
    (got,) = _run_jobs([job], tmp_path / "lru.npz")
    assert np.all(_bits(got[64][0]) == 0) and np.all(_bits(got[65][0]) == 0)      # the empty support: +0.0
    _check_job(ref, job, got, "lru")


_SIZES = (1, 2, 7, 8, 9, 15, 16, 17, 18, 23, 24, 25, 31, 32, 33, 63, 64, 65, 129)


@pytest.mark.parametrize("env", sorted(_ENVS))
def test_support_sizes_around_the_group_and_batch_boundaries(mih, tmp_path, env):
    """nnz on both sides of every boundary of the kernels (16 column groups, batches of 4 and 8 columns, per = 2, 3, 5, 9), the
    coefficients over ten decades, on ONE workspace that caches them all (384 slots) and on one of 80 slots where 129 columns take
    the direct kernel with regrown buffers; an all-zero coefficient vector with -0.0 entries gives +0.0 on every path."""
    n, p = 1003, 700
    rng = np.random.default_rng(20261)
    cols = make_bed(rng, n, p)
    jobs = [_Job(n, (1, 1, 1), 160, 0, cols=cols), _Job(n, (1, 1, 1), 64, 8)]
    zero = np.zeros(17); zero[[0, 3, 8, 16]] = -0.0
    zidx = np.sort(rng.choice(p, 17, replace=False))
    for jb in jobs:
        for k, nnz in enumerate(_SIZES):
            idx = rng.choice(p, nnz, replace=False)
            jb.call(idx, rng.standard_normal(nnz) * 10.0 ** rng.uniform(-5, 5, nnz), k % 4)
            if nnz in (1, 9, 17, 25, 65):
                jb.call(idx, rng.standard_normal((5, nnz)) * 10.0 ** rng.uniform(-5, 5, (5, nnz)))
        for fl in range(4):
            jb.call(zidx, zero, fl)
        for m in (2, 5, 13):
            jb.call(zidx, np.tile(zero, (m, 1)))
    ref = _Ref(mih, n, (1, 1, 1), cols=cols)
    got = _run_jobs(jobs, tmp_path / f"sizes_{env}.npz", _ENVS[env])
    for w, (jb, g) in enumerate(zip(jobs, got)):
        for (idx, val, _), (out, _) in zip(jb.calls, g):
            if not val.any():
                assert np.all(_bits(out) == 0), (w, val.shape)       # +0.0, never -0.0
        _check_job(ref, jb, g, f"sizes[{env}] workspace {w}", exact_traits=lambda m: (0, m - 1))


_MS = (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16, 17, 24, 25, 31, 32)
_MT_NNZ = (64, 1, 65, 7, 17, 8, 25, 9, 18, 16)          # not ascending: a short support finds a longer one's records behind its own


@pytest.mark.parametrize("env", sorted(_ENVS))
def test_trait_counts_cross_support_sizes(mih, tmp_path, env):
    """Every template of k_xv_snp_cached_mt (m <= 4, 6, 8, 10, 12), trait slots past m, two and three y-chunks (m = 13, 24, 25: the
    second chunk's record reads run into the next record), up to the largest trait count a multivariate fit accepts (m = 16, 17:
    a second chunk of 4 and 5 traits; m = 31, 32: 12 + 12 + 7 and 12 + 12 + 8, records of 32 doubles of which the last is
    padding at 31 and none is at 32), against nnz with empty trailing groups (17: 9 of 16 groups), padding of 7, 0 and 1 columns,
    per = 1 .. 5.  One workspace per m: the cache persists across the supports, the coefficient buffers regrow (cap 72: the first
    call's 64 m coefficients exceed it for every m >= 2, so the regrowth does not depend on the largest m).  (a) runs on the
    first and the last trait, (b) and (c) on every trait."""
    n, p = 1003, 700
    rng = np.random.default_rng(20262)
    cols = make_bed(rng, n, p)
    jobs = []
    for m in _MS:
        jb = _Job(n, (1, 1, 1), 72, 0, cols=cols if not jobs else None)
        for nnz in _MT_NNZ:
            jb.call(rng.choice(150, nnz, replace=False), rng.standard_normal((m, nnz)) * 10.0 ** rng.uniform(-2, 2, (m, nnz)))
        jobs.append(jb)
    ref = _Ref(mih, n, (1, 1, 1), cols=cols)
    got = _run_jobs(jobs, tmp_path / f"traits_{env}.npz", _ENVS[env])
    for jb, g, m in zip(jobs, got, _MS):
        _check_job(ref, jb, g, f"traits[{env}] m {m}", exact_traits=(0, m - 1))


_RAGGED_N = (1, 2, 15, 16, 17, 31, 33, 255, 256, 257, 4097)
_RAGGED_FLAGS = ((1, 1, 1), (0, 0, 0), (1, 0, 1), (0, 1, 0))


@pytest.mark.parametrize("env", sorted(_ENVS))
def test_ragged_row_counts(mih, tmp_path, env):
    """n around the 16-row dword, the row PAIR of a k_xv_snp_cached_mt thread (odd n: the second row of the last pair is not
    stored), the 256-row workgroup and the 128-row block pair, for m = 1, 5, 12 and nnz = 3, 17 under every use of the flags."""
    rng = np.random.default_rng(20263)
    jobs, refs = [], []
    for n in _RAGGED_N:
        cols = make_bed(rng, n, 40)
        for csi in _RAGGED_FLAGS:
            jb = _Job(n, csi, 64, 0, cols=cols)
            for nnz in (3, 17):
                idx = rng.choice(40, nnz, replace=False)
                jb.call(idx, rng.standard_normal(nnz), 1)
                jb.call(idx, rng.standard_normal(nnz), 2)
                for m in (5, 12):
                    jb.call(idx, rng.standard_normal((m, nnz)))
            jobs.append(jb)
            refs.append((n, csi, cols))
    got = _run_jobs(jobs, tmp_path / f"ragged_{env}.npz", _ENVS[env])
    for jb, g, (n, csi, cols) in zip(jobs, got, refs):
        _check_job(_Ref(mih, n, csi, cols=cols), jb, g, f"ragged[{env}] n {n} flags {csi}")


@pytest.mark.parametrize("env", sorted(_ENVS))
def test_missing_genotypes_fixup_and_clamp(mih, oracle, tmp_path, env):
    """5 % missing entries, a support column with two observed entries in 1003 and one without a missing entry, with and
    without impute.  clamp20 must act BEHIND the fix-up of the imputed entries: the coefficients are scaled so that rows cross
    +-20 in both directions through the fix-up.  A multi-trait call on a matrix that needs the fix-up takes the per-trait path
    and still gives the direct path's bits.  (a) on every row of every call.
    A column that is missing ENTIRELY has mu = 0 / 0 = NaN, here as in the reference (the mean over no observation), and with
    centring its -mu a term reaches every row: no exact value exists for (a).  Such a column (the last one) rides in calls of
    its own, where every path must give NaN in exactly the rows where the direct path does -- all of them."""
    n, p = 1003, 60
    rng = np.random.default_rng(20264)
    cols = make_bed(rng, n, p, missing_rate=0.05)
    for j in (0, p - 1):
        cols[j, :] = 0x55                                            # every entry missing (the pad entries of the last byte stay 0)
        cols[j, -1] = 0x15
    for row, code in ((5, 2), (700, 3)):                             # column 0: dosage 1 in row 5, dosage 2 in row 700
        cols[0, row // 4] = (int(cols[0, row // 4]) & (0xFF ^ (3 << 2 * (row % 4)))) | (code << 2 * (row % 4))
    cols[1] = make_bed(rng, n, 1)[0]
    G_all, miss_all = _decode(cols, n)
    assert miss_all[:, p - 1].all() and miss_all[:, 0].sum() == n - 2 and G_all[5, 0] == 1 and G_all[700, 0] == 2
    assert not miss_all[:, 1].any() and 0.03 < miss_all[:, 2:p - 1].mean() < 0.07
    jobs, refs = [], []
    for csi in ((1, 1, 1), (1, 1, 0)):
        ref = _Ref(mih, n, csi, cols=cols)
        assert np.isnan(ref.mu[p - 1]) and np.isfinite(ref.mu[:p - 1]).all() and np.isfinite(ref.sinv).all()
        jb = _Job(n, csi, 64, 0, cols=cols)
        idx = np.concatenate([[0, 1], 2 + rng.choice(p - 3, 18, replace=False)])
        val = rng.standard_normal(20) * 5.0
        if csi[2]:                                                   # the inputs do what the docstring says (mu and sinv of this handle)
            a = ref.sinv[idx] * val
            pre = xv_documented_order(G_all[:, idx], a, -ref.mu[idx] * a)
            post = pre + (miss_all[:, idx] * (ref.mu[idx] * a)).sum(axis=1)
            assert np.sum((np.abs(pre) > 20.5) & (np.abs(post) < 19.5)) >= 3 and np.sum((np.abs(pre) < 19.5) & (np.abs(post) > 20.5)) >= 3
        for fl in (0, 4, 1, 5, 2, 6, 3, 7):
            jb.call(idx, val, fl)
        for nnz in (1, 2, 17, 33):
            jdx = rng.choice(p - 1, nnz, replace=False)
            jb.call(jdx, rng.standard_normal(nnz) * 5.0, 5)
            jb.call(jdx, rng.standard_normal((3, nnz)))
            jb.call(jdx, rng.standard_normal((12, nnz)))
        jb.call(np.array([0]), np.array([2.5]), 4)                   # the nearly empty column alone
        jb.call(np.array([0, 1]), rng.standard_normal((5, 2)))
        nan_from = len(jb.calls)
        jb.call(np.array([p - 1, 1]), np.array([2.5, -1.0]), 1)      # the entirely missing column
        jb.call(np.array([1, 7, p - 1]), rng.standard_normal((5, 3)))
        jobs.append(jb); refs.append((ref, nan_from))
    got = _run_jobs(jobs, tmp_path / f"missing_{env}.npz", _ENVS[env])
    for jb, g, (ref, nan_from) in zip(jobs, got, refs):
        for (idx, val, _), (out, _) in zip(jb.calls[nan_from:], g[nan_from:]):
            for v in range(val.shape[0]):
                direct = ref.direct(idx, val[v])
                assert np.isnan(direct).all() and np.isnan(out[v]).all(), (ref.csi, idx, v)
        jb.calls = jb.calls[:nan_from]
        _check_job(ref, jb, g[:nan_from], f"missing[{env}] flags {ref.csi}")
    refs = [r for r, _ in refs]
    # the direct path itself against the oracle on this matrix (what (b) is anchored to)
    ox = oracle.Mat.from_bed_columns(cols, n, center=1, scale=1, impute=1)
    idx, val, _ = jobs[0].calls[0]
    mask = np.zeros(p, np.uint8); mask[idx] = 1
    coef = np.zeros(p); coef[idx] = val[0]
    assert rel(refs[0].direct(idx, val[0]), ox.xv_masked(mask, coef)) < 1e-11


def test_one_large_shape(mih, tmp_path):
    """n = 5,000,001 (odd; 312,501 dwords per column, cache slots of 1.25 MB): m = 10 over 40 columns, then m = 1 staged and
    gathered on the same workspace.  (b) and (c) on every row, (a) on rows 0..63, the last 64 and every 17th of the first
    trait and of the single-vector call."""
    n, p, seed = 5_000_001, 300, 20265
    rng = np.random.default_rng(seed)
    idx = rng.choice(p, 40, replace=False)
    job = _Job(n, (1, 1, 1), 64, 0, syn=(p, seed))
    job.call(idx, rng.standard_normal((10, 40)) * 0.2)
    job.call(idx, rng.standard_normal(40) * 0.2, 3)
    (got,) = _run_jobs([job], tmp_path / "large.npz")
    ref = _Ref(mih, n, (1, 1, 1), syn=(p, seed))
    assert not ref.decoded(idx)[1].any()                             # no missing entry: (c) applies
    _check_job(ref, job, got, "large", exact_traits=(0,))
