"""project_group_sparse! on the device at its edges: the three stable radix sorts of csrc/group.hip (k_rs_hist, k_rs_scan,
k_rs_scatter) and the kernels around them (k_grp_keys, k_grp_labels, k_grp_bounds, k_grp_norms, k_grp_rank, k_grp_apply) through
the public mih.project_group_sparse, against the oracle bit for bit on gpu_helpers.group_edge_cases() -- equal |y| (stability is
the only decider), signed zeros, denormals and infinities, keys that differ in one byte, lengths around the tile, the round, the
wave and the scan chunk, labels that use the third and fourth byte, empty groups, degenerate J and k, ties with a known answer --
and one fit whose labels are interleaved and whose projection spans three tiles.  tests/test_group_spec_cpu.py shows without a
device that the oracle is the set-based statement of tests/group_spec.py on every case and that every case is what its name says;
DESIGN.md ("The group projection at its edges") has the table of edges."""
import numpy as np
import pytest

from gpu_helpers import GROUP_FIT_N, group_edge_cases, group_fit_problem, group_known_answers

pytestmark = pytest.mark.gpu

_CASES = group_edge_cases()


@pytest.fixture(scope="module")
def projected(oracle):
    """oracle.project_group_sparse of every case, computed once."""
    return [oracle.project_group_sparse(y, group, J, k) for _, y, group, J, k in _CASES]


def _same_bits(got, want, name):
    diff = np.flatnonzero((got != want) | (np.signbit(got) != np.signbit(want)))
    assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want)), \
        (name, "first differing indices", diff[:8], "non-zeros", np.count_nonzero(got), np.count_nonzero(want))


@pytest.mark.parametrize("t", range(len(_CASES)), ids=[c[0] for c in _CASES])
def test_project_group_sparse_at_its_edges(mih, projected, t):
    """mih.project_group_sparse = oracle.project_group_sparse, entry for entry and sign for sign, no tolerance; the caller's y,
    group and k are left as they were; the hand-written answer of a tie case is met."""
    name, y, group, J, k = _CASES[t]
    before = (y.copy(), group.copy(), np.copy(k))
    got = mih.project_group_sparse(y, group, J, k)
    _same_bits(got, projected[t], name)
    assert np.array_equal(y.view(np.uint64), before[0].view(np.uint64)) and np.array_equal(group, before[1]) and np.array_equal(k, before[2]), name
    known = group_known_answers().get(name)
    if known is not None:
        _same_bits(got, known, name)


def test_a_second_call_gives_the_same_bits(mih, projected):
    for t, (name, y, group, J, k) in enumerate(_CASES):
        if group.max() > 2 ** 20:                            # (the one case whose scratch is sized by G = 2^24 + 3 runs once, above)
            continue
        _same_bits(mih.project_group_sparse(y, group, J, k), projected[t], name)


def test_argument_errors(mih):
    """What the reference answers with a BoundsError / what has no meaning is an error of the wrapper's hierarchy, not a result --
    and a vector k shorter than the largest label is refused before the library would read k[g] beyond the buffer."""
    y = np.random.default_rng(5).standard_normal(50)
    g = np.arange(50) % 5 + 1
    bad = [("label 0", (y, np.where(g == 3, 0, g), 2, 3)),
           ("negative label", (y, np.where(g == 3, -2, g), 2, 3)),
           ("J < 0", (y, g, -1, 3)),
           ("negative scalar k", (y, g, 2, -1)),
           ("negative entry in a vector k", (y, g, 2, np.array([1, 2, -1, 2, 1]))),
           ("group of another length", (y, g[:49], 2, 3)),
           ("group of another length, longer", (y, np.r_[g, 1], 2, 3)),
           ("vector k shorter than the largest label", (y, g, 2, np.array([1, 2, 3, 1]))),
           ("vector k of one entry, five labels", (y, g, 2, np.array([2])))]
    for what, args in bad:
        with pytest.raises(mih.MendelIHTError):
            mih.project_group_sparse(*args)
            pytest.fail(what)
    with pytest.raises(mih.api.DimensionMismatch, match="one entry per group"):
        mih.project_group_sparse(y, g, 2, np.array([1, 2, 3, 1]))
    # ... and the calls next to them are answered
    assert np.count_nonzero(mih.project_group_sparse(y, g, 2, np.array([1, 2, 3, 1, 2]))) <= 5
    assert np.count_nonzero(mih.project_group_sparse(y, g, 0, 3)) == 0


@pytest.mark.parametrize("family", ["normal", "bernoulli"])
@pytest.mark.parametrize("setting", [0, 1], ids=["k=2 J=3", "vector k J=4"])
def test_fit_with_interleaved_labels_over_three_tiles(mih, oracle, family, setting):
    """fit_iht with group = 1 + (7 j mod 41) (label 13 absent) on 4101 SNPs: every step's projection runs multi-block sorts whose
    label sort has real work to do.  Held to what test_fit_iht_group_projection holds its fit to: the same iterations, the same
    support, beta within rtol 1e-5 / atol 1e-12, the loglikelihood within 1e-9, and the two covariate effects c within 1e-9 as
    well (none of them is near zero: the intercept and 0.4 z2 are planted).  The CPU companion shows that the oracle reproduces
    these four trajectories -- iterations, support, beta and c to 1e-9 -- under ulp-sized nudges."""
    P = group_fit_problem()
    k, J = P["settings"][setting]
    y, z, group = P["y"][family], P["z"], P["group"]
    x = mih.SnpLinAlg(P["cols"], GROUP_FIT_N, center=True, scale=True, impute=True)
    ox = oracle.Mat.from_bed_columns(P["cols"], GROUP_FIT_N)
    if family == "bernoulli":
        res = mih.fit_iht(y, x, z, k=k, J=J, group=group, d=mih.Bernoulli(), l=mih.LogitLink(), verbose=False)
        o = oracle.fit_iht(ox, y, z, k=k, J=J, group=group, dist="bernoulli", link="logit")
    else:
        res = mih.fit_iht(y, x, z, k=k, J=J, group=group, verbose=False)
        o = oracle.fit_iht(ox, y, z, k=k, J=J, group=group)
    print(family, setting, "iter", res.iter, o["iter"], "max |beta - oracle|", float(np.max(np.abs(res.beta - o["beta"]))),
          "max |c - oracle|", float(np.max(np.abs(res.c - o["c"]))), "logl", res.logl, o["logl"])
    assert res.iter == o["iter"]
    assert np.array_equal(np.flatnonzero(res.beta), np.flatnonzero(o["beta"]))
    np.testing.assert_allclose(res.beta, o["beta"], rtol=1e-5, atol=1e-12)
    assert res.logl == pytest.approx(o["logl"], rel=1e-9)
    np.testing.assert_allclose(res.c, o["c"], rtol=1e-9, atol=0)
    assert np.isin(P["causal"], np.flatnonzero(res.beta)).all()
