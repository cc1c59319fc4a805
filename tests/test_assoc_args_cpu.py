"""The argument handling that score_test, score_test_spa, score_test_firth and set_test share (api._scan_args), pinned to what each
of them accepts and refuses.  It takes the row count, not a handle: no library and no device are needed."""
import numpy as np
import pytest

from mendeliht_amd.api import DimensionMismatch, _scan_args

N = 5
RNG = np.random.default_rng(7)
VEC = RNG.standard_normal(N)
MAT = RNG.standard_normal((N, 3))


def is_vec(a):
    return a.dtype == np.float64 and a.shape == (N,) and a.flags.c_contiguous


def is_cols(a, k):
    return a.dtype == np.float64 and a.shape == (N, k) and a.flags.f_contiguous


@pytest.mark.parametrize("A, one, t", [
    (VEC, True, 1), (list(VEC), True, 1), (VEC.astype(np.float32), True, 1), (np.arange(N), True, 1), (np.tile(VEC, 2)[::2], True, 1),
    (MAT, False, 3), (np.asfortranarray(MAT), False, 3), (MAT[:, :1], False, 1), (RNG.standard_normal((3, N)).T, False, 3),
    (MAT.astype(np.float32), False, 3)])
def test_traits_A_is_a_vector_or_a_matrix_of_n_rows(A, one, t):
    out = _scan_args(N, A, None, None, traits=True)
    assert len(out) == 5
    assert is_cols(out[0], t) and out[4] is one
    assert np.array_equal(out[0], np.asarray(A, dtype=np.float64).reshape(N, t))
    assert out[1] is None and out[3] is None
    assert is_cols(out[2], 1) and np.array_equal(out[2], np.ones((N, 1)))


@pytest.mark.parametrize("A", [VEC[:4], np.zeros((4, 2)), np.zeros((N, 2, 2)), 1.0, np.zeros(0)])
def test_traits_refuses_an_A_without_n_rows(A):
    with pytest.raises(DimensionMismatch, match=r"^A has shape .*, expected 5 rows$"):
        _scan_args(N, A, None, None, traits=True)


@pytest.mark.parametrize("A", [VEC, list(VEC), VEC.astype(np.float32), np.arange(N), np.tile(VEC, 2)[::2]])
def test_one_trait_A_is_a_contiguous_vector(A):
    for eta in (None, VEC):
        out = _scan_args(N, A, VEC, None, eta=eta)
        assert len(out) == 4
        assert is_vec(out[0]) and np.array_equal(out[0], np.asarray(A, dtype=np.float64))


@pytest.mark.parametrize("A", [VEC[:4], MAT, VEC[:, None], 1.0, None])
def test_one_trait_refuses_an_A_that_is_not_n_long(A):
    for eta in (None, VEC):
        with pytest.raises(DimensionMismatch, match=r"^A has shape .*, expected \(5,\)$"):
            _scan_args(N, A, VEC, None, eta=eta)


@pytest.mark.parametrize("Z, c", [
    (None, 1), (VEC, 1), (list(VEC), 1), (np.arange(2 * N), 2), (MAT, 3), (np.asfortranarray(MAT), 3), (MAT.astype(np.float32), 3),
    (np.zeros((N, 0)), 0)])
def test_Z_becomes_n_rows_in_fortran_order(Z, c):
    for kw in (dict(traits=True), dict(), dict(eta=VEC)):
        out = _scan_args(N, VEC, VEC, Z, **kw)
        assert is_cols(out[2], c)
        want = np.ones((N, 1)) if Z is None else np.asarray(Z, dtype=np.float64).reshape(N, -1)
        assert np.array_equal(out[2], want)


@pytest.mark.parametrize("Z", [np.zeros((4, 2)), np.zeros((N, 2, 2)), np.zeros((N + 1, 1)), 1.0])
def test_refuses_a_Z_without_n_rows(Z):
    for kw in (dict(traits=True), dict(), dict(eta=VEC)):
        with pytest.raises(DimensionMismatch, match=r"^Z has shape .*, expected 5 rows$"):
            _scan_args(N, VEC, VEC, Z, **kw)


def test_a_flat_Z_that_does_not_fill_n_rows_is_numpys_error():
    for kw in (dict(traits=True), dict(), dict(eta=VEC)):
        with pytest.raises(ValueError, match="cannot reshape") as e:
            _scan_args(N, VEC, VEC, np.zeros(N + 2), **kw)
        assert not isinstance(e.value, DimensionMismatch)


@pytest.mark.parametrize("v", [VEC, list(VEC), VEC.astype(np.float32), np.arange(N), np.tile(VEC, 2)[::2]])
def test_w_and_eta_are_contiguous_vectors(v):
    want = np.asarray(v, dtype=np.float64)
    for kw in (dict(traits=True), dict()):
        out = _scan_args(N, VEC, v, None, **kw)
        assert is_vec(out[1]) and np.array_equal(out[1], want) and out[3] is None
    out = _scan_args(N, VEC, v, None, eta=v)
    assert is_vec(out[1]) and is_vec(out[3]) and np.array_equal(out[1], want) and np.array_equal(out[3], want)


@pytest.mark.parametrize("v", [VEC[:4], MAT, VEC[:, None], 1.0, np.zeros(0)])
def test_refuses_a_w_or_an_eta_that_is_not_n_long(v):
    for kw in (dict(traits=True), dict(), dict(eta=VEC)):
        with pytest.raises(DimensionMismatch, match=r"^w has shape .*, expected \(5,\)$"):
            _scan_args(N, VEC, v, None, **kw)
    with pytest.raises(DimensionMismatch, match=r"^eta has shape .*, expected \(5,\)$"):
        _scan_args(N, VEC, VEC, None, eta=v)


def test_no_weights_are_unit_weights_for_score_test_and_set_test():
    assert _scan_args(N, VEC, None, None, traits=True)[1] is None
    assert _scan_args(N, VEC, None, MAT)[1] is None


def test_the_saddlepoint_and_firth_calls_refuse_a_missing_w_or_eta():
    """score_test_spa and score_test_firth hand eta over as np.asarray(eta, float64): None is a NaN there, and the vector check
    sees it, like a w of None, as one entry"""
    none = np.asarray(None, dtype=np.float64)
    assert none.shape == ()
    with pytest.raises(DimensionMismatch, match=r"^w has shape \(1,\), expected \(5,\)$"):
        _scan_args(N, VEC, None, None, eta=VEC)
    with pytest.raises(DimensionMismatch, match=r"^eta has shape \(1,\), expected \(5,\)$"):
        _scan_args(N, VEC, VEC, None, eta=none)
    with pytest.raises(DimensionMismatch, match=r"^w has shape \(1,\), expected \(5,\)$"):        # w is looked at first
        _scan_args(N, VEC, None, None, eta=none)


def test_the_first_wrong_argument_is_the_one_named():
    """A before everything; then w and eta before Z where eta is taken, Z before w where it is not"""
    bad = VEC[:4]
    with pytest.raises(DimensionMismatch, match="^A has shape"):
        _scan_args(N, bad, bad, np.zeros((4, 1)), traits=True)
    with pytest.raises(DimensionMismatch, match="^A has shape"):
        _scan_args(N, bad, bad, np.zeros((4, 1)), eta=bad)
    with pytest.raises(DimensionMismatch, match="^Z has shape"):
        _scan_args(N, VEC, bad, np.zeros((4, 1)))
    with pytest.raises(DimensionMismatch, match="^w has shape"):
        _scan_args(N, VEC, bad, np.zeros((4, 1)), eta=bad)
    with pytest.raises(DimensionMismatch, match="^eta has shape"):
        _scan_args(N, VEC, VEC, np.zeros((4, 1)), eta=bad)
