"""CPU side of the test-time augmentation: the ``tta`` argument's spellings (flair_amd.tta.tta_codes) and the numpy restatement the
GPU tests compare against (tests/tta_cases.py), held against numpy's own flip / rot90."""
import numpy as np
import pytest

import tta_cases as T


def test_tta_codes_spellings():
    import flair_amd
    from flair_amd.tta import tta_codes
    assert flair_amd.tta_codes is tta_codes and callable(flair_amd.tta_predict)
    for off in (None, "none", [], ()):
        assert tta_codes(off) is None
    assert tta_codes("flips") == [0, 1, 2, 3] == T.FLIPS
    assert tta_codes("d4") == [0, 1, 4, 5, 8, 9, 12, 13] == T.D4
    assert tta_codes([5]) == [5]
    assert tta_codes((3, 3, 0)) == [3, 3, 0]                  # taken as given, in that order, repeats included
    assert tta_codes(list(range(16))) == list(range(16))
    lst = [1, 2]
    assert tta_codes(lst) is not lst
    for bad in ("D4", "flip", "", 3, 1.5, [16], [-1], [0, 1.0], ["0"], [True], list(range(16)) + [0], {"d4"}, b"d4"):
        with pytest.raises(ValueError):
            tta_codes(bad)


def test_odd_rotation_needs_square_tiles():
    from flair_amd.tta import check_codes
    check_codes(T.ALL16, 8, 8)
    check_codes(T.EVEN_K, 8, 12)
    for code in (4, 5, 12, 15):
        with pytest.raises(ValueError):
            check_codes([0, code], 8, 12)
        with pytest.raises(ValueError):
            T.d4_np(np.zeros((8, 12)), code)


def test_d4_codes_are_the_eight_distinct_group_elements():
    a = np.arange(16).reshape(4, 4)   # no symmetry: every group element moves it somewhere else
    imgs = {T.d4_np(a, c).tobytes() for c in T.D4}
    assert len(imgs) == 8
    assert {T.d4_np(a, c).tobytes() for c in T.ALL16} == imgs          # the other eight codes repeat them
    assert len({T.d4_np(a, c).tobytes() for c in T.FLIPS}) == 4


@pytest.mark.parametrize("shape", [(4, 4), (2, 3, 8, 8), (1, 5, 7)])
def test_inverse_undoes_forward(shape):
    a = np.random.default_rng(1).normal(size=shape)
    for code in T.ALL16:
        if code & 4 and shape[-1] != shape[-2]:
            continue
        assert np.array_equal(T.d4_inv_np(T.d4_np(a, code), code), a), code
        assert np.array_equal(T.d4_np(T.d4_inv_np(a, code), code), a), code


@pytest.mark.parametrize("shape", [(4, 4), (2, 3, 8, 8), (3, 1, 6, 10), (5, 7)])
def test_restatement_equals_numpy_flip_and_rot90(shape):
    from flair_amd.data_feed import pack_d4
    a = np.random.default_rng(2).integers(0, 1000, size=shape)
    for v in (0, 1):
        for h in (0, 1):
            for k in range(4):
                if k & 1 and shape[-1] != shape[-2]:
                    continue
                code = pack_d4(v, h, k)
                want = np.rot90(np.flip(np.flip(a, -2) if v else a, -1) if h else (np.flip(a, -2) if v else a), k, axes=(-2, -1))
                assert np.array_equal(T.d4_np(a, code), want), code
                assert np.array_equal(T.d4_by_numpy(a, code), want), code


def test_ensemble_ref_of_one_identity_pass_is_softmax_argmax():
    lg = np.random.default_rng(3).normal(0, 3, size=(2, 5, 6, 6)).astype(np.float32)
    preds, prob, gap = T.ensemble_ref([lg], [0])
    p = T.softmax64(lg)
    assert np.array_equal(preds, p.argmax(1)) and np.array_equal(prob, p.max(1)) and (gap >= 0).all()
    # a transformed pass comes back to the original frame: f = identity on logits that are themselves transformed
    for code in T.ALL16:
        preds2, prob2, _ = T.ensemble_ref([T.d4_np(lg, code)], [code])
        assert np.array_equal(preds2, preds) and np.array_equal(prob2, prob), code


def test_vote_case_counts_every_pass_once():
    for n in T.PASSES:
        codes = T.vote_codes(n, n)
        assert len(codes) == n and (n != 16 or sorted(codes) == T.ALL16)
        logits, preds, prob = T.vote_case(2, 13, 8, 8, codes, 7)
        assert len(logits) == n and preds.dtype == np.uint8 and prob.dtype == np.float32
        ref_p, ref_prob, _ = T.ensemble_ref(logits, codes)             # one-hot softmaxes: fp64 sums are whole numbers too
        assert np.abs(ref_prob * n - np.round(ref_prob * n)).max() < 1e-12
        assert np.array_equal(preds, ref_p) and np.abs(prob - ref_prob).max() < 1e-7
    assert T.tol(3) == pytest.approx(1e-6 + 3 * 2.0 ** -24)
