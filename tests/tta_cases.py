"""Cases and the numpy restatement of the test-time augmentation (flair_amd/tta.py, csrc/tta.hip), shared by tests/test_tta_cases_cpu.py
and tests/test_gpu_tta.py.

A transform code is data_feed.pack_d4's: bit 0 V-flip, bit 1 H-flip, bits 2-3 the rot90 count k; the code means
rot90^k(hflip(vflip(a))) with numpy's counter-clockwise rot90.  ``d4_np`` states it by index arithmetic (the formulas of d4_source in
csrc/d4.h, one output pixel at a time), ``d4_by_numpy`` by composing np.flip / np.rot90 as the packing says; the CPU tests hold one
against the other.

The ensemble for codes t1..tn:  S = sum_k T_k^-1(softmax(f(T_k(x)))),  preds = lowest index of the largest S,  prob = max S / n.
"""
import numpy as np

from ce_head_cases import MAXPROB_ATOL   # the project's bound for one fp32 softmax probability against fp64

FLIPS = [0, 1, 2, 3]
D4 = [0, 1, 4, 5, 8, 9, 12, 13]
ALL16 = list(range(16))
EVEN_K = [c for c in ALL16 if not c & 4]
CLASSES = (1, 13, 19, 32)
PASSES = (1, 2, 3, 8, 16)
BIG = 120.0   # exp(-240) is 0 in fp32 and in fp64: a +BIG / -BIG logit row has an exactly one-hot softmax in any arithmetic


def source_index(code, i, j, H, W):
    """where output pixel (i, j) of the transform comes from"""
    k = (code >> 2) & 3
    if k == 0:
        si, sj = i, j
    elif k == 1:
        si, sj = j, W - 1 - i
    elif k == 2:
        si, sj = H - 1 - i, W - 1 - j
    else:
        si, sj = H - 1 - j, i
    if code & 2:
        sj = W - 1 - sj
    if code & 1:
        si = H - 1 - si
    return si, sj


def _index_maps(code, H, W):
    if code & 4 and H != W:
        raise ValueError("an odd rot90 count needs a square array")
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return source_index(code, ii, jj, H, W)


def d4_np(a, code):
    """T(a) over the last two axes, by index arithmetic"""
    a = np.asarray(a)
    si, sj = _index_maps(code, *a.shape[-2:])
    return np.ascontiguousarray(a[..., si, sj])


def d4_inv_np(a, code):
    """T^-1(a): out[..., si, sj] = a[..., i, j]"""
    a = np.asarray(a)
    si, sj = _index_maps(code, *a.shape[-2:])
    out = np.empty_like(a)
    out[..., si, sj] = a
    return out


def d4_by_numpy(a, code):
    """rot90^k(hflip(vflip(a))) with numpy's own functions"""
    a = np.asarray(a)
    if code & 1:
        a = np.flip(a, -2)
    if code & 2:
        a = np.flip(a, -1)
    return np.ascontiguousarray(np.rot90(a, (code >> 2) & 3, axes=(-2, -1)))


def softmax64(logits):
    x = np.asarray(logits, dtype=np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def tol(n):
    """|prob - fp64 reference| for n passes: MAXPROB_ATOL for the mean of n softmax probabilities each within MAXPROB_ATOL, plus the
    fp32 additions (each partial sum of k terms is <= k, so they lose at most n(n+1)/2 * 2^-24; / n leaves (n+1)/2 * 2^-24) and one
    more rounding for the division"""
    return MAXPROB_ATOL + ((n + 1) / 2 + 1) * 2.0 ** -24


def ensemble_ref(logits_per_pass, codes):
    """fp64: logits_per_pass[k] (B, C, H, W) are f(T_k(x)).  Returns preds (B, H, W) int64, prob (B, H, W) float64 and the top-2 gap of
    the mean probabilities (inf with one class)."""
    n = len(codes)
    assert n == len(logits_per_pass) and n >= 1
    S = None
    for lg, code in zip(logits_per_pass, codes):
        p = d4_inv_np(softmax64(lg), code)
        S = p if S is None else S + p
    mean = S / n
    preds = mean.argmax(axis=1)
    if mean.shape[1] == 1:
        gap = np.full(preds.shape, np.inf)
    else:
        top = np.sort(mean, axis=1)
        gap = top[:, -1] - top[:, -2]
    return preds, mean.max(axis=1), gap


def check_against_ref(name, preds, prob, ref, n, max_excluded=0.005):
    """preds u8 / prob f32 numpy arrays against ensemble_ref's triple: |prob - ref| <= tol(n) everywhere, preds equal wherever the
    reference's top-2 gap exceeds 2 tol(n); at most ``max_excluded`` of the pixels may lie within it.  Returns the figures."""
    rp, rprob, gap = ref
    t = tol(n)
    err = float(np.abs(prob.astype(np.float64) - rprob).max())
    sure = gap > 2 * t
    excluded = float(1.0 - sure.mean())
    flips = int((preds.astype(np.int64) != rp)[sure].sum())
    print(f"{name}: n {n}, max |prob - ref| {err:.3e} (tol {t:.3e}), excluded {excluded:.4%}, smallest gap {gap.min():.3e}, "
          f"mismatches among the sure {flips}")
    assert err <= t, (name, err, t)
    assert excluded <= max_excluded, (name, excluded)
    assert flips == 0, (name, flips)
    return {"err": err, "excluded": excluded, "flips": flips}


# ---- exact votes

def vote_codes(n, seed):
    """n codes out of all 16 (n = 16: every code once, in a shuffled order); ``even_k`` callers filter themselves"""
    rng = np.random.default_rng(seed)
    if n == 16:
        return [int(c) for c in rng.permutation(16)]
    return [int(c) for c in rng.integers(0, 16, size=n)]


def vote_case(B, C, H, W, codes, seed):
    """One independent random winner map per pass, in the transformed frame.  Returns the per-pass logits (+BIG at the winner, -BIG
    elsewhere; fp32) and the expected (preds u8, prob f32): votes counted at the original-frame pixel, prob = votes / n in fp32."""
    rng = np.random.default_rng(seed)
    n = len(codes)
    votes = np.zeros((B, C, H, W), dtype=np.int64)
    logits = []
    for code in codes:
        win = rng.integers(0, C, size=(B, H, W))
        onehot = (np.arange(C)[None, :, None, None] == win[:, None]).astype(np.int64)
        logits.append(np.where(onehot == 1, BIG, -BIG).astype(np.float32))
        votes += d4_inv_np(onehot, code)
    preds = votes.argmax(axis=1).astype(np.uint8)          # numpy's argmax: the first of equal counts
    prob = votes.max(axis=1).astype(np.float32) / np.float32(n)
    return logits, preds, prob
