"""An independent reference for the K = 7 code and its decoder, for the tests of
dsce.coding.viterbi_decode and of k_viterbi (tests/test_coding_ml_host.py,
tests/test_gpu_coded_ml.py).  Nothing here comes from dsce.coding: the encoder
is a shift register written from the generators' octal strings, and the decoder
is no decoder at all but the list of every codeword.

include/dsce.h: the decoder maximises, over the information words, the sum of
lam over the slots whose coded bit is 1 (step 2 adds z_{t,k} where o_k is set),
which is the correlation sum_i (2 c_i - 1) lam_i up to the constant sum(lam) and
a factor 2.  For integer-valued lam that sum is exact in int64 in any order, so
`lam @ A.T` with A from ml_table is the exact metric of every codeword."""
import numpy as np

GENERATORS = ("133", "171")   # octal; the most significant of the seven bits multiplies u_t, the least u_{t-6}
MEMORY = 6


def ref_encode(u):
    """uint8 [..][T][2]: the two outputs per step of a seven-cell shift register
    that starts empty and takes u [..][T] one input per step."""
    u = np.asarray(u).astype(np.uint8) & 1
    T = u.shape[-1]
    out = np.zeros(u.shape + (2,), dtype=np.uint8)
    reg = np.zeros(u.shape[:-1] + (MEMORY + 1,), dtype=np.uint8)              # reg[..][d] = u_{t-d}
    taps = [[int(c) for c in format(int(g, 8), "07b")] for g in GENERATORS]   # taps[k][d], d = 0 the MSB
    for t in range(T):
        reg[..., 1:] = reg[..., :-1].copy()
        reg[..., 0] = u[..., t]
        for k in range(2):
            out[..., t, k] = sum(reg[..., d] for d in range(MEMORY + 1) if taps[k][d]) & 1
    return out


def ml_table(src, n_slots, T, terminated):
    """Every information word of a code of T steps: words uint8 [2**K][T] (K = T - 6
    with six tail zeros if terminated, else T; bit t of the row index is u_t) and
    A int64 [2**K][n_slots], the coded bit that table src [T][2] puts into each
    slot; a punctured output (src < 0) appears nowhere, a slot src does not name
    stays 0."""
    src = np.asarray(src).reshape(T, 2)
    K = T - MEMORY if terminated else T
    assert K >= 1 and K <= 20
    words = np.zeros((1 << K, T), dtype=np.uint8)
    words[:, :K] = (np.arange(1 << K)[:, None] >> np.arange(K)) & 1
    coded = ref_encode(words)
    A = np.zeros((1 << K, int(n_slots)), dtype=np.int64)
    for t in range(T):
        for k in range(2):
            if src[t, k] >= 0:
                A[:, src[t, k]] = coded[:, t, k]
    return words, A


def word_index(decoded, terminated):
    """The row of ml_table's `words` that equals decoded [n][T]; asserts the tail
    zeros of a terminated word."""
    decoded = np.asarray(decoded).astype(np.int64)
    T = decoded.shape[-1]
    K = T - MEMORY if terminated else T
    assert not decoded[:, K:].any(), "a terminated word ends in six zeros"
    return (decoded[:, :K] << np.arange(K)).sum(axis=1)


def dyadic(x):
    """x rounded to a multiple of 2**-30: sums of a few thousand such values of
    moderate size are exact in fp64 in any order."""
    return np.round(np.asarray(x, dtype=np.float64) * 2.0 ** 30) / 2.0 ** 30
