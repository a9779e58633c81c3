"""CPU: dsce.coding.viterbi_decode, the NumPy twin of k_viterbi, against references
that share nothing with it (tests/coding_ref.py): the exhaustive list of
codewords, whose best member a maximum-likelihood decoder must return, and real
non-zero codewords, whose decoded error pattern must be the one of the all-zero
codeword that dsce_run_coded counts (include/dsce.h, "Why this is exact").
Every assertion is on integers or 0 / 1 arrays.  The inputs and the assertions
are functions of a decoder, so tests/test_gpu_coded_ml.py puts the kernel under
the same ones.  No GPU call."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import coding_ref

# (terminated, T): K = 1, 5, 12 information bits unterminated; 1 and 12 terminated
ML_CASES = ((False, 1), (False, 5), (False, 12), (True, 7), (True, 18))
N_ML = 200
# (T, terminated) of the invariance tests; 8 codewords each
INV_CASES = ((200, True), (1280, True), (1279, False))
N_INV = 8
# Noise of the invariance inputs (mean -1 per slot) per rate, chosen so that at least half of the
# eight codewords of every case decode with errors (asserted): the punctured codes need less noise
# for that than rate 1/2, but 0.6 (rate 3/4) and 0.45 (rate 5/6) leave the 200-step case almost clean.
SIGMA = {"1/2": 1.0, "3/4": 0.8, "5/6": 0.7}


def tables(T, terminated, rates=("1/2", "3/4", "5/6")):
    """Tables of exactly T steps: the identity at rate 1/2, and make_code's punctured
    rates over interleaver 5 with as many slots as T steps keep."""
    from dsce.coding import PUNCTURE, Code, info_bits, make_code
    out = []
    for rate in rates:
        if rate == "1/2":
            ident = np.arange(2 * T, dtype=np.int32).reshape(T, 2)
            out.append(Code(ident, terminated, 2 * T, "1/2", T, info_bits(T, terminated), 2 * T))
            continue
        mask = PUNCTURE[rate]
        kept = sum(sum(mask[t % len(mask)]) for t in range(T))
        c = make_code(kept, rate, terminated=terminated, interleaver=5)
        assert c.n_steps == T and c.n_slots == kept and (c.src < 0).any() == (T > 1)
        out.append(c)
    return out


def _frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def ml_inputs(T, terminated):
    """Per table and kind of input: N_ML integer-valued decoder inputs (float64)
    from default_rng(T), and M int64 [N_ML][2**K], the exact metric of every
    information word (coding_ref.ml_table).  wide: uniform in [-10**6, 10**6];
    narrow: in [-2, 2], ties everywhere."""
    rng = np.random.default_rng(T)
    out = []
    for code in tables(T, terminated):
        words, A = coding_ref.ml_table(code.src, code.n_slots, T, terminated)
        for kind, lim in (("wide", 10 ** 6), ("narrow", 2)):
            li = rng.integers(-lim, lim + 1, (N_ML, code.n_slots))
            out.append(SimpleNamespace(code=code, kind=kind, lam=_frozen(li.astype(np.float64)),
                                       M=_frozen(li @ A.T), words=_frozen(words)))
    return out


def check_ml(decode, T, terminated):
    """decode(lam, code) -> uint8 [n][T] returns a maximum-likelihood word for
    every input of ml_inputs(T, terminated): the unique maximiser of M for wide
    input (that it is unique for all N_ML codewords is asserted), a word of
    metric M.max for narrow input."""
    rows = np.arange(N_ML)
    for c in ml_inputs(T, terminated):
        got = decode(c.lam, c.code)
        assert got.shape == (N_ML, T) and got.max() <= 1
        idx = coding_ref.word_index(got, terminated)
        best = c.M.max(axis=1)
        unique = (c.M == best[:, None]).sum(axis=1) == 1
        what = (terminated, T, c.code.rate, c.kind)
        if c.kind == "wide":
            assert unique.all(), what
            assert np.array_equal(idx, c.M.argmax(axis=1)), (what, np.flatnonzero(idx != c.M.argmax(axis=1))[:4])
        else:
            assert np.array_equal(c.M[rows, idx], best), (what, np.flatnonzero(c.M[rows, idx] != best)[:4])
        assert np.array_equal(c.words[idx], got)
        # the decoded words are not trivially zero; a uniformly drawn word of K bits is zero with probability
        # 2**-K, so the 90 % hold from K = 5 on (every case of ML_CASES but the two with one information bit)
        if c.code.n_info >= 5:
            assert (idx != 0).mean() >= 0.9, (what, (idx != 0).mean())
        else:
            assert (idx != 0).any(), what


@functools.lru_cache(maxsize=None)
def inv_inputs(T, terminated):
    """Per table: lam0 [N_INV][n_slots], a noisy observation of the all-zero codeword
    (mean -1, SIGMA[rate], rounded to 2**-30: every path metric is exact in any
    order and ties have negligible probability); u [N_INV][T] random information
    words, tail zeroed if terminated; flip, -1 where conv_encode(u) puts a 1 in the
    slot and +1 elsewhere."""
    from dsce.coding import conv_encode
    rng = np.random.default_rng(1000 + T)
    out = []
    for code in tables(T, terminated):
        lam0 = coding_ref.dyadic(-1.0 + SIGMA[code.rate] * rng.standard_normal((N_INV, code.n_slots)))
        u = rng.integers(0, 2, (N_INV, T)).astype(np.uint8)
        u[:, code.n_info:] = 0
        out.append(SimpleNamespace(code=code, lam0=_frozen(lam0), u=_frozen(u), flip=_frozen(flip_of(u, code, conv_encode))))
    return out


def flip_of(u, code, encode):
    """float64 [..][n_slots]: -1 where encode(u) puts a 1 into the slot, +1 elsewhere."""
    coded = encode(u)
    use = code.src >= 0
    flip = np.ones(u.shape[:-1] + (code.n_slots,))
    flip[..., code.src[use]] = 1.0 - 2.0 * coded[..., use].astype(np.float64)
    return flip


def check_invariance(decode, T, terminated):
    """decode(lam0 * flip) ^ u == decode(lam0), all T inputs of every codeword, and at
    least half of the codewords of every table decode with errors.  Returns the
    two decoded arrays per table."""
    out = []
    for c in inv_inputs(T, terminated):
        zero = decode(c.lam0, c.code)
        sent = decode(c.lam0 * c.flip, c.code)
        what = (T, terminated, c.code.rate)
        assert c.u.any(axis=1).all() and (c.flip < 0).any(axis=1).all(), what
        assert np.array_equal(sent ^ c.u, zero), (what, np.argwhere((sent ^ c.u) != zero)[:4])
        assert zero.any(axis=1).sum() >= N_INV // 2, (what, zero.sum(axis=1))
        out.append((zero, sent))
    return out


def _twin(lam, code):
    from dsce.coding import viterbi_decode
    return viterbi_decode(lam, code.src, code.terminated)


def test_reference_encoder_agrees_with_conv_encode():
    """The one tie between the two encoders: the shift register written from "133"
    and "171" and dsce.coding.conv_encode on random input, and the impulse
    response read back as the octal strings."""
    from dsce.coding import conv_encode
    u = np.random.default_rng(4).integers(0, 2, (9, 131)).astype(np.uint8)
    assert np.array_equal(coding_ref.ref_encode(u), conv_encode(u))
    assert np.array_equal(coding_ref.ref_encode(u[0]), conv_encode(u)[0])
    imp = coding_ref.ref_encode([1, 0, 0, 0, 0, 0, 0])
    assert ["%o" % int("".join(map(str, imp[:, k])), 2) for k in range(2)] == list(coding_ref.GENERATORS)


def test_ml_table():
    """ml_table on a table small enough to read: three steps, output 1 of step 1
    punctured, slot 4 unused, the rest out of order."""
    src = np.array([[3, 0], [2, -1], [1, 5]])
    words, A = coding_ref.ml_table(src, 6, 3, False)
    assert words.tolist() == [[(i >> t) & 1 for t in range(3)] for i in range(8)]
    # u = (1, 0, 1): o0 = u_t ^ u_{t-2} ^ .. = 1, 0, 0; o1 = u_t ^ u_{t-1} ^ u_{t-2} ^ .. = 1, 1, 0
    assert A[5].tolist() == [1, 0, 0, 1, 0, 0]
    assert not A[0].any() and not A[:, 4].any()
    w7, A7 = coding_ref.ml_table(np.arange(14).reshape(7, 2), 14, 7, True)
    assert w7.tolist() == [[0] * 7, [1] + [0] * 6] and A7.sum(axis=1).tolist() == [0, 10]


@pytest.mark.parametrize("terminated,T", ML_CASES)
def test_twin_is_maximum_likelihood(terminated, T):
    check_ml(_twin, T, terminated)


@pytest.mark.parametrize("T,terminated", INV_CASES)
def test_twin_error_pattern_does_not_depend_on_the_codeword(T, terminated):
    check_invariance(_twin, T, terminated)
