"""GPU: k_viterbi under references that are not its twin (tests/coding_ref.py, the
inputs and assertions of tests/test_coding_ml_host.py): dsce_viterbi returns a
maximum-likelihood word of the exhaustive codeword list; its error pattern on a
noisy non-zero codeword is the one of the all-zero codeword; the LDS packings of
4, 3, 2 and 1 waves per block decode noisy codewords like the twin; and
dsce_run_coded, at step counts where its information-bit mask and its 32-step
operand groups have edges, counts what the twin counts and what decoding real
codewords through dsce_viterbi on the engine's own LLRs counts.  Every assertion
is on integers or 0 / 1 arrays."""
import numpy as np
import pytest

import coding_ref
import harness
from test_coding_ml_host import (INV_CASES, ML_CASES, SIGMA, check_invariance, check_ml, flip_of, inv_inputs, ml_inputs,
                                 tables)
from test_gpu_coded import BRANCHES, _coded, _same, _viterbi
from test_gpu_export import SEED, SNR, _export

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bare():
    from dsce import engine
    eng = engine.Engine(0)
    yield eng
    eng.close()


def _twin(lam, code):
    from dsce.coding import viterbi_decode
    return viterbi_decode(lam, code.src, code.terminated)


@pytest.mark.parametrize("terminated,T", ML_CASES + tuple((False, T) for T in (2, 3, 4, 6)))
def test_viterbi_is_maximum_likelihood(bare, terminated, T):
    """200 codewords (50 blocks of 4 waves) per table and kind of input; with the
    added cases, every unterminated step count from 1 to 6.  The twin is asked too:
    on wide input both are the unique maximiser, on narrow input the tie rule
    decides, and it is the same rule."""
    got = []

    def decode(lam, code):
        got.append(_viterbi(bare, lam, code.src, code.terminated))
        return got[-1]

    check_ml(decode, T, terminated)
    cases = ml_inputs(T, terminated)
    assert len(got) == len(cases) == 6
    for g, c in zip(got, cases):
        assert np.array_equal(g, _twin(c.lam, c.code)), (T, c.code.rate, c.kind)


@pytest.mark.parametrize("T,terminated", INV_CASES)
def test_viterbi_error_pattern_does_not_depend_on_the_codeword(bare, T, terminated):
    got = check_invariance(lambda lam, code: _viterbi(bare, lam, code.src, code.terminated), T, terminated)
    for (zero, sent), c in zip(got, inv_inputs(T, terminated)):
        assert np.array_equal(zero, _twin(c.lam0, c.code)), (T, terminated, c.code.rate)
        assert np.array_equal(sent, _twin(c.lam0 * c.flip, c.code)), (T, terminated, c.code.rate)


@pytest.mark.parametrize("T,wpb", [(2048, 4), (2730, 3), (2731, 2), (4096, 2), (4097, 1), (8192, 1)])
def test_viterbi_lds_packing_with_noise(bare, T, wpb):
    """A block holds min(4, 8192 // T) waves, T x 8 bytes of decision words each
    (exactly 64 KiB at T = 2048 and T = 4096): 2 wpb + 1 noisy random codewords, so
    the last block is partly filled, equal the twin, which gets every one of them
    wrong somewhere."""
    from dsce.coding import MAX_STEPS, conv_encode
    assert wpb == max(1, min(4, MAX_STEPS // T))
    n = 2 * wpb + 1
    rng = np.random.default_rng(T)
    for terminated in (True, False):
        for code in tables(T, terminated, ("1/2", "3/4") if T in (2731, 4097) else ("1/2",)):
            u = rng.integers(0, 2, (n, T)).astype(np.uint8)
            u[:, code.n_info:] = 0
            noisy = coding_ref.dyadic(-1.0 + SIGMA[code.rate] * rng.standard_normal((n, code.n_slots)))
            lam = noisy * flip_of(u, code, conv_encode)
            ref = _twin(lam, code)
            assert u.any(axis=1).all() and (ref != u).any(axis=1).all(), (T, terminated, code.rate)
            got = _viterbi(bare, lam, code.src, terminated)
            assert np.array_equal(got, ref), (T, terminated, code.rate, np.argwhere(got != ref)[:4])


def _truncated(code, T, terminated):
    """The first T steps of a table."""
    from dsce.coding import info_bits
    src = code.src[:T]
    return code._replace(src=src, terminated=terminated, n_steps=T, n_info=info_bits(T, terminated), n_kept=int((src >= 0).sum()))


# scheme -> rate and (T, terminated); T None = the whole table.  Terminated, K = T - 6 (the traceback walks 64-step
# chunks from c0 = 64 floor((T - 1) / 64) down and counts the inputs t < K): 1219, K = 1213 = 1216 - 3, the tail
# straddles the last two chunks; 1222, K = 1216 = 19 x 64, nothing of the last chunk counts and all of the one
# before; 1249 = 39 x 32 + 1, a last operand group of one step.  Unterminated: a whole number of chunks, and 19
# chunks and a step.
RUN_CASES = {"ofdm": ("1/2", ((1219, True), (1222, True), (1249, True), (1280, False), (1217, False))),
             "fbmc_aux": ("5/6", ((None, True), (None, False)))}


@pytest.mark.parametrize("name", sorted(RUN_CASES))
def test_run_coded_mask_and_group_edges(name):
    """Default setup, n_iter 4, SNR (10, 35), batch 64, realisations 5..7, exact
    LLRs, both branches.  Per code of RUN_CASES the counts of dsce_run_coded are
    the twin's on export_llr and sym, and they are the wrong information bits of
    random codewords decoded by dsce_viterbi: lam of the same LLRs, signed by sym
    and by the coded bits.  The second is the header's "which is exact" on the
    engine's own LLRs."""
    from dsce.coding import coded_counts, conv_encode, make_code
    rate, cases = RUN_CASES[name]
    S = harness.setup("default", schemes=(name,), snr_db=SNR, n_iter=4)
    sc = S.schemes[name]
    nd, m = sc["n_data"], sc["bits_per_symbol"]
    full = make_code(nd * m, rate, interleaver=7)
    rng = np.random.default_rng(23)
    eng = harness.engine(S, batch=64)
    try:
        sym = _export(eng, 0, SEED, 5, 3, fields=("sym",))["sym"]
        t = ((np.asarray(sym)[..., None] >> np.arange(m)) & 1).astype(bool).reshape(3, 1, 1, nd * m)
        seen = set()
        for branch in BRANCHES:
            llr = eng.export_llr(0, SEED, 5, 3, fields=("llr",), method="exact", branch=branch)["llr"]
            assert llr.dtype == np.float64 and np.isfinite(llr).all()
            n, nk, ns = llr.shape[:3]
            flat = llr.reshape(n, nk, ns, nd * m)
            lam = np.where(t, -flat, flat).reshape(n * nk * ns, nd * m)
            for T, terminated in cases:
                code = _truncated(full, full.n_steps if T is None else T, terminated)
                got = _coded(eng, 0, SEED, 5, 3, code, branch=branch)
                print("coded %s %s T %d terminated %d %s bit_err %s frame_err %s"
                      % (name, rate, code.n_steps, terminated, branch, got["bit_err"].tolist(), got["frame_err"].tolist()))
                _same(got, coded_counts(llr, sym, code))
                u = rng.integers(0, 2, (lam.shape[0], code.n_steps)).astype(np.uint8)
                u[:, code.n_info:] = 0
                dec = _viterbi(eng, lam * flip_of(u, code, conv_encode), code.src, terminated)
                bit = (dec ^ u)[:, :code.n_info].astype(np.int64).sum(axis=1).reshape(n, nk, ns)
                _same(got, dict(bit_err=bit.sum(axis=0), frame_err=(bit > 0).sum(axis=0)))
                seen.update(got["frame_err"].ravel().tolist())
        assert max(seen) > 0                                                    # there are errors to count
    finally:
        eng.close()
