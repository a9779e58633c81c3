"""The SNR-loop form of k_pic_fft (option snr_loop): a block owns 64
realisations x one symbol and walks the chunk's SNR points itself, the
per-realisation prologue once.  Forced on (1) it must give every counter the
per-unit form (0) gives, bit for bit, and both must equal the CPU oracle under
the borderline rule of test_gpu_parity.test_error_counts_match_oracle; a traced
unit of the last SNR point must match the oracle per element; and the default
(-1) picks the loop by grid size.

One oracle run (64 realisations x the script's 7 SNR points) serves every list
that is a prefix of the script's: the noise sub-stream of a point is keyed by
its index, so the oracle's counts of a prefix list are the leading columns."""
import numpy as np
import pytest

import harness
from test_gpu_parity import SEED, _check_trace, bench_path

pytestmark = pytest.mark.gpu


def _forms(eng, first, n, loop_expected=True):
    """Counts of [first, first + n) with snr_loop 0 and 1; the path bit follows
    the form that ran."""
    eng.set_option("snr_loop", 0)
    c0 = eng.run(SEED, first, n)
    assert "snr_loop" not in eng.path_info(0), eng.path_info(0)
    eng.set_option("snr_loop", 1)
    c1 = eng.run(SEED, first, n)
    path = eng.path_info(0)
    assert ("snr_loop" in path) == loop_expected, path
    if loop_expected:
        assert bench_path(eng) <= path, path
    eng.set_option("snr_loop", -1)
    np.testing.assert_array_equal(c1, c0)
    return c1


def _within_borderline(c, res, what):
    assert np.abs(c - res["err"]).sum() <= 8 * res["borderline"].sum(), (what, c - res["err"])


@pytest.fixture(scope="module")
def full():
    """The script's setup (7 SNR points, 4 iterations) and the oracle's counts
    and MSE sums of realisations [0, 64)."""
    S = harness.setup("default", schemes=("ofdm",))
    res = harness.simulate(S, SEED, 0, 64, ["ofdm"])
    assert res["err"].sum() > 0
    return S, res


@pytest.mark.parametrize("batch", [64, 128])
@pytest.mark.parametrize("nsnr", [1, 2, 3, 7])
def test_loop_equals_per_unit_form_and_oracle(full, nsnr, batch):
    """snr_db lists of 1, 2, 3 and 7 points; 64 realisations are one block per
    symbol, the smallest grid, and at batch 128 a second block column."""
    S7, res = full
    S = harness.setup("default", schemes=("ofdm",), snr_db=list(S7.snr_db[:nsnr]))
    eng = harness.engine(S, batch=batch)
    try:
        c = _forms(eng, 0, 64)
        assert c.shape[-2] == nsnr
        ref = dict(err=res["err"][..., :nsnr, :], borderline=res["borderline"])
        _within_borderline(c, ref, (nsnr, batch))
        if batch == 128:
            _forms(eng, 64, 128)        # both block columns full
    finally:
        eng.close()


def test_snr_chunks_of_two_and_one(full):
    """snr_chunk 2 over 3 SNR points: chunks of 2 + 1, snr0 = 2 in the second."""
    S7, res = full
    S = harness.setup("default", schemes=("ofdm",), snr_db=list(S7.snr_db[:3]))
    eng = harness.engine(S, batch=64, options={"snr_chunk": 2})
    try:
        c = _forms(eng, 0, 64)
        _within_borderline(c, dict(err=res["err"][..., :3, :], borderline=res["borderline"]), "chunk 2")
        eng.set_option("snr_chunk", 1)          # one point per chunk: the loop of length 1
        np.testing.assert_array_equal(_forms(eng, 0, 64), c)
    finally:
        eng.close()


def test_padding_realisations_inside_the_loop(full):
    """70 realisations in a batch of 128: the second block column has 6 valid
    lanes (rvalid) at every SNR point; additive over [0, 64) + [64, 70), and
    [0, 64) is the oracle's."""
    S, res = full
    eng = harness.engine(S, batch=128)
    try:
        c70 = _forms(eng, 0, 70)
        eng.set_batch(64)
        c64 = _forms(eng, 0, 64)
        np.testing.assert_array_equal(c64 + _forms(eng, 64, 6), c70)
        _within_borderline(c64, res, "64 of 70")
    finally:
        eng.close()


def test_mse_sums_are_the_same_in_both_forms(full):
    """MSE sums enabled (k_mic_data's flush_mse runs beside the looped chain)."""
    S, res = full
    eng = harness.engine(S, batch=64)
    try:
        sums = []
        for form in (0, 1):
            eng.set_option("snr_loop", form)
            eng.enable_mse()                    # resets the sums
            c = eng.run(SEED, 0, 64)
            _within_borderline(c, res, "mse form %d" % form)
            sums.append(eng.mse())
        eng.enable_mse(False)
        # (the sums are fp64 atomics: equal up to the order of the additions)
        np.testing.assert_allclose(sums[0][0], sums[1][0], rtol=1e-12, atol=0)
        np.testing.assert_allclose(sums[0][1], sums[1][1], rtol=1e-12, atol=0)
        np.testing.assert_allclose(sums[1][0], res["mse_err"], rtol=1e-9, atol=0)
        np.testing.assert_allclose(sums[1][1], res["mse_pow"], rtol=1e-12, atol=0)
    finally:
        eng.close()


@pytest.mark.parametrize("n_iter", [0, 1])
def test_other_iteration_counts(n_iter):
    """n_iter 1 (with 4, the fixture's, on either side of the W / W0 switch) in
    both forms and against the oracle.  n_iter 0 has no IC chain: the engine runs
    the stage kernels, snr_loop 1 has nothing to loop over and the counts stay."""
    S = harness.setup("default", schemes=("ofdm",), snr_db=[15.0, 35.0], n_iter=n_iter)
    eng = harness.engine(S, batch=64)
    try:
        c = _forms(eng, 0, 64, loop_expected=n_iter > 0)
        assert c.shape[-1] == n_iter + 1
        _within_borderline(c, harness.simulate(S, SEED, 0, 64, ["ofdm"]), n_iter)
    finally:
        eng.close()


def test_single_tap_channel():
    """NT = 1: PedestrianA collapses to one tap at 360 kHz (k_pic_fft<1, 0>)."""
    S = harness.setup("default", schemes=("ofdm",), snr_db=[15.0, 35.0], pdp="PedestrianA")
    assert list(S.chan["idx_taps"]) == [0]
    eng = harness.engine(S, batch=64)
    try:
        _within_borderline(_forms(eng, 0, 64), harness.simulate(S, SEED, 0, 64, ["ofdm"]), "PedestrianA")
    finally:
        eng.close()


def test_nonuniform_row_precoder_under_the_loop():
    """pv_uni 0 (data rows with different unit-modulus precoder factors, as
    test_gpu_parity.test_nonuniform_row_precoder_matches_oracle): the loop's
    re-precode takes the row value x the constellation branch."""
    import copy
    from types import SimpleNamespace
    S0 = harness.setup("default", schemes=("ofdm",), snr_db=[15.0, 35.0])
    S = SimpleNamespace(**vars(S0))
    S.name = "default_pv_rotated_2snr"     # its own oracle_mmse cache entry
    S.schemes = copy.deepcopy(S0.schemes)
    sc = S.schemes["ofdm"]
    NP = len(sc["pilot_pos"])
    P = sc["P"].copy()
    P[:, NP:] = P[:, NP:] * np.exp(1j * np.pi / 4 * (np.arange(P.shape[1] - NP) % 3))[None, :]
    sc["P"] = P
    eng = harness.engine(S, batch=64)
    try:
        c = _forms(eng, 0, 64)
        res = harness.simulate(S, SEED, 0, 64, ["ofdm"])
        assert res["err"].sum() > 0
        _within_borderline(c, res, "pv_uni 0")
    finally:
        eng.close()


def test_doubly_flat_setup_is_untouched():
    """The doubly-flat script (one flat tap, no IC iterations, one SNR point per
    run) never reaches the chain kernel: snr_loop changes no count there."""
    from dsce.doubly_flat import DoublyFlatSim
    sim = DoublyFlatSim(batch=64)
    try:
        got = []
        for form in (0, 1):
            sim.engine.set_option("snr_loop", form)
            got.append(sim.run(SEED, 0, 64))
            assert "snr_loop" not in sim.engine.path_info(sim.sid["ofdm"])
        np.testing.assert_array_equal(got[0], got[1])
        assert got[0].sum() > 1000
    finally:
        sim.close()


def test_traced_unit_of_the_last_snr_point(full):
    """A unit of the last of 3 SNR points with the loop forced: what the loop
    carries across points (1 / h, the centred taps, the constant rows, txp, the
    prefetched y) feeds y_perf and the decisions of every stage, per element
    at test_bench_kernels_trace_matches_oracle's tolerances; y_est, the LS
    pilots and diag(D_hat) of the MMSE branch ride along."""
    S7, _ = full
    S = harness.setup("default", schemes=("ofdm",), snr_db=list(S7.snr_db[:3]))
    rows = S.schemes["ofdm"]["data_pos"]
    eng = harness.engine(S, batch=64, options={"snr_loop": 1})
    try:
        for rep in (5, 70):
            tr = {}
            harness.simulate(S, SEED, rep, 1, ["ofdm"], trace=tr)
            g = eng.trace_unit(0, SEED, rep, 2)
            assert bench_path(eng) | {"snr_loop"} <= eng.path_info(0), eng.path_info(0)
            u = tr["units"][2]
            ns = _check_trace(g, u, "snr_loop rep %d" % rep)
            assert ns == S.n_iter + 1
            for st in range(1, ns):
                np.testing.assert_allclose(g["yperf"][st][rows], u["yperf"][st][rows], rtol=0, atol=1e-9)
    finally:
        eng.close()


def test_auto_rule_by_grid_size(full):
    """The default picks the loop at the bench's own shape (C2, batch 65 536:
    14 x 1024 looped blocks, 28 rounds of the device's resident slots) and at the
    engine's default batch 8192 (3.5 rounds, where it measured faster), the
    per-unit form at batch 4096 (1.75 rounds, where the loop measured slower)
    and at batch 64; the two forced forms agree at 65 536.  (The rounds are
    those of a 256-CU device; the rule counts the device's own CUs.)"""
    S, _ = full
    eng = harness.engine(S, batch=65536)
    try:
        assert eng.get_option("snr_loop") == -1
        ca = eng.run(SEED, 0, 65536)
        assert "snr_loop" in eng.path_info(0), eng.path_info(0)
        np.testing.assert_array_equal(_forms(eng, 0, 65536), ca)
        eng.set_batch(8192)
        eng.run(SEED, 0, 8192)
        assert "snr_loop" in eng.path_info(0), eng.path_info(0)
        for batch in (4096, 64):
            eng.set_batch(batch)
            eng.run(SEED, 0, batch)
            assert "snr_loop" not in eng.path_info(0), (batch, eng.path_info(0))
    finally:
        eng.close()


def test_option_is_validated():
    from dsce.engine import DsceError, Engine
    eng = Engine()
    try:
        for bad in (2, -2):
            with pytest.raises(DsceError):
                eng.set_option("snr_loop", bad)
        assert eng.get_option("snr_loop") == -1
        for ok in (0, 1, -1):
            eng.set_option("snr_loop", ok)
            assert eng.get_option("snr_loop") == ok
    finally:
        eng.close()
