"""GPU: dsce_run_soft (k_llr_info, DSCE_HAS_SOFT_RUN) — the BICM information loss
summed on the device — against dsce.modulation.bicm_info_loss applied in NumPy to
dsce_export_llr's own LLRs and dsce_export's sym of the same realisations; the
perfect-CSI one-tap figure against include/dsce.h's definitions evaluated on
dsce_export's y and h; and against itself across batch geometries, staging
bounds, SNR chunks and split calls.

Bar of one entry (SNR, stage, edge class), a sum of non-negative terms:
1e-10 ref + sum over its bits of 1e-12 (1 + E) / ln 2, E = max_i |x_est - s_i|^2
/ pn_eff of the bit's symbol.  The first term covers the order of summation (at
most 3.3e5 terms here: N 2^-53 < 4e-11 relative); the second is the LLR bar of
tests/test_gpu_llr.py passed through loss_b, which is 1/ln 2-Lipschitz in the
LLR.  Every host destination sits between guard regions (_soft)."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import harness
from test_gpu_export import EINVAL, ESTATE, GUARD, PATTERN, SEED, SNR, _export
from test_gpu_llr import METHODS, _bitmap, _emax, _llr
from test_llr_host import demapper_input

pytestmark = pytest.mark.gpu

BOTH = ("loss_est", "loss_perf0")
LN2 = np.log(2.0)
WORST = {}


def _note(key, ratio):
    """Worst error / bar seen per check (printed; DESIGN.md section 7h quotes them)."""
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))
    print("soft ratio %-28s %.3e" % (key, WORST[key]))


def _soft(eng, sid, seed, first, n, fields=BOTH, method="exact", flags=None, into=None):
    """dsce_run_soft into zeroed arrays (or copies of `into`) that share one buffer,
    guard | loss_est | guard | loss_perf0 | guard; only `fields` are passed.
    Asserts that the guards and the field not requested keep their bytes."""
    from dsce import engine
    shapes = eng.soft_shapes(sid)
    raw = np.full(3 * GUARD + sum(int(np.prod(shapes[f])) * 8 for f in BOTH), PATTERN, dtype=np.uint8)
    view, at = {}, GUARD
    for f in BOTH:
        nb = int(np.prod(shapes[f])) * 8
        view[f] = raw[at:at + nb].view(np.float64).reshape(shapes[f])
        at += nb + GUARD
    for f in fields:
        view[f][...] = 0.0 if into is None else into[f]
    before = raw.copy()
    o = engine.SoftOut(**{f: view[f].ctypes.data_as(engine.C.POINTER(engine.C.c_double)) for f in fields})
    if flags is None:
        flags = engine.LLR_METHODS[method]
    eng._chk(eng.lib.dsce_run_soft(eng.h, sid, seed, first, n, flags, engine.C.byref(o)), "dsce_run_soft")
    keep = np.ones(raw.size, dtype=bool)
    for f in fields:
        a0 = view[f].ctypes.data - raw.ctypes.data
        keep[a0:a0 + view[f].nbytes] = False
    assert np.array_equal(raw[keep], before[keep]), "bytes outside the requested fields were written"
    return {f: view[f].copy() for f in fields}


def _loss_sums(loss, cons):
    """[n][n_snr]...[ND][m] losses -> [n_snr]...[2] sums (all / considered symbols)."""
    nd_axis = loss.ndim - 2
    rest = (0, nd_axis, nd_axis + 1)
    return np.stack([loss.sum(axis=rest), np.take(loss, np.flatnonzero(cons), axis=nd_axis).sum(axis=rest)], axis=-1)


def _bars(ref, symbols, x, pn, m, cons):
    """The module docstring's bar, shaped like ref, from the demapper inputs x / pn [n][n_snr]...[ND]."""
    per_sym = m * 1e-12 * (1 + _emax(symbols, x, pn.reshape(-1)).reshape(pn.shape)) / LN2
    return 1e-10 * ref + _loss_sums(per_sym[..., None], cons)


def _tx_bits(sym, m, ndim):
    """bits of sym [n][ND] shaped to broadcast against LLRs [n][..][ND][m] of ndim axes"""
    b = ((sym[..., None] >> np.arange(m)) & 1).astype(bool)
    return b.reshape((sym.shape[0],) + (1,) * (ndim - 3) + b.shape[1:])


def _check_against_export(eng, S, sc, tag, first=5, n=3):
    """Tests 1 and 2 of one engine: both methods of loss_est against the LLR export,
    loss_perf0 against the definitions on dsce_export's y and h."""
    from dsce.modulation import bicm_info_loss, llr_awgn
    m, nd, symbols = sc["bits_per_symbol"], sc["n_data"], sc["symbols"]
    cons = np.asarray(sc["considered"]).astype(bool)
    e = _export(eng, 0, SEED, first, n, fields=("y", "h", "sym"))
    nk, ns = len(S.pn_time), S.n_iter + 1
    y = e["y"][:, :, None, :]
    xp, pp, _ = demapper_input(sc, S.pn_time, y, np.broadcast_to(e["h"][:, None, None, :], y.shape))
    for method in METHODS:
        got = _soft(eng, 0, SEED, first, n, method=method)
        assert got["loss_est"].shape == (nk, ns, 2) and got["loss_perf0"].shape == (nk, 2)
        g = _llr(eng, 0, SEED, first, n, method=method)
        ref = _loss_sums(bicm_info_loss(g["llr"], _tx_bits(e["sym"], m, 5)), cons)
        bar = _bars(ref, symbols, g["x_est"], g["pn_eff"], m, cons)
        err = np.abs(got["loss_est"] - ref)
        _note("est %s %s" % (tag, method), (err / bar).max())
        assert np.isfinite(got["loss_est"]).all() and (err <= bar).all(), (method, (err / bar).max())
        # perfect-CSI one-tap receiver: stage axis of length 1
        lp = llr_awgn(symbols, _bitmap(symbols.size), xp, pp, method).reshape(xp.shape + (m,))
        refp = _loss_sums(bicm_info_loss(lp, _tx_bits(e["sym"], m, 5)), cons)[:, 0]
        barp = _bars(refp[:, None], symbols, xp, pp, m, cons)[:, 0]
        errp = np.abs(got["loss_perf0"] - refp)
        _note("perf0 %s %s" % (tag, method), (errp / barp).max())
        assert np.isfinite(got["loss_perf0"]).all() and (got["loss_perf0"] > 0).all()
        assert (errp <= barp).all(), (method, (errp / barp).max())


@pytest.mark.parametrize("name", ["ofdm", "fbmc_aux", "fbmc_cod"])
def test_soft_against_the_export(name):
    """Default setup, n_iter 4, SNR (10, 35), batch 64, realisations 5..7 (three
    realisations in a 64-wide wave: a missing rvalid mask, a wrong unit % R or a
    wrong considered index changes the sums): loss_est of both methods is
    bicm_info_loss on export_llr's llr and the bits of export's sym; loss_perf0 is
    the same on the one-tap receiver formed from export's y and h."""
    S = harness.setup("default", schemes=(name,), snr_db=SNR, n_iter=4)
    eng = harness.engine(S, batch=64)
    try:
        assert eng.llr_info(0)["per_axis"]
        _check_against_export(eng, S, S.schemes[name], name)
    finally:
        eng.close()


def test_soft_full_table_demapper():
    """The permuted 16-QAM table of test_gpu_llr.test_full_table_form with the MMSE
    estimator built: the full-table form of llr_demap inside k_llr_info."""
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR, qam_order=16)
    sc = S.schemes["ofdm"]
    symbols = sc["symbols"][np.random.default_rng(16).permutation(16)]
    sc2 = dict(sc, symbols=symbols)
    S2 = SimpleNamespace(**dict(vars(S), schemes={"ofdm": sc2}))
    eng = harness.engine(S2, batch=64)
    try:
        assert eng.llr_info(0) == dict(per_axis=False, m=4)
        _check_against_export(eng, S2, sc2, "permuted-16")
    finally:
        eng.close()


@pytest.fixture(scope="module")
def soft_ofdm():
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR)
    eng = harness.engine(S, batch=64)
    yield S, eng
    eng.close()


def _close(a, b):
    for f in a:
        np.testing.assert_allclose(a[f], b[f], rtol=1e-10, atol=0, err_msg=f)


def test_soft_invariance_and_accumulation(soft_ofdm):
    """129 realisations from 5: batch 128, an export_stage_mb that cuts the batch
    into one-wave sub-batches and two calls adding into one array equal the
    batch-64 sums at rtol 1e-10; the same call twice is bit-identical; n_rep = 0
    adds nothing; one field requested leaves the other's memory alone (_soft)."""
    S, eng = soft_ofdm
    eng.set_batch(64)
    ref = _soft(eng, 0, SEED, 5, 129)
    again = _soft(eng, 0, SEED, 5, 129)
    for f in BOTH:
        assert (ref[f] > 0).all() and np.array_equal(ref[f], again[f]), f
    eng.set_batch(128)
    try:
        whole = _soft(eng, 0, SEED, 5, 129)
        eng.set_option("export_stage_mb", 12)
        cut = _soft(eng, 0, SEED, 5, 129)
    finally:
        eng.set_option("export_stage_mb", 1024)
        eng.set_batch(64)
    _close(whole, ref)
    _close(cut, ref)
    a = _soft(eng, 0, SEED, 5, 70)
    ab = _soft(eng, 0, SEED, 75, 59, into=a)
    _close(ab, ref)
    for f in BOTH:
        assert (ab[f] > a[f]).all(), f
    start = {f: np.full_like(ref[f], 1.5) for f in BOTH}
    z = _soft(eng, 0, SEED, 5, 0, into=start)
    for f in BOTH:
        assert np.array_equal(z[f], start[f]), f
    for f in BOTH:
        one = _soft(eng, 0, SEED, 5, 129, fields=(f,))
        assert list(one) == [f] and np.array_equal(one[f], ref[f]), f
    # the Python wrapper: from zero, and adding into `out`
    w = eng.run_soft(0, SEED, 5, 129)
    for f in BOTH:
        assert np.array_equal(w[f], ref[f]), f
    w2 = eng.run_soft(0, SEED, 5, 129, out={"loss_perf0": w["loss_perf0"]})
    assert list(w2) == ["loss_perf0"] and np.allclose(w2["loss_perf0"], 2 * ref["loss_perf0"], rtol=1e-14, atol=0)
    rate = eng.bicm_rate(0, ref["loss_est"], 129)
    nd = eng.bits_per_rep(0) / 8.0                                            # 256-QAM: ND of both edge classes
    assert rate.shape == ref["loss_est"].shape and (rate < 8).all() and nd[0] == S.schemes["ofdm"]["n_data"]
    assert np.array_equal(rate, 8 - ref["loss_est"] / (129 * nd))


def test_soft_snr_chunks():
    """Option snr_chunk = 1 with three SNR points equals the unchunked engine."""
    S = harness.setup("default", schemes=("ofdm",), snr_db=(10.0, 20.0, 35.0), n_iter=2)
    eng = harness.engine(S, batch=64, options={"snr_chunk": 1})
    whole = harness.engine(S, batch=64)
    try:
        e = _soft(eng, 0, SEED, 5, 129)
        assert e["loss_est"].shape == (3, 3, 2) and e["loss_perf0"].shape == (3, 2)
        _close(e, _soft(whole, 0, SEED, 5, 129))
    finally:
        eng.close()
        whole.close()


def test_soft_sub_batch_cuts(soft_ofdm):
    """Realisations [0, 130): batch 128 with export_stage_mb 1 (one-wave
    sub-batches), then with snr_chunk 1, give the batch-64 sums at rtol 1e-10 (the
    module docstring's bar for the order of summation)."""
    S, eng = soft_ofdm
    eng.set_batch(64)
    ref = _soft(eng, 0, SEED, 0, 130)
    try:
        eng.set_batch(128)
        eng.set_option("export_stage_mb", 1)
        _close(_soft(eng, 0, SEED, 0, 130), ref)
        eng.set_option("export_stage_mb", 1024)
        eng.set_option("snr_chunk", 1)
        _close(_soft(eng, 0, SEED, 0, 130), ref)
    finally:
        eng.set_option("export_stage_mb", 1024)
        eng.set_option("snr_chunk", 0)
        eng.set_batch(64)


def test_soft_errors_and_side_effects(soft_ofdm):
    from dsce import engine
    S, eng = soft_ofdm
    eng.set_batch(64)
    counts = eng.run(SEED, 0, 64)
    path = eng.path_info(0)

    def fails(code, *a, **k):
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % code):
            _soft(eng, *a, **k)
        assert np.array_equal(eng.run(SEED, 0, 64), counts)

    fails(EINVAL, 0, SEED, 5, 3, fields=())                                   # both fields null
    fails(EINVAL, 0, SEED, 5, 3, flags=1 << 3)                                # unknown flag
    fails(EINVAL, 0, SEED, 5, 3, flags=engine.EXPORT_F32)                     # the outputs are host doubles
    fails(EINVAL, 0, SEED, 5, 3, flags=engine.EXPORT_DEVICE)
    fails(EINVAL, 0, SEED, 5, 3, flags=engine.EXPORT_DEVICE | engine.LLR_MAXLOG)
    with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL):           # null out
        eng._chk(eng.lib.dsce_run_soft(eng.h, 0, SEED, 5, 3, 0, None), "dsce_run_soft")
    # no side effects: counters and path of a run, before and after a soft run
    eng.enable_timing(True)
    try:
        _soft(eng, 0, SEED, 3, 70)
        n, ms = eng.kernel_time("k_llr_info")
        assert n >= 1 and ms > 0
    finally:
        eng.enable_timing(False)
    assert eng.path_info(0) == path
    assert np.array_equal(eng.run(SEED, 0, 64), counts) and eng.path_info(0) == path and counts.sum() > 0
    # without dsce_build_mmse; after it the same context works
    bare = harness.engine(S, batch=64, mmse=False)
    try:
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % ESTATE):
            _soft(bare, 0, SEED, 5, 3)
        bare.build_mmse(S.zero_threshold)
        got = _soft(bare, 0, SEED, 5, 3)
        ref = _soft(eng, 0, SEED, 5, 3)
        for f in BOTH:
            assert np.array_equal(got[f], ref[f]), f
    finally:
        bare.close()
    # before channel, SNR points or scheme are set
    empty = engine.Engine(0)
    try:
        buf = np.zeros(8)
        o = engine.SoftOut(loss_perf0=buf.ctypes.data_as(engine.C.POINTER(engine.C.c_double)))
        assert empty.lib.dsce_run_soft(empty.h, 0, SEED, 0, 1, 0, engine.C.byref(o)) == ESTATE
        assert not buf.any()
    finally:
        empty.close()


def test_soft_interpolation_scheme_without_iterations():
    """An interpolation scheme with n_iter 0 needs no dsce_build_mmse (S = 1); with
    n_iter > 0 the call is DSCE_ESTATE."""
    from dsce.configs import build_doubly_flat_setup
    from dsce.engine import DsceError, Engine
    S = build_doubly_flat_setup()
    sc = S.schemes["ofdm"]
    for n_iter in (0, 1):
        eng = Engine(0)
        try:
            eng.set_channel(S.channel)
            eng.set_snr(S.pn_time[:2], n_iter)
            sid = eng.add_scheme(sc)
            eng.set_interpolation(sid, sc.extras["interp"])
            eng.set_batch(64)
            if n_iter == 0:
                e = _soft(eng, sid, SEED, 5, 65)
            else:
                with pytest.raises(DsceError, match=r"\(%d\)" % ESTATE):
                    _soft(eng, sid, SEED, 5, 3)
        finally:
            eng.close()
    assert e["loss_est"].shape == (2, 1, 2) and e["loss_perf0"].shape == (2, 2)
    assert all(np.isfinite(e[f]).all() and (e[f] > 0).all() for f in BOTH)


def test_simulate_rate(tmp_path):
    """python -m dsce.simulate --rate exact (a child process: the command line is
    what is tested): its bicm_rate is Engine.run_soft + bicm_rate on the same
    realisations."""
    from dsce.configs import build_setup
    from dsce.engine import build_engine, gpu_tx
    out = tmp_path / "rate.json"
    env = dict(os.environ, PYTHONPATH=harness.PKG)
    p = subprocess.run([sys.executable, "-m", "dsce.simulate", "--config", "default", "--schemes", "ofdm", "--reps", "65",
                        "--batch", "64", "--rate", "exact", "--out", str(out)], cwd=harness.PKG, env=env, timeout=240,
                       capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    assert "bicm_rate_ic_mmse" in p.stdout
    res = json.loads(out.read_text())
    r = res["bicm_rate"]["ofdm"]
    assert r["method"] == "exact" and res["bicm_rate_seconds"] > 0
    S = build_setup("default", schemes=("ofdm",), tx=gpu_tx(0))
    eng = build_engine(S, batch=64)
    try:
        loss = eng.run_soft(0, res["seed"], 0, 65)
        est, perf = eng.bicm_rate(0, loss["loss_est"], 65), eng.bicm_rate(0, loss["loss_perf0"], 65)
    finally:
        eng.close()
    assert est.shape == (len(S.snr_db), S.n_iter + 1, 2)
    for k, edge in enumerate(("all", "no_edge")):
        np.testing.assert_allclose(np.asarray(r["mmse"][edge]), est[:, :, k], rtol=1e-10, atol=0)
        np.testing.assert_allclose(np.asarray(r["perfect_onetap"][edge]), perf[:, k], rtol=1e-10, atol=0)
