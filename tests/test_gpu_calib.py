"""GPU: dsce_run_calib (k_llr_calib, DSCE_HAS_LLR_SCALE) — the demapper noise ratio
c |x_est - s_tx|^2 / pn_eff summed per SNR point, stage and data symbol on the
device — against dsce.modulation.demapper_noise_ratio applied in NumPy to
dsce_export_llr's own x_est / pn_eff and dsce_export's sym, y and h; the scale
tables of dsce_set_llr_scale through dsce_export_llr and dsce_run_soft; and the
call against itself across batch geometries, staging bounds, SNR chunks and split
calls.

Bar of one ratio entry (SNR, stage, symbol), a sum of non-negative terms:
1e-10 ref + sum over the realisations of 1e-12 c (|x_est| + |s_tx|)^2 / pn_eff.
The first term covers the order of summation, the second the rounding of
x_est - s_tx where the two nearly coincide (both kernels form x_est with the same
code).  The LLR and loss bars are those of tests/test_gpu_llr.py and
tests/test_gpu_soft.py.  Every host destination sits between guard regions
(_calib)."""
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
from test_gpu_soft import _bars, _loss_sums, _soft, _tx_bits
from test_llr_host import demapper_input

pytestmark = pytest.mark.gpu

BOTH = ("ratio_est", "ratio_perf0")
WORST = {}


def _note(key, ratio):
    """Worst error / bar seen per check (printed; DESIGN.md section 7i quotes them)."""
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))
    print("calib ratio %-28s %.3e" % (key, WORST[key]))


def _calib(eng, sid, seed, first, n, fields=BOTH, flags=0, into=None):
    """dsce_run_calib into zeroed arrays (or copies of `into`) that share one buffer,
    guard | ratio_est | guard | ratio_perf0 | guard; only `fields` are passed.
    Asserts that the guards and the field not requested keep their bytes."""
    from dsce import engine
    shapes = eng.calib_shapes(sid)
    raw = np.full(3 * GUARD + sum(int(np.prod(shapes[f])) * 8 for f in BOTH), PATTERN, dtype=np.uint8)
    view, at = {}, GUARD
    for f in BOTH:
        nb = int(np.prod(shapes[f])) * 8
        view[f] = raw[at:at + nb].view(np.float64).reshape(shapes[f])
        at += nb + GUARD
    for f in fields:
        view[f][...] = 0.0 if into is None else into[f]
    before = raw.copy()
    o = engine.CalibOut(**{f: view[f].ctypes.data_as(engine.C.POINTER(engine.C.c_double)) for f in fields})
    eng._chk(eng.lib.dsce_run_calib(eng.h, sid, seed, first, n, flags, engine.C.byref(o)), "dsce_run_calib")
    keep = np.ones(raw.size, dtype=bool)
    for f in fields:
        a0 = view[f].ctypes.data - raw.ctypes.data
        keep[a0:a0 + view[f].nbytes] = False
    assert np.array_equal(raw[keep], before[keep]), "bytes outside the requested fields were written"
    return {f: view[f].copy() for f in fields}


def _ratio_ref(x, pn, sym, symbols, real_detect):
    """(reference sums, bars) over the realisations (axis 0) of x / pn [n][..][ND] and sym [n][ND]"""
    from dsce.modulation import demapper_noise_ratio
    s = sym.reshape((sym.shape[0],) + (1,) * (x.ndim - 2) + sym.shape[1:])
    ref = demapper_noise_ratio(x, pn, s, symbols, real_detect).sum(axis=0)
    c = 2.0 if real_detect else 1.0
    bar = 1e-10 * ref + (1e-12 * c * (np.abs(x) + np.abs(np.asarray(symbols)[s])) ** 2 / pn).sum(axis=0)
    return ref, bar


def _check_against_export(eng, S, sc, tag, first=5, n=3):
    symbols, rd = sc["symbols"], bool(sc["real_detect"])
    e = _export(eng, 0, SEED, first, n, fields=("y", "h", "sym"))
    g = _llr(eng, 0, SEED, first, n, fields=("x_est", "pn_eff"))
    got = _calib(eng, 0, SEED, first, n)
    nk, ns, nd = len(S.pn_time), S.n_iter + 1, sc["n_data"]
    assert got["ratio_est"].shape == (nk, ns, nd) and got["ratio_perf0"].shape == (nk, nd)
    ref, bar = _ratio_ref(g["x_est"], g["pn_eff"], e["sym"], symbols, rd)
    y = e["y"][:, :, None, :]
    xp, pp, _ = demapper_input(sc, S.pn_time, y, np.broadcast_to(e["h"][:, None, None, :], y.shape))
    refp, barp = _ratio_ref(xp, pp, e["sym"], symbols, rd)
    for f, r, b in (("ratio_est", ref, bar), ("ratio_perf0", refp[:, 0], barp[:, 0])):
        err = np.abs(got[f] - r)
        _note("%s %s" % (f, tag), (err / b).max())
        assert np.isfinite(got[f]).all() and (got[f] > 0).all(), f
        assert (err <= b).all(), (f, (err / b).max())


@pytest.mark.parametrize("name", ["ofdm", "fbmc_aux", "fbmc_cod"])
def test_calib_against_the_exports(name):
    """Default setup, n_iter 4, SNR (10, 35), batch 64, realisations 5..7."""
    S = harness.setup("default", schemes=(name,), snr_db=SNR, n_iter=4)
    eng = harness.engine(S, batch=64)
    try:
        _check_against_export(eng, S, S.schemes[name], name)
    finally:
        eng.close()


def test_calib_full_table_engine():
    """The permuted 16-QAM table of test_soft_full_table_demapper: the lookup of the
    transmitted symbol goes through the caller's table."""
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR, qam_order=16)
    sc = S.schemes["ofdm"]
    sc2 = dict(sc, symbols=sc["symbols"][np.random.default_rng(16).permutation(16)])
    S2 = SimpleNamespace(**dict(vars(S), schemes={"ofdm": sc2}))
    eng = harness.engine(S2, batch=64)
    try:
        assert eng.llr_info(0) == dict(per_axis=False, m=4)
        _check_against_export(eng, S2, sc2, "permuted-16")
    finally:
        eng.close()


@pytest.fixture(scope="module", params=["ofdm", "fbmc_cod"])
def scaled(request):
    """Per scheme (default setup, n_iter 4, SNR (10, 35), batch 64): the engine, its
    unscaled LLR export and soft / calib sums of realisations 5..7, and seeded
    tables g = 10**uniform(-1, 2) (not yet installed)."""
    name = request.param
    S = harness.setup("default", schemes=(name,), snr_db=SNR, n_iter=4)
    eng = harness.engine(S, batch=64)
    shapes = eng.calib_shapes(0)
    rng = np.random.default_rng(77)
    g_est = 10.0 ** rng.uniform(-1, 2, shapes["ratio_est"])
    g_perf0 = 10.0 ** rng.uniform(-1, 2, shapes["ratio_perf0"])
    base = {m: _llr(eng, 0, SEED, 5, 3, method=m) for m in METHODS}
    soft = {m: _soft(eng, 0, SEED, 5, 3, method=m) for m in METHODS}
    calib = _calib(eng, 0, SEED, 5, 3)
    yield SimpleNamespace(name=name, S=S, sc=S.schemes[name], eng=eng, g_est=g_est, g_perf0=g_perf0, base=base,
                          soft=soft, calib=calib)
    eng.close()


def test_scaled_export(scaled):
    """With g installed x_est keeps its bits, pn_eff is unscaled * g to one rounding,
    llr is the probe's on the scaled pn_eff; removing the tables restores every bit;
    llr_scale round-trips."""
    eng, sc = scaled.eng, scaled.sc
    none = eng.llr_scale(0)
    assert none["set"] == (False, False) and (none["g_est"] == 1).all() and (none["g_perf0"] == 1).all()
    eng.set_llr_scale(0, scaled.g_est, scaled.g_perf0)
    try:
        back = eng.llr_scale(0)
        assert back["set"] == (True, True)
        assert np.array_equal(back["g_est"], scaled.g_est) and np.array_equal(back["g_perf0"], scaled.g_perf0)
        for method in METHODS:
            b, g = scaled.base[method], _llr(eng, 0, SEED, 5, 3, method=method)
            assert np.array_equal(g["x_est"], b["x_est"])
            np.testing.assert_allclose(g["pn_eff"], b["pn_eff"] * scaled.g_est[None], rtol=4e-16, atol=0)
            ref = eng.llr_awgn(0, g["x_est"], g["pn_eff"], method).reshape(g["llr"].shape)
            bar = 1e-12 * (1 + _emax(sc["symbols"], g["x_est"], g["pn_eff"].reshape(-1))).reshape(g["pn_eff"].shape + (1,))
            err = np.abs(g["llr"] - ref)
            _note("scaled llr %s %s" % (scaled.name, method), (err / bar).max())
            assert (err <= bar).all() and not np.array_equal(g["llr"], b["llr"])
        eng.set_llr_scale(0, scaled.g_est)                                    # a null argument removes that table
        assert eng.llr_scale(0)["set"] == (True, False)
    finally:
        eng.set_llr_scale(0)
    assert eng.llr_scale(0)["set"] == (False, False)
    for method in METHODS:
        g = _llr(eng, 0, SEED, 5, 3, method=method)
        for f in g:
            assert np.array_equal(g[f], scaled.base[method][f]), (method, f)


def test_run_soft_honours_the_tables(scaled):
    """loss_est is bicm_info_loss on the scaled export's LLRs, loss_perf0 the NumPy
    one-tap figure with g_perf0 pn_eff; with g_perf0 alone loss_est keeps its bits."""
    from dsce.modulation import bicm_info_loss, llr_awgn
    eng, sc, S = scaled.eng, scaled.sc, scaled.S
    m, symbols = sc["bits_per_symbol"], sc["symbols"]
    cons = np.asarray(sc["considered"]).astype(bool)
    e = _export(eng, 0, SEED, 5, 3, fields=("y", "h", "sym"))
    y = e["y"][:, :, None, :]
    xp, pp, _ = demapper_input(sc, S.pn_time, y, np.broadcast_to(e["h"][:, None, None, :], y.shape))
    pp = pp * scaled.g_perf0[None, :, None, :]
    eng.set_llr_scale(0, scaled.g_est, scaled.g_perf0)
    try:
        for method in METHODS:
            got = _soft(eng, 0, SEED, 5, 3, method=method)
            g = _llr(eng, 0, SEED, 5, 3, method=method)
            ref = _loss_sums(bicm_info_loss(g["llr"], _tx_bits(e["sym"], m, 5)), cons)
            bar = _bars(ref, symbols, g["x_est"], g["pn_eff"], m, cons)
            err = np.abs(got["loss_est"] - ref)
            _note("scaled est %s %s" % (scaled.name, method), (err / bar).max())
            assert np.isfinite(got["loss_est"]).all() and (err <= bar).all(), (method, (err / bar).max())
            assert not np.array_equal(got["loss_est"], scaled.soft[method]["loss_est"])
            lp = llr_awgn(symbols, _bitmap(symbols.size), xp, pp, method).reshape(xp.shape + (m,))
            refp = _loss_sums(bicm_info_loss(lp, _tx_bits(e["sym"], m, 5)), cons)[:, 0]
            barp = _bars(refp[:, None], symbols, xp, pp, m, cons)[:, 0]
            errp = np.abs(got["loss_perf0"] - refp)
            _note("scaled perf0 %s %s" % (scaled.name, method), (errp / barp).max())
            assert (errp <= barp).all(), (method, (errp / barp).max())
        eng.set_llr_scale(0, None, scaled.g_perf0)
        for method in METHODS:
            got = _soft(eng, 0, SEED, 5, 3, method=method)
            assert np.array_equal(got["loss_est"], scaled.soft[method]["loss_est"]), method
            assert not np.array_equal(got["loss_perf0"], scaled.soft[method]["loss_perf0"]), method
    finally:
        eng.set_llr_scale(0)


def test_run_calib_ignores_the_tables(scaled):
    eng = scaled.eng
    eng.set_llr_scale(0, scaled.g_est, scaled.g_perf0)
    try:
        got = _calib(eng, 0, SEED, 5, 3)
    finally:
        eng.set_llr_scale(0)
    for f in BOTH:
        assert np.array_equal(got[f], scaled.calib[f]), f


@pytest.fixture(scope="module")
def calib_ofdm():
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR)
    eng = harness.engine(S, batch=64)
    yield S, eng
    eng.close()


def _close(a, b):
    for f in a:
        np.testing.assert_allclose(a[f], b[f], rtol=1e-10, atol=0, err_msg=f)


def test_calib_invariance_and_accumulation(calib_ofdm):
    """129 realisations from 5: batch 128, an export_stage_mb that cuts the batch
    into one-wave sub-batches and two calls adding into one array equal the
    batch-64 sums at rtol 1e-10; the same call twice is bit-identical; n_rep = 0
    adds nothing; one field requested leaves the other's memory alone (_calib)."""
    S, eng = calib_ofdm
    eng.set_batch(64)
    ref = _calib(eng, 0, SEED, 5, 129)
    again = _calib(eng, 0, SEED, 5, 129)
    for f in BOTH:
        assert (ref[f] > 0).all() and np.array_equal(ref[f], again[f]), f
    eng.set_batch(128)
    try:
        whole = _calib(eng, 0, SEED, 5, 129)
        eng.set_option("export_stage_mb", 12)
        cut = _calib(eng, 0, SEED, 5, 129)
    finally:
        eng.set_option("export_stage_mb", 1024)
        eng.set_batch(64)
    _close(whole, ref)
    _close(cut, ref)
    a = _calib(eng, 0, SEED, 5, 70)
    ab = _calib(eng, 0, SEED, 75, 59, into=a)
    _close(ab, ref)
    for f in BOTH:
        assert (ab[f] > a[f]).all(), f
    start = {f: np.full_like(ref[f], 1.5) for f in BOTH}
    z = _calib(eng, 0, SEED, 5, 0, into=start)
    for f in BOTH:
        assert np.array_equal(z[f], start[f]), f
    for f in BOTH:
        one = _calib(eng, 0, SEED, 5, 129, fields=(f,))
        assert list(one) == [f] and np.array_equal(one[f], ref[f]), f
    # the Python wrapper: from zero, and adding into `out`
    w = eng.run_calib(0, SEED, 5, 129)
    for f in BOTH:
        assert np.array_equal(w[f], ref[f]), f
    w2 = eng.run_calib(0, SEED, 5, 129, out={"ratio_perf0": w["ratio_perf0"]})
    assert list(w2) == ["ratio_perf0"] and np.allclose(w2["ratio_perf0"], 2 * ref["ratio_perf0"], rtol=1e-14, atol=0)


def test_calib_snr_chunks():
    """Option snr_chunk = 1 with three SNR points equals the unchunked engine."""
    S = harness.setup("default", schemes=("ofdm",), snr_db=(10.0, 20.0, 35.0), n_iter=2)
    eng = harness.engine(S, batch=64, options={"snr_chunk": 1})
    whole = harness.engine(S, batch=64)
    try:
        e = _calib(eng, 0, SEED, 5, 129)
        nd = S.schemes["ofdm"]["n_data"]
        assert e["ratio_est"].shape == (3, 3, nd) and e["ratio_perf0"].shape == (3, nd)
        _close(e, _calib(whole, 0, SEED, 5, 129))
    finally:
        eng.close()
        whole.close()


def test_calib_sub_batch_cuts(calib_ofdm):
    """Realisations [0, 130): batch 128 with export_stage_mb 1 (one-wave
    sub-batches), then with snr_chunk 1, give the batch-64 sums at rtol 1e-10 (the
    module docstring's bar for the order of summation)."""
    S, eng = calib_ofdm
    eng.set_batch(64)
    ref = _calib(eng, 0, SEED, 0, 130)
    try:
        eng.set_batch(128)
        eng.set_option("export_stage_mb", 1)
        _close(_calib(eng, 0, SEED, 0, 130), ref)
        eng.set_option("export_stage_mb", 1024)
        eng.set_option("snr_chunk", 1)
        _close(_calib(eng, 0, SEED, 0, 130), ref)
    finally:
        eng.set_option("export_stage_mb", 1024)
        eng.set_option("snr_chunk", 0)
        eng.set_batch(64)


def test_calib_errors_and_side_effects(calib_ofdm):
    from dsce import engine
    S, eng = calib_ofdm
    eng.set_batch(64)
    counts = eng.run(SEED, 0, 64)
    path = eng.path_info(0)

    def fails(code, *a, **k):
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % code):
            _calib(eng, *a, **k)
        assert np.array_equal(eng.run(SEED, 0, 64), counts)

    fails(EINVAL, 0, SEED, 5, 3, fields=())                                   # both fields null
    for flags in (1, engine.LLR_MAXLOG, engine.EXPORT_F32, engine.EXPORT_DEVICE):
        fails(EINVAL, 0, SEED, 5, 3, flags=flags)                             # flags must be 0
    with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL):           # null out
        eng._chk(eng.lib.dsce_run_calib(eng.h, 0, SEED, 5, 3, 0, None), "dsce_run_calib")
    # a bad table entry is refused and the installed table stays in force
    shapes = eng.calib_shapes(0)
    g = np.full(shapes["ratio_est"], 2.0)
    gp = np.full(shapes["ratio_perf0"], 3.0)
    base = _llr(eng, 0, SEED, 5, 3, fields=("pn_eff",))["pn_eff"]
    eng.set_llr_scale(0, g, gp)
    try:
        for bad in (0.0, -1.0, np.nan, np.inf):
            for which in (0, 1):
                t = [g.copy(), gp.copy()]
                t[which].reshape(-1)[-1] = bad
                with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL):
                    eng.set_llr_scale(0, t[0], t[1])
        now = eng.llr_scale(0)
        assert now["set"] == (True, True) and np.array_equal(now["g_est"], g) and np.array_equal(now["g_perf0"], gp)
        assert np.array_equal(_llr(eng, 0, SEED, 5, 3, fields=("pn_eff",))["pn_eff"], 2.0 * base)
        # dsce_set_snr drops the tables
        eng.set_snr(S.pn_time, S.n_iter)
        assert eng.llr_scale(0)["set"] == (False, False)
        eng.build_mmse(S.zero_threshold)
        assert np.array_equal(_llr(eng, 0, SEED, 5, 3, fields=("pn_eff",))["pn_eff"], base)
    finally:
        eng.set_llr_scale(0)
    # no side effects: counters and path of a run, before and after a calibration run
    eng.enable_timing(True)
    try:
        _calib(eng, 0, SEED, 3, 70)
        n, ms = eng.kernel_time("k_llr_calib")
        assert n >= 1 and ms > 0
    finally:
        eng.enable_timing(False)
    assert eng.path_info(0) == path
    assert np.array_equal(eng.run(SEED, 0, 64), counts) and eng.path_info(0) == path and counts.sum() > 0
    # without dsce_build_mmse; after it the same context works
    bare = harness.engine(S, batch=64, mmse=False)
    try:
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % ESTATE):
            _calib(bare, 0, SEED, 5, 3)
        bare.set_llr_scale(0, g, gp)                                          # needs no estimator
        bare.set_llr_scale(0)
        bare.build_mmse(S.zero_threshold)
        got = _calib(bare, 0, SEED, 5, 3)
        ref = _calib(eng, 0, SEED, 5, 3)
        for f in BOTH:
            assert np.array_equal(got[f], ref[f]), f
    finally:
        bare.close()
    # before channel, SNR points or scheme are set
    empty = engine.Engine(0)
    try:
        buf = np.zeros(8)
        o = engine.CalibOut(ratio_perf0=buf.ctypes.data_as(engine.C.POINTER(engine.C.c_double)))
        assert empty.lib.dsce_run_calib(empty.h, 0, SEED, 0, 1, 0, engine.C.byref(o)) == ESTATE
        assert empty.lib.dsce_set_llr_scale(empty.h, 0, None, None) == ESTATE
        assert not buf.any()
    finally:
        empty.close()


def test_calib_interpolation_scheme_without_iterations():
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
                e = _calib(eng, sid, SEED, 5, 65)
            else:
                with pytest.raises(DsceError, match=r"\(%d\)" % ESTATE):
                    _calib(eng, sid, SEED, 5, 3)
        finally:
            eng.close()
    assert e["ratio_est"].shape == (2, 1, sc.n_data) and e["ratio_perf0"].shape == (2, sc.n_data)
    assert all(np.isfinite(e[f]).all() and (e[f] > 0).all() for f in BOTH)


def test_calibrated_rate_end_to_end():
    """Default ofdm, batch 64: rho from realisations 5..68, installed, run_soft exact
    on 69..132 with and without it.  At 35 dB, all symbols: the scaled rate is > 0
    and above the raw rate at every stage, the raw rate of stage 0 is < 0, and
    mean rho of stage 0 > mean rho of stage 4 > 1 (the CPU oracle on these
    realisations: scaled 4.98 .. 6.66, raw -43.1 .. -1.41, rho 50.5 and 13.9)."""
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR, n_iter=4)
    eng = harness.engine(S, batch=64)
    try:
        c = eng.run_calib(0, SEED, 5, 64)
        raw = eng.bicm_rate(0, eng.run_soft(0, SEED, 69, 64)["loss_est"], 64)
        eng.set_llr_scale(0, c["ratio_est"] / 64, c["ratio_perf0"] / 64)
        scaled = eng.bicm_rate(0, eng.run_soft(0, SEED, 69, 64)["loss_est"], 64)
    finally:
        eng.close()
    rho = (c["ratio_est"] / 64).mean(axis=-1)
    print("calib e2e scaled 35 dB", scaled[1, :, 0], "raw", raw[1, :, 0], "rho", rho[1], "10 dB scaled", scaled[0, :, 0],
          "raw", raw[0, :, 0], "rho", rho[0])
    assert (scaled[1, :, 0] > 0).all() and (scaled[1, :, 0] > raw[1, :, 0]).all()
    assert raw[1, 0, 0] < 0
    assert rho[1, 0] > rho[1, 4] > 1


def test_simulate_rate_calibrate(tmp_path):
    """python -m dsce.simulate --rate exact --calibrate (a child process: the command
    line is what is tested), 65 realisations at batch 64: the calibrated rates are
    run_calib -> set_llr_scale -> run_soft on a fresh engine, and the keys of a run
    without --calibrate hold what that run computes: run_soft with no table
    installed (tests/test_gpu_soft.py test_simulate_rate)."""
    from dsce.configs import build_setup
    from dsce.engine import build_engine, gpu_tx
    out = tmp_path / "cal.json"
    env = dict(os.environ, PYTHONPATH=harness.PKG)
    p = subprocess.run([sys.executable, "-m", "dsce.simulate", "--config", "default", "--schemes", "ofdm", "--reps", "65",
                        "--batch", "64", "--rate", "exact", "--calibrate", "--out", str(out)], cwd=harness.PKG, env=env,
                       timeout=240, capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    assert "bicm_rate_ic_mmse_calibrated" in p.stdout and "bicm_rate_ic_mmse\"" in p.stdout
    res = json.loads(out.read_text())
    r = res["bicm_rate"]["ofdm"]
    assert r["calibration"] == {"reps": 65, "in_sample": True} and r["method"] == "exact"
    S = build_setup("default", schemes=("ofdm",), tx=gpu_tx(0))
    eng = build_engine(S, batch=64)
    try:
        loss = eng.run_soft(0, res["seed"], 0, 65)
        raw_est, raw_perf = eng.bicm_rate(0, loss["loss_est"], 65), eng.bicm_rate(0, loss["loss_perf0"], 65)
        c = eng.run_calib(0, res["seed"], 0, 65)
        eng.set_llr_scale(0, c["ratio_est"] / 65, c["ratio_perf0"] / 65)
        loss = eng.run_soft(0, res["seed"], 0, 65)
        est, perf = eng.bicm_rate(0, loss["loss_est"], 65), eng.bicm_rate(0, loss["loss_perf0"], 65)
    finally:
        eng.close()
    cons = np.asarray(S.schemes["ofdm"].considered_symbols).astype(bool)
    close = lambda got, ref: np.testing.assert_allclose(np.asarray(got), ref, rtol=1e-10, atol=0)
    for k, (edge, sel) in enumerate((("all", np.ones_like(cons)), ("no_edge", cons))):
        close(r["mmse"][edge], raw_est[:, :, k])
        close(r["perfect_onetap"][edge], raw_perf[:, k])
        close(r["mmse_calibrated"][edge], est[:, :, k])
        close(r["perfect_onetap_calibrated"][edge], perf[:, k])
        close(r["noise_ratio"]["mmse"][edge], c["ratio_est"][:, :, sel].mean(axis=-1) / 65)
        close(r["noise_ratio"]["perfect_onetap"][edge], c["ratio_perf0"][:, sel].mean(axis=-1) / 65)
