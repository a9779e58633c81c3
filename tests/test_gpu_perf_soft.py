"""GPU: the perfect-CSI branch of the soft calls (DSCE_LLR_PERFECT,
DSCE_HAS_LLR_PERFECT): dsce_export_llr, dsce_run_soft and dsce_run_calib with the
flag, and the scale table of dsce_set_llr_scale_perf.  Every check fails on an
engine without the flag, where it is DSCE_EINVAL.

Shapes: the default setup, one scheme per engine, SNR (10, 35) dB, n_iter 4, seed
0x5EED0009, batch 64, realisations 5..7 (a tail wave, two SNR points, every stage).

Bars.  x_est / pn_eff against include/dsce.h's definitions evaluated in NumPy on
Engine.trace_unit's yperf and export's h: the bulk bars of tests/test_gpu_llr.py,
1e-12 x_terms and 1e-12 pn_eff.  Against the oracle's yperf and h the bar comes
from the project's trace bar, 1e-9 absolute on a y_perf row
(tests/test_gpu_poly.py): 1e-9 / (|h_l| data_div) per symbol of a select scheme,
sum_l |P[l, NP + j]| 1e-9 / |h_l| / data_div of a despread one.  LLRs 1e-12 (1 + E)
(tests/test_gpu_llr.py), loss sums the bar of tests/test_gpu_soft.py, ratio sums
the bar of tests/test_gpu_calib.py, sums across batch geometries rtol 1e-10."""
import functools
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import harness
from test_gpu_calib import _calib, _ratio_ref
from test_gpu_export import EINVAL, SEED, SNR, _export
from test_gpu_export_stages import _stages
from test_gpu_llr import ALL, METHODS, _bitmap, _emax, _llr
from test_gpu_soft import _bars, _loss_sums, _soft, _tx_bits
from test_llr_host import demapper_input

pytestmark = pytest.mark.gpu

FIRST, N = 5, 3
NAMES = ("ofdm", "fbmc_aux", "fbmc_cod")
WORST = {}


def _note(key, ratio):
    """Worst error / bar seen per check (printed; DESIGN.md section 7j quotes them)."""
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))
    print("perf-soft ratio %-32s %.3e" % (key, WORST[key]))


def _pf(method="exact", extra=0):
    from dsce import engine
    return engine.LLR_PERFECT | engine.LLR_METHODS[method] | extra


def _pllr(eng, first, n, method="exact", dtype=np.complex128, fields=ALL, rows=None):
    from dsce import engine
    f32 = engine.EXPORT_F32 if np.dtype(dtype) == np.dtype(np.complex64) else 0
    return _llr(eng, 0, SEED, first, n, fields=fields, dtype=dtype, flags=_pf(method, f32), rows=rows)


def _psoft(eng, first, n, method="exact", into=None):
    return _soft(eng, 0, SEED, first, n, fields=("loss_est",), flags=_pf(method), into=into)["loss_est"]


def _pcalib(eng, first, n, into=None):
    from dsce import engine
    return _calib(eng, 0, SEED, first, n, fields=("ratio_est",), flags=engine.LLR_PERFECT, into=into)["ratio_est"]


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The oracle's per-unit yperf [n][n_snr][S][LK] and h [n][LK] of realisations 5..7, computed once per scheme."""
    S = harness.setup("default", schemes=(name,), snr_db=SNR, n_iter=4)
    tr = {}
    harness.simulate(S, SEED, FIRST, N, [name], trace=tr)
    nk = len(SNR)
    yp = np.array([[np.asarray(tr["units"][i * nk + k]["yperf"]) for k in range(nk)] for i in range(N)])
    h = np.array([np.asarray(tr["units"][i * nk]["h"]) for i in range(N)])
    yp.setflags(write=False)
    h.setflags(write=False)
    return yp, h


def _snapshot(eng, S, name):
    """What tests 1 and 2 need of one engine, realisations 5..7: the traces, the
    exports, the run's counters and the flagged export of both methods; asserts
    that path_info is what it was before the flagged calls."""
    exp = _export(eng, 0, SEED, FIRST, N, fields=("y", "h", "sym"))
    counts = eng.run(SEED, FIRST, N)
    path = eng.path_info(0)
    st = _stages(eng, 0, SEED, FIRST, N, fields=("dec_perf",))
    tr = np.array([[eng.trace_unit(0, SEED, FIRST + i, k)["yperf"] for k in range(len(SNR))] for i in range(N)])
    eng.run(SEED, FIRST, N)                                  # the trace sets the path of its own unit
    path = eng.path_info(0)
    llr = {m: _pllr(eng, FIRST, N, method=m) for m in METHODS}
    assert eng.path_info(0) == path
    return SimpleNamespace(name=name, S=S, sc=S.schemes[name], exp=exp, counts=counts, path=path, st=st, tr=tr, llr=llr)


def _needed_rows(sc):
    """The rows of y_perf the demapper reads: data_pos, or the rows of P^H's data columns."""
    if sc["despread"]:
        NP = len(sc["pilot_pos"])
        return np.flatnonzero(np.abs(sc["P"][:, NP:]).sum(axis=1) > 0)
    return np.asarray(sc["data_pos"])


def _check_definitions(b):
    """Item 1 of the issue on one snapshot."""
    from dsce.modulation import llr_awgn
    sc, e = b.sc, b.llr["exact"]
    nd, m, dd = sc["n_data"], sc["bits_per_symbol"], sc["data_div"]
    ns = b.S.n_iter + 1
    rows = _needed_rows(sc)
    # the engine's own trace: stage 0 is y, and only the rows the path forms are compared
    yp = b.tr.copy()
    yp[:, :, 0] = b.exp["y"]
    assert np.isfinite(yp[..., rows]).all(), "a row the demapper reads is not formed"
    other = np.setdiff1d(np.arange(yp.shape[-1]), rows)
    yp[..., other] = np.where(np.isfinite(yp[..., other]), yp[..., other], 0.0)   # rows the demapper never reads
    h = np.broadcast_to(b.exp["h"][:, None, None, :], yp.shape)
    x, pe, terms = demapper_input(sc, b.S.pn_time, yp, h)
    assert e["x_est"].shape == e["pn_eff"].shape == (N, len(SNR), ns, nd) and e["llr"].shape == (N, len(SNR), ns, nd, m)
    for f in ALL:
        assert not np.isnan(e[f]).any() and not np.isnan(b.llr["maxlog"][f]).any(), f
    if sc["real_detect"]:
        assert not e["x_est"].imag.any()
    _note("x_est %s" % b.name, (np.abs(e["x_est"] - x) / (1e-12 * terms)).max())
    _note("pn_eff %s" % b.name, (np.abs(e["pn_eff"] - pe) / (1e-12 * pe)).max())
    assert (np.abs(e["x_est"] - x) <= 1e-12 * terms).all()
    assert (np.abs(e["pn_eff"] - pe) <= 1e-12 * pe).all() and (e["pn_eff"] > 0).all()
    assert np.array_equal(e["pn_eff"], np.broadcast_to(e["pn_eff"][:, :, :1], e["pn_eff"].shape))   # no stage in it
    # the oracle's yperf and h
    oy, oh = _oracle(b.name)
    ohb = np.broadcast_to(oh[:, None, None, :], oy.shape)
    xo, _, _ = demapper_input(sc, b.S.pn_time, oy, ohb)
    if sc["despread"]:
        NP = len(sc["pilot_pos"])
        bar = ((1e-9 / np.abs(ohb)) @ np.abs(sc["P"][:, NP:])) / dd
    else:
        bar = 1e-9 / (np.abs(ohb[..., np.asarray(sc["data_pos"])]) * dd)
    _note("x_est oracle %s" % b.name, (np.abs(e["x_est"] - xo) / bar).max())
    assert (np.abs(e["x_est"] - xo) <= bar).all()
    for method in METHODS:
        g = b.llr[method]
        assert np.array_equal(g["x_est"], e["x_est"]) and np.array_equal(g["pn_eff"], e["pn_eff"])
        ref = llr_awgn(sc["symbols"], _bitmap(sc["symbols"].size), g["x_est"], g["pn_eff"], method).reshape(g["llr"].shape)
        lbar = 1e-12 * (1 + _emax(sc["symbols"], g["x_est"], g["pn_eff"].reshape(-1))).reshape(g["pn_eff"].shape + (1,))
        err = np.abs(g["llr"] - ref)
        _note("llr %s %s" % (b.name, method), (err / lbar).max())
        assert (err <= lbar).all(), (method, (err / lbar).max())


def _check_closure(b):
    """Item 2 of the issue on one snapshot."""
    sc, g = b.sc, b.llr["maxlog"]
    m = sc["bits_per_symbol"]
    margin = np.abs(g["llr"] * g["pn_eff"][..., None]).min()
    print("perf-soft margin %s %.3e" % (b.name, margin))
    assert margin >= 1e-9
    bits = g["llr"] > 0
    dec = b.st["dec_perf"]
    assert (dec >= 0).all() and np.array_equal(bits, ((dec[..., None] >> np.arange(m)) & 1).astype(bool))
    tx = ((b.exp["sym"][:, None, None, :, None] >> np.arange(m)) & 1).astype(bool)
    wrong = bits != tx
    cons = np.asarray(sc["considered"]).astype(bool)
    assert b.counts.shape == (1, 2, 2, len(SNR), b.S.n_iter + 1) and b.counts[0, 1].min() > 0
    assert np.array_equal(wrong.sum(axis=(0, 3, 4)), b.counts[0, 1, 0])
    assert np.array_equal(wrong[:, :, :, cons].sum(axis=(0, 3, 4)), b.counts[0, 1, 1])


@pytest.fixture(scope="module", params=NAMES)
def pbulk(request):
    name = request.param
    S = harness.setup("default", schemes=(name,), snr_db=SNR, n_iter=4)
    eng = harness.engine(S, batch=64)
    b = _snapshot(eng, S, name)
    b.eng = eng
    yield b
    eng.close()


def test_definitions(pbulk):
    if pbulk.name == "ofdm":
        assert {"mic_stages", "pic_fft"} <= pbulk.path, pbulk.path
    _check_definitions(pbulk)


def test_closure_with_the_engine(pbulk):
    _check_closure(pbulk)


def test_sums(pbulk):
    """Flagged loss_est is bicm_info_loss on the flagged export's llr, flagged
    ratio_est is demapper_noise_ratio on its x_est / pn_eff; stage 0 of each is the
    unflagged call's perf0 figure to the bit; two calls give the same bits; a
    perf0 output with the flag is DSCE_EINVAL."""
    from dsce import engine
    from dsce.modulation import bicm_info_loss
    b, eng, sc = pbulk, pbulk.eng, pbulk.sc
    m, symbols = sc["bits_per_symbol"], sc["symbols"]
    cons = np.asarray(sc["considered"]).astype(bool)
    for method in METHODS:
        got = _psoft(eng, FIRST, N, method)
        g = b.llr[method]
        ref = _loss_sums(bicm_info_loss(g["llr"], _tx_bits(b.exp["sym"], m, 5)), cons)
        bar = _bars(ref, symbols, g["x_est"], g["pn_eff"], m, cons)
        err = np.abs(got - ref)
        _note("loss %s %s" % (b.name, method), (err / bar).max())
        assert got.shape == ref.shape and np.isfinite(got).all() and (err <= bar).all(), (method, (err / bar).max())
        plain = _soft(eng, 0, SEED, FIRST, N, method=method)
        assert np.array_equal(got[:, 0], plain["loss_perf0"])
        assert not np.array_equal(got[:, 1:], plain["loss_est"][:, 1:])
        assert np.array_equal(_psoft(eng, FIRST, N, method), got)
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL):
            _soft(eng, 0, SEED, FIRST, N, fields=("loss_est", "loss_perf0"), flags=_pf(method))
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL):
            _soft(eng, 0, SEED, FIRST, N, fields=("loss_perf0",), flags=_pf(method))
    e = b.llr["exact"]
    got = _pcalib(eng, FIRST, N)
    ref, bar = _ratio_ref(e["x_est"], e["pn_eff"], b.exp["sym"], symbols, bool(sc["real_detect"]))
    err = np.abs(got - ref)
    _note("ratio %s" % b.name, (err / bar).max())
    assert got.shape == ref.shape and np.isfinite(got).all() and (got > 0).all() and (err <= bar).all()
    plain = _calib(eng, 0, SEED, FIRST, N)
    assert np.array_equal(got[:, 0], plain["ratio_perf0"]) and not np.array_equal(got[:, 1:], plain["ratio_est"][:, 1:])
    assert np.array_equal(_pcalib(eng, FIRST, N), got)
    for fields in (("ratio_est", "ratio_perf0"), ("ratio_perf0",)):
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL):
            _calib(eng, 0, SEED, FIRST, N, fields=fields, flags=engine.LLR_PERFECT)
    # the sums are ADDED into the caller's arrays
    twice = _psoft(eng, FIRST, N, into={"loss_est": _psoft(eng, FIRST, N)})
    assert np.array_equal(twice, 2 * _psoft(eng, FIRST, N))


def test_tables(pbulk):
    """g_perf = 10^U(-1, 2): the flagged pn_eff is the unscaled one times g to one
    rounding, x_est keeps its bits, llr is Engine.llr_awgn on the scaled pn_eff to
    the bit; g_perf leaves the unflagged calls alone and g_est / g_perf0 the flagged
    ones; run_calib ignores it; removal restores the bits; bad entries are refused
    and the installed table stays; dsce_set_snr drops it."""
    from dsce import engine
    b, eng, sc = pbulk, pbulk.eng, pbulk.sc
    shapes = eng.calib_shapes(0)
    rng = np.random.default_rng(78)
    g = 10.0 ** rng.uniform(-1, 2, shapes["ratio_est"])
    g_est = 10.0 ** rng.uniform(-1, 2, shapes["ratio_est"])
    g_perf0 = 10.0 ** rng.uniform(-1, 2, shapes["ratio_perf0"])
    plain = {m: _llr(eng, 0, SEED, FIRST, N, method=m) for m in METHODS}
    plain_soft = _soft(eng, 0, SEED, FIRST, N)
    soft0, calib0 = _psoft(eng, FIRST, N), _pcalib(eng, FIRST, N)
    none = eng.llr_scale_perf(0)
    assert none["set"] is False and (none["g_perf"] == 1).all()
    eng.set_llr_scale_perf(0, g)
    try:
        back = eng.llr_scale_perf(0)
        assert back["set"] is True and np.array_equal(back["g_perf"], g)
        assert eng.llr_scale(0)["set"] == (False, False)
        for method in METHODS:
            u, s = b.llr[method], _pllr(eng, FIRST, N, method=method)
            assert np.array_equal(s["x_est"], u["x_est"])
            np.testing.assert_allclose(s["pn_eff"], u["pn_eff"] * g[None], rtol=4e-16, atol=0)
            ref = eng.llr_awgn(0, s["x_est"], s["pn_eff"], method).reshape(s["llr"].shape)
            assert np.array_equal(s["llr"], ref) and not np.array_equal(s["llr"], u["llr"])
            # the unflagged outputs do not see g_perf
            p = _llr(eng, 0, SEED, FIRST, N, method=method)
            for f in ALL:
                assert np.array_equal(p[f], plain[method][f]), (method, f)
        p = _soft(eng, 0, SEED, FIRST, N)
        assert all(np.array_equal(p[f], plain_soft[f]) for f in p)
        scaled_llr, scaled_soft = _pllr(eng, FIRST, N), _psoft(eng, FIRST, N)
        assert not np.array_equal(scaled_soft, soft0)
        assert np.array_equal(_pcalib(eng, FIRST, N), calib0)                     # run_calib ignores the table
        # the flagged outputs do not see g_est / g_perf0
        eng.set_llr_scale(0, g_est, g_perf0)
        s2 = _pllr(eng, FIRST, N)
        assert all(np.array_equal(s2[f], scaled_llr[f]) for f in ALL) and np.array_equal(_psoft(eng, FIRST, N), scaled_soft)
        eng.set_llr_scale_perf(0)
        assert eng.llr_scale(0)["set"] == (True, True) and eng.llr_scale_perf(0)["set"] is False
        s3 = _pllr(eng, FIRST, N)
        for f in ALL:
            assert np.array_equal(s3[f], b.llr["exact"][f]), f
        assert np.array_equal(_psoft(eng, FIRST, N), soft0)
        eng.set_llr_scale(0)
        # refused entries leave the installed table
        eng.set_llr_scale_perf(0, g)
        for bad in (0.0, -1.0, np.nan, np.inf):
            t = g.copy()
            t[-1, -1, -1] = bad
            with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL):
                eng.set_llr_scale_perf(0, t)
            back = eng.llr_scale_perf(0)
            assert back["set"] is True and np.array_equal(back["g_perf"], g)
        with pytest.raises(ValueError):
            eng.set_llr_scale_perf(0, g[:, :1])
        eng.set_llr_scale_perf(0)
        for method in METHODS:
            s = _pllr(eng, FIRST, N, method=method)
            for f in ALL:
                assert np.array_equal(s[f], b.llr[method][f]), (method, f)
        # dsce_set_snr drops it (the estimator is then rebuilt for the same SNR points)
        eng.set_llr_scale_perf(0, g)
        eng.set_snr(b.S.pn_time, b.S.n_iter)
        assert eng.llr_scale_perf(0)["set"] is False
        eng.build_mmse(b.S.zero_threshold)
    finally:
        eng.set_llr_scale(0)
        eng.set_llr_scale_perf(0)


@pytest.fixture(scope="module")
def ofdm():
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR)
    eng = harness.engine(S, batch=64)
    ref = SimpleNamespace(llr=_pllr(eng, 5, 129), soft=_psoft(eng, 5, 129), calib=_pcalib(eng, 5, 129))
    yield S, eng, ref
    eng.close()


def _close(a, b):
    np.testing.assert_allclose(a, b, rtol=1e-10, atol=0)


def test_geometry(ofdm):
    """129 realisations from 5: batch 128, one-wave sub-batches (a unit's staging
    with y_perf is 5 ((16 + 3 x 336) 16 + 2 x 320 x 4) = 94720 B, so 12 MiB hold one
    wave of two SNR points and not two), a split into two calls and DSCE_EXPORT_F32
    against the batch-64 calls."""
    S, eng, ref = ofdm
    eng.set_batch(128)
    try:
        whole = (_pllr(eng, 5, 129), _psoft(eng, 5, 129), _pcalib(eng, 5, 129))
        eng.set_option("export_stage_mb", 12)
        cut = (_pllr(eng, 5, 129), _psoft(eng, 5, 129), _pcalib(eng, 5, 129))
    finally:
        eng.set_option("export_stage_mb", 1024)
        eng.set_batch(64)
    for llr, soft, calib in (whole, cut):
        for f in ALL:
            assert np.array_equal(llr[f], ref.llr[f]), f
        _close(soft, ref.soft)
        _close(calib, ref.calib)
    a, b = _pllr(eng, 5, 70), _pllr(eng, 75, 59, rows=61)
    for f in ALL:
        assert np.array_equal(np.concatenate([a[f], b[f]]), ref.llr[f]), f
    _close(_psoft(eng, 75, 59, into={"loss_est": _psoft(eng, 5, 70)}), ref.soft)
    _close(_pcalib(eng, 75, 59, into={"ratio_est": _pcalib(eng, 5, 70)}), ref.calib)
    z = _pllr(eng, 5, 0, rows=1)                                                # n_rep = 0: OK, nothing written
    assert all(z[f].shape[0] == 0 for f in ALL)
    assert not _psoft(eng, 5, 0).any() and not _pcalib(eng, 5, 0).any()
    e32 = _pllr(eng, 5, 129, dtype=np.complex64)
    assert e32["x_est"].dtype == np.complex64 and e32["pn_eff"].dtype == e32["llr"].dtype == np.float32
    assert np.array_equal(e32["x_est"], ref.llr["x_est"].astype(np.complex64))
    for f in ("pn_eff", "llr"):
        assert np.array_equal(e32[f], ref.llr[f].astype(np.float32)), f


def test_snr_chunks():
    """Option snr_chunk = 1 with three SNR points equals the unchunked flagged calls."""
    S = harness.setup("default", schemes=("ofdm",), snr_db=(10.0, 20.0, 35.0), n_iter=2)
    eng = harness.engine(S, batch=64, options={"snr_chunk": 1})
    whole = harness.engine(S, batch=64)
    try:
        e, w = _pllr(eng, 5, 65), _pllr(whole, 5, 65)
        assert e["llr"].shape == (65, 3, 3, 320, 8)
        for f in ALL:
            assert np.array_equal(e[f], w[f]), f
        _close(_psoft(eng, 5, 65), _psoft(whole, 5, 65))
        _close(_pcalib(eng, 5, 65), _pcalib(whole, 5, 65))
    finally:
        eng.close()
        whole.close()


_TORCH_CHILD = r"""
import sys
import torch                       # before the engine: both then share torch's HIP runtime
import numpy as np
sys.path[:0] = [%(tests)r, %(pkg)r, %(root)r]
import harness
S = harness.setup("default", schemes=("ofdm",), snr_db=%(snr)r, n_iter=2)
eng = harness.engine(S, batch=64)
for name, method in (("complex128", "exact"), ("complex64", "maxlog")):
    dt = getattr(torch, name)
    ref = eng.export_llr(0, %(seed)d, 5, 129, method=method, dtype=np.dtype(name), branch="perfect")
    t = eng.export_llr_torch(0, %(seed)d, 5, 129, method=method, dtype=dt, branch="perfect")
    for f in ref:
        assert t[f].is_cuda and t[f].shape == ref[f].shape, (name, f)
        assert np.array_equal(t[f].cpu().numpy(), ref[f]), (name, f)
    assert np.abs(ref["llr"]).max() > 0 and np.isfinite(ref["llr"]).all()
    assert not np.array_equal(eng.export_llr(0, %(seed)d, 5, 129, method=method, dtype=np.dtype(name))["llr"], ref["llr"])
eng.close()
print("PERF_LLR_TORCH_OK")
"""


def test_torch_destination():
    """DSCE_EXPORT_DEVICE with the flag: the kernel writes torch's tensors, and they
    equal the flagged host export exactly (a child process: torch is imported
    before the engine's library is loaded, see Engine.export_torch)."""
    code = _TORCH_CHILD % dict(tests=os.path.join(harness.ROOT, "tests"), pkg=harness.PKG, root=harness.ROOT,
                               snr=SNR, seed=SEED)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "PERF_LLR_TORCH_OK" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])


@pytest.mark.parametrize("name,option,bit", [("ofdm", {"snr_loop": 1}, "snr_loop"), ("ofdm", {"pic_chain": 0}, "pic_poly"),
                                             ("ofdm", {"pic_chain": 0, "pic_poly": 0}, "pic_passes"),
                                             ("fbmc_aux", {"pic_poly": 0}, "pic_passes"),
                                             ("fbmc_cod", {"pic_poly": 0}, "pic_passes"), ("ofdm", {"mmse_ic": 0}, "pic_fft")],
                         ids=["ofdm-snr_loop", "ofdm-passes", "ofdm-banded", "fbmc_aux-banded", "fbmc_cod-banded",
                              "ofdm-chain-no-stage0"])
def test_paths(name, option, bit):
    """Definitions and closure on the other perfect-CSI paths: the looped trace
    instance of k_pic_fft, the per-iteration passes of OFDM without the chain
    (polyphase: k_poly_ana's bulk StorePerfectDetect; with pic_poly 0 the banded
    second pass), the banded passes of FBMC, and the chain without its stage 0."""
    S = harness.setup("default", schemes=(name,), snr_db=SNR, n_iter=4)
    eng = harness.engine(S, batch=64, options=option)
    try:
        b = _snapshot(eng, S, name)
        assert bit in b.path, b.path
        if option == {"mmse_ic": 0}:
            assert "mic_stages" not in b.path
        if "pic_poly" in option:
            assert "pic_poly" not in b.path
        if "pic_chain" in option:
            assert "pic_fft" not in b.path
        _check_definitions(b)
        _check_closure(b)
        assert eng.path_info(0) == b.path
    finally:
        eng.close()


def test_no_side_effects(ofdm):
    """Counters, MSE sums and path_info of a run are what they were after flagged
    calls; bit 3 stays an unknown flag on all three calls."""
    from dsce import engine
    S, eng, ref = ofdm
    eng.set_batch(64)
    eng.enable_mse()
    try:
        counts = eng.run(SEED, 0, 64)
        path = eng.path_info(0)
        mse = eng.mse()
        _pllr(eng, 3, 70)
        _psoft(eng, 3, 70)
        _pcalib(eng, 3, 70)
        assert eng.path_info(0) == path
        after = eng.mse()
        assert np.array_equal(after[0], mse[0]) and np.array_equal(after[1], mse[1])
        assert np.array_equal(eng.run(SEED, 0, 64), counts) and eng.path_info(0) == path and counts.sum() > 0
    finally:
        eng.enable_mse(False)
    for bad in (1 << 3, engine.LLR_PERFECT | (1 << 3), engine.LLR_PERFECT | (1 << 5)):
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL):
            _llr(eng, 0, SEED, 5, 3, flags=bad)
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL):
            _soft(eng, 0, SEED, 5, 3, fields=("loss_est",), flags=bad)
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL):
            _calib(eng, 0, SEED, 5, 3, fields=("ratio_est",), flags=bad)
    for bad in (engine.LLR_MAXLOG, engine.EXPORT_F32):                         # run_calib: 0 or the flag, nothing else
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL):
            _calib(eng, 0, SEED, 5, 3, fields=("ratio_est",), flags=engine.LLR_PERFECT | bad)
    with pytest.raises(ValueError):
        eng.export_llr(0, SEED, 5, 3, branch="both")
    # the Engine methods are the flagged calls
    assert np.array_equal(eng.export_llr(0, SEED, 5, 3, branch="perfect")["llr"], ref.llr["llr"][:3])
    assert set(eng.run_soft(0, SEED, 5, 3, branch="perfect")) == {"loss_est"}
    assert np.array_equal(eng.run_calib(0, SEED, 5, 129, branch="perfect")["ratio_est"], ref.calib)


def test_interpolation_scheme_without_iterations():
    """An interpolation scheme with n_iter 0: the single stage, which is the one-tap
    perfect-CSI receiver."""
    from dsce.configs import build_doubly_flat_setup
    from dsce.engine import Engine
    S = build_doubly_flat_setup()
    sc = S.schemes["ofdm"]
    eng = Engine(0)
    try:
        eng.set_channel(S.channel)
        eng.set_snr(S.pn_time[:2], 0)
        sid = eng.add_scheme(sc)
        eng.set_interpolation(sid, sc.extras["interp"])
        eng.set_batch(64)
        e = _pllr(eng, 5, 65)
        soft, plain = _psoft(eng, 5, 65), _soft(eng, sid, SEED, 5, 65)
        calib, cplain = _pcalib(eng, 5, 65), _calib(eng, sid, SEED, 5, 65)
    finally:
        eng.close()
    assert e["llr"].shape == (65, 2, 1, sc.n_data, sc.bits_per_symbol) and np.isfinite(e["llr"]).all()
    assert soft.shape == (2, 1, 2) and np.array_equal(soft[:, 0], plain["loss_perf0"])
    assert calib.shape == (2, 1, sc.n_data) and np.array_equal(calib[:, 0], cplain["ratio_perf0"])


def test_simulate_rate_calibrate(tmp_path):
    """python -m dsce.simulate --rate exact --calibrate over 65 realisations (a child
    process: the command line is what is tested): perfect_ic, perfect_ic_calibrated
    and noise_ratio["perfect_ic"] are the flagged Engine calls on the same
    realisations, and the keys that existed before hold the unflagged calls'
    figures."""
    from dsce.configs import build_setup
    from dsce.engine import build_engine, gpu_tx
    out = tmp_path / "cal.json"
    env = dict(os.environ, PYTHONPATH=harness.PKG)
    p = subprocess.run([sys.executable, "-m", "dsce.simulate", "--config", "default", "--schemes", "ofdm", "--reps", "65",
                        "--batch", "64", "--rate", "exact", "--calibrate", "--out", str(out)], cwd=harness.PKG, env=env,
                       timeout=240, capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    assert "bicm_rate_ic_perfect" in p.stdout and "bicm_rate_ic_mmse_calibrated" in p.stdout
    res = json.loads(out.read_text())
    r = res["bicm_rate"]["ofdm"]
    assert set(r) == {"mmse", "perfect_onetap", "perfect_ic", "method", "mmse_calibrated", "perfect_onetap_calibrated",
                      "perfect_ic_calibrated", "noise_ratio", "calibration"}
    assert set(r["noise_ratio"]) == {"mmse", "perfect_onetap", "perfect_ic"}
    S = build_setup("default", schemes=("ofdm",), tx=gpu_tx(0))
    eng = build_engine(S, batch=64)
    try:
        seed = res["seed"]
        rate = lambda loss: eng.bicm_rate(0, loss, 65)
        loss = eng.run_soft(0, seed, 0, 65)
        raw_est, raw_p0 = rate(loss["loss_est"]), rate(loss["loss_perf0"])
        raw_pi = rate(eng.run_soft(0, seed, 0, 65, branch="perfect")["loss_est"])
        c = eng.run_calib(0, seed, 0, 65)
        cp = eng.run_calib(0, seed, 0, 65, branch="perfect")["ratio_est"]
        eng.set_llr_scale(0, c["ratio_est"] / 65, c["ratio_perf0"] / 65)
        eng.set_llr_scale_perf(0, cp / 65)
        loss = eng.run_soft(0, seed, 0, 65)
        est, p0 = rate(loss["loss_est"]), rate(loss["loss_perf0"])
        pi = rate(eng.run_soft(0, seed, 0, 65, branch="perfect")["loss_est"])
    finally:
        eng.close()
    cons = np.asarray(S.schemes["ofdm"].considered_symbols).astype(bool)
    close = lambda got, ref: np.testing.assert_allclose(np.asarray(got), ref, rtol=1e-10, atol=0)
    for k, (edge, sel) in enumerate((("all", np.ones_like(cons)), ("no_edge", cons))):
        close(r["perfect_ic"][edge], raw_pi[:, :, k])
        close(r["perfect_ic_calibrated"][edge], pi[:, :, k])
        close(r["noise_ratio"]["perfect_ic"][edge], cp[:, :, sel].mean(axis=-1) / 65)
        close(np.asarray(r["perfect_ic"][edge])[:, 0], raw_p0[:, k])
        # the keys that existed before
        close(r["mmse"][edge], raw_est[:, :, k])
        close(r["perfect_onetap"][edge], raw_p0[:, k])
        close(r["mmse_calibrated"][edge], est[:, :, k])
        close(r["perfect_onetap_calibrated"][edge], p0[:, k])
        close(r["noise_ratio"]["mmse"][edge], c["ratio_est"][:, :, sel].mean(axis=-1) / 65)
        close(r["noise_ratio"]["perfect_onetap"][edge], c["ratio_perf0"][:, sel].mean(axis=-1) / 65)
    rho = np.asarray(r["noise_ratio"]["perfect_ic"]["all"])
    assert (rho[-1, 1:] < np.asarray(r["noise_ratio"]["mmse"]["all"])[-1, 1:]).all()   # estimation error adds noise
