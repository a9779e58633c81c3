"""GPU: every kind of frame dsce_add_scheme accepts (tests/geometries.py: pilot
counts 1, 3, 5, 8, 12, 16, 32, 36, 40 and 64, LK with a partial row block, blocks
that straddle OFDM symbols, ND off a multiple of 32, FBMC off L = 24 / 48), where
the rest of the suite hands it the reference script's three frames (NP 16 or 32,
LK a multiple of 24).

Behind that boundary the engine branches on exactly those numbers; what any
other frame gets are the generic kernels (k_wcontract_valu, k_ls_hest + k_detect
+ k_precode, the banded TX / Q^H / HD matvecs and perfect-CSI passes) and pair-
tile instances no script frame selects (k_wpair3<24, 2, false> at NP 8,
<24, 8, false> at NP 32, k_wrow3<2> and <4> at FBMC's NP 8 and 16,
k_stage_fused<8> with IC iterations).  Per geometry:
the setup kernels against the oracle (R_hP, R_est, R_noI at 1e-12 max|R_hP|; W
and W0 at _check_W's cond-scaled bar), dsce_run's counters over a tail wave
against refsim.simulate (exact: tests/test_geometries_host.py shows the oracle
flags no borderline decision there), one unit traced per element, the
dimensions the engine reports, and the kernel path, written from the guards'
text.  k_rinv's working set passes 64 KiB at NP 37 and gfx950's LDS at NP 59:
NP 40 and 64 build through its device-memory form; a context whose LDS limit
does not hold the [NP][64] tiles refuses the scheme before any launch."""
from types import SimpleNamespace

import numpy as np
import pytest

import geometries as geo
import harness
from test_gpu_export import SEED as XSEED
from test_gpu_export import _check_against_units, _export, _oracle_units
from test_gpu_export_stages import _check_against_oracle, _stages
from test_gpu_llr import _bitmap, _emax, _llr
from test_gpu_parity import _check_W
from test_gpu_script_params import _check_counts, _check_unit
from test_llr_host import demapper_input

pytestmark = pytest.mark.gpu

FFT_FORM = {"pic_fft", "mic_fft", "mic_stages", "txrx_fft", "wpair3_fused"}
PAIR = {"wpair3", "wpair3_fused", "wrow3"}
PATHS = {}


@pytest.fixture(scope="module", params=list(geo.GEOMETRIES))
def ctx(request):
    """Per geometry: its setup, the oracle's estimator and one engine at batch 64
    with the default options, shared by the geometry's tests."""
    gid = request.param
    T, S = geo.geometry_setup(gid)
    eng = harness.engine(S, batch=64)
    yield SimpleNamespace(id=gid, T=T, S=S, eng=eng, name=T.scheme, sc=S.schemes[T.scheme],
                          mm=harness.oracle_mmse(S, T.scheme))
    eng.close()


def _expected_path(gid, T, sc):
    """(must, must_not, one_of) from the guards of launch_rx_front, run_batch,
    launch_wcontract, launch_stage and launch_perfect_ic (kernels_mc.hip,
    dsce_api.hip).  pf_ok (24-row blocks on 24-sample windows) holds on the
    default OFDM frame only; the chain kernel and the fused perfect-CSI pass
    need stage_fused_ok (NP in {8, 16, 32}, select mode); the pair tiles NP / 4
    in {2, 4, 8}; the MMSE chain and the fused contraction NP = 16; the
    polyphase passes L in {24, 48}."""
    NP = len(sc["pilot_pos"])
    fused = NP in (8, 16, 32) and not sc["despread"]
    must = {"stage_fused" if fused else "stage_split"}
    must_not = {"stage_split" if fused else "stage_fused", "mic_fft", "mic_stages", "mic_lr", "wpair3_fused"}
    if NP in (8, 16, 32):
        one_of = {"wpair3", "wrow3"}
        must_not |= {"wcontract_valu"}
    else:
        one_of = None
        must |= {"wcontract_valu"}
        must_not |= PAIR
    if gid in geo.OFDM_DEFAULT_FRAME:
        must |= {"txrx_fft", "noise_fused"}
        if fused:
            must |= {"pic_fft", "wpair3"}
            must_not |= {"pic_passes", "pic_poly"}
        else:
            must |= {"pic_poly"}                         # L = 24 factorises: the polyphase passes
            must_not |= {"pic_fft", "pic_passes"}
    else:
        must |= {"pic_passes"}                           # L = 12, 20: no polyphase form
        must_not |= FFT_FORM | {"pic_poly"}
        if one_of:
            must |= {"wrow3"}                            # FBMC's W blocks have 32 rows: k_wrow3<NP / 4>
    return must, must_not, one_of


def test_dimensions(ctx):
    N, LK, NP, ND = geo.dims(ctx.id)
    d = ctx.eng.scheme_dims(0)
    assert (d.n_samples, d.lk, d.n_pilots, d.n_data, d.n_tx_symbols) == (N, LK, NP, ND, NP + ND)
    assert (d.n_schemes, d.n_snr, d.n_iter) == (1, 2, 2)
    m = ctx.sc["bits_per_symbol"]
    bits = ctx.eng.bits_per_rep(0)
    assert bits[0] == ND * m and bits[1] == int(np.sum(ctx.sc["considered"])) * m


def test_setup_kernels_match_oracle(ctx):
    """k_mcoef, k_rhp, k_rest_diag (R_hP, R_est, R_noI), then k_rinv, k_rdij and
    k_w (W, W0 of both SNR points) at this NP, N and row-block layout."""
    mm = ctx.mm
    rhp, rest, rnoi = ctx.eng.correlation(0)
    scale = np.abs(mm["R_hP"]).max()
    np.testing.assert_allclose(rhp, mm["R_hP"], rtol=0, atol=1e-12 * scale)
    np.testing.assert_allclose(rest, mm["R_est"], rtol=0, atol=1e-12 * scale)
    np.testing.assert_allclose(rnoi, mm["R_noI"], rtol=0, atol=1e-12 * scale)
    _check_W(ctx.eng, mm, 2)


def test_counts_and_path(ctx):
    """dsce_run over realisations 0..n_rep-1 (a tail wave: 48 or more padding
    lanes) equals refsim.simulate to the bit, on the kernels the guards select."""
    T, eng = ctx.T, ctx.eng
    res = geo.oracle_counts(ctx.id)
    assert res["borderline"].sum() == 0 and res["err"][0, 0].min() > 0
    path = _check_counts(eng, res, ctx.id, n=T.n_rep, seed=T.seed)
    PATHS[ctx.id] = path
    N, LK, NP, ND = geo.dims(ctx.id)
    print("geometry %-18s NP %2d LK %3d ND %3d cond %.1e path %s" % (
        ctx.id, NP, LK, ND, max(np.linalg.cond(R) for k in ("R_est", "R_noI") for R in ctx.mm[k]),
        ",".join(sorted(path))))
    must, must_not, one_of = _expected_path(ctx.id, T, ctx.sc)
    assert must <= path and not path & must_not, (ctx.id, sorted(path), sorted(must - path), sorted(path & must_not))
    if one_of:
        assert path & one_of, (ctx.id, path)
    # padding lanes count nowhere: the same range as two runs
    a = T.n_rep // 2 - 1
    np.testing.assert_array_equal(eng.run(T.seed, 0, a) + eng.run(T.seed, a, T.n_rep - a), eng.run(T.seed, 0, T.n_rep))


def test_unit_trace_matches_oracle(ctx):
    """Every stage of one unit per element (1e-10 for y and h, 1e-9 per stage);
    y_perf of the IC iterations on the rows the path forms (include/dsce.h at
    dsce_trace): the data rows under k_pic_fft (NP 8 and 32 on the default
    frame), every row on the unfused perfect-CSI passes."""
    NP = len(ctx.sc["pilot_pos"])
    chain = ctx.id in geo.OFDM_DEFAULT_FRAME and NP in (8, 32)
    rows = ctx.sc["data_pos"] if chain else np.arange(ctx.sc["G"].shape[1])
    _check_unit(ctx.S, ctx.eng, ctx.name, yperf_rows=rows, seed=ctx.T.seed)
    if ctx.id in PATHS:
        assert ctx.eng.path_info(0) == PATHS[ctx.id]     # the trace ran the run's kernels


FORCED = ({"wcontract_valu": 1}, {"stage_split": 1}, {"pfuse": 0}, {"noise_fuse": 0}, {"tx_rows": 0}, {"jakes_win": 0})


@pytest.mark.parametrize("gid", ["ofdm12x7_np5", "ofdm20x5_np12", "fbmc12x11_aux_np3"])
def test_forced_options_change_no_count(gid):
    """The un-fused noise, k_tx_symbols, the Jakes taps at every sample and the
    options that already hold on these frames: the counts of the default run."""
    T, S = geo.geometry_setup(gid)
    res = geo.oracle_counts(gid)
    eng = harness.engine(S, batch=64)
    try:
        ref = eng.run(T.seed, 0, T.n_rep)
        np.testing.assert_array_equal(ref, res["err"])
        for opts in FORCED:
            old = {k: eng.get_option(k) for k in opts}
            for k, v in opts.items():
                eng.set_option(k, v)
            np.testing.assert_array_equal(eng.run(T.seed, 0, T.n_rep), ref, err_msg="%s %s" % (gid, opts))
            path = eng.path_info(0)
            assert {"wcontract_valu", "stage_split", "pic_passes"} <= path, (opts, path)
            if "noise_fuse" in opts:
                assert "noise_fused" not in path, path
            for k, v in old.items():
                eng.set_option(k, v)
    finally:
        eng.close()


@pytest.mark.parametrize("gid", ["ofdm12x7_np5", "fbmc12x11_cod_np3"])
def test_bulk_exports(gid):
    """dsce_export, dsce_export_stages and dsce_export_llr of realisations 5..7 on
    frames whose 32-element tiles are partial (NP 5 / 3, LK 84 = 2 x 32 + 20 / 132,
    ND 79 / 126): every field against the oracle's units at the existing helpers'
    bars (y, h 1e-10; LS pilots, diag(D_hat), y_ic 1e-9; decisions equal); the
    demapper input by include/dsce.h from the engine's own stage export at
    1e-12, the LLRs against the host reference on the engine's x_est."""
    from dsce.modulation import llr_awgn
    T, S = geo.geometry_setup(gid)
    sc = S.schemes[T.scheme]
    units = _oracle_units(S, T.scheme, 5, 3, seed=XSEED)
    eng = harness.engine(S, batch=64)
    try:
        e = _export(eng, 0, XSEED, 5, 3)
        st = _stages(eng, 0, XSEED, 5, 3)
        llr = {m: _llr(eng, 0, XSEED, 5, 3, method=m) for m in ("exact", "maxlog")}
    finally:
        eng.close()
    N, LK, NP, ND = geo.dims(gid)
    assert e["y"].shape == (3, 2, LK) and e["hp_ls"].shape == (3, 2, NP) and e["sym"].shape == (3, ND)
    _check_against_units(e, units, range(3))
    assert ((e["sym"] >= 0) & (e["sym"] < sc["symbols"].size)).all()
    np.testing.assert_allclose(np.abs(e["xp"]), 1.0, rtol=0, atol=1e-15)
    _check_against_oracle(st, units, 3, S, T.scheme)
    x, pe, terms = demapper_input(sc, S.pn_time, st["y_ic"], st["h_est"])
    g = llr["exact"]
    assert g["x_est"].shape == (3, 2, 3, ND) and g["llr"].shape == (3, 2, 3, ND, sc["bits_per_symbol"])
    assert (np.abs(g["x_est"] - x) <= 1e-12 * terms).all()
    assert (np.abs(g["pn_eff"] - pe) <= 1e-12 * pe).all() and (g["pn_eff"] > 0).all()
    for method, g in llr.items():
        assert not np.isnan(g["llr"]).any()
        ref = llr_awgn(sc["symbols"], _bitmap(sc["symbols"].size), g["x_est"], g["pn_eff"], method).reshape(g["llr"].shape)
        bar = 1e-12 * (1 + _emax(sc["symbols"], g["x_est"], g["pn_eff"].reshape(-1))).reshape(g["pn_eff"].shape + (1,))
        assert (np.abs(g["llr"] - ref) <= bar).all(), (gid, method)


def test_two_pilot_counts_in_one_context():
    """ofdm12x7_np5 and ofdm12x7_np1 share N and differ in NP: the joint context
    (buffers sized by the larger scheme, one channel and noise draw for both)
    counts like the two single-scheme contexts."""
    (Ta, Sa), (Tb, Sb) = geo.geometry_setup("ofdm12x7_np5"), geo.geometry_setup("ofdm12x7_np1")
    assert Sa.N == Sb.N and np.array_equal(Sa.pn_time, Sb.pn_time)
    single = []
    for T, S in ((Ta, Sa), (Tb, Sb)):
        eng = harness.engine(S, batch=64)
        try:
            single.append(eng.run(geo.SEED, 0, 16)[0])
        finally:
            eng.close()
    np.testing.assert_array_equal(single[0], geo.oracle_counts("ofdm12x7_np5")["err"][0])
    np.testing.assert_array_equal(single[1], geo.oracle_counts("ofdm12x7_np1")["err"][0])
    joint = harness.engine(Sa, batch=64, mmse=False)
    try:
        assert joint.add_scheme(harness._engine_scheme(Sb, "ofdm")) == 1
        joint.build_mmse(Sa.zero_threshold)
        cj = joint.run(geo.SEED, 0, 16)
        assert (joint.scheme_dims(0).n_pilots, joint.scheme_dims(1).n_pilots) == (5, 1)
    finally:
        joint.close()
    np.testing.assert_array_equal(cj[0], single[0])
    np.testing.assert_array_equal(cj[1], single[1])


def test_lds_limit_is_checked_on_the_host():
    """A context whose LDS limit (option lds_max, which only lowers the device's
    hipDeviceAttributeMaxSharedMemoryPerBlock) does not hold the [NP][64] tile of
    k_ls_hest / k_wcontract_valu refuses the scheme with DSCE_EINVAL naming
    n_pilots and the limit, before anything is built or launched; the context
    stays usable.  Between 62 208 B (k_rinv's in-LDS form at NP 36) and the tile's
    36 864 B the scheme is taken and k_rinv works in device memory: the same W."""
    from dsce.engine import DsceError
    T, S = geo.geometry_setup("ofdm24x14_np36")
    mm = harness.oracle_mmse(S, "ofdm")
    eng = harness.engine(S, batch=64)
    try:
        dev = eng.get_option("lds_max")
        assert dev >= 64 * 1024
        with pytest.raises(DsceError, match=r"\(-1\).*lds_max"):
            eng.set_option("lds_max", dev + 1)
        before = eng.run(T.seed, 0, T.n_rep)
        w_lds = [eng.W(0, k, v) for k in range(2) for v in range(2)]
        eng.set_option("lds_max", 32 * 1024)
        with pytest.raises(DsceError, match=r"\(-1\).*n_pilots 36.*limit.*32768"):
            eng.add_scheme(harness._engine_scheme(S, "ofdm"))
        assert eng.scheme_dims(0).n_schemes == 1
        with pytest.raises(DsceError, match=r"\(-1\).*n_pilots 36.*32768"):
            eng.build_mmse(S.zero_threshold)
        np.testing.assert_array_equal(eng.run(T.seed, 0, T.n_rep), before)
        eng.set_option("lds_max", 40 * 1024)                 # the tiles fit, k_rinv's 62 208 B do not
        eng.build_mmse(S.zero_threshold)
        _check_W(eng, mm, 2)
        for i, (k, v) in enumerate((k, v) for k in range(2) for v in range(2)):
            np.testing.assert_array_equal(eng.W(0, k, v), w_lds[i])
        np.testing.assert_array_equal(eng.run(T.seed, 0, T.n_rep), before)
        eng.set_option("lds_max", dev)
    finally:
        eng.close()
