"""GPU parity over the reference script's own parameters: QAM order, power
delay profile, velocity, number of paths and Doppler model (oracle/setup.py
script_setup's keyword parameters).  The engine takes all of them as data
through the C-ABI and selects different compiled kernels for them; every test
here asserts, through dsce_path_info / dsce_jakes_info, which kernel ran, and
compares it with the CPU oracle at the suite's existing tolerances (1e-12 for
the impulse response and the D probe, 1e-10 / 1e-9 for the traces, the
cond-scaled bar of _check_W, identical counts up to 8 x the oracle's borderline
decisions, of which every point here has none).

Jakes instances at the C2 window geometry (14 windows of 24 samples, stride
26; theta = 2 pi fD dt = 4.04e-5 per km/h): of the 9 k_jakes_grp2<MT, 16/NG>
instances the sweep reaches <16,16> <24,16> <28,16> (1 group), <24,8> <28,8>
(2 groups) and <28,4> (4 groups); of the 9 k_jakes_grp<MT, LG> instances
<16,16> <24,16> <28,16>, <28,8> (3 or 4 groups), <24,4> and <28,4> (7 and 5
groups).  Not reachable at this geometry at any velocity, because the widest
run's x = theta span / 2 that two or more groups imply needs more Taylor
terms: k_jakes_grp2<16,8>, <16,4>, <24,4> and k_jakes_grp<16,8>, <24,8>,
<16,4> (with 14 windows two groups appear from 412 km/h, where x is already
1.5: MT 24; four groups from 1169 km/h, x >= 2.3: MT 28).  Of update_jakes_groups'
fall-throughs, `2 groups > windows` is reached (3100 km/h: 14 single-window
groups, the recurrence runs); `no MT with remainder <= 1e-17` cannot happen
(x <= JAKES_XMAX = 3 always admits MT 28: 3^29 / 29! = 7.8e-18); k_jakes_mom is
never an automatic fall-through here (the grouping accepts every velocity at
which its own gate theta 11.5 <= 0.3 holds), so it is reached by option
jakes_mom 1, whose gate then hands over to the recurrence above 645 km/h."""
import math

import numpy as np
import pytest

import harness
from oracle import refsim
from test_gpu_parity import BENCH_BASE, SEED, W_PATH, _check_trace, _check_W, bench_path

pytestmark = pytest.mark.gpu

REPS = (0, 1, 6, 77, 1 << 33)
SNR = [15.0, 35.0]
JAKES_LEN, JAKES_XMAX = 24, 3.0


# ---------------------------------------------------------------------------
# the engine's own selection rule, restated (update_jakes_chunks,
# update_jakes_groups, launch_jakes), so the velocity table below cannot rot
# ---------------------------------------------------------------------------
def _window_chunks(S, name="ofdm"):
    """First samples of the 24-sample chunks covering every sample some Q^H row
    reads; none when they cover more than 90 % of the samples."""
    need = (S.schemes[name]["Q"] != 0).any(axis=1)
    n0, covered, n, N = [], 0, 0, need.size
    while n < N:
        if not need[n]:
            n += 1
            continue
        e = n
        while e < N and need[e]:
            e += 1
        n0 += list(range(n, e, JAKES_LEN))
        covered += -(-(e - n) // JAKES_LEN) * JAKES_LEN
        n = e
    return [] if covered > 0.9 * N else n0


def _groups(n0, th):
    """(ngrp, lg, mt) of the anchor grouping, or None where it declines."""
    L = JAKES_LEN
    if not n0 or not th > 0 or th * 0.5 * (L - 1) > JAKES_XMAX:
        return None

    def runs(smax):
        g, i = [], 0
        while i < len(n0):
            j = i + 1
            while j < len(n0) and n0[j] + L - 1 - n0[i] <= smax:
                j += 1
            g.append((i, j - i))
            i = j
        return g

    hi = int(min(math.floor(2.0 * JAKES_XMAX / th), 1e9))
    g = runs(hi)
    lo = L - 1
    while lo < hi:
        mid = (lo + hi) // 2
        if len(runs(mid)) <= len(g):
            hi = mid
        else:
            lo = mid + 1
    g = runs(hi)
    xmax = max(th * 0.5 * (n0[a + b - 1] + L - 1 - n0[a]) for a, b in g)
    if 2 * len(g) > len(n0):
        return None
    for m in (16, 24, 28):
        b = 1.0
        for k in range(1, m + 2):
            b *= xmax / k
        if b <= 1e-17:
            return len(g), (16 if len(g) <= 2 else 8 if len(g) <= 4 else 4), m
    return None


def _rule(S, opts):
    """What launch_jakes must choose for the windows of setup S under options
    `opts` (the engine's defaults: jakes_mom 2, jakes_grp2 1)."""
    ch = S.chan
    none = dict(grp2=False, ngrp=0, lg=0, mt=0)
    n0 = _window_chunks(S)
    if not n0 or 8 * 4 * ch["paths"] * 8 > 64 * 1024:
        return dict(kernel="full", chunks=0, **none)
    th = 2.0 * math.pi * abs(ch["fD"]) * ch["dt"]
    mom, grp2 = opts.get("jakes_mom", 2), opts.get("jakes_grp2", 1)
    g = _groups(n0, th)
    if mom == 2 and g:
        ngrp, lg, mt = g
        if grp2 and len(ch["idx_taps"]) == 2 and ngrp in (1, 2, 4) and 32 * ch["paths"] * 8 <= 64 * 1024:
            return dict(kernel="win_grp", grp2=True, ngrp=ngrp, lg=16 // ngrp, mt=mt, chunks=len(n0))
        return dict(kernel="win_grp", grp2=False, ngrp=ngrp, lg=lg, mt=mt, chunks=len(n0))
    if mom and th * 11.5 <= 0.3:
        return dict(kernel="win_mom", chunks=len(n0), **none)
    return dict(kernel="win_rec", chunks=len(n0), **none)


def _grp(grp2, ngrp, lg, mt):
    return dict(kernel="win_grp", grp2=bool(grp2), ngrp=ngrp, lg=lg, mt=mt, chunks=14)


def _other(kernel, chunks=14):
    return dict(kernel=kernel, grp2=False, ngrp=0, lg=0, mt=0, chunks=chunks)


def _check_ir(S, opts, expect):
    """channel_impulse_response against refsim.jakes_ir, 1e-12: the run's
    window kernels (realise_win 1: the instance asserted through
    dsce_jakes_info, against the table's entry and the restated rule) and the
    recurrence over every sample (realise_win 0)."""
    ch = S.chan
    assert _rule(S, opts) == expect, (_rule(S, opts), expect)
    ntap = len(ch["idx_taps"])
    eng = harness.engine(S, batch=64, options=opts, mmse=False)
    try:
        ref = {rep: refsim.jakes_ir(SEED, rep, S.N, ch["dt"], ch["pdp_norm"], ch["idx_taps"], ch["fD"], ch["paths"],
                                    ch["model"]) for rep in REPS}
        eng.set_option("realise_win", 1)
        for rep in REPS:
            ir_g = eng.channel_impulse_response(SEED, rep)
            assert eng.jakes_info() == expect, (eng.jakes_info(), expect)
            assert ir_g.shape == ref[rep].shape
            mask = ir_g != 0
            # every tap's window samples: C2 reads 14 windows of 24
            assert mask.sum() >= 14 * 24 * ntap, mask.sum()
            assert not mask[:, [q for q in range(mask.shape[1]) if q not in ch["idx_taps"]]].any()
            np.testing.assert_allclose(ir_g[mask], ref[rep][mask], rtol=0, atol=1e-12, err_msg=str((opts, rep)))
        eng.set_option("realise_win", 0)
        for rep in REPS:
            ir_g = eng.channel_impulse_response(SEED, rep)
            assert eng.jakes_info() == _other("full", 0), eng.jakes_info()
            np.testing.assert_allclose(ir_g, ref[rep], rtol=0, atol=1e-12, err_msg=str((opts, rep)))
    finally:
        eng.close()


# (velocity km/h, options, the instance launch_jakes must run) at C2, VehicularA
# (two taps), 200 paths
VELOCITY_TABLE = [
    (3.0, {}, _grp(1, 1, 16, 16)),                      # walking speed
    (50.0, {}, _grp(1, 1, 16, 16)),
    (250.0, {}, _grp(1, 1, 16, 24)),
    (350.0, {}, _grp(1, 1, 16, 28)),
    (500.0, {}, _grp(1, 2, 8, 24)),                     # the script's point
    (700.0, {}, _grp(1, 2, 8, 28)),
    (1000.0, {}, _grp(0, 3, 8, 28)),                    # 3 groups: k_jakes_grp2 takes 1 / 2 / 4 only
    (1300.0, {}, _grp(1, 4, 4, 28)),
    (1700.0, {}, _grp(0, 5, 4, 28)),                    # 5 groups of <= 3 windows
    (2000.0, {}, _grp(0, 7, 4, 24)),                    # 7 pairs of windows
    (3100.0, {}, _other("win_rec")),                    # 14 single windows: 2 groups > windows, theta 11.5 > 0.3
    (50.0, {"jakes_grp2": 0}, _grp(0, 1, 16, 16)),
    (250.0, {"jakes_grp2": 0}, _grp(0, 1, 16, 24)),
    (700.0, {"jakes_grp2": 0}, _grp(0, 2, 16, 28)),
    (1300.0, {"jakes_grp2": 0}, _grp(0, 4, 8, 28)),
    (3.0, {"jakes_mom": 1}, _other("win_mom")),
    (500.0, {"jakes_mom": 1}, _other("win_mom")),
    (1000.0, {"jakes_mom": 1}, _other("win_rec")),      # k_jakes_mom's own gate: theta 11.5 = 0.46 > 0.3
    (500.0, {"jakes_mom": 0}, _other("win_rec")),
]


@pytest.mark.parametrize("v,opts,expect", VELOCITY_TABLE,
                         ids=["%g-%s" % (v, "-".join("%s%d" % kv for kv in o.items()) or "default")
                              for v, o, _ in VELOCITY_TABLE])
def test_jakes_instances_over_velocity(v, opts, expect):
    """Every Jakes kernel instance the C2 windows can reach (module docstring),
    chosen by velocity, against the oracle's per-sample sum of sinusoids."""
    _check_ir(harness.setup("default", schemes=("ofdm",), snr_db=SNR, velocity_kmh=v), opts, expect)


def test_velocity_table_covers_what_the_rule_can_reach():
    """The table above holds every (kernel, MT, lanes) instance the restated
    rule gives at ANY velocity for the C2 windows (1 .. 7000 km/h in 1 km/h
    steps, with and without k_jakes_grp2), so an instance missing from it is
    unreachable at this geometry, not forgotten."""
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR)
    n0 = _window_chunks(S)
    assert n0 == [90 + 26 * k for k in range(14)]
    reach = set()
    for v in range(1, 7001):
        g = _groups(n0, 2.0 * math.pi * (v / 3.6 * 2.5e9 / 2.998e8) * S.chan["dt"])
        if g:
            ngrp, lg, mt = g
            reach.add((False, lg, mt))
            if ngrp in (1, 2, 4):
                reach.add((True, 16 // ngrp, mt))
    table = {(e["grp2"], e["lg"], e["mt"]) for _, _, e in VELOCITY_TABLE if e["kernel"] == "win_grp"}
    assert reach == table, (sorted(reach - table), sorted(table - reach))
    assert len([t for t in table if t[0]]) == 6 and len([t for t in table if not t[0]]) == 6


@pytest.mark.parametrize("pdp,expect", [("PedestrianA", _grp(0, 2, 16, 24)),        # one tap: k_jakes_grp
                                        ("PedestrianB", _grp(1, 2, 8, 24)),         # two taps: k_jakes_grp2
                                        ("VehicularB", _grp(0, 2, 16, 24))])        # five taps: k_jakes_grp
def test_jakes_over_power_delay_profiles(pdp, expect):
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR, pdp=pdp)
    assert len(S.chan["idx_taps"]) == {"PedestrianA": 1, "PedestrianB": 2, "VehicularB": 5}[pdp]
    _check_ir(S, {}, expect)


@pytest.mark.parametrize("paths,expect", [(1, _grp(1, 2, 8, 24)), (7, _grp(1, 2, 8, 24)), (200, _grp(1, 2, 8, 24)),
                                          (256, _grp(1, 2, 8, 24)),                  # the LDS tables' last fit
                                          (300, _other("full", 0))])                 # they do not fit: every sample
def test_jakes_over_path_counts(paths, expect):
    """Odd and small path counts (the lanes of an anchor split the paths), the
    largest count whose path tables fit the window kernels' LDS (256) and one
    past it, which must run the recurrence over every sample instead."""
    _check_ir(harness.setup("default", schemes=("ofdm",), snr_db=SNR, paths=paths), {}, expect)


@pytest.mark.parametrize("opts,expect", [({}, _grp(1, 2, 8, 24)), ({"jakes_grp2": 0}, _grp(0, 2, 16, 24)),
                                         ({"jakes_mom": 1}, _other("win_mom")), ({"jakes_mom": 0}, _other("win_rec"))])
def test_jakes_uniform_doppler_model(opts, expect):
    """Doppler model 'Uniform' (FastFading.m:229-231): the other angle law in
    each of the window kernels and in the recurrence."""
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR, doppler_model="Uniform")
    assert S.chan["model"] == "Uniform"
    _check_ir(S, opts, expect)


# ---------------------------------------------------------------------------
# Monte-Carlo points: counts of 64 realisations at two SNR points against the
# oracle, one unit traced per element
# ---------------------------------------------------------------------------
_ORACLE = {}


def _oracle_counts(S, name):
    """The oracle's counts of realisations 0..63 (computed once per point).  The
    count bar forgives 8 per borderline decision and is empty where every
    counter is 0, so a point is used only if the oracle flags no borderline
    decision and every counter is above zero."""
    key = (name, tuple(S.variant))
    if key not in _ORACLE:
        _ORACLE[key] = harness.simulate(S, SEED, 0, 64, [name])
    res = _ORACLE[key]
    assert res["borderline"].sum() == 0, res["borderline"]
    assert res["err"].min() > 0, res["err"]
    return res


def _check_counts(eng, res, what="", n=64, seed=SEED):
    """The run's counters of realisations 0..n-1 against the oracle's res of the same range."""
    cg = eng.run(seed, 0, n)
    assert cg.shape == res["err"].shape
    assert np.abs(cg - res["err"]).sum() <= 8 * res["borderline"].sum(), (what, eng.path_info(0), cg - res["err"])
    return eng.path_info(0)


def _check_unit(S, eng, name, rep=3, yperf_rows=None, seed=SEED):
    """One unit (rep 3, both SNR points) per element through _check_trace
    (1e-10 for y and h, 1e-9 per stage); y_perf of the IC iterations on
    `yperf_rows` (the rows the path forms)."""
    tr = {}
    harness.simulate(S, seed, rep, 1, [name], trace=tr)
    for k in range(len(S.pn_time)):
        g = eng.trace_unit(0, seed, rep, k)
        u = tr["units"][k]
        ns = _check_trace(g, u, "%s %s snr %d" % (name, S.variant, k))
        assert ns == S.n_iter + 1
        if yperf_rows is not None:
            for st in range(1, ns):
                np.testing.assert_allclose(g["yperf"][st][yperf_rows], u["yperf"][st][yperf_rows], rtol=0, atol=1e-9)


@pytest.mark.parametrize("qam", [4, 16, 64])
def test_ofdm_constellation_orders(qam):
    """2, 4 and 8 levels per axis through the bench path's byte-grid slicer
    (k_pic_fft / k_mic_data: the 16-stride table mostly unused, the clamp to
    the top level, the folded scale), 6-bit symbols straddling the words of the
    BITS stream at 64-QAM; at 16-QAM also the fused W contraction's slicer."""
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR, qam_order=qam)
    sc = S.schemes["ofdm"]
    assert sc["symbols"].size == qam and sc["bits_per_symbol"] == int(math.log2(qam))
    res = _oracle_counts(S, "ofdm")
    eng = harness.engine(S, batch=64)
    try:
        path = _check_counts(eng, res, "qam %d" % qam)
        assert bench_path(eng) <= path, path
        b = eng.bits_per_rep(0)
        assert b[0] == sc["n_data"] * sc["bits_per_symbol"]
        _check_unit(S, eng, "ofdm", yperf_rows=sc["data_pos"])
        assert bench_path(eng) <= eng.path_info(0), eng.path_info(0)
        if qam == 16:
            eng.set_option("mmse_ic", 0)
            path = _check_counts(eng, res, "qam 16 mmse_ic 0")
            assert W_PATH <= path, path
    finally:
        eng.close()


@pytest.mark.parametrize("qam", [4, 64])
def test_fbmc_constellation_orders(qam):
    """2-PAM and 8-PAM (real_detect, one level on the other axis; 3-bit symbols
    straddle the BITS stream's words) through FBMC's stage kernels."""
    S = harness.setup("default", schemes=("fbmc_aux",), snr_db=SNR, qam_order=qam)
    sc = S.schemes["fbmc_aux"]
    assert sc["symbols"].size == int(math.sqrt(qam)) and np.all(sc["symbols"].imag == 0)
    res = _oracle_counts(S, "fbmc_aux")
    eng = harness.engine(S, batch=64)
    try:
        path = _check_counts(eng, res, "fbmc_aux qam %d" % qam)
        assert {"wrow3", "pic_poly"} <= path and not path & {"pic_fft", "mic_fft", "txrx_fft"}, path
    finally:
        eng.close()


def test_1024_qam_is_rejected_cleanly():
    """The engine's symbol indices and LDS constellation hold at most 256
    symbols.  1024-QAM is turned away at dsce_add_scheme with DSCE_EINVAL before
    anything is built, so no kernel ever sees more than 256 symbols (32 levels on
    an axis do reach the engine, with 32-PAM or 32 x 8: the fallback slicer of
    tests/test_gpu_constellations.py); the context stays usable: the scheme it
    already holds counts exactly as before and on the same kernels."""
    from dsce.engine import DsceError
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR)
    S1024 = harness.setup("default", schemes=("ofdm",), snr_db=SNR, qam_order=1024)
    assert S1024.schemes["ofdm"]["symbols"].size == 1024
    eng = harness.engine(S, batch=64)
    try:
        before = eng.run(SEED, 0, 64)
        path = eng.path_info(0)
        assert {"pic_fft", "mic_stages"} <= path, path
        with pytest.raises(DsceError, match=r"\(-1\).*modulation order"):
            eng.add_scheme(harness._engine_scheme(S1024, "ofdm"))
        assert eng.scheme_dims(0).n_schemes == 1
        np.testing.assert_array_equal(eng.run(SEED, 0, 64), before)
        assert eng.path_info(0) == path
    finally:
        eng.close()


FFT_FORM = {"mic_fft", "mic_stages", "pic_fft", "txrx_fft"}


def _check_lr(eng, path):
    """The structured MMSE IC was kept by its guard; mic_lr only where build_mic
    also kept the low-rank fit (and the option is on)."""
    chk = eng.structured_check(0)
    assert 0.0 <= chk["ratio"] <= 1.0 and "mic_fft" in path, (path, chk)
    if chk["lr"] and eng.get_option("mic_lr"):
        assert "mic_lr" in path, (path, chk)
    else:
        assert "mic_lr" not in path, (path, chk)
    return chk


def test_pedestrian_a_single_tap_instances():
    """PedestrianA collapses to one tap at 360 kHz: the <1, 0> instances of
    k_txrx_fft, k_pic_fft, k_mic_pilot and k_mic_data, and the setup kernels'
    tap loops (k_mcoef, k_rdij, k_bv) with a single tap."""
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR, pdp="PedestrianA")
    assert list(S.chan["idx_taps"]) == [0]
    res = _oracle_counts(S, "ofdm")
    mm = harness.oracle_mmse(S, "ofdm")
    eng = harness.engine(S, batch=64)
    try:
        path = _check_counts(eng, res, "PedestrianA")
        assert FFT_FORM <= path, (path, eng.structured_check(0))
        _check_lr(eng, path)
        rhp, rest, rnoi = eng.correlation(0)
        scale = np.abs(mm["R_hP"]).max()
        np.testing.assert_allclose(rhp, mm["R_hP"], rtol=0, atol=1e-12 * scale)
        np.testing.assert_allclose(rest, mm["R_est"], rtol=0, atol=1e-12 * scale)
        np.testing.assert_allclose(rnoi, mm["R_noI"], rtol=0, atol=1e-12 * scale)
        _check_W(eng, mm, 2)
        _check_unit(S, eng, "ofdm", yperf_rows=S.schemes["ofdm"]["data_pos"])
        assert FFT_FORM <= eng.path_info(0), eng.path_info(0)
    finally:
        eng.close()


def test_pedestrian_b_two_taps_other_power_split():
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR, pdp="PedestrianB")
    assert list(S.chan["idx_taps"]) == [0, 1]
    res = _oracle_counts(S, "ofdm")
    eng = harness.engine(S, batch=64)
    try:
        path = _check_counts(eng, res, "PedestrianB")
        assert bench_path(eng) <= path, (path, eng.structured_check(0))
        _check_unit(S, eng, "ofdm", yperf_rows=S.schemes["ofdm"]["data_pos"])
    finally:
        eng.close()


def test_vehicular_b_five_taps_fall_back():
    """VehicularB: taps at delays 0, 3, 5, 6, 7, longer than the 2-sample cyclic
    prefix, so D = Q'HG is no longer block-diagonal and every FFT-form guard
    must decline (pic_fft_shift, txrx_fft_ok, build_mic): the W contraction
    and the banded perfect-CSI passes run, and match the oracle's literal W."""
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR, pdp="VehicularB")
    ch, sc = S.chan, S.schemes["ofdm"]
    assert list(ch["idx_taps"]) == [0, 3, 5, 6, 7] and S.ofdm.CP == 2
    res = _oracle_counts(S, "ofdm")
    mm = harness.oracle_mmse(S, "ofdm")
    eng = harness.engine(S, batch=64)
    try:
        path = _check_counts(eng, res, "VehicularB")
        assert not path & {"pic_fft", "mic_fft", "mic_stages", "txrx_fft"}, path
        assert path & {"wpair3_fused", "wpair3", "wrow3", "wcontract_valu"}, path
        _check_W(eng, mm, 2)
        # OFDM's precoder is row-local, so the perfect-CSI detection rides on the
        # second banded pass (pfuse), which forms y_perf on the data rows only
        # (NaN elsewhere, include/dsce.h dsce_trace); as separate passes
        # (pfuse 0) y_perf of every row
        _check_unit(S, eng, "ofdm", yperf_rows=sc["data_pos"])
        assert not eng.path_info(0) & {"pic_fft", "mic_fft", "mic_stages", "txrx_fft"}, eng.path_info(0)
        eng.set_option("pfuse", 0)
        _check_unit(S, eng, "ofdm", yperf_rows=np.arange(sc["G"].shape[1]))
        path = eng.path_info(0)
        assert "pic_passes" in path and not path & {"pic_fft", "mic_fft", "mic_stages", "txrx_fft"}, path
        eng.set_option("pfuse", 1)
        rep = 3
        D = eng.transmission_matrix(0, SEED, rep)
        ir = refsim.jakes_ir(SEED, rep, S.N, ch["dt"], ch["pdp_norm"], ch["idx_taps"], ch["fD"], ch["paths"])
        Do = sc["Q"].conj().T @ (refsim.conv_matrix(ir, ch["pdp"], S.N) @ sc["G"])
        scale = np.abs(Do).max()
        np.testing.assert_allclose(D, Do, rtol=0, atol=1e-12 * scale)
        L = S.L                                              # not block-diagonal: energy between symbols
        blk = np.arange(Do.shape[0]) // L
        assert np.abs(Do[blk[:, None] != blk[None, :]]).max() > 1e-3 * scale
    finally:
        eng.close()


def test_every_parameter_off_its_default_at_once():
    """64-QAM, PedestrianA, 50 km/h: one tap, 8 levels per axis, one anchor
    group, cond(R) ~ 7e4 at 35 dB."""
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR, qam_order=64, pdp="PedestrianA", velocity_kmh=50.0)
    res = _oracle_counts(S, "ofdm")
    eng = harness.engine(S, batch=64)
    try:
        path = _check_counts(eng, res, "64-QAM PedestrianA 50 km/h")
        assert FFT_FORM <= path, (path, eng.structured_check(0))
        _check_lr(eng, path)
        assert eng.jakes_info() == _grp(0, 1, 16, 16), eng.jakes_info()
        _check_unit(S, eng, "ofdm", yperf_rows=S.schemes["ofdm"]["data_pos"])
    finally:
        eng.close()


def test_fbmc_single_tap_point():
    """fbmc_aux (16-PAM), PedestrianA, 250 km/h: FBMC's kernels on one tap."""
    S = harness.setup("default", schemes=("fbmc_aux",), snr_db=SNR, pdp="PedestrianA", velocity_kmh=250.0)
    res = _oracle_counts(S, "fbmc_aux")
    eng = harness.engine(S, batch=64)
    try:
        path = _check_counts(eng, res, "fbmc_aux PedestrianA 250 km/h")
        assert {"wrow3", "pic_poly"} <= path, path
    finally:
        eng.close()


@pytest.mark.parametrize("v", [3.0, 50.0])
def test_low_velocity_conditioning(v):
    """3 and 50 km/h: the pilot correlation R is nearly singular in time
    (cond(R_est) 9.5e4 / 7.1e4 at 35 dB against 1.2e3 at 500 km/h), where
    k_rinv's Gauss-Jordan is furthest from the oracle's pinv; _check_W's bar
    scales with cond(R).

    At 3 km/h the script's own 1e-8 threshold on R_Dij (script:263-264),
    amplified by pinv(R), changes W by 2.8e-5 (CPU oracle: max |W(thr 1e-8) -
    W(thr 0)| = 2.77e-5 at 35 dB, 2.9e-7 at 15 dB, against 4.8e-13 at 50 km/h
    and 2.1e-13 at 500 km/h; the engine's dsce_structured_check reports the same
    2.77e-5).  Q' H_hat G reproduces the unthresholded W, so build_mic's
    rounding-level guard must decline there and the W contraction of the
    literal thresholded W must run; at 50 km/h it keeps the structured path.
    Either way the counts, W and every traced stage equal the oracle's."""
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR, velocity_kmh=v)
    res = _oracle_counts(S, "ofdm")
    mm = harness.oracle_mmse(S, "ofdm")
    assert np.linalg.cond(mm["R_est"][1]) > 5e4
    eng = harness.engine(S, batch=64)
    try:
        path = _check_counts(eng, res, "%g km/h" % v)
        chk = eng.structured_check(0)
        if v == 3.0:
            assert chk["ratio"] > 1e2 and 1e-5 < chk["dev"] < 1e-4, chk
            assert {"wpair3_fused", "pic_fft", "txrx_fft"} <= path and not path & {"mic_fft", "mic_stages"}, path
        else:
            assert BENCH_BASE <= path, (path, chk)
            _check_lr(eng, path)
        _check_W(eng, mm, 2)
        _check_unit(S, eng, "ofdm", yperf_rows=S.schemes["ofdm"]["data_pos"])
    finally:
        eng.close()
