"""GPU: the detector and the demapper on every kind of constellation the C-ABI
accepts (tests/constellations.py: rectangular grids with nI != nQ, 1-, 3-, 5-
and 7-bit symbols, non-Gray labellings, grids off the origin, more than 16
levels on an axis), where the rest of the suite hands dsce_add_scheme the
reference script's square Gray QAM / PAM tables only.

Behind that boundary sit three hard slicers (slice from global memory, slice_fast
from LDS tables of 16 levels per axis, the linear byte-grid slice6 of the chain
kernels), two demapper forms and the guards that route a table between them.
Per table: dsce_run's counters against the CPU oracle (exact: the oracle flags
no borderline decision over these realisations), every stage's fields against
the oracle's trace (1e-9; decisions equal), the kernel path that ran, the
engine's hard decisions against the brute-force nearest symbol of its own soft
demapper input on both CSI branches, and the demapper probe against the host
reference (1e-12 (1 + E), test_gpu_llr).  A table with unequally spaced levels is
refused (include/dsce.h at dsce_scheme_desc.symbols): every slicer takes the
cell index from (x - lv[0]) / (lv[1] - lv[0])."""
from types import SimpleNamespace

import numpy as np
import pytest

import harness
from constellations import SNR, TABLES, grid_table, table_setup, with_constellation
from test_gpu_export import _oracle_units
from test_gpu_export_stages import DEC, _check_against_oracle, _stages
from test_gpu_llr import _bitmap, _check_probe, _llr
from test_gpu_parity import SEED, W_PATH, bench_path
from test_gpu_script_params import _check_counts

pytestmark = pytest.mark.gpu

RUNNABLE = [t for t in TABLES if t != "nonuni16"]
FAST_ONLY = {"pic_fft", "mic_stages", "stage_fused"}         # kernels with 16-level LDS tables / the byte grid
_COUNTS = {}


@pytest.fixture(scope="module", params=RUNNABLE)
def ctx(request):
    """Per table: its setup (the table's scheme alone, SNR (15, 35) dB) and one
    engine at batch 64 with the default options, shared by the table's tests."""
    T, S = table_setup(request.param)
    eng = harness.engine(S, batch=64)
    yield SimpleNamespace(id=request.param, T=T, S=S, eng=eng, name=T.scheme, sc=S.schemes[T.scheme])
    eng.close()


def _oracle_counts(tid, T, S):
    """The oracle's counts of realisations 0..n_rep-1 (once per table).  The count
    bar is 8 per borderline decision: none is flagged, so the comparison is exact;
    every counter is above zero, except bpsk's at 35 dB."""
    if tid not in _COUNTS:
        _COUNTS[tid] = harness.simulate(S, SEED, 0, T.n_rep, [T.scheme])
    res = _COUNTS[tid]
    assert res["borderline"].sum() == 0, res["borderline"]
    if tid == "bpsk":
        assert res["err"].sum() > 0, res["err"]
    else:
        assert res["err"].min() > 0, res["err"]
    return res


def _check_default_path(T, path, eng):
    if not T.wide:
        assert T.scheme == "ofdm" and bench_path(eng) <= path, path
    else:
        # launch_stage reports stage_split for k_ls_hest + k_detect (global-memory slicer) + k_precode;
        # launch_perfect_ic pic_poly or pic_passes
        assert not path & FAST_ONLY and "stage_split" in path and path & {"pic_poly", "pic_passes"}, path


def test_counts_and_path(ctx):
    """dsce_run over realisations 0..n_rep-1 equals refsim.simulate of the same
    table to the bit, on the path the table's grid selects: the bench path for up
    to 16 levels per axis, the split stage kernels and the polyphase / banded
    perfect-CSI passes beyond."""
    T, eng = ctx.T, ctx.eng
    res = _oracle_counts(ctx.id, T, ctx.S)
    path = _check_counts(eng, res, ctx.id, n=T.n_rep)
    print("constellation %-12s path %s" % (ctx.id, ",".join(sorted(path))))
    _check_default_path(T, path, eng)
    bits = eng.bits_per_rep(0)
    assert bits[0] == ctx.sc["n_data"] * T.m
    assert eng.scheme_dims(0).n_iter == T.n_iter


def test_stages_match_oracle(ctx):
    """Every stage's hp_ls, h_est, y_ic (1e-9), dec_est and dec_perf (equal) of 2
    realisations against the oracle's trace: the grid -> symbol maps and the
    re-precoding of the decided symbols in every IC iteration."""
    e = _stages(ctx.eng, 0, SEED, 0, 2)
    _check_against_oracle(e, _oracle_units(ctx.S, ctx.name, 0, 2, seed=SEED), 2, ctx.S, ctx.name)


OPTION_SETS = {
    # slice_fast in the epilogue of k_wpair3, beside k_pic_fft
    "mmse_ic0": ({"mmse_ic": 0}, lambda p: W_PATH <= p and "mic_stages" not in p),
    # the unfused contraction + k_ls + k_stage_fused
    "mmse_ic0-fuse_stage0": ({"mmse_ic": 0, "fuse_stage": 0},
                             lambda p: {"stage_fused", "pic_fft"} <= p and p & {"wpair3", "wrow3"} and
                             not p & {"wpair3_fused", "mic_stages"}),
    # k_ls_hest + k_detect (LDS slicer) + k_precode
    "stage_split1": ({"stage_split": 1}, lambda p: "stage_split" in p and not p & {"stage_fused", "mic_stages"}),
    # the fused perfect-CSI pass of every iteration instead of the chain kernel
    "pic_chain0": ({"pic_chain": 0}, lambda p: p & {"pic_poly", "pic_passes"} and
                   not p & {"pic_fft", "mic_stages", "pic_chain", "pic_mfma"}),
}


@pytest.mark.parametrize("tid", ["rect32", "rect128b", "perm64", "offset16"])
@pytest.mark.parametrize("opts", list(OPTION_SETS))
def test_each_slicer_in_place(tid, opts):
    """The counts of test_counts_and_path again with the options that put each
    LDS-table slicer into the run, and the path of each."""
    options, path_ok = OPTION_SETS[opts]
    T, S = table_setup(tid)
    res = _oracle_counts(tid, T, S)
    eng = harness.engine(S, batch=64, options=options)
    try:
        path = _check_counts(eng, res, "%s %s" % (tid, options), n=T.n_rep)
        assert path_ok(path), (tid, options, path)
    finally:
        eng.close()


@pytest.mark.parametrize("tid", ["rect32", "rect128b"])
def test_symbol_draw_of_the_other_tx_kernel(tid):
    """5- and 7-bit symbols cross the words of the BITS stream at offsets 3 and 6
    bits never produce.  The default run draws them row-parallel (k_tx_rows);
    option tx_rows 0 draws them in k_tx_symbols: the same counts, the same path."""
    T, S = table_setup(tid)
    res = _oracle_counts(tid, T, S)
    eng = harness.engine(S, batch=64, options={"tx_rows": 0})
    try:
        assert eng.get_option("tx_rows") == 0
        path = _check_counts(eng, res, "%s tx_rows 0" % tid, n=T.n_rep)
        assert bench_path(eng) <= path, path
    finally:
        eng.close()


def test_hard_decisions_are_the_nearest_symbol_of_the_soft_input(ctx):
    """Both CSI branches, 3 realisations, every SNR point and stage: the
    brute-force argmin_i |x_est - s_i| (first index on ties) of export_llr's
    x_est is export_stages' decision at every entry whose nearest and
    second-nearest distances differ by at least 1e-9 (at most 0.1 % may not; the
    oracle flags none, the share is printed), and the sign of the max-log LLR
    gives that decision's bits: hard and soft outputs of one call agree."""
    from dsce import engine
    eng, sym, m = ctx.eng, ctx.sc["symbols"], ctx.T.m
    dec = _stages(eng, 0, SEED, 0, 3, fields=DEC)
    for branch, f in (("mmse", "dec_est"), ("perfect", "dec_perf")):
        g = _llr(eng, 0, SEED, 0, 3, method="maxlog", flags=engine.LLR_MAXLOG | engine.LLR_BRANCHES[branch])
        x = g["x_est"]
        assert x.shape == dec[f].shape and g["llr"].shape == x.shape + (m,) and not np.isnan(x).any()
        if ctx.sc["real_detect"]:
            assert not x.imag.any()
        d = np.abs(x[..., None] - sym)
        near = d.argmin(axis=-1)
        two = np.partition(d, 1, axis=-1)[..., :2]
        safe = two[..., 1] - two[..., 0] >= 1e-9
        share = 1.0 - safe.mean()
        print("constellation %-12s %-7s entries under the 1e-9 gap: %.3e" % (ctx.id, branch, share))
        assert share <= 1e-3, (ctx.id, branch, share)
        bad = safe & (near != dec[f])
        assert not bad.any(), (ctx.id, branch, int(bad.sum()), np.argwhere(bad)[:4], near[bad][:4], dec[f][bad][:4])
        bits = ((near[..., None] >> np.arange(m)) & 1).astype(bool)
        assert np.array_equal((g["llr"] > 0)[safe], bits[safe]), (ctx.id, branch)


def test_demapper_probe(ctx):
    """dsce_llr_awgn of the table against the host reference, in the form the
    labelling and the grid select: per axis for the unpermuted tables with up to
    16 levels per axis, the full table otherwise (at M = 256 too)."""
    T, eng, sym = ctx.T, ctx.eng, ctx.sc["symbols"]
    assert eng.llr_info(0) == dict(per_axis=T.perm is None and not T.wide, m=T.m)
    _check_probe(eng, 0, sym, ctx.id)
    assert np.isnan(eng.llr_awgn(0, [np.nan, 0.1], [1.0, np.nan])).all()
    assert np.isnan(eng.llr_awgn(0, [np.nan, 0.1], [1.0, np.nan], "maxlog")).all()


def test_unequal_spacing_is_rejected_cleanly():
    """Levels {-7, -1, 1, 3} x {-3, -1, 1, 7}: the slicers would pick the wrong
    level on a fifth of the plane while the demapper, which reads the level table
    itself, would not.  dsce_add_scheme refuses the table with DSCE_EINVAL naming
    the axis (the I axis first, the Q axis when only that one is unequal), and a
    non-finite symbol likewise; the context stays usable: the scheme it already
    holds counts exactly as before and on the same kernels."""
    from dsce.engine import DsceError
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR)
    T = TABLES["nonuni16"]
    bad = [("I axis", with_constellation(S, "ofdm", grid_table(T.lvI, T.lvQ))),
           ("Q axis", with_constellation(S, "ofdm", grid_table([-3.0, -1.0, 1.0, 3.0], T.lvQ)))]
    for v in (complex(np.nan, 0.5), complex(0.5, np.inf)):
        sym = S.schemes["ofdm"]["symbols"].copy()
        sym[3] = v
        bad.append(("not finite", SimpleNamespace(**dict(vars(S), schemes={"ofdm": dict(S.schemes["ofdm"], symbols=sym)}))))
    eng = harness.engine(S, batch=64)
    try:
        before = eng.run(SEED, 0, 64)
        path = eng.path_info(0)
        assert bench_path(eng) <= path and before.sum() > 0, path
        for what, S2 in bad:
            with pytest.raises(DsceError, match=r"\(-1\).*" + what):
                eng.add_scheme(harness._engine_scheme(S2, "ofdm"))
            assert eng.scheme_dims(0).n_schemes == 1
        np.testing.assert_array_equal(eng.run(SEED, 0, 64), before)
        assert eng.path_info(0) == path
        # an equally spaced table is still taken, next to the first scheme
        _, S3 = table_setup("offset16")
        assert eng.add_scheme(harness._engine_scheme(S3, "ofdm")) == 1 and eng.scheme_dims(0).n_schemes == 2
    finally:
        eng.close()
