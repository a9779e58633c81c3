"""GPU: the bulk per-stage export (dsce_export_stages / k_export_stages, ABI 10)
against the CPU oracle's per-unit trace on the same Philox streams, against the
engine's own single-unit trace (dsce_trace_unit_ex), against dsce_run's counters
and MSE sums (closed loops: the run launches the kernel instances without a
trace), against dsce_export's stage 0, and against itself across batch
geometries, SNR chunks, staging bounds, precisions and destinations.

Bars (tests/test_gpu_parity.py::_check_trace, tests/test_gpu_export.py): the LS
pilot estimates, diag(D_hat) and y_ic 1e-9 per stage against the oracle and the
trace; decisions equal unless the oracle's nearest-point margin is below 1e-9;
counts exact; MSE sums rtol 1e-9; an export against itself 1e-12 (decisions
exact).  Every host export in this file goes through _stages, which surrounds
each array with guard bytes and checks them."""
import os
import subprocess
import sys

import numpy as np
import pytest

import harness
from test_gpu_export import EINVAL, ESTATE, GUARD, PATTERN, SEED, SNR, _export, _oracle_units

pytestmark = pytest.mark.gpu

ALL = ("hp_ls", "h_est", "y_ic", "dec_est", "dec_perf")
CPLX = ("hp_ls", "h_est", "y_ic")
DEC = ("dec_est", "dec_perf")
FFT_PATH = {"mic_stages", "mic_lr", "pic_fft"}


def _stages(eng, sid, seed, first, n, fields=ALL, dtype=np.complex128, flags=None):
    """eng.export_stages into arrays that sit between two guard regions of GUARD
    bytes each; asserts that the export wrote neither."""
    from dsce import engine
    dt = np.dtype(dtype)
    shapes = eng.export_stages_shapes(sid, n)
    raw, out = {}, {}
    for f in fields:
        fdt = np.dtype(np.int32) if f in DEC else dt
        nb = int(np.prod(shapes[f])) * fdt.itemsize
        raw[f] = np.full(nb + 2 * GUARD, PATTERN, dtype=np.uint8)
        out[f] = raw[f][GUARD:GUARD + nb].view(fdt).reshape(shapes[f])
    if flags is None:
        flags = engine.EXPORT_F32 if dt == np.dtype(np.complex64) else 0
    eng._export_stages(sid, seed, first, n, flags, {f: raw[f].ctypes.data + GUARD for f in fields})
    for f in fields:
        assert (raw[f][:GUARD] == PATTERN).all(), "bytes before %s were written" % f
        assert (raw[f][-GUARD:] == PATTERN).all(), "bytes past %s were written" % f
    return out


def _same(a, b, atol=1e-12, rows=None):
    """Two exports of the same realisations: complex fields at atol, decisions exact."""
    for f in a:
        x, y = (a[f], b[f]) if rows is None else (a[f][rows], b[f][rows])
        if f in DEC:
            assert np.array_equal(x, y), f
        else:
            np.testing.assert_allclose(x, y, rtol=0, atol=atol, err_msg=f)


@pytest.fixture(scope="module")
def ofdm():
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR)
    eng = harness.engine(S, batch=64)
    yield S, eng
    eng.close()


@pytest.fixture(scope="module")
def ofdm_ref(ofdm):
    """One export of 129 realisations from first_rep 5 at batch 64, shared (read-only)."""
    S, eng = ofdm
    eng.set_batch(64)
    return _stages(eng, 0, SEED, 5, 129)


@pytest.fixture(scope="module")
def ofdm_counts(ofdm):
    S, eng = ofdm
    eng.set_batch(64)
    return eng.run(SEED, 0, 64)


def _check_against_oracle(e, units, n, S, name):
    sc = S.schemes[name]
    ns, LK, NP, ND = S.n_iter + 1, sc["G"].shape[1], len(sc["pilot_pos"]), sc["n_data"]
    nk = len(S.pn_time)
    assert e["hp_ls"].shape == (n, nk, ns, NP) and e["h_est"].shape == (n, nk, ns, LK)
    assert e["y_ic"].shape == (n, nk, ns, LK)
    assert e["dec_est"].shape == (n, nk, ns, ND) and e["dec_perf"].shape == (n, nk, ns, ND)
    for f in CPLX:
        assert e[f].dtype == np.complex128 and not np.isnan(e[f]).any(), f
    for f in DEC:
        assert e[f].dtype == np.int32 and (e[f] >= 0).all(), f
    for i in range(n):
        for k, u in enumerate(units[i]):
            for st in range(ns):
                tag = "%s row %d snr %d stage %d" % (name, i, k, st)
                np.testing.assert_allclose(e["hp_ls"][i, k, st], u["hp"][st], rtol=0, atol=1e-9, err_msg=tag)
                np.testing.assert_allclose(e["h_est"][i, k, st], u["hest"][st], rtol=0, atol=1e-9, err_msg=tag)
                np.testing.assert_allclose(e["y_ic"][i, k, st], u["yest"][st], rtol=0, atol=1e-9, err_msg=tag)
                for f, key, mk in (("dec_est", "dec_e", "margin_e"), ("dec_perf", "dec_p", "margin_p")):
                    ok = (e[f][i, k, st] == u[key][st]) | (u[mk][st] < 1e-9)
                    assert ok.all(), (tag, f, np.flatnonzero(~ok)[:8])


def test_stages_match_oracle_ofdm(ofdm):
    """Default OFDM, n_iter 4, 3 realisations from first_rep 5, both SNR points:
    every field of every stage against refsim.simulate's per-unit trace, on the
    FFT-form path of dsce_run (asserted through path_info of a run)."""
    S, eng = ofdm
    eng.set_batch(64)
    e = _stages(eng, 0, SEED, 5, 3)
    _check_against_oracle(e, _oracle_units(S, "ofdm", 5, 3), 3, S, "ofdm")
    eng.run(SEED, 0, 64)
    assert FFT_PATH <= eng.path_info(0), eng.path_info(0)


def test_stages_match_oracle_fbmc():
    """FBMC with auxiliary symbols: the W contraction, k_ls + k_stage_fused and
    the polyphase perfect-CSI passes; 2 realisations, n_iter 2 (stage 2 uses W0:
    the W / W0 switch is crossed)."""
    S = harness.setup("default", schemes=("fbmc_aux",), snr_db=SNR, n_iter=2)
    eng = harness.engine(S, batch=64)
    try:
        e = _stages(eng, 0, SEED, 5, 2)
        eng.run(SEED, 0, 64)
        path = eng.path_info(0)
    finally:
        eng.close()
    _check_against_oracle(e, _oracle_units(S, "fbmc_aux", 5, 2), 2, S, "fbmc_aux")
    assert {"stage_fused", "pic_poly"} <= path and path & {"wrow3", "wpair3"}, path


def test_stages_match_engine_trace(ofdm):
    """70 realisations from first_rep 5 at batch 128 (two waves, the second
    ragged) against dsce_trace_unit_ex of the same units: rows 0, 58, 69 and the
    wave boundary (63 / 64), every SNR point and stage."""
    S, eng = ofdm
    eng.set_batch(128)
    e = _stages(eng, 0, SEED, 5, 70)
    for i in (0, 58, 63, 64, 69):
        for k in range(len(SNR)):
            g = eng.trace_unit(0, SEED, 5 + i, k)
            tag = "row %d snr %d" % (i, k)
            np.testing.assert_allclose(e["hp_ls"][i, k], g["hp"], rtol=0, atol=1e-9, err_msg=tag)
            np.testing.assert_allclose(e["h_est"][i, k], g["hest"], rtol=0, atol=1e-9, err_msg=tag)
            np.testing.assert_allclose(e["y_ic"][i, k], g["yest"], rtol=0, atol=1e-9, err_msg=tag)
            for f, key in (("dec_est", "dec_e"), ("dec_perf", "dec_p")):
                m = g[key] >= 0
                assert m.any() and np.array_equal(e[f][i, k][m], g[key][m]), (tag, f)


@pytest.mark.parametrize("options", [
    {"mmse_ic": 0},                                       # k_pilot_pre + k_wpair3 epilogue, k_pic_fft without stage 0
    {"mmse_ic": 0, "fuse_stage": 0},                      # unfused k_wpair3 + k_ls + k_stage_fused
    {"mmse_ic": 0, "fuse_stage": 0, "stage_split": 1},    # k_ls_hest + k_detect + k_precode
    {"mmse_ic": 0, "pic_chain": 0, "pic_poly": 0},        # the banded perfect-CSI passes (k_band)
], ids=lambda o: "-".join("%s%d" % kv for kv in o.items()))
def test_stages_follow_the_options(options):
    """The export takes the kernel path the context's options select: OFDM off
    the FFT-form MMSE path, n_iter 2, 65 realisations; rows 0 and 64 against
    dsce_trace_unit_ex under the same options.  Entries the path does not form
    are NaN / -1 in both and at the same places."""
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR, n_iter=2)
    eng = harness.engine(S, batch=64, options=options)
    try:
        e = _stages(eng, 0, SEED, 5, 65)
        for i in (0, 64):
            for k in range(len(SNR)):
                g = eng.trace_unit(0, SEED, 5 + i, k)
                assert "mic_stages" not in eng.path_info(0)
                tag = "%s row %d snr %d" % (options, i, k)
                for f, key in (("hp_ls", "hp"), ("h_est", "hest"), ("y_ic", "yest")):
                    nan = np.isnan(g[key])
                    assert np.array_equal(np.isnan(e[f][i, k]), nan) and not nan.all(), (tag, f)
                    np.testing.assert_allclose(e[f][i, k][~nan], g[key][~nan], rtol=0, atol=1e-9, err_msg=tag)
                for f, key in (("dec_est", "dec_e"), ("dec_perf", "dec_p")):
                    assert np.array_equal(e[f][i, k], g[key]) and (g[key] >= 0).any(), (tag, f)
    finally:
        eng.close()


def test_recount_of_exported_decisions_equals_the_run(ofdm):
    """Closed loop: the bit errors of the exported decisions against the
    exported transmitted symbols are dsce_run's counters of the same range,
    exactly, both CSI branches and both edge classes (edge 1 = the scheme's
    considered flags).  The run launches the kernel instances without a trace.
    Realisations 3..72: refsim.simulate's borderline count over this range at
    these SNR points is 0 (checked on the CPU when this test was written), so no
    decision hangs on the last bits of its slicer input."""
    from dsce import dataset
    S, eng = ofdm
    eng.set_batch(64)
    counts = eng.run(SEED, 3, 70)
    sym = _export(eng, 0, SEED, 3, 70, fields=("sym",))["sym"]
    e = _stages(eng, 0, SEED, 3, 70, fields=DEC)
    cons = S.schemes["ofdm"]["considered"]
    assert counts.shape == (1, 2, 2, len(SNR), S.n_iter + 1) and counts.min() > 0
    for csi, f in enumerate(DEC):
        assert np.array_equal(dataset.bit_errors(sym, e[f]), counts[0, csi, 0]), f
        assert np.array_equal(dataset.bit_errors(sym, e[f], considered=cons), counts[0, csi, 1]), f


def test_mse_of_exported_estimates_equals_the_run(ofdm):
    """Closed loop: sum |h_est - h|^2 of the exported estimates is dsce_run's MSE
    sum of the same range per (SNR, stage), and sum |h|^2 its power sum, at the
    bar test_gpu_parity.py holds those sums to against the oracle (rtol 1e-9)."""
    S, eng = ofdm
    eng.set_batch(64)
    eng.enable_mse(True)
    try:
        eng.run(SEED, 3, 70)
        err, pw = eng.mse()
    finally:
        eng.enable_mse(False)
    h = _export(eng, 0, SEED, 3, 70, fields=("h",))["h"]
    he = _stages(eng, 0, SEED, 3, 70, fields=("h_est",))["h_est"]
    got = (np.abs(he - h[:, None, None, :]) ** 2).sum(axis=(0, 3))
    assert err.shape == (1, len(SNR), S.n_iter + 1) and err.min() > 0
    np.testing.assert_allclose(got, err[0], rtol=1e-9, atol=0)
    np.testing.assert_allclose(np.full(len(SNR), (np.abs(h) ** 2).sum()), pw[0], rtol=1e-9, atol=0)


@pytest.mark.parametrize("n_rep", [1, 64, 65, 129])
def test_stages_batch_geometries(ofdm, ofdm_ref, n_rep):
    """Batch 64: one ragged wave, one full batch, a batch and one realisation,
    three batches with a last one of a single realisation; every row equals an
    export of that realisation alone."""
    S, eng = ofdm
    eng.set_batch(64)
    e = ofdm_ref if n_rep == 129 else _stages(eng, 0, SEED, 5, n_rep)
    assert e["y_ic"].shape[0] == n_rep
    for i in range(n_rep):
        _same({f: e[f][i:i + 1] for f in ALL}, _stages(eng, 0, SEED, 5 + i, 1))


def test_stages_snr_chunks():
    """Option snr_chunk = 1 with three SNR points equals the unchunked export."""
    S = harness.setup("default", schemes=("ofdm",), snr_db=(10.0, 20.0, 35.0), n_iter=2)
    eng = harness.engine(S, batch=64, options={"snr_chunk": 1})
    whole = harness.engine(S, batch=64)
    try:
        e = _stages(eng, 0, SEED, 5, 65)
        assert e["y_ic"].shape == (65, 3, 3, 336)
        _same(e, _stages(whole, 0, SEED, 5, 65))
    finally:
        eng.close()
        whole.close()


def test_stages_staging_bound_cuts_the_batch(ofdm, ofdm_ref):
    """Option export_stage_mb 12 at batch 128: a unit's bulk arrays are 5 (16 +
    2 336) 16 + 5 2 320 4 = 67840 B, so two SNR points x 128 realisations need
    16.6 MiB and the batch is cut into sub-batches of one wave (8.3 MiB); the
    result equals the uncut export of the same batch and the batch-64 export."""
    S, eng = ofdm
    eng.set_batch(128)
    try:
        whole = _stages(eng, 0, SEED, 5, 129)
        eng.set_option("export_stage_mb", 12)
        assert eng.get_option("export_stage_mb") == 12
        cut = _stages(eng, 0, SEED, 5, 129)
    finally:
        eng.set_option("export_stage_mb", 1024)
        eng.set_batch(64)
    _same(cut, whole)
    _same(cut, ofdm_ref)


def test_stage0_agrees_with_dsce_export(ofdm, ofdm_ref):
    """Stage 0 of the per-stage export against dsce_export of the same range:
    y_ic is y exactly (a copy), the LS pilot estimates and diag(D_hat) come from
    other kernels with the same operations in the same order (1e-12)."""
    S, eng = ofdm
    eng.set_batch(64)
    e = _export(eng, 0, SEED, 5, 129, fields=("y", "hp_ls", "h_est"))
    assert np.array_equal(ofdm_ref["y_ic"][:, :, 0], e["y"])
    np.testing.assert_allclose(ofdm_ref["hp_ls"][:, :, 0], e["hp_ls"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(ofdm_ref["h_est"][:, :, 0], e["h_est"], rtol=0, atol=1e-12)


def test_stages_fp32_is_the_rounded_fp64_export(ofdm, ofdm_ref):
    """DSCE_EXPORT_F32 rounds each fp64 value once, at the store."""
    S, eng = ofdm
    eng.set_batch(64)
    e32 = _stages(eng, 0, SEED, 5, 129, dtype=np.complex64)
    for f in CPLX:
        assert e32[f].dtype == np.complex64
        assert np.array_equal(e32[f], ofdm_ref[f].astype(np.complex64)), f
    for f in DEC:
        assert np.array_equal(e32[f], ofdm_ref[f]), f


_TORCH_CHILD = r"""
import sys
import torch                       # before the engine: both then share torch's HIP runtime
import numpy as np
sys.path[:0] = [%(tests)r, %(pkg)r, %(root)r]
import harness
S = harness.setup("default", schemes=("ofdm",), snr_db=%(snr)r, n_iter=2)
eng = harness.engine(S, batch=64)
for name in ("complex128", "complex64"):
    dt = getattr(torch, name)
    ref = eng.export_stages(0, %(seed)d, 5, 129, dtype=np.dtype(name))
    t = eng.export_stages_torch(0, %(seed)d, 5, 129, dtype=dt)
    for f in ref:
        assert t[f].is_cuda and t[f].dtype == (torch.int32 if f.startswith("dec") else dt), (name, f)
        assert t[f].shape == ref[f].shape and np.array_equal(t[f].cpu().numpy(), ref[f]), (name, f)
    assert np.abs(ref["y_ic"]).max() > 0 and (ref["dec_est"] >= 0).all()
# a host pointer is refused with the device flag, and the context still exports
try:
    eng._export_stages(0, %(seed)d, 5, 3, 2, {"y_ic": np.zeros(3 * 2 * 3 * 336, dtype=np.complex128).ctypes.data})
    raise SystemExit("host pointer accepted as device memory")
except Exception as e:
    assert "(-1)" in str(e), e
assert np.array_equal(eng.export_stages(0, %(seed)d, 5, 3)["dec_est"], ref["dec_est"][:3])
eng.close()
print("EXPORT_STAGES_TORCH_OK")
"""


def test_stages_torch_equals_host_export():
    """DSCE_EXPORT_DEVICE: the kernel writes torch's tensors directly, and they
    equal the host export exactly, for both dtypes; a host pointer with the
    device flag is DSCE_EINVAL.  A child process, because torch has to be
    imported before the engine's library is loaded (Engine.export_torch)."""
    code = _TORCH_CHILD % dict(tests=os.path.join(harness.ROOT, "tests"), pkg=harness.PKG, root=harness.ROOT,
                               snr=SNR, seed=SEED)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "EXPORT_STAGES_TORCH_OK" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])


def test_stages_have_no_side_effects(ofdm):
    """Counts, MSE sums and path_info of a run are the same with and without an
    export_stages before it (the IC kernels of the export add into scratch
    counters and no MSE sums); the MSE totals right after the export are exactly
    zero.  MSE sums of two runs at rtol 1e-12: the reordering bound of their
    atomic adds (tests/test_gpu_export.py::test_export_has_no_side_effects)."""
    S, eng = ofdm
    eng.set_batch(64)
    eng.enable_mse(True)
    try:
        c1 = eng.run(SEED, 0, 128)
        e1, p1 = eng.mse()
        path = eng.path_info(0)
        eng.enable_mse(True)                       # reset the sums
        _stages(eng, 0, SEED, 3, 70)
        assert eng.path_info(0) == path
        e_mid, p_mid = eng.mse()
        assert not e_mid.any() and not p_mid.any()
        c2 = eng.run(SEED, 0, 128)
        e2, p2 = eng.mse()
        assert eng.path_info(0) == path
    finally:
        eng.enable_mse(False)
    assert np.array_equal(c1, c2) and c1.sum() > 0
    assert e1.min() > 0 and p1.min() > 0
    np.testing.assert_allclose(e2, e1, rtol=1e-12, atol=0)
    np.testing.assert_allclose(p2, p1, rtol=1e-12, atol=0)


def test_stages_errors_leave_the_context_usable(ofdm, ofdm_counts):
    from dsce import engine
    S, eng = ofdm
    eng.set_batch(64)

    def fails(code, *a, **k):
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % code):
            _stages(eng, *a, **k)
        assert np.array_equal(eng.run(SEED, 0, 64), ofdm_counts)

    fails(EINVAL, 0, SEED, 5, 3, fields=())                                   # every field null
    fails(EINVAL, 0, SEED, 5, 3, flags=1 << 2)                                # unknown flag
    fails(EINVAL, 0, SEED, 5, 3, flags=engine.EXPORT_DEVICE)                  # host pointers as device memory
    with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL):           # null out
        eng._chk(eng.lib.dsce_export_stages(eng.h, 0, SEED, 5, 3, 0, None), "dsce_export_stages")
    assert np.array_equal(eng.run(SEED, 0, 64), ofdm_counts)
    z = _stages(eng, 0, SEED, 5, 0)                                           # n_rep = 0: OK, nothing written
    assert all(z[f].shape[0] == 0 for f in ALL)
    assert np.array_equal(eng.run(SEED, 0, 64), ofdm_counts)
    # without dsce_build_mmse; after it the same context runs and exports
    bare = harness.engine(S, batch=64, mmse=False)
    try:
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % ESTATE):
            _stages(bare, 0, SEED, 5, 3)
        bare.build_mmse(S.zero_threshold)
        assert np.array_equal(bare.run(SEED, 0, 64), ofdm_counts)
        assert (_stages(bare, 0, SEED, 5, 3, fields=DEC)["dec_est"] >= 0).all()
    finally:
        bare.close()
    # before channel, SNR points or scheme are set
    empty = engine.Engine(0)
    try:
        buf = np.zeros(8)
        rc = empty.lib.dsce_export_stages(empty.h, 0, SEED, 0, 1, 0, engine.ExportStagesOut(y_ic=buf.ctypes.data))
        assert rc == ESTATE
    finally:
        empty.close()


def test_stages_interpolation_scheme_without_iterations():
    """An interpolation scheme with n_iter 0 needs no dsce_build_mmse: S = 1, and
    the stage is dsce_export's; with n_iter > 0 the export is DSCE_ESTATE."""
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
                e = _stages(eng, sid, SEED, 5, 65)
                x = _export(eng, sid, SEED, 5, 65, fields=("y", "hp_ls", "h_est"))
            else:
                with pytest.raises(DsceError, match=r"\(%d\)" % ESTATE):
                    _stages(eng, sid, SEED, 5, 3)
        finally:
            eng.close()
    assert e["y_ic"].shape == (65, 2, 1, sc.LK) and (e["dec_est"] >= 0).all() and (e["dec_perf"] >= 0).all()
    assert np.array_equal(e["y_ic"][:, :, 0], x["y"])
    np.testing.assert_allclose(e["hp_ls"][:, :, 0], x["hp_ls"], rtol=0, atol=1e-12 * np.abs(x["hp_ls"]).max())
    np.testing.assert_allclose(e["h_est"][:, :, 0], x["h_est"], rtol=0, atol=1e-12 * np.abs(x["h_est"]).max())


def test_dataset_tool_writes_stage_arrays(tmp_path):
    """python -m dsce.dataset --stages in a child process: 96 realisations in
    shards of 64 (two files); load() of them equals one Engine.export plus one
    Engine.export_stages, and the metadata carries n_iter."""
    from dsce import dataset
    from dsce.configs import build_setup
    from dsce.engine import ABI_VERSION, build_engine, gpu_tx
    prefix = str(tmp_path / "data" / "ofdm")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([harness.PKG] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    p = subprocess.run([sys.executable, "-m", "dsce.dataset", "--config", "default", "--scheme", "ofdm", "--snr-db", "10",
                        "35", "--seed", str(SEED), "--first-rep", "5", "--reps", "96", "--shard-reps", "64", "--dtype",
                        "complex64", "--stages", "--n-iter", "2", "--out", prefix],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / "data")) == ["ofdm-00000.npz", "ofdm-00001.npz"]
    arrays, meta = dataset.load(prefix)
    S = build_setup("default", schemes=("ofdm",), snr_db=list(SNR), n_iter=2, tx=gpu_tx(0))
    eng = build_engine(S, batch=64)                 # the shards' batch geometry: 64 + 32 realisations
    try:
        e = eng.export(0, SEED, 5, 96, dtype=np.complex64)
        st = eng.export_stages(0, SEED, 5, 96, dtype=np.complex64)
    finally:
        eng.close()
    assert sorted(arrays) == sorted(list(e) + list(dataset.STAGE_ARRAYS))
    for f in e:
        assert arrays[f].dtype == e[f].dtype and np.array_equal(arrays[f], e[f]), f
    for f, name in dataset.STAGE_NAMES.items():
        assert arrays[name].dtype == st[f].dtype and np.array_equal(arrays[name], st[f]), f
    assert arrays["dec_est"].shape == (96, 2, 3, 320) and arrays["y_ic_stages"].shape == (96, 2, 3, 336)
    assert (meta["n_iter"], meta["seed"], meta["first_rep"], meta["n_rep"], meta["abi"]) == (2, SEED, 5, 96, ABI_VERSION)
