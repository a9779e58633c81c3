"""GPU: the bulk export (dsce_export / k_export, ABI 9) against the CPU oracle on
the same Philox streams, against the engine's own per-unit trace
(dsce_trace_unit_ex runs the Monte-Carlo kernels, so it is an independent
yardstick for the export kernel), and against itself across batch geometries,
SNR chunks, precisions and destinations.

Bars (tests/test_gpu_parity.py::_check_trace): y and h 1e-10, the LS pilot
estimates and diag(D_hat) 1e-9; the pilots 1e-15 (one hypot against one
np.abs); symbol indices exact.  Every host export in this file goes through
_export, which surrounds each array with guard bytes and checks them."""
import os
import subprocess
import sys

import numpy as np
import pytest

import harness
from oracle import philox

pytestmark = pytest.mark.gpu

SEED = 0x5EED0009
SNR = (10.0, 35.0)
ALL = ("y", "hp_ls", "h_est", "h", "xp", "sym")
GUARD = 256
PATTERN = 0xA5
EINVAL, ESTATE = -1, -3


def _export(eng, sid, seed, first, n, fields=ALL, dtype=np.complex128, flags=None):
    """eng.export into arrays that sit between two guard regions of GUARD bytes
    each; asserts that the export wrote neither."""
    from dsce import engine
    dt = np.dtype(dtype)
    shapes = eng.export_shapes(sid, n)
    raw, out = {}, {}
    for f in fields:
        fdt = np.dtype(np.int32) if f == "sym" else dt
        nb = int(np.prod(shapes[f])) * fdt.itemsize
        raw[f] = np.full(nb + 2 * GUARD, PATTERN, dtype=np.uint8)
        out[f] = raw[f][GUARD:GUARD + nb].view(fdt).reshape(shapes[f])
    if flags is None:
        flags = engine.EXPORT_F32 if dt == np.dtype(np.complex64) else 0
    eng._export(sid, seed, first, n, flags, {f: raw[f].ctypes.data + GUARD for f in fields})
    for f in fields:
        assert (raw[f][:GUARD] == PATTERN).all(), "bytes before %s were written" % f
        assert (raw[f][-GUARD:] == PATTERN).all(), "bytes past %s were written" % f
    return out


_ORACLE = {}


def _oracle_units(S, name, first, n, seed=SEED):
    """refsim.simulate's per-unit trace of realisations [first, first + n),
    as units[i][k] (realisation i, SNR index k); computed once per range (and
    per seed and constellation table: tests replace a setup's table)."""
    key = (S.name, tuple(S.snr_db), S.n_iter, name, first, n, seed, np.asarray(S.schemes[name]["symbols"]).tobytes())
    if key not in _ORACLE:
        tr = {}
        harness.simulate(S, seed, first, n, [name], trace=tr)
        ns = len(S.pn_time)
        _ORACLE[key] = [[tr["units"][i * ns + k] for k in range(ns)] for i in range(n)]
    return _ORACLE[key]


def _oracle_symbols(S, name, rep):
    """(sym, xp) of realisation rep: bi2de of the BITS stream (script:355-357)
    and the unit-modulus pilots (script:365-368)."""
    sc = S.schemes[name]
    nd, m = sc["n_data"], sc["bits_per_symbol"]
    b = philox.bits(SEED, rep, sc["bits_slot"], nd * m)
    sym = (b.reshape(nd, m).astype(np.int64) << np.arange(m)).sum(axis=1)
    pidx = philox.indices(SEED, rep, sc["pilot_slot"], len(sc["pilot_pos"]), sc["symbols"].size)
    xp = sc["symbols"][pidx]
    return sym, xp / np.abs(xp)


def _check_against_units(e, units, rows, fields=("y", "h", "hp_ls", "h_est")):
    for i in rows:
        for k, u in enumerate(units[i]):
            tag = "row %d snr %d" % (i, k)
            if "y" in fields:
                np.testing.assert_allclose(e["y"][i, k], u["y"], rtol=0, atol=1e-10, err_msg=tag)
            if "h" in fields:
                np.testing.assert_allclose(e["h"][i], u["h"], rtol=0, atol=1e-10, err_msg=tag)
            if "hp_ls" in fields:
                np.testing.assert_allclose(e["hp_ls"][i, k], u["hp"][0], rtol=0, atol=1e-9, err_msg=tag)
            if "h_est" in fields:
                np.testing.assert_allclose(e["h_est"][i, k], u["hest"][0], rtol=0, atol=1e-9, err_msg=tag)


@pytest.fixture(scope="module")
def ofdm():
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR)
    eng = harness.engine(S, batch=64)
    yield S, eng
    eng.close()


@pytest.fixture(scope="module")
def ofdm_ref(ofdm):
    """One export of 129 realisations from first_rep 5, shared (read-only)."""
    S, eng = ofdm
    eng.set_batch(64)
    return _export(eng, 0, SEED, 5, 129)


@pytest.fixture(scope="module")
def ofdm_counts(ofdm):
    S, eng = ofdm
    eng.set_batch(64)
    return eng.run(SEED, 0, 64)


@pytest.mark.parametrize("name,lk,npil", [("ofdm", 336, 16), ("fbmc_aux", 720, None)])
def test_export_matches_oracle(name, lk, npil):
    """Default config, 3 realisations from first_rep 5, both SNR points: every
    field against refsim.simulate's trace and the oracle's own symbol draws."""
    S = harness.setup("default", schemes=(name,), snr_db=SNR, n_iter=0)
    eng = harness.engine(S, batch=64)
    try:
        e = _export(eng, 0, SEED, 5, 3)
    finally:
        eng.close()
    sc = S.schemes[name]
    NP, ND = len(sc["pilot_pos"]), sc["n_data"]
    assert e["y"].shape == (3, 2, lk) and e["h_est"].shape == (3, 2, lk) and e["h"].shape == (3, lk)
    assert e["hp_ls"].shape == (3, 2, NP) and e["xp"].shape == (3, NP) and e["sym"].shape == (3, ND)
    if npil:
        assert (NP, ND) == (npil, lk - npil)
    _check_against_units(e, _oracle_units(S, name, 5, 3), range(3))
    for i in range(3):
        sym, xp = _oracle_symbols(S, name, 5 + i)
        assert e["sym"].dtype == np.int32 and np.array_equal(e["sym"][i], sym), i
        np.testing.assert_allclose(e["xp"][i], xp, rtol=0, atol=1e-15)


def test_export_matches_engine_trace(ofdm, ofdm_ref):
    """70 realisations from first_rep 5 (two waves, the second ragged) against
    dsce_trace_unit_ex of the same units: rows 0, 58, 59, 69 and the wave
    boundary of the batch (rows 63 / 64), every SNR point."""
    S, eng = ofdm
    eng.set_batch(128)
    e = _export(eng, 0, SEED, 5, 70)
    for i in (0, 58, 59, 63, 64, 69):
        for k in range(len(SNR)):
            g = eng.trace_unit(0, SEED, 5 + i, k)
            tag = "row %d snr %d" % (i, k)
            np.testing.assert_allclose(e["y"][i, k], g["y"], rtol=0, atol=1e-10, err_msg=tag)
            np.testing.assert_allclose(e["h"][i], g["h"], rtol=0, atol=1e-10, err_msg=tag)
            np.testing.assert_allclose(e["hp_ls"][i, k], g["hp"][0], rtol=0, atol=1e-9, err_msg=tag)
            np.testing.assert_allclose(e["h_est"][i, k], g["hest"][0], rtol=0, atol=1e-9, err_msg=tag)


def _check_rowwise(eng, sid, first, e, fields):
    """Every row of export e against an export of that realisation alone."""
    n = e[fields[0]].shape[0]
    for i in range(n):
        one = _export(eng, sid, SEED, first + i, 1, fields=fields)
        for f in fields:
            if f == "sym":
                assert np.array_equal(e[f][i], one[f][0]), (f, i)
            else:
                np.testing.assert_allclose(e[f][i], one[f][0], rtol=0, atol=1e-12, err_msg="%s row %d" % (f, i))


@pytest.mark.parametrize("n_rep", [1, 64, 65, 129])
def test_export_batch_geometries(ofdm, ofdm_ref, n_rep):
    """Batch 64: one ragged wave, one full batch, a batch and one realisation,
    three batches with a last one of a single realisation."""
    S, eng = ofdm
    eng.set_batch(64)
    e = ofdm_ref if n_rep == 129 else _export(eng, 0, SEED, 5, n_rep)
    assert e["y"].shape[0] == n_rep
    _check_rowwise(eng, 0, 5, e, ALL)


def test_export_snr_chunks():
    """Option snr_chunk = 1 with three SNR points: the per-unit fields of every
    chunk land at their SNR index, the per-realisation fields once."""
    S = harness.setup("default", schemes=("ofdm",), snr_db=(10.0, 20.0, 35.0), n_iter=0)
    eng = harness.engine(S, batch=64, options={"snr_chunk": 1})
    whole = harness.engine(S, batch=64)
    try:
        e = _export(eng, 0, SEED, 5, 65)
        assert e["y"].shape == (65, 3, 336)
        _check_rowwise(eng, 0, 5, e, ALL)
        w = _export(whole, 0, SEED, 5, 65)        # all SNR points in one chunk
        for f in ALL:
            if f == "sym":
                assert np.array_equal(e[f], w[f])
            else:
                np.testing.assert_allclose(e[f], w[f], rtol=0, atol=1e-12, err_msg=f)
    finally:
        eng.close()
        whole.close()


def test_export_c5_without_mmse():
    """C5 OFDM (LK 672, NP 32: two LS chunks, a 21-tile grid) without
    dsce_build_mmse: everything but h_est."""
    fields = ("y", "h", "hp_ls", "xp", "sym")
    S = harness.setup("c5", schemes=("ofdm",), snr_db=SNR, n_iter=0)
    eng = harness.engine(S, batch=64, mmse=False)
    try:
        e = _export(eng, 0, SEED, 5, 65, fields=fields)
        assert e["y"].shape == (65, 2, 672) and e["hp_ls"].shape == (65, 2, 32)
        _check_rowwise(eng, 0, 5, e, fields)
        sc = S.schemes["ofdm"]
        # the LS estimates restated from the exported y and xp (script:412-414)
        ls = e["y"][:, :, sc["pilot_pos"]] / e["xp"][:, None, :] / np.sqrt(sc["kappa"])
        np.testing.assert_allclose(e["hp_ls"], ls, rtol=0, atol=1e-12 * np.abs(ls).max())
        sym, xp = _oracle_symbols(S, "ofdm", 5 + 64)
        assert np.array_equal(e["sym"][64], sym)
        np.testing.assert_allclose(e["xp"][64], xp, rtol=0, atol=1e-15)
    finally:
        eng.close()


def test_export_far_realisation_indices(ofdm):
    """first_rep = 2^32 - 30: the realisation index crosses the Philox counter's
    low word inside the wave, and the output rows are still 0..63."""
    S, eng = ofdm
    eng.set_batch(64)
    first = (1 << 32) - 30
    e = _export(eng, 0, SEED, first, 64, fields=("y", "h"))
    for i in (0, 63):
        u = _oracle_units(S, "ofdm", first + i, 1)
        _check_against_units({"y": e["y"][i:i + 1], "h": e["h"][i:i + 1]}, u, [0], fields=("y", "h"))


def test_export_fp32_is_the_rounded_fp64_export(ofdm, ofdm_ref):
    """DSCE_EXPORT_F32 rounds each fp64 value once, at the store."""
    S, eng = ofdm
    eng.set_batch(64)
    e32 = _export(eng, 0, SEED, 5, 129, dtype=np.complex64)
    for f in ALL:
        if f == "sym":
            assert np.array_equal(e32[f], ofdm_ref[f])
        else:
            assert e32[f].dtype == np.complex64
            assert np.array_equal(e32[f], ofdm_ref[f].astype(np.complex64)), f


_TORCH_CHILD = r"""
import sys
import torch                       # before the engine: both then share torch's HIP runtime
import numpy as np
sys.path[:0] = [%(tests)r, %(pkg)r, %(root)r]
import harness
S = harness.setup("default", schemes=("ofdm",), snr_db=%(snr)r, n_iter=0)
eng = harness.engine(S, batch=64)
for name in ("complex128", "complex64"):
    dt = getattr(torch, name)
    ref = eng.export(0, %(seed)d, 5, 129, dtype=np.dtype(name))
    t = eng.export_torch(0, %(seed)d, 5, 129, dtype=dt)
    for f in ref:
        assert t[f].is_cuda and t[f].dtype == (torch.int32 if f == "sym" else dt), (name, f)
        assert t[f].shape == ref[f].shape and np.array_equal(t[f].cpu().numpy(), ref[f]), (name, f)
    assert np.abs(ref["y"]).max() > 0
# a host pointer is refused with the device flag, and the context still exports
try:
    eng._export(0, %(seed)d, 5, 3, 2, {"y": np.zeros(3 * 2 * 336, dtype=np.complex128).ctypes.data})
    raise SystemExit("host pointer accepted as device memory")
except Exception as e:
    assert "(-1)" in str(e), e
eng.close()
print("EXPORT_TORCH_OK")
"""


def test_export_torch_equals_host_export():
    """DSCE_EXPORT_DEVICE: the kernel writes torch's tensors directly, and they
    equal the host export exactly, for both dtypes.  A child process, because
    torch brings its own HIP runtime and has to be imported before the engine's
    library is loaded for the two to share one (dsce.engine.Engine.export_torch)."""
    code = _TORCH_CHILD % dict(tests=os.path.join(harness.ROOT, "tests"), pkg=harness.PKG, root=harness.ROOT,
                               snr=SNR, seed=SEED)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "EXPORT_TORCH_OK" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])


def test_export_has_no_side_effects(ofdm):
    """Counts, MSE sums and path_info of a run are the same with and without an
    export before it.  The counts are integers and compared exactly, and the
    export itself leaves the MSE totals at exactly zero.  The MSE sums of a run
    are fp64 atomic adds, one per wave and row block, whose order the hardware
    chooses: two plain runs of the same realisations already differ in the
    last bits (measured over six runs: 6.2e-16 relative), so the sums of the two runs are
    compared at the reordering bound of a sum of n non-negative terms,
    (n - 1) eps with n <= 4096 atomics per sum here: rtol 1e-12."""
    S, eng = ofdm
    eng.set_batch(64)
    eng.enable_mse(True)
    try:
        c1 = eng.run(SEED, 0, 128)
        e1, p1 = eng.mse()
        path = eng.path_info(0)
        eng.enable_mse(True)                       # reset the sums
        _export(eng, 0, SEED, 3, 70)
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


def test_export_interpolation_scheme():
    """A doubly-flat OFDM scheme with an interpolation matrix instead of W (no
    dsce_build_mmse): h_est = I hP_LS."""
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
        e = _export(eng, sid, SEED, 5, 65, fields=("hp_ls", "h_est"))
    finally:
        eng.close()
    I = np.asarray(sc.extras["interp"]).reshape(sc.LK, sc.n_pilots)
    want = np.einsum("cp,rkp->rkc", I, e["hp_ls"])
    tol = 1e-12 * np.abs(I).max() * np.abs(e["hp_ls"]).max()
    np.testing.assert_allclose(e["h_est"], want, rtol=0, atol=tol)
    assert np.abs(e["h_est"]).max() > 100 * tol


def test_export_errors_leave_the_context_usable(ofdm, ofdm_counts):
    from dsce import engine
    S, eng = ofdm
    eng.set_batch(64)

    def fails(code, *a, **k):
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % code):
            _export(eng, *a, **k)
        assert np.array_equal(eng.run(SEED, 0, 64), ofdm_counts)

    fails(EINVAL, 0, SEED, 5, 3, fields=())                                   # every field null
    fails(EINVAL, 0, SEED, 5, 3, flags=1 << 2)                                # unknown flag
    fails(EINVAL, 0, SEED, 5, 3, flags=engine.EXPORT_DEVICE)                  # host pointers as device memory
    with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL):           # null out
        eng._chk(eng.lib.dsce_export(eng.h, 0, SEED, 5, 3, 0, None), "dsce_export")
    assert np.array_equal(eng.run(SEED, 0, 64), ofdm_counts)
    z = _export(eng, 0, SEED, 5, 0)                                           # n_rep = 0: OK, nothing written
    assert all(z[f].shape[0] == 0 for f in ALL)
    assert np.array_equal(eng.run(SEED, 0, 64), ofdm_counts)
    # h_est without W or an interpolation matrix; the other fields need neither
    bare = harness.engine(S, batch=64, mmse=False)
    try:
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % ESTATE):
            _export(bare, 0, SEED, 5, 3, fields=("h_est",))
        e = _export(bare, 0, SEED, 5, 3, fields=("y", "sym"))
        assert np.abs(e["y"]).max() > 0
        bare.build_mmse(S.zero_threshold)
        assert np.array_equal(bare.run(SEED, 0, 64), ofdm_counts)
    finally:
        bare.close()
    # before channel, SNR points or scheme are set
    from dsce.engine import Engine
    empty = Engine(0)
    try:
        buf = np.zeros(8)
        rc = empty.lib.dsce_export(empty.h, 0, SEED, 0, 1, 0, engine.ExportOut(y=buf.ctypes.data))
        assert rc == ESTATE
    finally:
        empty.close()


def test_dataset_tool_writes_shards_equal_to_one_export(tmp_path):
    """python -m dsce.dataset in a child process: 96 realisations in shards of
    64 (two files), and load() of them equals one Engine.export."""
    from dsce import dataset
    from dsce.configs import build_setup
    from dsce.engine import ABI_VERSION, build_engine, gpu_tx
    prefix = str(tmp_path / "data" / "ofdm")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([harness.PKG] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    p = subprocess.run([sys.executable, "-m", "dsce.dataset", "--config", "default", "--scheme", "ofdm", "--snr-db", "10",
                        "35", "--seed", str(SEED), "--first-rep", "5", "--reps", "96", "--shard-reps", "64", "--dtype",
                        "complex64", "--out", prefix], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / "data")) == ["ofdm-00000.npz", "ofdm-00001.npz"]
    arrays, meta = dataset.load(prefix)
    S = build_setup("default", schemes=("ofdm",), snr_db=list(SNR), tx=gpu_tx(0))
    eng = build_engine(S, batch=64)                 # the shards' batch geometry: 64 + 32 realisations
    try:
        e = eng.export(0, SEED, 5, 96, dtype=np.complex64)
    finally:
        eng.close()
    assert sorted(arrays) == sorted(ALL)
    for f in ALL:
        assert arrays[f].dtype == e[f].dtype and np.array_equal(arrays[f], e[f]), f
    sc = S.schemes["ofdm"]
    assert (meta["config"], meta["scheme"], meta["dtype"]) == ("default", "ofdm", "complex64")
    assert (meta["seed"], meta["first_rep"], meta["n_rep"], meta["abi"]) == (SEED, 5, 96, ABI_VERSION)
    assert (meta["L"], meta["K"]) == (24, 14) and meta["kappa"] == sc.kappa and meta["data_div"] == sc.data_div
    assert np.array_equal(meta["snr_db"], SNR) and np.array_equal(meta["pn_time"], S.pn_time)
    assert np.array_equal(meta["pilot_pos"], sc.pilot_pos) and np.array_equal(meta["data_pos"], sc.data_pos)
    assert np.array_equal(meta["symbols"], np.asarray(sc.const.SymbolMapping).ravel())
