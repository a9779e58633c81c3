"""GPU: the soft outputs (dsce_llr_awgn / k_llr_probe and dsce_export_llr / k_llr,
DSCE_HAS_LLR) against the NumPy reference dsce.modulation.llr_awgn, against the
definitions of include/dsce.h evaluated on dsce_export_stages' own y_ic / h_est,
against the engine's hard decisions and dsce_run's counters, and against itself
across batch geometries, SNR chunks, staging bounds, precisions and destinations.

Bars.  An LLR is a difference of two log-sums of exponents e_i = |x - s_i|^2 / pn,
so its rounding error scales with the largest exponent: |d| <= 1e-12 (1 + E),
E = max_i e_i of that symbol (a few eps = 1.1e-16 on numbers of size E, with
about 1e4 of headroom; two differently ordered NumPy evaluations differ by
1.1e-13 (1 + E)).  x_est / pn_eff of select schemes rtol 1e-12, the despread sums
1e-12 of the sum of their terms' moduli.  An export against itself 1e-12,
precision and destination variants exact.  Every host destination sits between
guard regions (_llr)."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import harness
from test_gpu_export import EINVAL, ESTATE, GUARD, PATTERN, SEED, SNR, _export
from test_gpu_export_stages import _stages
from test_llr_host import demapper_input

pytestmark = pytest.mark.gpu

ALL = ("x_est", "pn_eff", "llr")
METHODS = ("exact", "maxlog")
WORST = {}


def _note(key, ratio):
    """Worst error / bar seen per check (printed; DESIGN.md section 7g quotes them)."""
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))
    print("llr ratio %-28s %.3e" % (key, WORST[key]))


def _llr(eng, sid, seed, first, n, fields=ALL, method="exact", dtype=np.complex128, flags=None, rows=None):
    """eng.export_llr into arrays that sit between two guard regions of GUARD
    bytes each; asserts that the export wrote neither.  rows > n: destinations of
    that many realisations, and the rows past n must stay untouched too."""
    from dsce import engine
    dt = np.dtype(dtype)
    rdt = np.dtype(np.float32 if dt == np.dtype(np.complex64) else np.float64)
    shapes = eng.export_llr_shapes(sid, n if rows is None else rows)
    raw, out = {}, {}
    for f in fields:
        fdt = dt if f == "x_est" else rdt
        nb = int(np.prod(shapes[f])) * fdt.itemsize
        raw[f] = np.full(nb + 2 * GUARD, PATTERN, dtype=np.uint8)
        out[f] = raw[f][GUARD:GUARD + nb].view(fdt).reshape(shapes[f])
    if flags is None:
        flags = engine.LLR_METHODS[method] | (engine.EXPORT_F32 if dt == np.dtype(np.complex64) else 0)
    eng._export_llr(sid, seed, first, n, flags, {f: raw[f].ctypes.data + GUARD for f in fields})
    for f in fields:
        assert (raw[f][:GUARD] == PATTERN).all(), "bytes before %s were written" % f
        assert (raw[f][-GUARD:] == PATTERN).all(), "bytes past %s were written" % f
        if rows is not None:
            assert (out[f][n:].view(np.uint8) == PATTERN).all(), "rows past n_rep of %s were written" % f
            out[f] = out[f][:n]
    return out


def _bitmap(M):
    return ((np.arange(M)[:, None] >> np.arange(int(np.log2(M)))) & 1).astype(bool)


def _emax(symbols, x, pn):
    """E = max_i |x - s_i|^2 / pn per observation."""
    d = np.asarray(x).reshape(-1)[:, None] - np.asarray(symbols).reshape(-1)[None, :]
    return (d.real ** 2 + d.imag ** 2).max(axis=1) / np.broadcast_to(pn, np.asarray(x).reshape(-1).shape)


def _probe_inputs(symbols):
    """1000 observations: the constellation points, the midpoints between grid
    neighbours, points at |x| = 1e3, in a fixed shuffled order."""
    s = np.asarray(symbols).reshape(-1)
    lvI, lvQ = np.unique(s.real), np.unique(s.imag)
    mids = [(a + b) / 2 + 1j * q for a, b in zip(lvI[:-1], lvI[1:]) for q in lvQ]
    mids += [i + 1j * (a + b) / 2 for a, b in zip(lvQ[:-1], lvQ[1:]) for i in lvI]
    far = 1e3 * np.exp(2j * np.pi * np.arange(16) / 16)
    if lvQ.size == 1:
        far = np.concatenate([far.real[far.real != 0], far])      # real observations of a PAM scheme, and complex ones
    pool = np.concatenate([s, np.asarray(mids, dtype=complex), far])
    x = np.resize(pool, 1000)
    return x[np.random.default_rng(5).permutation(1000)]


def _check_probe(eng, sid, symbols, tag):
    from dsce.modulation import llr_awgn
    bm = _bitmap(symbols.size)
    xs = _probe_inputs(symbols)
    pns = np.array([1e-8, 1e-2, 1.0, 1e4])
    for method in METHODS:
        for n in (1, 63, 65, 1000):
            x = xs[:n] if n > 1 else xs[7:8]
            for pn in list(pns) + [np.resize(pns, n)]:
                got = eng.llr_awgn(sid, x, pn, method)
                ref = llr_awgn(symbols, bm, x, pn, method)
                assert got.shape == ref.shape == (n, bm.shape[1]) and np.isfinite(got).all(), (tag, method, n)
                bar = 1e-12 * (1 + _emax(symbols, x, pn))[:, None]
                err = np.abs(got - ref)
                _note("probe %s %s" % (tag, method), (err / bar).max())
                assert (err <= bar).all(), (tag, method, n, pn, (err / bar).max())


@pytest.mark.parametrize("name,order", [("ofdm", 4), ("ofdm", 64), ("ofdm", 256), ("fbmc_aux", 256)],
                         ids=["qam4", "qam64", "qam256", "pam16"])
def test_probe_against_host_reference(name, order):
    """dsce_llr_awgn (needs only dsce_add_scheme) on the per-axis form."""
    S = harness.setup("default", schemes=(name,), snr_db=SNR, qam_order=order)
    symbols = S.schemes[name]["symbols"]
    assert symbols.size == (order if name == "ofdm" else int(np.sqrt(order)))
    eng = harness.engine(S, batch=64, mmse=False)
    try:
        assert eng.llr_info(0) == dict(per_axis=True, m=int(np.log2(symbols.size)))
        _check_probe(eng, 0, symbols, "%s-%d" % (name, symbols.size))
        assert np.isnan(eng.llr_awgn(0, [np.nan, 0.1], [1.0, np.nan])).all()
    finally:
        eng.close()


def test_full_table_form():
    """16-QAM with its symbols table permuted (the C-ABI takes the table as caller
    data): bits depend on both axes, the full-table form runs."""
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR, qam_order=16)
    sc = S.schemes["ofdm"]
    perm = np.random.default_rng(16).permutation(16)
    symbols = sc["symbols"][perm]
    bm = _bitmap(16)
    # bit b is a function of one coordinate alone iff it is constant on every level set of that coordinate
    alone = lambda b, c: all(len(set(bm[c == v, b])) == 1 for v in np.unique(c))
    assert any(not alone(b, symbols.real) and not alone(b, symbols.imag) for b in range(4)), \
        "the permutation must make a bit depend on both axes"
    S2 = SimpleNamespace(**dict(vars(S), schemes={"ofdm": dict(sc, symbols=symbols)}))
    eng = harness.engine(S2, batch=64, mmse=False)
    try:
        assert eng.llr_info(0) == dict(per_axis=False, m=4)
        _check_probe(eng, 0, symbols, "permuted-16")
        assert np.isnan(eng.llr_awgn(0, [np.nan, 0.1], [1.0, np.nan])).all()
    finally:
        eng.close()


@pytest.fixture(scope="module", params=["ofdm", "fbmc_aux", "fbmc_cod"])
def bulk(request):
    """Per scheme (default setup, n_iter 4, SNR (10, 35), batch 64), realisations
    5..7: the stage export, the transmitted symbols, the run's counters and the
    LLR export of both methods, shared (read-only)."""
    name = request.param
    S = harness.setup("default", schemes=(name,), snr_db=SNR, n_iter=4)
    eng = harness.engine(S, batch=64)
    try:
        st = _stages(eng, 0, SEED, 5, 3, fields=("h_est", "y_ic", "dec_est"))
        sym = _export(eng, 0, SEED, 5, 3, fields=("sym",))["sym"]
        counts = eng.run(SEED, 5, 3)
        path = eng.path_info(0)
        llr = {m: _llr(eng, 0, SEED, 5, 3, method=m) for m in METHODS}
        assert eng.llr_info(0)["per_axis"]
    finally:
        eng.close()
    return SimpleNamespace(name=name, S=S, sc=S.schemes[name], st=st, sym=sym, counts=counts, path=path, llr=llr)


def test_bulk_against_the_stage_export(bulk):
    """x_est and pn_eff are include/dsce.h's definitions evaluated in NumPy on
    export_stages' y_ic / h_est of the same realisations; llr of both methods is
    the host reference applied to the engine's own x_est / pn_eff; no NaN."""
    from dsce.modulation import llr_awgn
    sc, e = bulk.sc, bulk.llr["exact"]
    if bulk.name == "ofdm":
        assert {"mic_stages", "pic_fft"} <= bulk.path, bulk.path
    nd, m = sc["n_data"], sc["bits_per_symbol"]
    x, pe, terms = demapper_input(sc, bulk.S.pn_time, bulk.st["y_ic"], bulk.st["h_est"])
    assert e["x_est"].shape == e["pn_eff"].shape == (3, 2, 5, nd) and e["llr"].shape == (3, 2, 5, nd, m)
    for f in ALL:
        assert not np.isnan(e[f]).any() and not np.isnan(bulk.llr["maxlog"][f]).any(), f
    if sc["real_detect"]:
        assert not e["x_est"].imag.any()
    _note("bulk x_est %s" % bulk.name, (np.abs(e["x_est"] - x) / (1e-12 * terms)).max())
    _note("bulk pn_eff %s" % bulk.name, (np.abs(e["pn_eff"] - pe) / (1e-12 * pe)).max())
    assert (np.abs(e["x_est"] - x) <= 1e-12 * terms).all()
    assert (np.abs(e["pn_eff"] - pe) <= 1e-12 * pe).all() and (e["pn_eff"] > 0).all()
    for method in METHODS:
        g = bulk.llr[method]
        assert np.array_equal(g["x_est"], e["x_est"]) and np.array_equal(g["pn_eff"], e["pn_eff"])
        ref = llr_awgn(sc["symbols"], _bitmap(sc["symbols"].size), g["x_est"], g["pn_eff"], method).reshape(g["llr"].shape)
        bar = 1e-12 * (1 + _emax(sc["symbols"], g["x_est"], g["pn_eff"].reshape(-1))).reshape(g["pn_eff"].shape + (1,))
        err = np.abs(g["llr"] - ref)
        _note("bulk llr %s %s" % (bulk.name, method), (err / bar).max())
        assert (err <= bar).all(), (method, (err / bar).max())


def test_closure_with_the_engine(bulk):
    """The bits from the sign of the max-log llr are the bits of export_stages'
    dec_est in every entry, and their errors against dsce_export's sym are the
    run's MMSE counters of both edge classes, exactly.  Safe because no entry of
    these realisations sits on a decision boundary: the smallest max-log margin
    |LLR pn| is asserted >= 1e-9 (CPU oracle: 9.9e-7 ofdm, 1.2e-5 fbmc_aux, 1.5e-6
    fbmc_cod)."""
    sc, g = bulk.sc, bulk.llr["maxlog"]
    m = sc["bits_per_symbol"]
    margin = np.abs(g["llr"] * g["pn_eff"][..., None]).min()
    print("llr margin %s %.3e" % (bulk.name, margin))
    assert margin >= 1e-9
    bits = g["llr"] > 0
    dec_bits = ((bulk.st["dec_est"][..., None] >> np.arange(m)) & 1).astype(bool)
    assert (bulk.st["dec_est"] >= 0).all() and np.array_equal(bits, dec_bits)
    tx = ((bulk.sym[:, None, None, :, None] >> np.arange(m)) & 1).astype(bool)
    wrong = bits != tx
    cons = np.asarray(sc["considered"]).astype(bool)
    assert bulk.counts.shape == (1, 2, 2, 2, 5) and bulk.counts[0, 0].min() > 0
    assert np.array_equal(wrong.sum(axis=(0, 3, 4)), bulk.counts[0, 0, 0])
    assert np.array_equal(wrong[:, :, :, cons].sum(axis=(0, 3, 4)), bulk.counts[0, 0, 1])


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
    return _llr(eng, 0, SEED, 5, 129)


def _same(a, b, atol=1e-12):
    for f in a:
        np.testing.assert_allclose(a[f], b[f], rtol=0, atol=atol, err_msg=f)


def test_llr_invariance(ofdm, ofdm_ref):
    """129 realisations from 5: batch 128, an export_stage_mb that cuts the batch
    into one-wave sub-batches (the bound of test_gpu_export_stages.py: a unit's
    bulk arrays are 67840 B), and two calls over a split range equal the batch-64
    export; rows past n_rep and the guard bytes stay untouched."""
    S, eng = ofdm
    eng.set_batch(128)
    try:
        whole = _llr(eng, 0, SEED, 5, 129)
        eng.set_option("export_stage_mb", 12)
        cut = _llr(eng, 0, SEED, 5, 129)
    finally:
        eng.set_option("export_stage_mb", 1024)
        eng.set_batch(64)
    _same(whole, ofdm_ref)
    _same(cut, ofdm_ref)
    a, b = _llr(eng, 0, SEED, 5, 70), _llr(eng, 0, SEED, 75, 59, rows=61)
    for f in ALL:
        assert np.array_equal(np.concatenate([a[f], b[f]]), ofdm_ref[f]), f
    z = _llr(eng, 0, SEED, 5, 0, rows=1)                                       # n_rep = 0: OK, nothing written
    assert all(z[f].shape[0] == 0 for f in ALL)


def test_llr_snr_chunks():
    """Option snr_chunk = 1 with three SNR points equals the unchunked export."""
    S = harness.setup("default", schemes=("ofdm",), snr_db=(10.0, 20.0, 35.0), n_iter=2)
    eng = harness.engine(S, batch=64, options={"snr_chunk": 1})
    whole = harness.engine(S, batch=64)
    try:
        e = _llr(eng, 0, SEED, 5, 65)
        assert e["llr"].shape == (65, 3, 3, 320, 8)
        _same(e, _llr(whole, 0, SEED, 5, 65))
    finally:
        eng.close()
        whole.close()


def test_llr_fp32_is_the_rounded_fp64_export(ofdm, ofdm_ref):
    """DSCE_EXPORT_F32 rounds each fp64 value once, at the store."""
    S, eng = ofdm
    eng.set_batch(64)
    e32 = _llr(eng, 0, SEED, 5, 129, dtype=np.complex64)
    assert e32["x_est"].dtype == np.complex64 and e32["pn_eff"].dtype == e32["llr"].dtype == np.float32
    assert np.array_equal(e32["x_est"], ofdm_ref["x_est"].astype(np.complex64))
    for f in ("pn_eff", "llr"):
        assert np.array_equal(e32[f], ofdm_ref[f].astype(np.float32)), f


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
    ref = eng.export_llr(0, %(seed)d, 5, 129, method=method, dtype=np.dtype(name))
    t = eng.export_llr_torch(0, %(seed)d, 5, 129, method=method, dtype=dt)
    for f in ref:
        assert t[f].is_cuda and t[f].shape == ref[f].shape, (name, f)
        assert t[f].dtype == (dt if f == "x_est" else torch.float64 if name == "complex128" else torch.float32), (name, f)
        assert np.array_equal(t[f].cpu().numpy(), ref[f]), (name, f)
    assert np.abs(ref["llr"]).max() > 0 and np.isfinite(ref["llr"]).all()
# a host pointer is refused with the device flag, and the context still exports
try:
    eng._export_llr(0, %(seed)d, 5, 3, 2, {"pn_eff": np.zeros(3 * 2 * 3 * 320).ctypes.data})
    raise SystemExit("host pointer accepted as device memory")
except Exception as e:
    assert "(-1)" in str(e), e
assert np.array_equal(eng.export_llr(0, %(seed)d, 5, 3, method="maxlog", dtype=np.complex64)["llr"], ref["llr"][:3])
eng.close()
print("EXPORT_LLR_TORCH_OK")
"""


def test_llr_torch_equals_host_export():
    """DSCE_EXPORT_DEVICE: the kernel writes torch's tensors directly, and they
    equal the host export exactly, for both dtypes; a host pointer with the
    device flag is DSCE_EINVAL.  A child process, because torch has to be
    imported before the engine's library is loaded (Engine.export_torch)."""
    code = _TORCH_CHILD % dict(tests=os.path.join(harness.ROOT, "tests"), pkg=harness.PKG, root=harness.ROOT,
                               snr=SNR, seed=SEED)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "EXPORT_LLR_TORCH_OK" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])


def test_llr_errors_and_side_effects(ofdm):
    from dsce import engine
    S, eng = ofdm
    eng.set_batch(64)
    counts = eng.run(SEED, 0, 64)
    path = eng.path_info(0)

    def fails(code, *a, **k):
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % code):
            _llr(eng, *a, **k)
        assert np.array_equal(eng.run(SEED, 0, 64), counts)

    fails(EINVAL, 0, SEED, 5, 3, fields=())                                   # every field null
    fails(EINVAL, 0, SEED, 5, 3, flags=1 << 3)                                # unknown flag
    fails(EINVAL, 0, SEED, 5, 3, flags=engine.EXPORT_DEVICE)                  # host pointers as device memory
    with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL):           # null out
        eng._chk(eng.lib.dsce_export_llr(eng.h, 0, SEED, 5, 3, 0, None), "dsce_export_llr")
    # no side effects: counters and path of a run, before and after an export
    eng.enable_timing(True)
    try:
        _llr(eng, 0, SEED, 3, 70)
        assert eng.kernel_time("k_llr")[0] >= 2 and eng.kernel_time("k_llr")[1] > 0
    finally:
        eng.enable_timing(False)
    assert eng.path_info(0) == path
    assert np.array_equal(eng.run(SEED, 0, 64), counts) and eng.path_info(0) == path and counts.sum() > 0
    # dsce_llr_awgn's argument checks
    x, pn, out = np.zeros(8), np.ones(4), np.zeros(4 * 8)
    dp = lambda a: a.ctypes.data_as(engine.C.POINTER(engine.C.c_double))
    call = lambda flags, xp, pp, n_pn, n, op: eng.lib.dsce_llr_awgn(eng.h, 0, flags, xp, pp, n_pn, n, op)
    assert call(0, dp(x), dp(pn), 4, 4, dp(out)) == 0 and call(0, dp(x), dp(pn), 1, 4, dp(out)) == 0
    assert call(0, None, None, 1, 0, None) == 0                               # n = 0 does nothing
    assert call(0, None, dp(pn), 4, 4, dp(out)) == EINVAL and call(0, dp(x), None, 4, 4, dp(out)) == EINVAL
    assert call(0, dp(x), dp(pn), 4, 4, None) == EINVAL
    assert call(0, dp(x), dp(pn), 1, -1, dp(out)) == EINVAL                   # n < 0
    assert call(0, dp(x), dp(pn), 3, 4, dp(out)) == EINVAL                    # n_pn neither 1 nor n
    assert call(1, dp(x), dp(pn), 4, 4, dp(out)) == EINVAL                    # unknown flag
    assert call(engine.LLR_MAXLOG, dp(x), dp(pn), 4, 4, dp(out)) == 0
    assert np.array_equal(eng.run(SEED, 0, 64), counts)
    # without dsce_build_mmse; after it the same context exports
    bare = harness.engine(S, batch=64, mmse=False)
    try:
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % ESTATE):
            _llr(bare, 0, SEED, 5, 3)
        bare.build_mmse(S.zero_threshold)
        assert np.isfinite(_llr(bare, 0, SEED, 5, 3, fields=("llr",))["llr"]).all()
    finally:
        bare.close()
    # before channel, SNR points or scheme are set
    empty = engine.Engine(0)
    try:
        buf = np.zeros(8)
        rc = empty.lib.dsce_export_llr(empty.h, 0, SEED, 0, 1, 0, engine.ExportLlrOut(llr=buf.ctypes.data))
        assert rc == ESTATE
    finally:
        empty.close()


def test_llr_interpolation_scheme_without_iterations():
    """An interpolation scheme with n_iter 0 needs no dsce_build_mmse (S = 1); with
    n_iter > 0 the export is DSCE_ESTATE."""
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
                e = _llr(eng, sid, SEED, 5, 65)
            else:
                with pytest.raises(DsceError, match=r"\(%d\)" % ESTATE):
                    _llr(eng, sid, SEED, 5, 3)
        finally:
            eng.close()
    assert e["llr"].shape == (65, 2, 1, sc.n_data, sc.bits_per_symbol) and np.isfinite(e["llr"]).all()
