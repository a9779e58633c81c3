"""GPU: dsce_ldpc_fixed and dsce_run_ldpc_fixed (k_ldpc_fixed_probe, k_ldpc_fixed,
DSCE_HAS_LDPC_FIXED) — the fixed-point min-sum decoder on the device against its
NumPy twin dsce.coding.ldpc_decode_fixed, equal in decided bits, iteration counts
and a-posteriori sums: on drawn inputs over the limit codes of test_gpu_ldpc
(check degrees 2 and 32, a variable of degree 40, of degree 1 and 0, punctured
variables, a slot used twice) for every word length, normalisation, offset and
input class of tests/test_ldpc_fixed_host.py; against dsce_ldpc, the fp64 kernel,
on integer inputs that nothing clips; on the engine's own export_llr output and
export's sym for both LLR methods, both CSI branches, installed scale tables,
with and without a codeword; across batch geometries, SNR chunks, staging bounds
and split calls; and every refusal.  Every comparison is exact.  Host outputs
sit between guard regions."""
import ctypes as C

import numpy as np
import pytest

import harness
from test_gpu_export import EINVAL, ESTATE, GUARD, PATTERN, SEED, SNR, _export
from test_gpu_ldpc import ALL, BRANCHES, METHODS, _desc, _same, limit_code
from test_gpu_ldpc import _ldpc as _ldpc_fp64
from test_gpu_ldpc import _run as _run_fp64
from test_ldpc_fixed_host import ORACLE_LDPC_FIXED, integer_case

pytestmark = pytest.mark.gpu


def _fx(fx):
    from dsce import engine
    return engine.Engine._ldpc_fixed(fx)


def _ldpc(eng, lam, code, fx, iters=True, app=True):
    """dsce_ldpc_fixed into a uint8, an int32 and an int16 array, each between two guard regions."""
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    n, N = lam.shape[0], int(code.n_vars)
    raw = np.full(n * N + 2 * GUARD, PATTERN, dtype=np.uint8)
    rit = np.full(n * 4 + 2 * GUARD, PATTERN, dtype=np.uint8)
    rap = np.full(n * N * 2 + 2 * GUARD, PATTERN, dtype=np.uint8)
    desc, keep = _desc(code)
    fd = _fx(fx)
    ip = rit[GUARD:].ctypes.data_as(C.POINTER(C.c_int32)) if iters else None
    ap = rap[GUARD:].ctypes.data_as(C.POINTER(C.c_int16)) if app else None
    eng._chk(eng.lib.dsce_ldpc_fixed(eng.h, C.byref(desc), C.byref(fd), lam.shape[1],
                                     lam.ctypes.data_as(C.POINTER(C.c_double)), n,
                                     raw[GUARD:].ctypes.data_as(C.POINTER(C.c_uint8)), ip, ap), "dsce_ldpc_fixed")
    for name, r, on in (("bits_out", raw, True), ("iters_out", rit, iters), ("app_out", rap, app)):
        assert (r[:GUARD] == PATTERN).all() and (r[-GUARD:] == PATTERN).all(), "bytes outside %s were written" % name
        if not on:
            assert (r == PATTERN).all(), name
    return (raw[GUARD:GUARD + n * N].reshape(n, N).copy(), rit[GUARD:GUARD + 4 * n].view(np.int32).copy(),
            rap[GUARD:GUARD + 2 * n * N].view(np.int16).reshape(n, N).copy())


def _run(eng, sid, seed, first, n, code, fx, word=None, fields=ALL, method="exact", branch="mmse", flags=None, into=None):
    """dsce_run_ldpc_fixed as test_gpu_ldpc._run calls dsce_run_ldpc: zeroed int64 arrays (or copies of `into`) in one
    buffer between guards; only `fields` are passed.  Asserts that the guards and the fields not requested keep
    their bytes, and that a refused call writes nothing."""
    from dsce import engine
    shapes = eng.ldpc_shapes(sid)
    raw = np.full(4 * GUARD + sum(int(np.prod(shapes[f])) * 8 for f in ALL), PATTERN, dtype=np.uint8)
    view, at = {}, GUARD
    for f in ALL:
        nb = int(np.prod(shapes[f])) * 8
        view[f] = raw[at:at + nb].view(np.int64).reshape(shapes[f])
        at += nb + GUARD
    for f in fields:
        view[f][...] = 0 if into is None else into[f]
    before = raw.copy()
    o = engine.LdpcOut(**{f: view[f].ctypes.data_as(C.POINTER(C.c_int64)) for f in fields})
    if flags is None:
        flags = engine.LLR_METHODS[method] | engine.LLR_BRANCHES[branch]
    desc, keep = _desc(code)
    fd = C.byref(_fx(fx)) if fx is not None else None
    w = None if word is None else np.ascontiguousarray(word, dtype=np.uint8)
    wp = None if w is None else w.ctypes.data_as(C.POINTER(C.c_uint8))
    try:
        eng._chk(eng.lib.dsce_run_ldpc_fixed(eng.h, sid, seed, first, n, flags, C.byref(desc), fd, wp, C.byref(o)),
                 "dsce_run_ldpc_fixed")
    except engine.DsceError:
        assert np.array_equal(raw, before), "a refused call wrote"
        raise
    mask = np.ones(raw.size, dtype=bool)
    for f in fields:
        a0 = view[f].ctypes.data - raw.ctypes.data
        mask[a0:a0 + view[f].nbytes] = False
    assert np.array_equal(raw[mask], before[mask]), "bytes outside the requested fields were written"
    return {f: view[f].copy() for f in fields}


def _twin_counts(eng, sid, first, n, code, fx, word, method, branch):
    from dsce.coding import ldpc_counts_fixed
    llr = eng.export_llr(sid, SEED, first, n, fields=("llr",), method=method, branch=branch)["llr"]
    sym = _export(eng, sid, SEED, first, n, fields=("sym",))["sym"]
    assert llr.dtype == np.float64 and np.isfinite(llr).all()
    return ldpc_counts_fixed(llr, sym, code, fx, codeword=word)


def _word(code, seed=11):
    from dsce.coding import ldpc_encode
    return ldpc_encode(np.random.RandomState(seed).randint(0, 2, code.n_info), code)


@pytest.fixture(scope="module")
def bare():
    """A context with nothing set: dsce_ldpc_fixed needs no more."""
    from dsce import engine
    eng = engine.Engine(0)
    yield eng
    eng.close()


# (q_ch, q_msg, q_app), (alpha_num, alpha_shift), beta (None: X), scale, early_stop, max_iter: every word length of the
# host test, alpha 1, 3/4 and 13/16, beta 0, 1 and >= X, scales that zero and that saturate everything, both early_stop
# values, 1, 2 and 25 iterations
PARAMS = (((6, 6, 8), (1, 0), 1, 2.0, 1, 25), ((6, 6, 8), (3, 2), 0, 2.0, 1, 25), ((2, 2, 2), (1, 0), 0, 1.0, 1, 25),
          ((4, 4, 6), (1, 0), 0, 1.0, 0, 25), ((8, 4, 8), (13, 4), 1, 4.0, 1, 25), ((16, 16, 16), (3, 2), 1, 100.0, 0, 2),
          ((16, 16, 16), (1, 0), 0, 1.0, 1, 2), ((6, 6, 8), (13, 4), None, 2.0, 1, 25), ((4, 4, 6), (3, 2), 32767, 1.0, 0, 1),
          ((6, 6, 8), (1, 0), 1, 1e-6, 1, 25), ((6, 6, 8), (3, 2), 1, 1e6, 1, 1), ((16, 16, 16), (1, 0), 1, 1e6, 0, 25))


@pytest.mark.parametrize("N", [8, 63, 64, 65, 255, 256, 257, 600])
def test_ldpc_fixed_against_the_twin(bare, N):
    """dsce_ldpc_fixed == ldpc_decode_fixed in bits, iterations and app for 1, 3 and 65 codewords on limit_code(N):
    variable counts around the wavefront and the 256-thread marks and one that takes several strides per phase, the
    parameter sets of PARAMS, and three kinds of input: normal, k + 0.5 (the half-away rule, zeros and ties
    everywhere), and normal with +-inf and NaN entries.  iters_out and app_out are each left out in turn."""
    from dsce.coding import ldpc_decode_fixed, make_fixed
    rng = np.random.default_rng(500 + N)
    code0 = limit_code(N, rng)
    ones, stops = 0, set()
    for n in (1, 3, 65):
        base = 2.0 * rng.standard_normal((n, code0.n_slots)) - 1.5
        halves = rng.integers(-6, 6, base.shape).astype(np.float64) + 0.5
        odd = base.copy()
        odd[0, :3] = [np.inf, -np.inf, np.nan]
        odd[n // 2, ::2] = np.nan
        odd[-1, 1::3] = -np.inf
        for words, (an, sh), beta, scale, early, max_iter in (PARAMS if n < 65 else PARAMS[N % 2::2]):
            X = (1 << (words[1] - 1)) - 1
            fx = make_fixed(*words, scale=scale, alpha_num=an, alpha_shift=sh, beta=X if beta is None else beta)
            code = code0._replace(early_stop=bool(early), max_iter=max_iter)
            for kind, lam in (("normal", base), ("halves", halves), ("odd", odd)):
                got, git, gapp = _ldpc(bare, lam, code, fx)
                ref, rit, rapp = ldpc_decode_fixed(lam, code, fx)
                what = (n, words, an, sh, beta, scale, early, max_iter, kind)
                assert got.dtype == np.uint8 and got.max() <= 1 and gapp.dtype == np.int16
                assert np.array_equal(git, rit), (what, git[:8], rit[:8])
                assert np.array_equal(gapp, rapp), (what, np.argwhere(gapp != rapp)[:4])
                assert np.array_equal(got, ref) and np.array_equal(got, (gapp < 0).astype(np.uint8)), what
                assert np.abs(gapp.astype(np.int32)).max() <= (1 << (words[2] - 1)) - 1
                if scale == 1e-6 and kind != "odd":
                    assert not gapp.any() and (git == (1 if early else max_iter)).all()
                if not early:
                    assert (git == max_iter).all()
                ones += int(got.sum())
                stops.update(git.tolist())
        # iters_out and app_out left out in turn, and the Python wrapper, one codeword without the leading axis too
        fx = make_fixed(6, 6, 8, alpha_num=3, alpha_shift=2, beta=0)
        code = code0._replace(max_iter=25)
        ref, rit, rapp = ldpc_decode_fixed(base, code, fx)
        x, it, app = _ldpc(bare, base, code, fx, iters=False)
        assert np.array_equal(x, ref) and np.array_equal(app, rapp)
        x, it, app = _ldpc(bare, base, code, fx, app=False)
        assert np.array_equal(x, ref) and np.array_equal(it, rit)
        x, it, app = bare.ldpc(base, code, fixed=fx)
        assert np.array_equal(x, ref) and np.array_equal(it, rit) and np.array_equal(app, rapp) and app.dtype == np.int16
        x, it, app = bare.ldpc(base[0], code, fixed=fx)
        assert np.array_equal(x, ref[0]) and it == rit[0] and np.array_equal(app, rapp[0])
    assert ones > 0 and {1, 2, 25} <= stops


@pytest.mark.parametrize("rate", ["1/2", "3/4"])
def test_ldpc_fixed_full_size_codes(bare, rate):
    """make_ldpc(2560, rate) at 6 / 6 / 8 bit over BPSK / AWGN noise where some frames fail: five real codewords
    against the twin, offset and normalised rule; noiseless words come back after one iteration."""
    from dsce.coding import ldpc_decode_fixed, ldpc_encode, ldpc_lam, make_fixed, make_ldpc
    from test_ldpc_host import bpsk_lam0, flip_of
    code = make_ldpc(2560, rate)
    lam0, raw = bpsk_lam0(code, 0.80 if rate == "1/2" else 0.62, 5, 77)
    cw = ldpc_encode(np.random.default_rng(8).integers(0, 2, (5, code.n_info)), code)
    lam = lam0 * flip_of(cw, code)
    for fx in (make_fixed(), make_fixed(6, 6, 8, alpha_num=3, alpha_shift=2, beta=0)):
        got = _ldpc(bare, lam, code, fx)
        ref = ldpc_decode_fixed(lam, code, fx)
        for g, r in zip(got, ref):
            assert np.array_equal(g, r)
        assert got[1].max() > 1
    x, it, app = _ldpc(bare, ldpc_lam(cw, code, 2.5), code, make_fixed())
    assert np.array_equal(x, cw) and (it == 1).all()


@pytest.mark.parametrize("N,rate", [(96, "1/2"), (96, "3/4"), (600, "1/2")])
def test_integer_inputs_equal_the_fp64_kernel(bare, N, rate):
    """Integer-valued lam, scale 1, 16 / 16 / 16 bit, alpha 1 / 1, beta 0: k_ldpc_fixed_probe and k_ldpc_probe, two
    different kernels, give the same bits and iterations (tests/test_ldpc_fixed_host.py has the premise)."""
    from test_ldpc_host import code_of
    lam, code, fx = integer_case(code_of(N, rate))
    x, it, app = _ldpc(bare, lam, code, fx)
    rx, rit = _ldpc_fp64(bare, lam, code)
    assert int(np.abs(app.astype(np.int32)).max()) < 32767
    assert np.array_equal(x, rx) and np.array_equal(it, rit) and x.any()


@pytest.mark.parametrize("name,rate", [("ofdm", "1/2"), ("ofdm", "3/4"), ("fbmc_aux", "1/2"), ("fbmc_cod", "3/4")])
def test_run_ldpc_fixed_against_the_twin(name, rate):
    """Default setup, n_iter 4, SNR (10, 35), batch 64, realisations 5..7: the counts of both methods and both
    branches with the RandomState(11) codeword equal ldpc_counts_fixed on export_llr's fp64 LLRs and export's sym,
    exactly, and so do those of the all-zero word (null codeword).  For ofdm, max-log, MMSE branch they are the
    counts recorded from the oracle's LLRs (ORACLE_LDPC_FIXED)."""
    from dsce.coding import make_fixed, make_ldpc
    S = harness.setup("default", schemes=(name,), snr_db=SNR, n_iter=4)
    sc = S.schemes[name]
    B = sc["n_data"] * sc["bits_per_symbol"]
    eng = harness.engine(S, batch=64)
    try:
        code = make_ldpc(B, rate)
        fx, word = make_fixed(), _word(code)
        for method in METHODS:
            for branch in BRANCHES:
                got = _run(eng, 0, SEED, 5, 3, code, fx, word, method=method, branch=branch)
                print("ldpc fixed %s %s %s %s %s" % (name, rate, method, branch, {f: got[f].tolist() for f in ALL}))
                assert got["bit_err"].shape == (len(SNR), S.n_iter + 1) and got["bit_err"].dtype == np.int64
                _same(got, _twin_counts(eng, 0, 5, 3, code, fx, word, method, branch))
                assert (got["frame_err"] <= 3).all() and ((got["bit_err"] > 0) == (got["frame_err"] > 0)).all()
                assert (got["iter_sum"] >= 3).all() and (got["iter_sum"] <= 3 * code.max_iter).all()
                if name == "ofdm" and method == "maxlog" and branch == "mmse":
                    for f in ALL:
                        assert got[f].tolist() == ORACLE_LDPC_FIXED[rate][f], (rate, f, got[f])
        zero = _run(eng, 0, SEED, 5, 3, code, fx, None, method="maxlog")
        _same(zero, _twin_counts(eng, 0, 5, 3, code, fx, None, "maxlog", "mmse"))
        _same(zero, _run(eng, 0, SEED, 5, 3, code, fx, np.zeros(code.n_vars, dtype=np.uint8), method="maxlog"))
        # the Python wrapper
        w = eng.run_ldpc(0, SEED, 5, 3, code, method="maxlog", fixed=fx, codeword=word)
        _same(w, _run(eng, 0, SEED, 5, 3, code, fx, word, method="maxlog"))
    finally:
        eng.close()


@pytest.fixture(scope="module")
def fixed_ofdm():
    """The default OFDM scheme with a rate-3/4 code over all 2560 slots, and a 200-variable code scattered over them
    for the runs of many realisations, each with a codeword."""
    from dsce.coding import make_fixed, make_ldpc
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR, n_iter=4)
    eng = harness.engine(S, batch=64)
    sc = S.schemes["ofdm"]
    B = sc["n_data"] * sc["bits_per_symbol"]
    small = make_ldpc(200, "1/2", max_iter=12)
    small = small._replace(slot=np.random.default_rng(4).permutation(B)[:200].astype(np.int32), n_slots=B)
    code = make_ldpc(B, "3/4")
    yield S, eng, code, _word(code), small, _word(small), make_fixed()
    eng.close()


def test_run_ldpc_fixed_with_scale_tables(fixed_ofdm):
    """Random tables g = 10**uniform(-1, 2) on each branch: the counts equal the twin on the scaled export, with a
    normalised 4 / 4 / 6 bit decoder too, and the tables change them."""
    from dsce.coding import make_fixed
    S, eng, code, word, small, sword, fx = fixed_ofdm
    eng.set_batch(64)
    rng = np.random.default_rng(21)
    shape = eng.calib_shapes(0)["ratio_est"]
    plain = {b: _run(eng, 0, SEED, 5, 3, code, fx, word, branch=b) for b in BRANCHES}
    fx4 = make_fixed(4, 4, 6, scale=0.5, alpha_num=3, alpha_shift=2, beta=0)
    try:
        eng.set_llr_scale(0, 10.0 ** rng.uniform(-1, 2, shape))
        got = _run(eng, 0, SEED, 5, 3, code, fx, word)
        _same(got, _twin_counts(eng, 0, 5, 3, code, fx, word, "exact", "mmse"))
        assert not np.array_equal(got["bit_err"], plain["mmse"]["bit_err"])
        _same(_run(eng, 0, SEED, 5, 3, code, fx4, word), _twin_counts(eng, 0, 5, 3, code, fx4, word, "exact", "mmse"))
        _same(_run(eng, 0, SEED, 5, 3, code, fx, word, branch="perfect"), plain["perfect"])
        eng.set_llr_scale_perf(0, 10.0 ** rng.uniform(-1, 2, shape))
        gotp = _run(eng, 0, SEED, 5, 3, code, fx, word, branch="perfect")
        _same(gotp, _twin_counts(eng, 0, 5, 3, code, fx, word, "exact", "perfect"))
        assert not np.array_equal(gotp["bit_err"], plain["perfect"]["bit_err"])
    finally:
        eng.set_llr_scale(0)
        eng.set_llr_scale_perf(0)
    _same(_run(eng, 0, SEED, 5, 3, code, fx, word), plain["mmse"])


def test_run_ldpc_fixed_geometry(fixed_ofdm):
    """Realisations [0, 130) with the 200-variable code and its codeword: batch 128, snr_chunk 1, export_stage_mb 1
    and the split [0, 64) + [64, 130) added into the same arrays give the counts of batch 64, exactly; those are the
    twin's.  The full-size code over the same geometries, three realisations."""
    S, eng, code, word, small, sword, fx = fixed_ofdm
    eng.set_batch(64)
    ref = _run(eng, 0, SEED, 0, 130, small, fx, sword, method="maxlog")
    assert ref["bit_err"].sum() > 0 and (ref["frame_err"] <= 130).all() and (ref["frame_err"] < 130).any()
    _same(ref, _twin_counts(eng, 0, 0, 130, small, fx, sword, "maxlog", "mmse"))
    try:
        eng.set_batch(128)
        _same(_run(eng, 0, SEED, 0, 130, small, fx, sword, method="maxlog"), ref)
        eng.set_option("export_stage_mb", 1)
        _same(_run(eng, 0, SEED, 0, 130, small, fx, sword, method="maxlog"), ref)
        eng.set_option("export_stage_mb", 1024)
        eng.set_option("snr_chunk", 1)
        _same(_run(eng, 0, SEED, 0, 130, small, fx, sword, method="maxlog"), ref)
    finally:
        eng.set_option("export_stage_mb", 1024)
        eng.set_option("snr_chunk", 0)
        eng.set_batch(64)
    a = _run(eng, 0, SEED, 0, 64, small, fx, sword, method="maxlog")
    _same(_run(eng, 0, SEED, 64, 66, small, fx, sword, method="maxlog", into=a), ref)
    full = _run(eng, 0, SEED, 5, 3, code, fx, word)
    try:
        eng.set_batch(128)
        eng.set_option("snr_chunk", 1)
        eng.set_option("export_stage_mb", 1)
        _same(_run(eng, 0, SEED, 5, 3, code, fx, word), full)
    finally:
        eng.set_option("export_stage_mb", 1024)
        eng.set_option("snr_chunk", 0)
        eng.set_batch(64)
    _same(_run(eng, 0, SEED, 6, 2, code, fx, word, into=_run(eng, 0, SEED, 5, 1, code, fx, word)), full)


def test_run_ldpc_fixed_repeatability_and_side_effects(fixed_ofdm):
    """A second call doubles the arrays, n_rep = 0 adds nothing, a field subset leaves the rest untouched, the
    decoder is timed under its names, and dsce_run's counters, path_info, dsce_run_ldpc and dsce_run_ldpc_layered
    keep their bits around fixed calls."""
    from dsce.coding import make_layers
    S, eng, code, word, small, sword, fx = fixed_ofdm
    eng.set_batch(64)
    counts = eng.run(SEED, 0, 64)
    path = eng.path_info(0)
    flood = _run_fp64(eng, 0, SEED, 5, 70, small)
    layers = make_layers(small)
    layered = eng.run_ldpc(0, SEED, 5, 70, small, layers=layers)
    ref = _run(eng, 0, SEED, 5, 70, small, fx, sword)
    twice = _run(eng, 0, SEED, 5, 70, small, fx, sword, into=ref)
    for f in ALL:
        assert np.array_equal(twice[f], 2 * ref[f]) and ref[f].sum() > 0, f
    start = {f: np.full_like(ref[f], 7) for f in ALL}
    _same(_run(eng, 0, SEED, 5, 0, small, fx, sword, into=start), start)          # n_rep = 0 adds nothing
    for fields in (("bit_err",), ("frame_err",), ("iter_sum",), ("bit_err", "iter_sum")):
        one = _run(eng, 0, SEED, 5, 70, small, fx, sword, fields=fields)
        assert sorted(one) == sorted(fields)
        for f in fields:
            assert np.array_equal(one[f], ref[f]), f
    w = eng.run_ldpc(0, SEED, 5, 70, small, fixed=fx, codeword=sword)
    _same(w, ref)
    w2 = eng.run_ldpc(0, SEED, 5, 70, small, fixed=fx, codeword=sword, out={"iter_sum": w["iter_sum"]})
    assert list(w2) == ["iter_sum"] and np.array_equal(w2["iter_sum"], 2 * ref["iter_sum"])
    eng.enable_timing(True)
    try:
        _run(eng, 0, SEED, 5, 70, small, fx, sword)
        n, ms = eng.kernel_time("k_ldpc_fixed")
        assert n >= 1 and ms > 0
        _ldpc(eng, np.zeros((2, small.n_slots)), small, fx)
        n, ms = eng.kernel_time("k_ldpc_fixed_probe")
        assert n >= 1 and ms > 0
    finally:
        eng.enable_timing(False)
    assert eng.path_info(0) == path
    assert np.array_equal(eng.run(SEED, 0, 64), counts) and eng.path_info(0) == path and counts.sum() > 0
    _same(_run_fp64(eng, 0, SEED, 5, 70, small), flood)
    _same(eng.run_ldpc(0, SEED, 5, 70, small, layers=layers), layered)


@pytest.fixture(scope="module")
def code200():
    from dsce.coding import make_ldpc
    return make_ldpc(200, "1/2")


FX_BAD = ((dict(scale=0.0), "scale"), (dict(scale=-2.0), "scale"), (dict(scale=float("nan")), "scale"),
          (dict(scale=float("inf")), "scale"), (dict(q_ch=1), "q_ch"), (dict(q_ch=17), "q_ch"), (dict(q_msg=1), "q_msg"),
          (dict(q_msg=17), "q_msg"), (dict(q_app=5), "q_app"), (dict(q_app=17), "q_app"), (dict(q_ch=8, q_app=7), "q_app"),
          (dict(alpha_shift=-1), "alpha_shift"), (dict(alpha_shift=9), "alpha_shift"), (dict(alpha_num=0), "alpha_num"),
          (dict(alpha_num=2), "alpha_num"), (dict(alpha_num=5, alpha_shift=2), "alpha_num"), (dict(beta=-1), "beta"),
          (dict(beta=32768), "beta"))


def test_ldpc_fixed_errors(bare, code200):
    """Every refusal through dsce_ldpc_fixed: DSCE_EINVAL, the offender named, nothing written, and the context
    decodes afterwards."""
    from dsce.coding import ldpc_decode_fixed, ldpc_from_rows, make_fixed
    code, fx = code200, make_fixed()
    lam = np.random.default_rng(1).standard_normal((2, 200))
    ref = ldpc_decode_fixed(lam, code, fx)
    out = np.zeros((2, 200), dtype=np.uint8)
    its = np.zeros(2, dtype=np.int32)
    app = np.zeros((2, 200), dtype=np.int16)
    lp, op, ip, ap = (lam.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_uint8)),
                      its.ctypes.data_as(C.POINTER(C.c_int32)), app.ctypes.data_as(C.POINTER(C.c_int16)))

    def works():
        for g, r in zip(_ldpc(bare, lam, code, fx), ref):
            assert np.array_equal(g, r)

    def rc(c=code, f=fx, n_slots=200, l=lp, n=2, o=op, null=None, word=None):
        desc, keep = _desc(c)
        if null:
            setattr(desc, null, None)
        fd = C.byref(_fx(f)) if f is not None else None
        r = bare.lib.dsce_ldpc_fixed(bare.h, C.byref(desc), fd, n_slots, l, n, o, ip, ap)
        assert not out.any() and not its.any() and not app.any()
        if word:
            msg = bare.lib.dsce_last_error(bare.h).decode()
            assert word in msg and "dsce_ldpc_fixed" in msg, msg
        works()
        return r

    works()
    assert bare.lib.dsce_ldpc_fixed(bare.h, None, C.byref(_fx(fx)), 200, lp, 2, op, ip, ap) == EINVAL     # null code
    assert rc(f=None, word="null fx") == EINVAL
    for kw, word in FX_BAD:
        assert rc(f=fx._replace(**kw), word=word) == EINVAL, kw
    for f in ("row_ptr", "col", "slot"):
        assert rc(null=f, word="null") == EINVAL
    rp, col, slot = code.row_ptr, code.col, code.slot

    def edit(a, i, v):
        b = a.copy()
        b[i] = v
        return b

    bad = [(code._replace(max_iter=0), "max_iter"), (code._replace(max_iter=101), "max_iter"),
           (code._replace(alpha=0.0), "alpha"), (code._replace(alpha=1.25), "alpha"),
           (code._replace(alpha=float("nan")), "alpha"), (code._replace(early_stop=2), "early_stop"),
           (code._replace(n_info=0), "n_info"), (code._replace(n_info=201), "n_info"),
           (code._replace(row_ptr=edit(rp, 0, 1)), "row_ptr"), (code._replace(row_ptr=edit(rp, 3, rp[2])), "row_ptr"),
           (code._replace(row_ptr=edit(rp, 3, rp[2] + 1)), "degree"),
           (code._replace(col=edit(col, 7, 200)), "col"), (code._replace(col=edit(col, 7, -1)), "col"),
           (code._replace(col=edit(col, rp[4] + 1, col[rp[4]])), "ascending"),
           (code._replace(slot=edit(slot, 9, 200)), "slot"), (code._replace(slot=edit(slot, 9, -2)), "slot"),
           (ldpc_from_rows([list(range(33)), [0, 1]], 200, 100), "degree")]
    for c, word in bad:
        assert rc(c=c, word=word) == EINVAL, word
    for f in ("n_vars", "n_checks"):
        desc, keep = _desc(code)
        setattr(desc, f, 0)
        assert bare.lib.dsce_ldpc_fixed(bare.h, C.byref(desc), C.byref(_fx(fx)), 200, lp, 2, op, ip, ap) == EINVAL
        assert f in bare.lib.dsce_last_error(bare.h).decode()
    assert rc(l=None) == EINVAL and rc(o=None) == EINVAL                         # null data with n_cw > 0
    assert rc(n=-1, word="n_cw") == EINVAL
    assert rc(n_slots=-1, word="n_slots") == EINVAL
    assert rc(n_slots=199, word="slot") == EINVAL
    assert rc(n=0, l=None, o=None) == 0                                          # n_cw = 0 does nothing
    with pytest.raises(ValueError, match="fixed and layers"):
        from dsce.coding import make_layers
        bare.ldpc(lam, code, layers=make_layers(code), fixed=fx)


def test_ldpc_fixed_lds_limit(bare, code200):
    """Option lds_max lowered to 1024: the 200-variable code is refused with the bytes of ldpc_fixed_lds_bytes
    (1808, where the fp64 kernel needs 4008) and the limit in the message and nothing launched; it decodes with
    exactly enough and again once the option is restored."""
    from dsce import engine
    from dsce.coding import ldpc_decode_fixed, ldpc_fixed_lds_bytes, make_fixed
    code, fx = code200, make_fixed()
    need = ldpc_fixed_lds_bytes(code.n_vars, code.n_checks)
    lam = np.random.default_rng(2).standard_normal((3, 200))
    ref = ldpc_decode_fixed(lam, code, fx)
    limit = bare.get_option("lds_max")
    assert limit >= 64 * 1024 and need == 1808

    def works():
        for g, r in zip(_ldpc(bare, lam, code, fx), ref):
            assert np.array_equal(g, r)

    try:
        bare.set_option("lds_max", 1024)
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL) as e:
            _ldpc(bare, lam, code, fx)
        assert str(need) in str(e.value) and "1024" in str(e.value) and "lds_max" in str(e.value), e.value
        assert "k_ldpc_fixed" in str(e.value)
        bare.set_option("lds_max", need)                                          # exactly enough, less than k_ldpc's
        works()
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL):
            _ldpc_fp64(bare, lam, code)
        bare.set_option("lds_max", need - 1)
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL):
            _ldpc(bare, lam, code, fx)
    finally:
        bare.set_option("lds_max", limit)
    works()


def test_run_ldpc_fixed_errors(fixed_ofdm):
    from dsce import engine
    S, eng, code, word, small, sword, fx = fixed_ofdm
    eng.set_batch(64)
    ref = _run(eng, 0, SEED, 5, 3, small, fx, sword)
    B = code.n_slots

    def fails(err, c=small, f=fx, w=sword, word=None, **k):
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % err) as e:
            _run(eng, 0, SEED, 5, 3, c, f, w, **k)                               # asserts that nothing was written
        if word:
            assert word in str(e.value), e.value
        _same(_run(eng, 0, SEED, 5, 3, small, fx, sword), ref)                   # the context still works

    def edit(a, i, v):
        b = a.copy()
        b[i] = v
        return b

    fails(EINVAL, fields=())                                                    # no field requested
    for flags in (1 << 3, engine.EXPORT_F32, engine.EXPORT_DEVICE, engine.EXPORT_DEVICE | engine.LLR_MAXLOG):
        fails(EINVAL, flags=flags)
    fails(EINVAL, f=None, word="null fx")
    for kw, w in FX_BAD:
        fails(EINVAL, f=fx._replace(**kw), word=w)
    # a word that is not a codeword: parity bit 7 flipped leaves check 7 the first unsatisfied; an entry of 2
    fails(EINVAL, w=edit(sword, small.n_info + 7, sword[small.n_info + 7] ^ 1), word="check 7")
    fails(EINVAL, w=edit(sword, 0, sword[0] ^ 1), word="codeword")
    fails(EINVAL, w=edit(sword, 5, 2), word="entry 5")
    rp, col, slot = small.row_ptr, small.col, small.slot
    for c, w in ((small._replace(slot=edit(slot, 11, B)), "slot"), (small._replace(slot=edit(slot, 11, -2)), "slot"),
                 (small._replace(col=edit(col, 7, 200)), "col"),
                 (small._replace(col=edit(col, rp[4] + 1, col[rp[4]])), "ascending"),
                 (small._replace(row_ptr=edit(rp, 0, 1)), "row_ptr"), (small._replace(row_ptr=edit(rp, 3, rp[2])), "row_ptr"),
                 (small._replace(max_iter=0), "max_iter"), (small._replace(max_iter=101), "max_iter"),
                 (small._replace(alpha=0.0), "alpha"), (small._replace(alpha=1.5), "alpha"),
                 (small._replace(early_stop=-1), "early_stop"),
                 (small._replace(n_info=0), "n_info"), (small._replace(n_info=201), "n_info")):
        fails(EINVAL, c=c, w=None, word=w)
    buf = np.zeros(eng.ldpc_shapes(0)["bit_err"], dtype=np.int64)
    o = engine.LdpcOut(bit_err=buf.ctypes.data_as(C.POINTER(C.c_int64)))
    desc, keep = _desc(small)
    fd = _fx(fx)
    tables = []
    for f in ("row_ptr", "col", "slot"):
        d, k2 = _desc(small)
        setattr(d, f, None)
        tables.append(d)
    for f in ("n_vars", "n_checks"):
        d, k3 = _desc(small)
        setattr(d, f, 0)
        tables.append(d)
    for d, oo in [(None, C.byref(o)), (C.byref(desc), None)] + [(C.byref(d), C.byref(o)) for d in tables]:
        assert eng.lib.dsce_run_ldpc_fixed(eng.h, 0, SEED, 5, 3, 0, d, C.byref(fd), None, oo) == EINVAL
    assert not buf.any()
    # the LDS limit: the bytes of ldpc_fixed_lds_bytes and the limit; restored afterwards
    limit = eng.get_option("lds_max")
    try:
        eng.set_option("lds_max", 1024)
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL) as e:
            _run(eng, 0, SEED, 5, 3, small, fx, sword)
        assert "1808" in str(e.value) and "1024" in str(e.value), e.value
    finally:
        eng.set_option("lds_max", limit)
    _same(_run(eng, 0, SEED, 5, 3, small, fx, sword), ref)
    with pytest.raises(ValueError, match="fixed and layers"):
        from dsce.coding import make_layers
        eng.run_ldpc(0, SEED, 5, 3, small, layers=make_layers(small), fixed=fx)
    # without dsce_build_mmse; after it the same context works
    nommse = harness.engine(S, batch=64, mmse=False)
    try:
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % ESTATE):
            _run(nommse, 0, SEED, 5, 3, small, fx, sword)
        nommse.build_mmse(S.zero_threshold)
        _same(_run(nommse, 0, SEED, 5, 3, small, fx, sword), ref)
    finally:
        nommse.close()
    empty = engine.Engine(0)
    try:
        assert empty.lib.dsce_run_ldpc_fixed(empty.h, 0, SEED, 0, 1, 0, C.byref(desc), C.byref(fd), None, C.byref(o)) == ESTATE
        assert not buf.any()
    finally:
        empty.close()


def test_simulate_ldpc_fixed(tmp_path):
    """python -m dsce.simulate --ldpc 3/4 --ldpc-fixed 6,6,8 --ldpc-scale 2 (a child process: the command line is
    what is tested): the fixed results beside the fp64 ones are Engine.run_ldpc(fixed=, codeword=) on the same
    realisations with the codeword of --ldpc-seed, both branches."""
    import json
    import os
    import subprocess
    import sys

    from dsce.coding import ldpc_encode, make_fixed, make_ldpc
    from dsce.configs import build_setup
    from dsce.engine import build_engine, gpu_tx
    out = tmp_path / "ldpc.json"
    env = dict(os.environ, PYTHONPATH=harness.PKG)
    p = subprocess.run([sys.executable, "-m", "dsce.simulate", "--config", "default", "--schemes", "ofdm", "--reps", "3",
                        "--batch", "64", "--ldpc", "3/4", "--ldpc-iters", "20", "--ldpc-seed", "9", "--ldpc-fixed", "6,6,8",
                        "--ldpc-scale", "2", "--ldpc-offset", "0", "--ldpc-alpha-q", "3/2^2", "--out", str(out)],
                       cwd=harness.PKG, env=env, timeout=240, capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    res = json.loads(out.read_text())
    r = res["ldpc"]["ofdm"]
    fr = r["fixed"]
    assert (fr["q_ch"], fr["q_msg"], fr["q_app"], fr["scale"], fr["alpha_num"], fr["alpha_shift"], fr["beta"]) == (6, 6, 8, 2.0, 3, 2, 0)
    assert fr["clip"] == 15.5 and r["schedule"] == "flooding"
    S = build_setup("default", schemes=("ofdm",), tx=gpu_tx(0))
    eng = build_engine(S, batch=64)
    try:
        code = make_ldpc(2560, "3/4", seed=9, max_iter=20)
        fx = make_fixed(6, 6, 8, scale=2.0, alpha_num=3, alpha_shift=2, beta=0)
        word = ldpc_encode(np.random.RandomState(9).randint(0, 2, code.n_info), code)
        for key, branch in (("mmse", "mmse"), ("perfect_ic", "perfect")):
            c = eng.run_ldpc(0, res["seed"], 0, 3, code, branch=branch, fixed=fx, codeword=word)
            assert np.array_equal(np.asarray(fr[key]["ber"]), c["bit_err"] / (3.0 * 1920)), key
            assert np.array_equal(np.asarray(fr[key]["fer"]), c["frame_err"] / 3.0), key
            assert np.array_equal(np.asarray(fr[key]["mean_iter"]), c["iter_sum"] / 3.0), key
            c0 = eng.run_ldpc(0, res["seed"], 0, 3, code, branch=branch)
            assert np.array_equal(np.asarray(r[key]["ber"]), c0["bit_err"] / (3.0 * 1920)), key
    finally:
        eng.close()
