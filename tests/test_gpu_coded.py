"""GPU: dsce_viterbi and dsce_run_coded (k_viterbi, DSCE_HAS_CODED_RUN) — the
K = 7 Viterbi decoder on the device against its NumPy twin
dsce.coding.viterbi_decode, equal to the bit: on drawn decoder inputs, ties
included; on the engine's own export_llr output (fp64) and export's sym for both
LLR methods, both CSI branches and installed scale tables; and against itself
across batch geometries, SNR chunks, staging bounds and split calls.  Every
comparison is exact: the counts are integers and the twin performs the fp64
operations of include/dsce.h in the same order.  Host outputs sit between guard
regions.  tests/test_gpu_coded_ml.py holds the checks against references other
than the twin."""
import ctypes as C

import numpy as np
import pytest

import harness
from test_coding_host import ORACLE_COUNTS
from test_gpu_export import EINVAL, ESTATE, GUARD, PATTERN, SEED, SNR, _export

pytestmark = pytest.mark.gpu

BOTH = ("bit_err", "frame_err")
METHODS = ("exact", "maxlog")
BRANCHES = ("mmse", "perfect")


def _desc(src, terminated):
    from dsce import engine
    src = np.ascontiguousarray(src, dtype=np.int32)
    return engine.CodeDesc(src.shape[0], int(terminated), src.ctypes.data_as(C.POINTER(C.c_int32))), src


def _viterbi(eng, lam, src, terminated):
    """dsce_viterbi into a uint8 array between two guard regions."""
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    n, T = lam.shape[0], np.asarray(src).shape[0]
    raw = np.full(n * T + 2 * GUARD, PATTERN, dtype=np.uint8)
    desc, keep = _desc(src, terminated)
    eng._chk(eng.lib.dsce_viterbi(eng.h, C.byref(desc), lam.shape[1], lam.ctypes.data_as(C.POINTER(C.c_double)), n,
                                  raw[GUARD:].ctypes.data_as(C.POINTER(C.c_uint8))), "dsce_viterbi")
    assert (raw[:GUARD] == PATTERN).all() and (raw[-GUARD:] == PATTERN).all(), "bytes outside info_out were written"
    return raw[GUARD:GUARD + n * T].reshape(n, T).copy()


def _coded(eng, sid, seed, first, n, code, fields=BOTH, method="exact", branch="mmse", flags=None, into=None):
    """dsce_run_coded into zeroed int64 arrays (or copies of `into`) that share one
    buffer, guard | bit_err | guard | frame_err | guard; only `fields` are passed.
    Asserts that the guards and the field not requested keep their bytes."""
    from dsce import engine
    shapes = eng.coded_shapes(sid)
    raw = np.full(3 * GUARD + sum(int(np.prod(shapes[f])) * 8 for f in BOTH), PATTERN, dtype=np.uint8)
    view, at = {}, GUARD
    for f in BOTH:
        nb = int(np.prod(shapes[f])) * 8
        view[f] = raw[at:at + nb].view(np.int64).reshape(shapes[f])
        at += nb + GUARD
    for f in fields:
        view[f][...] = 0 if into is None else into[f]
    before = raw.copy()
    o = engine.CodedOut(**{f: view[f].ctypes.data_as(C.POINTER(C.c_int64)) for f in fields})
    if flags is None:
        flags = engine.LLR_METHODS[method] | engine.LLR_BRANCHES[branch]
    desc, keep = _desc(code.src, code.terminated)
    eng._chk(eng.lib.dsce_run_coded(eng.h, sid, seed, first, n, flags, C.byref(desc), C.byref(o)), "dsce_run_coded")
    mask = np.ones(raw.size, dtype=bool)
    for f in fields:
        a0 = view[f].ctypes.data - raw.ctypes.data
        mask[a0:a0 + view[f].nbytes] = False
    assert np.array_equal(raw[mask], before[mask]), "bytes outside the requested fields were written"
    return {f: view[f].copy() for f in fields}


def _same(a, b):
    assert sorted(a) == sorted(b)
    for f in a:
        assert np.array_equal(a[f], b[f]), (f, a[f], b[f])


def _twin_counts(eng, sid, first, n, code, method, branch):
    from dsce.coding import coded_counts
    llr = eng.export_llr(sid, SEED, first, n, fields=("llr",), method=method, branch=branch)["llr"]
    sym = _export(eng, sid, SEED, first, n, fields=("sym",))["sym"]
    assert llr.dtype == np.float64 and np.isfinite(llr).all()
    return coded_counts(llr, sym, code)


@pytest.fixture(scope="module")
def bare():
    """A context with nothing set: dsce_viterbi needs no more."""
    from dsce import engine
    eng = engine.Engine(0)
    yield eng
    eng.close()


def _tables(T, terminated):
    """identity rate 1/2, and punctured 3/4 over an interleaver, each of exactly T steps"""
    from dsce.coding import Code, PUNCTURE, info_bits, make_code
    ident = np.arange(2 * T, dtype=np.int32).reshape(T, 2)
    yield Code(ident, terminated, 2 * T, "1/2", T, info_bits(T, terminated), 2 * T)
    mask = PUNCTURE["3/4"]
    kept = sum(sum(mask[t % 3]) for t in range(T))
    c = make_code(kept, "3/4", terminated=terminated, interleaver=5)
    assert c.n_steps == T and (c.src < 0).any() == (T > 1)
    yield c


@pytest.mark.parametrize("T", [7, 8, 31, 32, 33, 64, 65, 200])
def test_viterbi_against_the_twin(bare, T):
    """dsce_viterbi == viterbi_decode for 1, 3 and 65 codewords (one wave, a partly
    filled block, more than one block), step counts around the 32-step operand
    groups and the 64-step traceback chunks, both terminations, an identity and a
    punctured, interleaved table, and four kinds of input: normal, normal x 1e8
    (no renormalisation), all zero, and integers from {-1, 0, 1}, which tie at
    almost every step: the tie rule, the lane order and the traceback start."""
    from dsce.coding import viterbi_decode
    rng = np.random.default_rng(100 + T)
    ones = 0
    for terminated in (True, False):
        for code in _tables(T, terminated):
            for n in (1, 3, 65):
                base = rng.standard_normal((n, code.n_slots))
                for kind, lam in (("normal", base), ("large", base * 1e8), ("zero", np.zeros_like(base)),
                                  ("ties", rng.integers(-1, 2, base.shape).astype(np.float64))):
                    got = _viterbi(bare, lam, code.src, terminated)
                    ref = viterbi_decode(lam, code.src, terminated)
                    assert got.dtype == np.uint8 and got.max() <= 1
                    assert np.array_equal(got, ref), (terminated, code.rate, n, kind, np.argwhere(got != ref)[:4])
                    if kind == "zero":
                        assert not got.any()
                    ones += int(got.sum())
                # the Python wrapper, one codeword without the leading axis too
                assert np.array_equal(bare.viterbi(base, code), viterbi_decode(base, code.src, terminated))
                assert np.array_equal(bare.viterbi(base[0], code), viterbi_decode(base[0], code.src, terminated))
    assert ones > 0


def test_viterbi_decodes_any_codeword(bare):
    """Nothing is descrambled: a noiseless random codeword comes back, at the
    largest step count (8192: the whole 64 KiB of decision words, one wave per
    block) and at 2049 (three waves per block)."""
    from dsce.coding import Code, code_lam, conv_encode, info_bits
    rng = np.random.default_rng(8)
    for T, n in ((8192, 2), (2049, 7)):
        src = np.arange(2 * T, dtype=np.int32).reshape(T, 2)
        u = rng.integers(0, 2, (n, T)).astype(np.uint8)
        u[:, T - 6:] = 0
        lam = code_lam(conv_encode(u), src, 2 * T, 2.5)
        assert np.array_equal(_viterbi(bare, lam, src, True), u)
        assert np.array_equal(bare.viterbi(lam, Code(src, True, 2 * T, "1/2", T, info_bits(T, True), 2 * T)), u)


def test_viterbi_errors(bare):
    from dsce import engine
    T = 16
    src = np.arange(2 * T, dtype=np.int32).reshape(T, 2)
    lam = np.random.default_rng(1).standard_normal((2, 2 * T))
    out = np.zeros((2, T), dtype=np.uint8)
    lp, op = lam.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_uint8))
    sp = src.ctypes.data_as(C.POINTER(C.c_int32))
    ref = _viterbi(bare, lam, src, True)

    def rc(desc, n_slots=2 * T, l=lp, n=2, o=op):
        r = bare.lib.dsce_viterbi(bare.h, None if desc is None else C.byref(desc), n_slots, l, n, o)
        assert not out.any()
        assert np.array_equal(_viterbi(bare, lam, src, True), ref)              # the context still works
        return r

    assert rc(None) == EINVAL                                                   # null code
    assert rc(engine.CodeDesc(T, 1, None)) == EINVAL                            # null src
    assert rc(engine.CodeDesc(0, 0, sp)) == EINVAL                              # n_steps < 1
    assert rc(engine.CodeDesc(6, 1, sp)) == EINVAL                              # terminated with n_steps < 7
    big = np.zeros((8193, 2), dtype=np.int32)
    assert rc(engine.CodeDesc(8193, 1, big.ctypes.data_as(C.POINTER(C.c_int32))), n_slots=4) == EINVAL
    for bad in (-2, 2 * T):                                                     # a src entry outside [-1, n_slots)
        s2 = src.copy()
        s2[5, 1] = bad
        assert rc(engine.CodeDesc(T, 1, s2.ctypes.data_as(C.POINTER(C.c_int32)))) == EINVAL
    good = engine.CodeDesc(T, 1, sp)
    assert rc(good, l=None) == EINVAL and rc(good, o=None) == EINVAL            # null data with n_cw > 0
    assert rc(good, n=-1) == EINVAL
    assert rc(good, n_slots=-1) == EINVAL
    assert rc(good, n=0, l=None, o=None) == 0                                   # n_cw = 0 does nothing
    # unterminated: any n_steps >= 1 is a code
    assert bare.lib.dsce_viterbi(bare.h, C.byref(engine.CodeDesc(6, 0, sp)), 2 * T, lp, 2, op) == 0
    assert not out.reshape(-1)[12:].any()


@pytest.mark.parametrize("name", ["ofdm", "fbmc_aux", "fbmc_cod"])
def test_run_coded_against_the_twin(name):
    """Default setup, n_iter 4, SNR (10, 35), batch 64, realisations 5..7: the
    counts of both methods, both branches and rates 1/2 and 3/4 equal the twin on
    export_llr's fp64 LLRs and export's sym, exactly.  For ofdm, max-log, MMSE
    branch they are also the counts recorded from the oracle's LLRs
    (test_coding_host.ORACLE_COUNTS)."""
    from dsce.coding import make_code
    S = harness.setup("default", schemes=(name,), snr_db=SNR, n_iter=4)
    sc = S.schemes[name]
    B = sc["n_data"] * sc["bits_per_symbol"]
    eng = harness.engine(S, batch=64)
    try:
        seen = set()
        for rate in ("1/2", "3/4"):
            code = make_code(B, rate, interleaver=7)
            for method in METHODS:
                for branch in BRANCHES:
                    got = _coded(eng, 0, SEED, 5, 3, code, method=method, branch=branch)
                    ref = _twin_counts(eng, 0, 5, 3, code, method, branch)
                    print("coded %s %s %s %s bit_err %s frame_err %s" % (name, rate, method, branch,
                                                                         got["bit_err"].tolist(), got["frame_err"].tolist()))
                    assert got["bit_err"].shape == (len(SNR), S.n_iter + 1) and got["bit_err"].dtype == np.int64
                    _same(got, ref)
                    assert (got["frame_err"] <= 3).all() and ((got["bit_err"] > 0) == (got["frame_err"] > 0)).all()
                    seen.update(got["frame_err"].ravel().tolist())
                    if name == "ofdm" and method == "maxlog" and branch == "mmse":
                        for f in BOTH:
                            assert got[f].tolist() == ORACLE_COUNTS[rate][f], (rate, f, got[f])
        if name == "ofdm":
            assert {0, 3} <= seen                                               # cells with no and with total failure
    finally:
        eng.close()


@pytest.fixture(scope="module")
def coded_ofdm():
    from dsce.coding import make_code
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR, n_iter=4)
    eng = harness.engine(S, batch=64)
    sc = S.schemes["ofdm"]
    yield S, eng, make_code(sc["n_data"] * sc["bits_per_symbol"], "3/4", interleaver=7)
    eng.close()


def test_run_coded_with_scale_tables(coded_ofdm):
    """Random tables g = 10**uniform(-1, 2): g_est on the MMSE branch, then g_perf
    with the flag; the counts equal the twin on the scaled export, and the tables
    change them."""
    S, eng, code = coded_ofdm
    eng.set_batch(64)
    rng = np.random.default_rng(21)
    shape = eng.calib_shapes(0)["ratio_est"]
    plain = {b: _coded(eng, 0, SEED, 5, 3, code, branch=b) for b in BRANCHES}
    try:
        eng.set_llr_scale(0, 10.0 ** rng.uniform(-1, 2, shape))
        got = _coded(eng, 0, SEED, 5, 3, code)
        _same(got, _twin_counts(eng, 0, 5, 3, code, "exact", "mmse"))
        assert not np.array_equal(got["bit_err"], plain["mmse"]["bit_err"])
        _same(_coded(eng, 0, SEED, 5, 3, code, branch="perfect"), plain["perfect"])      # g_est does not touch it
        eng.set_llr_scale_perf(0, 10.0 ** rng.uniform(-1, 2, shape))
        gotp = _coded(eng, 0, SEED, 5, 3, code, branch="perfect")
        _same(gotp, _twin_counts(eng, 0, 5, 3, code, "exact", "perfect"))
        assert not np.array_equal(gotp["bit_err"], plain["perfect"]["bit_err"])
    finally:
        eng.set_llr_scale(0)
        eng.set_llr_scale_perf(0)
    _same(_coded(eng, 0, SEED, 5, 3, code), plain["mmse"])


def test_run_coded_invariance(coded_ofdm):
    """Realisations [0, 130): batch 128, snr_chunk 1, export_stage_mb 1 (one-wave
    sub-batches) and the split [0, 64) + [64, 130) added into the same arrays give
    the counts of batch 64, exactly."""
    S, eng, code = coded_ofdm
    eng.set_batch(64)
    ref = _coded(eng, 0, SEED, 0, 130, code, method="maxlog")
    assert ref["bit_err"].sum() > 0 and (ref["frame_err"] <= 130).all()
    try:
        eng.set_batch(128)
        _same(_coded(eng, 0, SEED, 0, 130, code, method="maxlog"), ref)
        eng.set_option("export_stage_mb", 1)
        _same(_coded(eng, 0, SEED, 0, 130, code, method="maxlog"), ref)
        eng.set_option("export_stage_mb", 1024)
        eng.set_option("snr_chunk", 1)
        _same(_coded(eng, 0, SEED, 0, 130, code, method="maxlog"), ref)
    finally:
        eng.set_option("export_stage_mb", 1024)
        eng.set_option("snr_chunk", 0)
        eng.set_batch(64)
    a = _coded(eng, 0, SEED, 0, 64, code, method="maxlog")
    _same(_coded(eng, 0, SEED, 64, 66, code, method="maxlog", into=a), ref)


def test_run_coded_repeatability_and_side_effects(coded_ofdm):
    S, eng, code = coded_ofdm
    eng.set_batch(64)
    counts = eng.run(SEED, 0, 64)
    path = eng.path_info(0)
    soft = eng.run_soft(0, SEED, 5, 70)
    ref = _coded(eng, 0, SEED, 5, 70, code)
    twice = _coded(eng, 0, SEED, 5, 70, code, into=ref)
    for f in BOTH:
        assert np.array_equal(twice[f], 2 * ref[f]) and ref[f].sum() > 0, f
    start = {f: np.full_like(ref[f], 7) for f in BOTH}
    _same(_coded(eng, 0, SEED, 5, 0, code, into=start), start)                  # n_rep = 0 adds nothing
    for f in BOTH:                                                              # one field: the other's memory is left alone
        one = _coded(eng, 0, SEED, 5, 70, code, fields=(f,))
        assert list(one) == [f] and np.array_equal(one[f], ref[f]), f
    # the Python wrapper: from zero, and adding into `out`
    w = eng.run_coded(0, SEED, 5, 70, code)
    _same(w, ref)
    w2 = eng.run_coded(0, SEED, 5, 70, code, out={"bit_err": w["bit_err"]})
    assert list(w2) == ["bit_err"] and np.array_equal(w2["bit_err"], 2 * ref["bit_err"])
    # the decoder is timed as k_viterbi
    eng.enable_timing(True)
    try:
        _coded(eng, 0, SEED, 5, 70, code)
        n, ms = eng.kernel_time("k_viterbi")
        assert n >= 1 and ms > 0
    finally:
        eng.enable_timing(False)
    # no side effects
    assert eng.path_info(0) == path
    assert np.array_equal(eng.run(SEED, 0, 64), counts) and eng.path_info(0) == path and counts.sum() > 0
    after = eng.run_soft(0, SEED, 5, 70)
    for f in soft:
        assert np.array_equal(after[f], soft[f]), f


def test_simulate_coded(tmp_path):
    """python -m dsce.simulate --coded 3/4 (a child process: the command line is
    what is tested): its ber / fer are Engine.run_coded on the same realisations,
    both branches."""
    import json
    import os
    import subprocess
    import sys

    from dsce.coding import make_code
    from dsce.configs import build_setup
    from dsce.engine import build_engine, gpu_tx
    out = tmp_path / "coded.json"
    env = dict(os.environ, PYTHONPATH=harness.PKG)
    p = subprocess.run([sys.executable, "-m", "dsce.simulate", "--config", "default", "--schemes", "ofdm", "--reps", "65",
                        "--batch", "64", "--coded", "3/4", "--coded-interleaver", "9", "--out", str(out)],
                       cwd=harness.PKG, env=env, timeout=240, capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    assert "coded_ber_ic_mmse" in p.stdout
    res = json.loads(out.read_text())
    r = res["coded"]["ofdm"]
    assert (r["rate"], r["info_bits"], r["method"], r["interleaver"]) == ("3/4", 1914, "exact", 9)
    assert res["coded_seconds"] > 0
    S = build_setup("default", schemes=("ofdm",), tx=gpu_tx(0))
    eng = build_engine(S, batch=64)
    try:
        code = make_code(2560, "3/4", interleaver=9)
        for key, branch in (("mmse", "mmse"), ("perfect_ic", "perfect")):
            c = eng.run_coded(0, res["seed"], 0, 65, code, branch=branch)
            assert c["bit_err"].shape == (len(S.snr_db), S.n_iter + 1)
            assert np.array_equal(np.asarray(r[key]["ber"]), c["bit_err"] / (65.0 * 1914)), key
            assert np.array_equal(np.asarray(r[key]["fer"]), c["frame_err"] / 65.0), key
    finally:
        eng.close()


def test_run_coded_errors(coded_ofdm):
    from dsce import engine
    from dsce.coding import Code, make_code
    S, eng, code = coded_ofdm
    eng.set_batch(64)
    ref = _coded(eng, 0, SEED, 5, 3, code)
    B = code.n_slots

    def fails(err, c=code, **k):
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % err):
            _coded(eng, 0, SEED, 5, 3, c, **k)
        _same(_coded(eng, 0, SEED, 5, 3, code), ref)                            # the context still works

    fails(EINVAL, fields=())                                                    # no field requested
    for flags in (1 << 3, engine.EXPORT_F32, engine.EXPORT_DEVICE, engine.EXPORT_DEVICE | engine.LLR_MAXLOG):
        fails(EINVAL, flags=flags)
    for bad in (-2, B):                                                         # a src entry outside [-1, B)
        src = code.src.copy()
        src[11, 0] = bad
        fails(EINVAL, c=code._replace(src=src))
    fails(EINVAL, c=code._replace(src=code.src[:6]))                            # terminated with n_steps < 7
    fails(EINVAL, c=code._replace(src=np.full((8193, 2), -1, dtype=np.int32)))  # n_steps > 8192
    buf = np.zeros(eng.coded_shapes(0)["bit_err"], dtype=np.int64)
    o = engine.CodedOut(bit_err=buf.ctypes.data_as(C.POINTER(C.c_int64)))
    desc, keep = _desc(code.src, True)
    for d, oo in ((None, C.byref(o)), (C.byref(engine.CodeDesc(code.n_steps, 1, None)), C.byref(o)),
                  (C.byref(engine.CodeDesc(0, 0, desc.src)), C.byref(o)), (C.byref(desc), None)):
        assert eng.lib.dsce_run_coded(eng.h, 0, SEED, 5, 3, 0, d, oo) == EINVAL   # null code, null src, n_steps < 1, null out
    assert not buf.any()
    _same(_coded(eng, 0, SEED, 5, 3, code), ref)
    # an unterminated code of 6 steps is accepted
    short = Code(code.src[:6], False, B, "3/4", 6, 6, 0)
    assert (_coded(eng, 0, SEED, 5, 3, short)["bit_err"] <= 18).all()
    # without dsce_build_mmse; after it the same context works
    bare = harness.engine(S, batch=64, mmse=False)
    try:
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % ESTATE):
            _coded(bare, 0, SEED, 5, 3, code)
        bare.build_mmse(S.zero_threshold)
        _same(_coded(bare, 0, SEED, 5, 3, code), ref)
    finally:
        bare.close()
    # before channel, SNR points or scheme are set
    empty = engine.Engine(0)
    try:
        assert empty.lib.dsce_run_coded(empty.h, 0, SEED, 0, 1, 0, C.byref(desc), C.byref(o)) == ESTATE
        assert not buf.any()
    finally:
        empty.close()
    assert make_code(B, "3/4", interleaver=7).n_steps == code.n_steps
