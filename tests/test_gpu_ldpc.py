"""GPU: dsce_ldpc and dsce_run_ldpc (k_ldpc, DSCE_HAS_LDPC_RUN) — the normalised
min-sum decoder on the device against its NumPy twin dsce.coding.ldpc_decode,
equal to the bit, decided bits and iteration counts: on drawn decoder inputs
over codes that sit on the limits of the description (check degrees 2 and 32, a
variable of degree 40, of degree 1 and of degree 0, punctured variables, a slot
used twice), exact zeros and ties included; on the engine's own export_llr
output (fp64) and export's sym for both LLR methods, both CSI branches and
installed scale tables; and against itself across batch geometries, SNR chunks,
staging bounds and split calls.  Every comparison is exact: the counts are
integers and the twin performs the fp64 operations of include/dsce.h in the same
order.  Host outputs sit between guard regions.  tests/test_gpu_ldpc_ref.py
holds the checks against references other than the twin."""
import ctypes as C

import numpy as np
import pytest

import harness
from test_gpu_export import EINVAL, ESTATE, GUARD, PATTERN, SEED, SNR, _export
from test_ldpc_host import ORACLE_LDPC

pytestmark = pytest.mark.gpu

ALL = ("bit_err", "frame_err", "iter_sum")
METHODS = ("exact", "maxlog")
BRANCHES = ("mmse", "perfect")


def _desc(code):
    from dsce import engine
    return engine.Engine._ldpc_desc(code)


def _ldpc(eng, lam, code, iters=True):
    """dsce_ldpc into a uint8 and an int32 array, each between two guard regions."""
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    n, N = lam.shape[0], int(code.n_vars)
    raw = np.full(n * N + 2 * GUARD, PATTERN, dtype=np.uint8)
    rit = np.full(n * 4 + 2 * GUARD, PATTERN, dtype=np.uint8)
    desc, keep = _desc(code)
    ip = rit[GUARD:].ctypes.data_as(C.POINTER(C.c_int32)) if iters else None
    eng._chk(eng.lib.dsce_ldpc(eng.h, C.byref(desc), lam.shape[1], lam.ctypes.data_as(C.POINTER(C.c_double)), n,
                               raw[GUARD:].ctypes.data_as(C.POINTER(C.c_uint8)), ip), "dsce_ldpc")
    assert (raw[:GUARD] == PATTERN).all() and (raw[-GUARD:] == PATTERN).all(), "bytes outside bits_out were written"
    assert (rit[:GUARD] == PATTERN).all() and (rit[-GUARD:] == PATTERN).all(), "bytes outside iters_out were written"
    if not iters:
        assert (rit == PATTERN).all()
    return raw[GUARD:GUARD + n * N].reshape(n, N).copy(), rit[GUARD:GUARD + 4 * n].view(np.int32).copy()


def _run(eng, sid, seed, first, n, code, fields=ALL, method="exact", branch="mmse", flags=None, into=None):
    """dsce_run_ldpc into zeroed int64 arrays (or copies of `into`) that share one
    buffer, guard | bit_err | guard | frame_err | guard | iter_sum | guard; only
    `fields` are passed.  Asserts that the guards and the fields not requested keep
    their bytes."""
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
    try:
        eng._chk(eng.lib.dsce_run_ldpc(eng.h, sid, seed, first, n, flags, C.byref(desc), C.byref(o)), "dsce_run_ldpc")
    except engine.DsceError:
        assert np.array_equal(raw, before), "a refused call wrote"
        raise
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
    from dsce.coding import ldpc_counts
    llr = eng.export_llr(sid, SEED, first, n, fields=("llr",), method=method, branch=branch)["llr"]
    sym = _export(eng, sid, SEED, first, n, fields=("sym",))["sym"]
    assert llr.dtype == np.float64 and np.isfinite(llr).all()
    return ldpc_counts(llr, sym, code)


@pytest.fixture(scope="module")
def bare():
    """A context with nothing set: dsce_ldpc needs no more."""
    from dsce import engine
    eng = engine.Engine(0)
    yield eng
    eng.close()


def limit_code(N, rng):
    """A random code of N variables on the limits of the description: check 0 has
    degree 2, check 1 degree min(32, N - 3); variable 0 is in the first 40 checks
    (all of them if there are fewer), variable N - 2 in check 1 only, variable N - 1 in
    none; two variables are punctured and two share a slot; three slots are unused."""
    from dsce.coding import ldpc_from_rows
    M = max(4, 2 * N // 3)
    pool = np.arange(1, N - 2)
    rows = []
    for c in range(M):
        d = 2 if c == 0 else min(32, N - 3) if c == 1 else int(rng.integers(2, min(6, N - 3) + 1))
        special = ([0] if c < 40 else []) + ([N - 2] if c == 1 else [])
        rows.append(special + [int(v) for v in rng.choice(pool, d - len(special), replace=False)])
    slot = rng.permutation(N + 3)[:N].astype(np.int32)
    slot[3] = slot[5] = -1
    slot[2] = slot[1]
    code = ldpc_from_rows(rows, N, max(1, N // 2), slot=slot, n_slots=N + 3)
    deg = np.diff(code.row_ptr)
    vdeg = np.bincount(code.col, minlength=N)
    assert deg[0] == 2 and deg.max() == min(32, N - 3) and vdeg[0] == min(40, M) and vdeg[N - 2] == 1 and vdeg[N - 1] == 0
    return code


# (early_stop, max_iter, alpha): each value of each parameter, and the pairs that matter (a stop after 1 and 2)
PARAMS = ((0, 1, 1.0), (1, 2, 0.75), (0, 25, 0.8), (1, 25, 0.75), (1, 25, 1.0), (0, 2, 0.8), (1, 1, 0.8))


@pytest.mark.parametrize("N", [8, 63, 64, 65, 255, 256, 257, 600])
def test_ldpc_against_the_twin(bare, N):
    """dsce_ldpc == ldpc_decode, bits and iterations, for 1, 3 and 65 codewords,
    variable counts around the wavefront and the 256-thread marks and one that takes
    more than one pass of 64-lane groups per phase, both early_stop values, 1, 2 and 25
    iterations, three alphas, and four kinds of input: normal, normal x 1e8 (no
    clipping), all zero, and integers from {-1, 0, 1}: exact zeros and ties m1 == m2,
    that is the lowest-position rule and the `< 0` rule."""
    from dsce.coding import ldpc_decode
    rng = np.random.default_rng(300 + N)
    code0 = limit_code(N, rng)
    ones, stops = 0, set()
    for n in (1, 3, 65):
        base = 2.0 * rng.standard_normal((n, code0.n_slots)) - 1.5
        for early, max_iter, alpha in PARAMS:
            code = code0._replace(early_stop=bool(early), max_iter=max_iter, alpha=alpha)
            for kind, lam in (("normal", base), ("large", base * 1e8), ("zero", np.zeros_like(base)),
                              ("ties", rng.integers(-1, 2, base.shape).astype(np.float64))):
                got, git = _ldpc(bare, lam, code)
                ref, rit = ldpc_decode(lam, code)
                assert got.dtype == np.uint8 and got.max() <= 1
                assert np.array_equal(git, rit), (n, early, max_iter, alpha, kind, git[:8], rit[:8])
                assert np.array_equal(got, ref), (n, early, max_iter, alpha, kind, np.argwhere(got != ref)[:4])
                if kind == "zero":
                    assert not got.any() and (git == (1 if early else max_iter)).all()
                if not early:
                    assert (git == max_iter).all()
                ones += int(got.sum())
                stops.update(git.tolist())
        # without iters_out, and the Python wrapper, one codeword without the leading axis too
        code = code0._replace(max_iter=25)
        ref, rit = ldpc_decode(base, code)
        assert np.array_equal(_ldpc(bare, base, code, iters=False)[0], ref)
        x, it = bare.ldpc(base, code)
        assert np.array_equal(x, ref) and np.array_equal(it, rit) and it.dtype == np.int32
        x, it = bare.ldpc(base[0], code)
        assert np.array_equal(x, ref[0]) and it == rit[0]
    assert ones > 0 and {1, 2, 25} <= stops


def test_ldpc_decodes_any_codeword(bare):
    """Nothing is descrambled: noiseless random codewords of make_ldpc's codes come back
    after one iteration, at N = 2560 (three variables per thread) for the rates whose
    working set is the largest and the smallest."""
    from dsce.coding import ldpc_encode, ldpc_lam, make_ldpc
    rng = np.random.default_rng(8)
    for rate in ("1/2", "5/6"):
        code = make_ldpc(2560, rate)
        cw = ldpc_encode(rng.integers(0, 2, (7, code.n_info)), code)
        x, it = _ldpc(bare, ldpc_lam(cw, code, 2.5), code)
        assert np.array_equal(x, cw) and (it == 1).all()


def test_ldpc_codes_beyond_64_kib(bare):
    """Where the context's lds_max allows it, codes whose working set exceeds 64 KiB:
    9000 variables (16 per thread, ell in registers) and 16500 (ell read again each
    iteration), each against the twin.  A context whose limit is 64 KiB refuses both
    with the bytes and the limit."""
    from dsce import engine
    from dsce.coding import ldpc_decode, ldpc_from_rows
    rng = np.random.default_rng(12)
    limit = bare.get_option("lds_max")
    for N, M in ((9000, 300), (16500, 200)):
        rows = [rng.choice(N, 32 if c % 2 else 7, replace=False) for c in range(M)]
        code = ldpc_from_rows(rows, N, N // 2, max_iter=6)
        need = 8 * N + 24 * M + 8
        assert need > 64 * 1024
        lam = 2.0 * rng.standard_normal((3, N)) - 1.0
        if need <= limit:
            x, it = _ldpc(bare, lam, code)
            rx, rit = ldpc_decode(lam, code)
            assert np.array_equal(x, rx) and np.array_equal(it, rit) and x.any()
        else:
            with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL) as e:
                _ldpc(bare, lam, code)
            assert str(need) in str(e.value) and str(limit) in str(e.value), e.value
    print("lds_max %d" % limit)


@pytest.fixture(scope="module")
def code200():
    from dsce.coding import make_ldpc
    return make_ldpc(200, "1/2")


def test_ldpc_errors(bare, code200):
    from dsce import engine
    from dsce.coding import ldpc_decode
    code = code200
    lam = np.random.default_rng(1).standard_normal((2, 200))
    ref = ldpc_decode(lam, code)
    out = np.zeros((2, 200), dtype=np.uint8)
    its = np.zeros(2, dtype=np.int32)
    lp, op, ip = (lam.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_uint8)),
                  its.ctypes.data_as(C.POINTER(C.c_int32)))

    def works():
        x, it = _ldpc(bare, lam, code)
        assert np.array_equal(x, ref[0]) and np.array_equal(it, ref[1])

    def rc(c=code, n_slots=200, l=lp, n=2, o=op, null=None, word=None):
        desc, keep = _desc(c)
        if null:
            setattr(desc, null, None)
        r = bare.lib.dsce_ldpc(bare.h, C.byref(desc), n_slots, l, n, o, ip)
        assert not out.any() and not its.any()
        if word:
            msg = bare.lib.dsce_last_error(bare.h).decode()
            assert word in msg, msg
        works()                                                                  # the context still works
        return r

    works()
    assert bare.lib.dsce_ldpc(bare.h, None, 200, lp, 2, op, ip) == EINVAL         # null code
    for f in ("row_ptr", "col", "slot"):
        assert rc(null=f, word="null") == EINVAL
    rp, col, slot = code.row_ptr, code.col, code.slot

    def edit(a, i, v):
        b = a.copy()
        b[i] = v
        return b

    bad = [(code._replace(max_iter=0), "max_iter"), (code._replace(max_iter=101), "max_iter"),
           (code._replace(alpha=0.0), "alpha"), (code._replace(alpha=1.25), "alpha"),
           (code._replace(alpha=float("nan")), "alpha"), (code._replace(alpha=float("inf")), "alpha"),
           (code._replace(early_stop=2), "early_stop"),
           (code._replace(n_info=0), "n_info"), (code._replace(n_info=201), "n_info"),
           (code._replace(row_ptr=edit(rp, 0, 1)), "row_ptr"),                   # does not start at 0
           (code._replace(row_ptr=edit(rp, 3, rp[2])), "row_ptr"),               # not increasing: a check of degree 0
           (code._replace(row_ptr=edit(rp, 3, rp[2] + 1)), "degree"),            # a check of degree 1
           (code._replace(col=edit(col, 7, 200)), "col"), (code._replace(col=edit(col, 7, -1)), "col"),
           (code._replace(col=edit(col, rp[4] + 1, col[rp[4]])), "ascending"),   # a variable twice in a check
           (code._replace(slot=edit(slot, 9, 200)), "slot"), (code._replace(slot=edit(slot, 9, -2)), "slot")]
    for c, word in bad:
        assert rc(c=c, word=word) == EINVAL, word
    # n_vars / n_checks < 1 (the arrays are not read), a check of 33 variables
    for f in ("n_vars", "n_checks"):
        desc, keep = _desc(code)
        setattr(desc, f, 0)
        assert bare.lib.dsce_ldpc(bare.h, C.byref(desc), 200, lp, 2, op, ip) == EINVAL
        assert f in bare.lib.dsce_last_error(bare.h).decode()
    from dsce.coding import ldpc_from_rows
    wide = ldpc_from_rows([list(range(33)), [0, 1]], 200, 100)
    assert rc(c=wide, word="degree") == EINVAL
    assert rc(l=None) == EINVAL and rc(o=None) == EINVAL                         # null data with n_cw > 0
    assert rc(n=-1, word="n_cw") == EINVAL
    assert rc(n_slots=-1, word="n_slots") == EINVAL
    assert rc(n_slots=199, word="slot") == EINVAL                                # slot 199 is used
    assert rc(n=0, l=None, o=None) == 0                                          # n_cw = 0 does nothing
    assert not out.any()


def test_ldpc_lds_limit(bare, code200):
    """Option lds_max lowered to 1024: the 200-variable code (4008 bytes) is refused with
    the bytes and the limit in the message and nothing launched; it decodes again once
    the option is restored."""
    from dsce import engine
    from dsce.coding import ldpc_decode
    code = code200
    need = 8 * code.n_vars + 24 * code.n_checks + 8
    lam = np.random.default_rng(2).standard_normal((3, 200))
    ref = ldpc_decode(lam, code)
    limit = bare.get_option("lds_max")
    assert limit >= 64 * 1024 and need == 4008
    try:
        bare.set_option("lds_max", 1024)
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL) as e:
            _ldpc(bare, lam, code)
        assert str(need) in str(e.value) and "1024" in str(e.value) and "lds_max" in str(e.value), e.value
        bare.set_option("lds_max", need)                                          # exactly enough
        x, it = _ldpc(bare, lam, code)
        assert np.array_equal(x, ref[0]) and np.array_equal(it, ref[1])
        bare.set_option("lds_max", need - 1)
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL):
            _ldpc(bare, lam, code)
    finally:
        bare.set_option("lds_max", limit)
    x, it = _ldpc(bare, lam, code)
    assert np.array_equal(x, ref[0]) and np.array_equal(it, ref[1])


@pytest.mark.parametrize("rate", ["1/2", "3/4"])
@pytest.mark.parametrize("name", ["ofdm", "fbmc_aux", "fbmc_cod"])
def test_run_ldpc_against_the_twin(name, rate):
    """Default setup, n_iter 4, SNR (10, 35), batch 64, realisations 5..7: the counts of
    both methods and both branches equal the twin on export_llr's fp64 LLRs and
    export's sym, exactly.  For ofdm, max-log, MMSE branch they are also the counts
    recorded from the oracle's LLRs (test_ldpc_host.ORACLE_LDPC)."""
    from dsce.coding import make_ldpc
    S = harness.setup("default", schemes=(name,), snr_db=SNR, n_iter=4)
    sc = S.schemes[name]
    B = sc["n_data"] * sc["bits_per_symbol"]
    eng = harness.engine(S, batch=64)
    try:
        code = make_ldpc(B, rate)
        seen = set()
        for method in METHODS:
            for branch in BRANCHES:
                got = _run(eng, 0, SEED, 5, 3, code, method=method, branch=branch)
                ref = _twin_counts(eng, 0, 5, 3, code, method, branch)
                print("ldpc %s %s %s %s %s" % (name, rate, method, branch, {f: got[f].tolist() for f in ALL}))
                assert got["bit_err"].shape == (len(SNR), S.n_iter + 1) and got["bit_err"].dtype == np.int64
                _same(got, ref)
                assert (got["frame_err"] <= 3).all() and ((got["bit_err"] > 0) == (got["frame_err"] > 0)).all()
                assert (got["iter_sum"] >= 3).all() and (got["iter_sum"] <= 3 * code.max_iter).all()
                assert (got["iter_sum"][got["frame_err"] == 3] == 3 * code.max_iter).all()
                seen.update(got["frame_err"].ravel().tolist())
                if name == "ofdm" and method == "maxlog" and branch == "mmse":
                    for f in ALL:
                        assert got[f].tolist() == ORACLE_LDPC[rate][f], (rate, f, got[f])
        if name == "ofdm":
            assert {0, 3} <= seen                                               # cells with no and with total failure
    finally:
        eng.close()


@pytest.fixture(scope="module")
def ldpc_ofdm():
    """The default OFDM scheme with a rate-3/4 code over all 2560 slots, and a
    200-variable code scattered over them for the runs of many realisations."""
    from dsce.coding import make_ldpc
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR, n_iter=4)
    eng = harness.engine(S, batch=64)
    sc = S.schemes["ofdm"]
    B = sc["n_data"] * sc["bits_per_symbol"]
    small = make_ldpc(200, "1/2", max_iter=12)
    small = small._replace(slot=np.random.default_rng(4).permutation(B)[:200].astype(np.int32), n_slots=B)
    yield S, eng, make_ldpc(B, "3/4"), small
    eng.close()


def test_run_ldpc_with_scale_tables(ldpc_ofdm):
    """Random tables g = 10**uniform(-1, 2): g_est on the MMSE branch, then g_perf with
    the flag; the counts equal the twin on the scaled export, and the tables change
    them."""
    S, eng, code, small = ldpc_ofdm
    eng.set_batch(64)
    rng = np.random.default_rng(21)
    shape = eng.calib_shapes(0)["ratio_est"]
    plain = {b: _run(eng, 0, SEED, 5, 3, code, branch=b) for b in BRANCHES}
    try:
        eng.set_llr_scale(0, 10.0 ** rng.uniform(-1, 2, shape))
        got = _run(eng, 0, SEED, 5, 3, code)
        _same(got, _twin_counts(eng, 0, 5, 3, code, "exact", "mmse"))
        assert not np.array_equal(got["bit_err"], plain["mmse"]["bit_err"])
        _same(_run(eng, 0, SEED, 5, 3, code, branch="perfect"), plain["perfect"])        # g_est does not touch it
        eng.set_llr_scale_perf(0, 10.0 ** rng.uniform(-1, 2, shape))
        gotp = _run(eng, 0, SEED, 5, 3, code, branch="perfect")
        _same(gotp, _twin_counts(eng, 0, 5, 3, code, "exact", "perfect"))
        assert not np.array_equal(gotp["bit_err"], plain["perfect"]["bit_err"])
    finally:
        eng.set_llr_scale(0)
        eng.set_llr_scale_perf(0)
    _same(_run(eng, 0, SEED, 5, 3, code), plain["mmse"])


def test_run_ldpc_real_codewords(ldpc_ofdm):
    """The counts without the all-zero shortcut: on the LLRs the engine exports, signed
    by sym, a random codeword per (realisation, SNR point, stage) goes through
    dsce_ldpc; decoded XOR sent gives the counts of dsce_run_ldpc, iterations included."""
    from dsce.coding import ldpc_encode
    from test_ldpc_host import flip_of
    S, eng, code, small = ldpc_ofdm
    eng.set_batch(64)
    got = _run(eng, 0, SEED, 5, 3, code, method="maxlog")
    llr = eng.export_llr(0, SEED, 5, 3, fields=("llr",), method="maxlog")["llr"]
    sym = _export(eng, 0, SEED, 5, 3, fields=("sym",))["sym"]
    n, nk, ns, nd, m = llr.shape
    t = ((np.asarray(sym)[..., None] >> np.arange(m)) & 1).astype(bool).reshape(n, 1, 1, nd * m)
    flat = llr.reshape(n, nk, ns, nd * m)
    lam = np.where(t, -flat, flat).reshape(-1, nd * m)
    cw = ldpc_encode(np.random.default_rng(17).integers(0, 2, (lam.shape[0], code.n_info)), code)
    x, it = _ldpc(eng, lam * flip_of(cw, code), code)
    bit = (x ^ cw)[:, :code.n_info].astype(np.int64).sum(axis=1).reshape(n, nk, ns)
    assert np.array_equal(bit.sum(axis=0), got["bit_err"]) and got["bit_err"].sum() > 0
    assert np.array_equal((bit > 0).sum(axis=0), got["frame_err"])
    assert np.array_equal(it.astype(np.int64).reshape(n, nk, ns).sum(axis=0), got["iter_sum"])


def test_run_ldpc_invariance(ldpc_ofdm):
    """Realisations [0, 130) with the 200-variable code: batch 128, snr_chunk 1,
    export_stage_mb 1 (one-wave sub-batches) and the split [0, 64) + [64, 130) added into
    the same arrays give the counts of batch 64, exactly; those are the twin's."""
    S, eng, code, small = ldpc_ofdm
    eng.set_batch(64)
    ref = _run(eng, 0, SEED, 0, 130, small, method="maxlog")
    assert ref["bit_err"].sum() > 0 and (ref["frame_err"] <= 130).all() and (ref["frame_err"] < 130).any()
    assert (ref["iter_sum"] >= 130).all() and (ref["iter_sum"] <= 130 * small.max_iter).all()
    _same(ref, _twin_counts(eng, 0, 0, 130, small, "maxlog", "mmse"))
    try:
        eng.set_batch(128)
        _same(_run(eng, 0, SEED, 0, 130, small, method="maxlog"), ref)
        eng.set_option("export_stage_mb", 1)
        _same(_run(eng, 0, SEED, 0, 130, small, method="maxlog"), ref)
        eng.set_option("export_stage_mb", 1024)
        eng.set_option("snr_chunk", 1)
        _same(_run(eng, 0, SEED, 0, 130, small, method="maxlog"), ref)
    finally:
        eng.set_option("export_stage_mb", 1024)
        eng.set_option("snr_chunk", 0)
        eng.set_batch(64)
    a = _run(eng, 0, SEED, 0, 64, small, method="maxlog")
    _same(_run(eng, 0, SEED, 64, 66, small, method="maxlog", into=a), ref)
    # the full-size code over the same geometries, three realisations
    full = _run(eng, 0, SEED, 5, 3, code)
    try:
        eng.set_batch(128)
        eng.set_option("snr_chunk", 1)
        eng.set_option("export_stage_mb", 1)
        _same(_run(eng, 0, SEED, 5, 3, code), full)
    finally:
        eng.set_option("export_stage_mb", 1024)
        eng.set_option("snr_chunk", 0)
        eng.set_batch(64)
    _same(_run(eng, 0, SEED, 6, 2, code, into=_run(eng, 0, SEED, 5, 1, code)), full)


def test_run_ldpc_repeatability_and_side_effects(ldpc_ofdm):
    from dsce.coding import make_code
    S, eng, code, small = ldpc_ofdm
    eng.set_batch(64)
    counts = eng.run(SEED, 0, 64)
    path = eng.path_info(0)
    soft = eng.run_soft(0, SEED, 5, 70)
    conv = make_code(code.n_slots, "3/4")
    coded = eng.run_coded(0, SEED, 5, 70, conv)
    ref = _run(eng, 0, SEED, 5, 70, small)
    twice = _run(eng, 0, SEED, 5, 70, small, into=ref)
    for f in ALL:
        assert np.array_equal(twice[f], 2 * ref[f]) and ref[f].sum() > 0, f
    start = {f: np.full_like(ref[f], 7) for f in ALL}
    _same(_run(eng, 0, SEED, 5, 0, small, into=start), start)                    # n_rep = 0 adds nothing
    for fields in (("bit_err",), ("frame_err",), ("iter_sum",), ("bit_err", "iter_sum")):
        one = _run(eng, 0, SEED, 5, 70, small, fields=fields)                    # the others' memory is left alone
        assert sorted(one) == sorted(fields)
        for f in fields:
            assert np.array_equal(one[f], ref[f]), f
    # the Python wrapper: from zero, and adding into `out`
    w = eng.run_ldpc(0, SEED, 5, 70, small)
    _same(w, ref)
    w2 = eng.run_ldpc(0, SEED, 5, 70, small, out={"iter_sum": w["iter_sum"]})
    assert list(w2) == ["iter_sum"] and np.array_equal(w2["iter_sum"], 2 * ref["iter_sum"])
    # the decoder is timed as k_ldpc
    eng.enable_timing(True)
    try:
        _run(eng, 0, SEED, 5, 70, small)
        n, ms = eng.kernel_time("k_ldpc")
        assert n >= 1 and ms > 0
    finally:
        eng.enable_timing(False)
    # no side effects
    assert eng.path_info(0) == path
    assert np.array_equal(eng.run(SEED, 0, 64), counts) and eng.path_info(0) == path and counts.sum() > 0
    after = eng.run_soft(0, SEED, 5, 70)
    for f in soft:
        assert np.array_equal(after[f], soft[f]), f
    again = eng.run_coded(0, SEED, 5, 70, conv)
    for f in coded:
        assert np.array_equal(again[f], coded[f]), f


def test_simulate_ldpc(tmp_path):
    """python -m dsce.simulate --ldpc 3/4 (a child process: the command line is what is
    tested): its ber / fer / mean_iter are Engine.run_ldpc on the same realisations,
    both branches."""
    import json
    import os
    import subprocess
    import sys

    from dsce.coding import make_ldpc
    from dsce.configs import build_setup
    from dsce.engine import build_engine, gpu_tx
    out = tmp_path / "ldpc.json"
    env = dict(os.environ, PYTHONPATH=harness.PKG)
    p = subprocess.run([sys.executable, "-m", "dsce.simulate", "--config", "default", "--schemes", "ofdm", "--reps", "3",
                        "--batch", "64", "--ldpc", "3/4", "--ldpc-iters", "20", "--ldpc-alpha", "0.8", "--ldpc-seed", "9",
                        "--out", str(out)],
                       cwd=harness.PKG, env=env, timeout=240, capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    assert "ldpc_ber_ic_mmse" in p.stdout
    res = json.loads(out.read_text())
    r = res["ldpc"]["ofdm"]
    assert (r["rate"], r["info_bits"], r["n_checks"], r["max_iter"], r["alpha"], r["seed"]) == ("3/4", 1920, 640, 20, 0.8, 9)
    assert res["ldpc_seconds"] > 0
    S = build_setup("default", schemes=("ofdm",), tx=gpu_tx(0))
    eng = build_engine(S, batch=64)
    try:
        code = make_ldpc(2560, "3/4", seed=9, max_iter=20, alpha=0.8)
        for key, branch in (("mmse", "mmse"), ("perfect_ic", "perfect")):
            c = eng.run_ldpc(0, res["seed"], 0, 3, code, branch=branch)
            assert c["bit_err"].shape == (len(S.snr_db), S.n_iter + 1)
            assert np.array_equal(np.asarray(r[key]["ber"]), c["bit_err"] / (3.0 * 1920)), key
            assert np.array_equal(np.asarray(r[key]["fer"]), c["frame_err"] / 3.0), key
            assert np.array_equal(np.asarray(r[key]["mean_iter"]), c["iter_sum"] / 3.0), key
    finally:
        eng.close()


def test_run_ldpc_errors(ldpc_ofdm):
    from dsce import engine
    S, eng, code, small = ldpc_ofdm
    eng.set_batch(64)
    ref = _run(eng, 0, SEED, 5, 3, small)
    B = code.n_slots

    def fails(err, c=small, word=None, **k):
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % err) as e:
            _run(eng, 0, SEED, 5, 3, c, **k)                                     # asserts that nothing was written
        if word:
            assert word in str(e.value), e.value
        _same(_run(eng, 0, SEED, 5, 3, small), ref)                              # the context still works

    def edit(a, i, v):
        b = a.copy()
        b[i] = v
        return b

    fails(EINVAL, fields=())                                                    # no field requested
    for flags in (1 << 3, engine.EXPORT_F32, engine.EXPORT_DEVICE, engine.EXPORT_DEVICE | engine.LLR_MAXLOG):
        fails(EINVAL, flags=flags)
    rp, col, slot = small.row_ptr, small.col, small.slot
    for c, word in ((small._replace(slot=edit(slot, 11, B)), "slot"), (small._replace(slot=edit(slot, 11, -2)), "slot"),
                    (small._replace(col=edit(col, 7, 200)), "col"),
                    (small._replace(col=edit(col, rp[4] + 1, col[rp[4]])), "ascending"),
                    (small._replace(row_ptr=edit(rp, 0, 1)), "row_ptr"),
                    (small._replace(row_ptr=edit(rp, 3, rp[2])), "row_ptr"),
                    (small._replace(max_iter=0), "max_iter"), (small._replace(max_iter=101), "max_iter"),
                    (small._replace(alpha=0.0), "alpha"), (small._replace(alpha=1.5), "alpha"),
                    (small._replace(early_stop=-1), "early_stop"),
                    (small._replace(n_info=0), "n_info"), (small._replace(n_info=201), "n_info")):
        fails(EINVAL, c=c, word=word)
    buf = np.zeros(eng.ldpc_shapes(0)["bit_err"], dtype=np.int64)
    o = engine.LdpcOut(bit_err=buf.ctypes.data_as(C.POINTER(C.c_int64)))
    desc, keep = _desc(small)
    nulls = []
    for f in ("row_ptr", "col", "slot"):
        d, k2 = _desc(small)
        setattr(d, f, None)
        nulls.append(d)
    zero_n, k3 = _desc(small)
    zero_n.n_vars = 0
    zero_m, k4 = _desc(small)
    zero_m.n_checks = 0
    for d, oo in [(None, C.byref(o)), (C.byref(desc), None)] + [(C.byref(d), C.byref(o)) for d in nulls + [zero_n, zero_m]]:
        assert eng.lib.dsce_run_ldpc(eng.h, 0, SEED, 5, 3, 0, d, oo) == EINVAL   # null code / out / table, N or M < 1
    assert not buf.any()
    # the LDS limit: read by the call, restored afterwards
    limit = eng.get_option("lds_max")
    try:
        eng.set_option("lds_max", 1024)
        fails_msg = None
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL) as e:
            _run(eng, 0, SEED, 5, 3, small)
        fails_msg = str(e.value)
        assert "4008" in fails_msg and "1024" in fails_msg, fails_msg
    finally:
        eng.set_option("lds_max", limit)
    _same(_run(eng, 0, SEED, 5, 3, small), ref)
    # without dsce_build_mmse; after it the same context works
    bare = harness.engine(S, batch=64, mmse=False)
    try:
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % ESTATE):
            _run(bare, 0, SEED, 5, 3, small)
        bare.build_mmse(S.zero_threshold)
        _same(_run(bare, 0, SEED, 5, 3, small), ref)
    finally:
        bare.close()
    # before channel, SNR points or scheme are set
    empty = engine.Engine(0)
    try:
        assert empty.lib.dsce_run_ldpc(empty.h, 0, SEED, 0, 1, 0, C.byref(desc), C.byref(o)) == ESTATE
        assert not buf.any()
    finally:
        empty.close()
