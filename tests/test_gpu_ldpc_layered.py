"""GPU: dsce_ldpc_layered and dsce_run_ldpc_layered (k_ldpc_layered,
DSCE_HAS_LDPC_LAYERED) — the layered min-sum decoder on the device against its
NumPy twin dsce.coding.ldpc_decode_layered, equal to the bit, decided bits and
iteration counts: on the limit codes of tests/test_gpu_ldpc.py under first-fit
layers and under one check per layer, on a single layer of disjoint checks, on
a layer wider than any workgroup, on make_ldpc's codes and on a code beyond 64
KiB of LDS; on the engine's own export_llr output for both LLR methods, both
CSI branches and installed scale tables; and against itself across batch
geometries, SNR chunks, staging bounds and split calls.  The existing calls
return what they returned before a layered call, and every refusal of the
header comes back with nothing written.  Every comparison is exact.  Host
outputs sit between guard regions."""
import ctypes as C

import numpy as np
import pytest

import harness
from test_gpu_export import EINVAL, ESTATE, GUARD, PATTERN, SEED, SNR, _export
from test_gpu_ldpc import ALL, BRANCHES, METHODS, PARAMS, _desc, _ldpc, _run, _same, limit_code
from test_ldpc_host import bpsk_lam0, flip_of
from test_ldpc_layered_host import ORACLE_LDPC_LAYERED

pytestmark = pytest.mark.gpu


def _layers(code, layers):
    from dsce import engine
    return engine.Engine._ldpc_layers(layers, code)


def _dec(eng, lam, code, layers, iters=True):
    """dsce_ldpc_layered into a uint8 and an int32 array, each between two guard regions."""
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    n, N = lam.shape[0], int(code.n_vars)
    raw = np.full(n * N + 2 * GUARD, PATTERN, dtype=np.uint8)
    rit = np.full(n * 4 + 2 * GUARD, PATTERN, dtype=np.uint8)
    desc, keep = _desc(code)
    ly, keep_l = _layers(code, layers)
    ip = rit[GUARD:].ctypes.data_as(C.POINTER(C.c_int32)) if iters else None
    eng._chk(eng.lib.dsce_ldpc_layered(eng.h, C.byref(desc), C.byref(ly), lam.shape[1],
                                       lam.ctypes.data_as(C.POINTER(C.c_double)), n,
                                       raw[GUARD:].ctypes.data_as(C.POINTER(C.c_uint8)), ip), "dsce_ldpc_layered")
    assert (raw[:GUARD] == PATTERN).all() and (raw[-GUARD:] == PATTERN).all(), "bytes outside bits_out were written"
    assert (rit[:GUARD] == PATTERN).all() and (rit[-GUARD:] == PATTERN).all(), "bytes outside iters_out were written"
    if not iters:
        assert (rit == PATTERN).all()
    return raw[GUARD:GUARD + n * N].reshape(n, N).copy(), rit[GUARD:GUARD + 4 * n].view(np.int32).copy()


def _runl(eng, sid, seed, first, n, code, layers, fields=ALL, method="exact", branch="mmse", flags=None, into=None):
    """dsce_run_ldpc_layered as test_gpu_ldpc._run calls dsce_run_ldpc: zeroed int64 arrays (or copies of `into`)
    in one buffer between guards, only `fields` passed; the guards and the other fields keep their bytes."""
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
    ly, keep_l = _layers(code, layers)
    try:
        eng._chk(eng.lib.dsce_run_ldpc_layered(eng.h, sid, seed, first, n, flags, C.byref(desc), C.byref(ly), C.byref(o)),
                 "dsce_run_ldpc_layered")
    except engine.DsceError:
        assert np.array_equal(raw, before), "a refused call wrote"
        raise
    mask = np.ones(raw.size, dtype=bool)
    for f in fields:
        a0 = view[f].ctypes.data - raw.ctypes.data
        mask[a0:a0 + view[f].nbytes] = False
    assert np.array_equal(raw[mask], before[mask]), "bytes outside the requested fields were written"
    return {f: view[f].copy() for f in fields}


def _twin_counts(eng, sid, first, n, code, layers, method, branch):
    from dsce.coding import ldpc_counts
    llr = eng.export_llr(sid, SEED, first, n, fields=("llr",), method=method, branch=branch)["llr"]
    sym = _export(eng, sid, SEED, first, n, fields=("sym",))["sym"]
    assert llr.dtype == np.float64 and np.isfinite(llr).all()
    return ldpc_counts(llr, sym, code, layers=layers)


@pytest.fixture(scope="module")
def bare():
    """A context with nothing set: dsce_ldpc_layered needs no more."""
    from dsce import engine
    eng = engine.Engine(0)
    yield eng
    eng.close()


def _equal(eng, lam, code, layers, note):
    from dsce.coding import ldpc_decode_layered
    got, git = _dec(eng, lam, code, layers)
    ref, rit = ldpc_decode_layered(lam, code, layers)
    assert got.dtype == np.uint8 and got.max() <= 1
    assert np.array_equal(git, rit), (note, git[:8], rit[:8])
    assert np.array_equal(got, ref), (note, np.argwhere(got != ref)[:4])
    return got, git


@pytest.mark.parametrize("N", [8, 63, 64, 65, 255, 256, 257, 600])
def test_layered_against_the_twin(bare, N):
    """dsce_ldpc_layered == ldpc_decode_layered, bits and iterations, on limit_code(N): check degrees 2 and 32 in
    one graph (lane groups of 2 and of 32 in one wave), variables of degree 0, 1 and 40 (at least 40 layers),
    punctured variables and a shared slot.  First-fit layers: 1, 3 and 65 codewords, every PARAMS entry (both
    early_stop values, 1, 2 and 25 iterations, three alphas), inputs normal and from {-1, 0, 1} (exact zeros and
    ties m1 == m2: the lowest-position rule of the butterfly and the `< 0` rule), and with 3 codewords also normal x
    1e8 (no clipping) and all zero.  One check per layer, the serial schedule: 3 codewords, a stop after 2 and a
    run of 25, normal and tie inputs."""
    from dsce.coding import ldpc_decode_layered, make_layers, serial_layers
    rng = np.random.default_rng(300 + N)
    code0 = limit_code(N, rng)
    first = make_layers(code0)
    assert first[0].size - 1 >= min(40, code0.n_checks)
    ones, stops = 0, set()
    for n in (1, 3, 65):
        base = 2.0 * rng.standard_normal((n, code0.n_slots)) - 1.5
        kinds = [("normal", base), ("ties", rng.integers(-1, 2, base.shape).astype(np.float64))]
        if n == 3:
            kinds += [("large", base * 1e8), ("zero", np.zeros_like(base))]
        for early, max_iter, alpha in PARAMS:
            code = code0._replace(early_stop=bool(early), max_iter=max_iter, alpha=alpha)
            for kind, lam in kinds:
                got, git = _equal(bare, lam, code, first, (n, early, max_iter, alpha, kind))
                if kind == "zero":
                    assert not got.any() and (git == (1 if early else max_iter)).all()
                if not early:
                    assert (git == max_iter).all()
                ones += int(got.sum())
                stops.update(git.tolist())
        if n == 3:
            serial = serial_layers(code0)
            for early, max_iter, alpha in ((1, 25, 0.75), (0, 2, 1.0)):
                code = code0._replace(early_stop=bool(early), max_iter=max_iter, alpha=alpha)
                for kind, lam in kinds[:2]:
                    _equal(bare, lam, code, serial, ("serial", early, max_iter, alpha, kind))
            # without iters_out, and the Python wrapper, one codeword without the leading axis too
            code = code0._replace(max_iter=25)
            ref, rit = ldpc_decode_layered(base, code, first)
            assert np.array_equal(_dec(bare, base, code, first, iters=False)[0], ref)
            x, it = bare.ldpc(base, code, layers=first)
            assert np.array_equal(x, ref) and np.array_equal(it, rit) and it.dtype == np.int32
            x, it = bare.ldpc(base[0], code, layers=first)
            assert np.array_equal(x, ref[0]) and it == rit[0]
    assert ones > 0 and {1, 2, 25} <= stops


def test_layered_single_layer_of_disjoint_checks(bare):
    """90 disjoint checks of degrees 2 .. 32 in one layer (every group size, 1386 padded lanes: one stride beyond
    the workgroup), and the same code one check per layer: both equal the twin, and each other, since disjoint
    checks never see each other's sums."""
    from dsce.coding import ldpc_from_rows, make_layers, serial_layers
    rng = np.random.default_rng(41)
    degs = [2, 3, 4, 5, 8, 9, 16, 17, 31, 32] * 9
    starts = np.concatenate([[0], np.cumsum(degs)])
    N = int(starts[-1]) + 3
    rows = [list(range(starts[i], starts[i + 1])) for i in range(len(degs))]
    perm = rng.permutation(len(rows))
    code = ldpc_from_rows([rows[i] for i in perm], N, N // 2, max_iter=5, alpha=0.75)
    one = make_layers(code)
    assert one[0].tolist() == [0, len(rows)]
    lam = rng.integers(-3, 4, (5, N)).astype(np.float64)
    a = _equal(bare, lam, code, one, "one layer")
    b = _equal(bare, lam, code, serial_layers(code), "serial")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].any()


def test_layered_layer_wider_than_the_workgroup(bare):
    """N = 2400: layer 0 holds the 1200 disjoint checks (2 i, 2 i + 1), layer 1 the 1199 checks (2 i + 1, 2 i + 2)
    that chain them: 2400 lanes per layer against 1024 threads.  77 KiB of LDS: refused with the bytes where the
    context's limit is lower."""
    from dsce import engine
    from dsce.coding import ldpc_from_rows, make_layers
    rng = np.random.default_rng(43)
    rows = [[2 * i, 2 * i + 1] for i in range(1200)] + [[2 * i + 1, 2 * i + 2] for i in range(1199)]
    code = ldpc_from_rows(rows, 2400, 1200, max_iter=8, alpha=0.75)
    layers = (np.array([0, 1200, 2399], dtype=np.int32), np.arange(2399, dtype=np.int32))
    first = make_layers(code)
    assert np.array_equal(first[0], layers[0]) and np.array_equal(first[1], layers[1])
    lam = 2.0 * rng.standard_normal((3, 2400)) - 0.5
    need, limit = 8 * 2400 + 24 * 2399 + 8, bare.get_option("lds_max")
    if need <= limit:
        x, it = _equal(bare, lam, code, layers, "wide")
        assert x.any() and (it > 1).any()
        _equal(bare, lam, code._replace(early_stop=False), layers, "wide, every iteration")
    else:
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL) as e:
            _dec(bare, lam, code, layers)
        assert str(need) in str(e.value) and str(limit) in str(e.value), e.value


@pytest.mark.parametrize("rate", ["1/2", "5/6"])
def test_layered_make_ldpc_codes(bare, rate):
    """make_ldpc(2560, rate) with its first-fit layers (7 layers of up to 298 checks, 14 of up to 45), 3 noisy
    codewords that take several iterations, and noiseless random codewords, back after one iteration."""
    from dsce.coding import ldpc_encode, ldpc_lam, make_layers, make_ldpc
    code = make_ldpc(2560, rate)
    layers = make_layers(code)
    lam, raw = bpsk_lam0(code, {"1/2": 0.84, "5/6": 0.55}[rate], 3, 7)
    x, it = _equal(bare, lam, code, layers, rate)
    assert it.min() > 1
    cw = ldpc_encode(np.random.default_rng(8).integers(0, 2, (3, code.n_info)), code)
    x, it = _dec(bare, ldpc_lam(cw, code, 2.5), code, layers)
    assert np.array_equal(x, cw) and (it == 1).all()


def test_layered_code_beyond_64_kib(bare):
    """9000 variables and 300 checks of degrees 7 and 32: 79 KiB, the dynamic-LDS attribute path.  A context whose
    limit is lower refuses it with the bytes and the limit."""
    from dsce import engine
    from dsce.coding import ldpc_from_rows, make_layers
    rng = np.random.default_rng(12)
    N, M = 9000, 300
    rows = [rng.choice(N, 32 if c % 2 else 7, replace=False) for c in range(M)]
    code = ldpc_from_rows(rows, N, N // 2, max_iter=6)
    layers = make_layers(code)
    need, limit = 8 * N + 24 * M + 8, bare.get_option("lds_max")
    assert need > 64 * 1024
    lam = 2.0 * rng.standard_normal((3, N)) - 1.0
    if need <= limit:
        x, it = _equal(bare, lam, code, layers, "79 KiB")
        assert x.any()
    else:
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL) as e:
            _dec(bare, lam, code, layers)
        assert str(need) in str(e.value) and str(limit) in str(e.value), e.value


@pytest.fixture(scope="module")
def code200():
    from dsce.coding import make_layers, make_ldpc
    code = make_ldpc(200, "1/2")
    return code, make_layers(code)


def test_layered_errors(bare, code200):
    """Every refusal of the header through dsce_ldpc_layered: DSCE_EINVAL, the offender named, nothing written, and
    the context decodes afterwards."""
    from dsce.coding import ldpc_decode_layered, ldpc_from_rows
    code, layers = code200
    lp, lc = layers
    M = code.n_checks
    lam = np.random.default_rng(1).standard_normal((2, 200))
    ref = ldpc_decode_layered(lam, code, layers)
    out = np.zeros((2, 200), dtype=np.uint8)
    its = np.zeros(2, dtype=np.int32)
    lptr, op, ip = (lam.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_uint8)),
                    its.ctypes.data_as(C.POINTER(C.c_int32)))

    def works():
        x, it = _dec(bare, lam, code, layers)
        assert np.array_equal(x, ref[0]) and np.array_equal(it, ref[1])

    def rc(c=code, y=layers, n_slots=200, l=lptr, n=2, o=op, null=None, n_layers=None, word=None):
        from dsce import engine
        desc, keep = _desc(c)
        keep_l = tuple(np.ascontiguousarray(a, dtype=np.int32) for a in y)
        ly = engine.LdpcLayers(keep_l[0].size - 1, keep_l[0].ctypes.data_as(C.POINTER(C.c_int32)),
                               keep_l[1].ctypes.data_as(C.POINTER(C.c_int32)))
        if null:
            setattr(ly, null, None)
        if n_layers is not None:
            ly.n_layers = n_layers
        r = bare.lib.dsce_ldpc_layered(bare.h, C.byref(desc), C.byref(ly), n_slots, l, n, o, ip)
        assert not out.any() and not its.any()
        if word:
            msg = bare.lib.dsce_last_error(bare.h).decode()
            assert word in msg and "dsce_ldpc_layered" in msg, msg
        works()                                                                  # the context still works
        return r

    def edit(a, i, v):
        b = a.copy()
        b[i] = v
        return b

    works()
    desc, keep = _desc(code)
    assert bare.lib.dsce_ldpc_layered(bare.h, C.byref(desc), None, 200, lptr, 2, op, ip) == EINVAL     # null layers
    assert "null layers" in bare.lib.dsce_last_error(bare.h).decode()
    ly, keep_l = _layers(code, layers)
    assert bare.lib.dsce_ldpc_layered(bare.h, None, C.byref(ly), 200, lptr, 2, op, ip) == EINVAL       # null code
    for f in ("layer_ptr", "layer_check"):
        assert rc(null=f, word="null") == EINVAL
    assert rc(n_layers=0, word="n_layers") == EINVAL and rc(n_layers=-1, word="n_layers") == EINVAL
    assert rc(n_layers=M + 1, word="n_layers") == EINVAL
    L = lp.size - 1
    # a check of layer 1 that shares a variable with a check of layer 0, moved there
    c1 = int(lc[lp[1]])
    held = {int(v): int(c) for c in lc[:lp[1]] for v in code.col[code.row_ptr[c]:code.row_ptr[c + 1]]}
    v = next(int(v) for v in code.col[code.row_ptr[c1]:code.row_ptr[c1 + 1]] if int(v) in held)   # the first one met
    c0 = held[v]
    clash = (edit(lp, 1, lp[1] + 1), lc)
    bad = [((edit(lp, 0, 1), lc), "layer_ptr[0]"),
           ((edit(lp, 2, lp[1]), lc), "layer 1 no check"),                       # an empty layer
           ((edit(lp, 2, lp[1] - 1), lc), "layer 1 no check"),                   # a decreasing layer_ptr
           ((lp[:-1], lc), "layer_ptr[n_layers]"),                               # the last layer left out
           ((edit(lp, L, M + 1), lc), "beyond n_checks"),
           ((lp, edit(lc, 5, M)), "layer_check entry"), ((lp, edit(lc, 5, -1)), "layer_check entry"),
           ((lp, edit(lc, 5, lc[4])), "check %d appears twice" % lc[4]),
           (clash, "layer 0: checks %d and %d share variable %d" % (c0, c1, v))]
    for y, word in bad:
        assert rc(y=y, word=word) == EINVAL, word
    # the code errors of dsce_ldpc come first, under this call's name
    rp, col, slot = code.row_ptr, code.col, code.slot
    for c, word in ((code._replace(max_iter=0), "max_iter"), (code._replace(alpha=0.0), "alpha"),
                    (code._replace(early_stop=2), "early_stop"), (code._replace(n_info=201), "n_info"),
                    (code._replace(row_ptr=edit(rp, 3, rp[2] + 1)), "degree"),
                    (code._replace(col=edit(col, 7, 200)), "col"),
                    (code._replace(col=edit(col, rp[4] + 1, col[rp[4]])), "ascending"),
                    (code._replace(slot=edit(slot, 9, 200)), "slot")):
        assert rc(c=c, word=word) == EINVAL, word
    wide = ldpc_from_rows([list(range(33)), [0, 1]], 200, 100)
    assert rc(c=wide, y=(np.array([0, 1, 2]), np.array([0, 1])), word="degree") == EINVAL
    assert rc(l=None) == EINVAL and rc(o=None) == EINVAL                         # null data with n_cw > 0
    assert rc(n=-1, word="n_cw") == EINVAL
    assert rc(n_slots=-1, word="n_slots") == EINVAL
    assert rc(n_slots=199, word="slot") == EINVAL
    assert rc(n=0, l=None, o=None) == 0                                          # n_cw = 0 does nothing
    assert not out.any()


def test_layered_lds_limit(bare, code200):
    """Option lds_max lowered to 1024: the 200-variable code (4008 bytes) is refused with the bytes and the limit
    and nothing launched; it decodes again with exactly enough and once the option is restored."""
    from dsce import engine
    from dsce.coding import ldpc_decode_layered
    code, layers = code200
    need = 8 * code.n_vars + 24 * code.n_checks + 8
    lam = np.random.default_rng(2).standard_normal((3, 200))
    ref = ldpc_decode_layered(lam, code, layers)
    limit = bare.get_option("lds_max")
    assert limit >= 64 * 1024 and need == 4008
    try:
        bare.set_option("lds_max", 1024)
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL) as e:
            _dec(bare, lam, code, layers)
        assert str(need) in str(e.value) and "1024" in str(e.value) and "lds_max" in str(e.value), e.value
        bare.set_option("lds_max", need)                                          # exactly enough
        x, it = _dec(bare, lam, code, layers)
        assert np.array_equal(x, ref[0]) and np.array_equal(it, ref[1])
        bare.set_option("lds_max", need - 1)
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL):
            _dec(bare, lam, code, layers)
    finally:
        bare.set_option("lds_max", limit)
    x, it = _dec(bare, lam, code, layers)
    assert np.array_equal(x, ref[0]) and np.array_equal(it, ref[1])


@pytest.mark.parametrize("name", ["ofdm", "fbmc_aux"])
def test_run_ldpc_layered_against_the_twin(name):
    """Default setup, n_iter 4, SNR (10, 35), batch 64, realisations 5..7, rate 3/4, first-fit layers: the counts of
    both methods and both branches equal the twin on export_llr's fp64 LLRs and export's sym, exactly.  For ofdm,
    max-log, MMSE branch they are also the counts recorded from the oracle's LLRs (ORACLE_LDPC_LAYERED), and they
    differ from the flooding counts of the same call."""
    from dsce.coding import make_layers, make_ldpc
    S = harness.setup("default", schemes=(name,), snr_db=SNR, n_iter=4)
    sc = S.schemes[name]
    B = sc["n_data"] * sc["bits_per_symbol"]
    eng = harness.engine(S, batch=64)
    try:
        code = make_ldpc(B, "3/4")
        layers = make_layers(code)
        seen = set()
        for method in METHODS:
            for branch in BRANCHES:
                got = _runl(eng, 0, SEED, 5, 3, code, layers, method=method, branch=branch)
                ref = _twin_counts(eng, 0, 5, 3, code, layers, method, branch)
                print("ldpc layered %s %s %s %s" % (name, method, branch, {f: got[f].tolist() for f in ALL}))
                assert got["bit_err"].shape == (len(SNR), S.n_iter + 1) and got["bit_err"].dtype == np.int64
                _same(got, ref)
                assert (got["frame_err"] <= 3).all() and ((got["bit_err"] > 0) == (got["frame_err"] > 0)).all()
                assert (got["iter_sum"] >= 3).all() and (got["iter_sum"] <= 3 * code.max_iter).all()
                assert (got["iter_sum"][got["frame_err"] == 3] == 3 * code.max_iter).all()
                seen.update(got["frame_err"].ravel().tolist())
                if name == "ofdm" and method == "maxlog" and branch == "mmse":
                    for f in ALL:
                        assert got[f].tolist() == ORACLE_LDPC_LAYERED["3/4"][f], (f, got[f])
                    flood = _run(eng, 0, SEED, 5, 3, code, method=method, branch=branch)
                    assert not np.array_equal(flood["bit_err"], got["bit_err"])
                    _same(eng.run_ldpc(0, SEED, 5, 3, code, method=method, branch=branch, layers=layers), got)
        if name == "ofdm":
            assert {0, 3} <= seen                                               # cells with no and with total failure
    finally:
        eng.close()


@pytest.fixture(scope="module")
def ldpc_ofdm():
    """The default OFDM scheme with a rate-3/4 code over all 2560 slots, and a 200-variable code scattered over
    them for the runs of many realisations; each with its first-fit layers."""
    from dsce.coding import make_layers, make_ldpc
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR, n_iter=4)
    eng = harness.engine(S, batch=64)
    sc = S.schemes["ofdm"]
    B = sc["n_data"] * sc["bits_per_symbol"]
    small = make_ldpc(200, "1/2", max_iter=12)
    small = small._replace(slot=np.random.default_rng(4).permutation(B)[:200].astype(np.int32), n_slots=B)
    code = make_ldpc(B, "3/4")
    yield S, eng, (code, make_layers(code)), (small, make_layers(small))
    eng.close()


def test_run_ldpc_layered_with_scale_tables_and_real_codewords(ldpc_ofdm):
    """Random tables g = 10**uniform(-1, 2) on the MMSE branch: the counts equal the twin on the scaled export and
    the table changes them.  Then, without tables: on the LLRs the engine exports, signed by sym, a random codeword
    per (realisation, SNR point, stage) goes through dsce_ldpc_layered; decoded XOR sent gives the counts of
    dsce_run_ldpc_layered, iterations included."""
    from dsce.coding import ldpc_encode
    S, eng, (code, layers), _ = ldpc_ofdm
    eng.set_batch(64)
    plain = _runl(eng, 0, SEED, 5, 3, code, layers, method="maxlog")
    try:
        eng.set_llr_scale(0, 10.0 ** np.random.default_rng(21).uniform(-1, 2, eng.calib_shapes(0)["ratio_est"]))
        got = _runl(eng, 0, SEED, 5, 3, code, layers, method="maxlog")
        _same(got, _twin_counts(eng, 0, 5, 3, code, layers, "maxlog", "mmse"))
        assert not np.array_equal(got["bit_err"], plain["bit_err"])
    finally:
        eng.set_llr_scale(0)
    _same(_runl(eng, 0, SEED, 5, 3, code, layers, method="maxlog"), plain)
    llr = eng.export_llr(0, SEED, 5, 3, fields=("llr",), method="maxlog")["llr"]
    sym = _export(eng, 0, SEED, 5, 3, fields=("sym",))["sym"]
    n, nk, ns, nd, m = llr.shape
    t = ((np.asarray(sym)[..., None] >> np.arange(m)) & 1).astype(bool).reshape(n, 1, 1, nd * m)
    flat = llr.reshape(n, nk, ns, nd * m)
    lam = np.where(t, -flat, flat).reshape(-1, nd * m)
    cw = ldpc_encode(np.random.default_rng(17).integers(0, 2, (lam.shape[0], code.n_info)), code)
    x, it = _dec(eng, lam * flip_of(cw, code), code, layers)
    bit = (x ^ cw)[:, :code.n_info].astype(np.int64).sum(axis=1).reshape(n, nk, ns)
    assert np.array_equal(bit.sum(axis=0), plain["bit_err"]) and plain["bit_err"].sum() > 0
    assert np.array_equal((bit > 0).sum(axis=0), plain["frame_err"])
    assert np.array_equal(it.astype(np.int64).reshape(n, nk, ns).sum(axis=0), plain["iter_sum"])


def test_run_ldpc_layered_geometry(ldpc_ofdm):
    """Realisations [0, 130) with the 200-variable code: batch 128, snr_chunk 1, export_stage_mb 1 and the split
    [0, 64) + [64, 130) added into the same arrays give the counts of batch 64, exactly; those are the twin's.  A
    second call doubles the arrays, n_rep = 0 adds nothing, a field subset leaves the others alone, and the
    decoder is timed as k_ldpc_layered."""
    S, eng, (code, layers), (small, slayers) = ldpc_ofdm
    eng.set_batch(64)
    ref = _runl(eng, 0, SEED, 0, 130, small, slayers, method="maxlog")
    assert ref["bit_err"].sum() > 0 and (ref["frame_err"] < 130).any()
    assert (ref["iter_sum"] >= 130).all() and (ref["iter_sum"] <= 130 * small.max_iter).all()
    _same(ref, _twin_counts(eng, 0, 0, 130, small, slayers, "maxlog", "mmse"))
    try:
        eng.set_batch(128)
        _same(_runl(eng, 0, SEED, 0, 130, small, slayers, method="maxlog"), ref)
        eng.set_option("export_stage_mb", 1)
        _same(_runl(eng, 0, SEED, 0, 130, small, slayers, method="maxlog"), ref)
        eng.set_option("export_stage_mb", 1024)
        eng.set_option("snr_chunk", 1)
        _same(_runl(eng, 0, SEED, 0, 130, small, slayers, method="maxlog"), ref)
    finally:
        eng.set_option("export_stage_mb", 1024)
        eng.set_option("snr_chunk", 0)
        eng.set_batch(64)
    a = _runl(eng, 0, SEED, 0, 64, small, slayers, method="maxlog")
    _same(_runl(eng, 0, SEED, 64, 66, small, slayers, method="maxlog", into=a), ref)
    twice = _runl(eng, 0, SEED, 0, 130, small, slayers, method="maxlog", into=ref)
    for f in ALL:
        assert np.array_equal(twice[f], 2 * ref[f]) and ref[f].sum() > 0, f
    start = {f: np.full_like(ref[f], 7) for f in ALL}
    _same(_runl(eng, 0, SEED, 5, 0, small, slayers, into=start), start)          # n_rep = 0 adds nothing
    for fields in (("bit_err",), ("frame_err",), ("iter_sum",), ("bit_err", "iter_sum")):
        one = _runl(eng, 0, SEED, 0, 130, small, slayers, fields=fields, method="maxlog")
        assert sorted(one) == sorted(fields)
        for f in fields:
            assert np.array_equal(one[f], ref[f]), f
    w2 = eng.run_ldpc(0, SEED, 0, 130, small, method="maxlog", layers=slayers, out={"iter_sum": ref["iter_sum"].copy()})
    assert list(w2) == ["iter_sum"] and np.array_equal(w2["iter_sum"], 2 * ref["iter_sum"])
    # the full-size code over the same geometries, three realisations
    full = _runl(eng, 0, SEED, 5, 3, code, layers)
    try:
        eng.set_batch(128)
        eng.set_option("snr_chunk", 1)
        eng.set_option("export_stage_mb", 1)
        _same(_runl(eng, 0, SEED, 5, 3, code, layers), full)
    finally:
        eng.set_option("export_stage_mb", 1024)
        eng.set_option("snr_chunk", 0)
        eng.set_batch(64)
    _same(_runl(eng, 0, SEED, 6, 2, code, layers, into=_runl(eng, 0, SEED, 5, 1, code, layers)), full)
    eng.enable_timing(True)
    try:
        before = eng.kernel_time("k_ldpc")
        _runl(eng, 0, SEED, 5, 3, small, slayers)
        n, ms = eng.kernel_time("k_ldpc_layered")
        assert n >= 1 and ms > 0 and eng.kernel_time("k_ldpc") == before
    finally:
        eng.enable_timing(False)


def test_existing_calls_stay_bit_exact(ldpc_ofdm):
    """dsce_run, dsce_run_ldpc, dsce_run_coded and dsce_run_soft return after layered calls what they returned
    before them, and dsce_path_info is unchanged."""
    from dsce.coding import make_code
    S, eng, (code, layers), (small, slayers) = ldpc_ofdm
    eng.set_batch(64)
    counts = eng.run(SEED, 0, 64)
    path = eng.path_info(0)
    soft = eng.run_soft(0, SEED, 5, 70)
    conv = make_code(code.n_slots, "3/4")
    coded = eng.run_coded(0, SEED, 5, 70, conv)
    flood = _run(eng, 0, SEED, 5, 70, small)
    lam = np.random.default_rng(3).standard_normal((4, small.n_slots))
    probe = _ldpc(eng, lam, small)
    lay = _runl(eng, 0, SEED, 5, 70, small, slayers)
    _dec(eng, lam, small, slayers)
    assert eng.path_info(0) == path
    assert np.array_equal(eng.run(SEED, 0, 64), counts) and eng.path_info(0) == path and counts.sum() > 0
    _same(_run(eng, 0, SEED, 5, 70, small), flood)
    again = _ldpc(eng, lam, small)
    assert np.array_equal(again[0], probe[0]) and np.array_equal(again[1], probe[1])
    after = eng.run_soft(0, SEED, 5, 70)
    for f in soft:
        assert np.array_equal(after[f], soft[f]), f
    again = eng.run_coded(0, SEED, 5, 70, conv)
    for f in coded:
        assert np.array_equal(again[f], coded[f]), f
    _same(_runl(eng, 0, SEED, 5, 70, small, slayers), lay)
    assert not np.array_equal(lay["iter_sum"], flood["iter_sum"])


def test_run_ldpc_layered_errors(ldpc_ofdm):
    from dsce import engine
    S, eng, _, (small, slayers) = ldpc_ofdm
    eng.set_batch(64)
    ref = _runl(eng, 0, SEED, 5, 3, small, slayers)
    lp, lc = slayers
    M, B = small.n_checks, small.n_slots

    def fails(err, c=small, y=slayers, word=None, **k):
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % err) as e:
            _runl(eng, 0, SEED, 5, 3, c, y, **k)                                 # asserts that nothing was written
        if word:
            assert word in str(e.value), e.value
        _same(_runl(eng, 0, SEED, 5, 3, small, slayers), ref)                    # the context still works

    def edit(a, i, v):
        b = a.copy()
        b[i] = v
        return b

    fails(EINVAL, fields=())                                                    # no field requested
    for flags in (1 << 3, engine.EXPORT_F32, engine.EXPORT_DEVICE, engine.EXPORT_DEVICE | engine.LLR_MAXLOG):
        fails(EINVAL, flags=flags)
    for c, word in ((small._replace(slot=edit(small.slot, 11, B)), "slot"), (small._replace(max_iter=101), "max_iter"),
                    (small._replace(col=edit(small.col, 7, 200)), "col"), (small._replace(alpha=1.5), "alpha")):
        fails(EINVAL, c=c, word=word)
    for y, word in (((edit(lp, 0, 1), lc), "layer_ptr[0]"), ((edit(lp, 2, lp[1]), lc), "layer 1 no check"),
                    ((lp[:-1], lc), "layer_ptr[n_layers]"), ((lp, edit(lc, 5, M)), "layer_check entry"),
                    ((lp, edit(lc, 5, lc[4])), "check %d appears twice" % lc[4]),
                    ((np.array([0, M]), np.arange(M)), "share variable")):
        fails(EINVAL, y=y, word=word)
    buf = np.zeros(eng.ldpc_shapes(0)["bit_err"], dtype=np.int64)
    o = engine.LdpcOut(bit_err=buf.ctypes.data_as(C.POINTER(C.c_int64)))
    desc, keep = _desc(small)
    ly, keep_l = _layers(small, slayers)
    nulls = []
    for f in ("layer_ptr", "layer_check"):
        d, k2 = _layers(small, slayers)
        setattr(d, f, None)
        nulls.append(d)
    zero_l, k3 = _layers(small, slayers)
    zero_l.n_layers = 0
    for d, y, oo in [(None, C.byref(ly), C.byref(o)), (C.byref(desc), None, C.byref(o)), (C.byref(desc), C.byref(ly), None)] + \
            [(C.byref(desc), C.byref(y), C.byref(o)) for y in nulls + [zero_l]]:
        assert eng.lib.dsce_run_ldpc_layered(eng.h, 0, SEED, 5, 3, 0, d, y, oo) == EINVAL
    assert not buf.any()
    limit = eng.get_option("lds_max")
    try:
        eng.set_option("lds_max", 1024)
        with pytest.raises(engine.DsceError, match=r"\(%d\)" % EINVAL) as e:
            _runl(eng, 0, SEED, 5, 3, small, slayers)
        assert "4008" in str(e.value) and "1024" in str(e.value), e.value
    finally:
        eng.set_option("lds_max", limit)
    _same(_runl(eng, 0, SEED, 5, 3, small, slayers), ref)
    # before channel, SNR points or scheme are set
    empty = engine.Engine(0)
    try:
        assert empty.lib.dsce_run_ldpc_layered(empty.h, 0, SEED, 0, 1, 0, C.byref(desc), C.byref(ly), C.byref(o)) == ESTATE
        assert not buf.any()
    finally:
        empty.close()


def test_simulate_ldpc_layered(tmp_path):
    """python -m dsce.simulate --ldpc 3/4 --ldpc-schedule layered (a child process: the command line is what is
    tested): its record names the schedule and the layers, and its ber / fer / mean_iter are Engine.run_ldpc with
    make_layers on the same realisations, both branches."""
    import json
    import os
    import subprocess
    import sys

    from dsce.coding import make_layers, make_ldpc
    from dsce.configs import build_setup
    from dsce.engine import build_engine, gpu_tx
    out = tmp_path / "ldpc.json"
    env = dict(os.environ, PYTHONPATH=harness.PKG)
    p = subprocess.run([sys.executable, "-m", "dsce.simulate", "--config", "default", "--schemes", "ofdm", "--reps", "3",
                        "--batch", "64", "--ldpc", "3/4", "--ldpc-iters", "15", "--ldpc-schedule", "layered",
                        "--out", str(out)],
                       cwd=harness.PKG, env=env, timeout=240, capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    res = json.loads(out.read_text())
    r = res["ldpc"]["ofdm"]
    assert (r["rate"], r["max_iter"], r["schedule"], r["n_layers"]) == ("3/4", 15, "layered", 12)
    S = build_setup("default", schemes=("ofdm",), tx=gpu_tx(0))
    eng = build_engine(S, batch=64)
    try:
        code = make_ldpc(2560, "3/4", max_iter=15)
        for key, branch in (("mmse", "mmse"), ("perfect_ic", "perfect")):
            c = eng.run_ldpc(0, res["seed"], 0, 3, code, branch=branch, layers=make_layers(code))
            assert np.array_equal(np.asarray(r[key]["ber"]), c["bit_err"] / (3.0 * 1920)), key
            assert np.array_equal(np.asarray(r[key]["fer"]), c["frame_err"] / 3.0), key
            assert np.array_equal(np.asarray(r[key]["mean_iter"]), c["iter_sum"] / 3.0), key
    finally:
        eng.close()
