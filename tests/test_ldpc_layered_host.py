"""CPU: the host side of the layered LDPC schedule (dsce_run_ldpc_layered /
dsce_ldpc_layered, DSCE_HAS_LDPC_LAYERED) — dsce.coding: make_layers' first-fit
partitions, check_layers (the mirror of the host's refusals) and
ldpc_decode_layered, the NumPy twin of k_ldpc_layered, against the references of
tests/test_ldpc_host.py that are not the twin: the brute-force maximum-likelihood
codeword on cycle-free codes and the codeword invariance with a separate encoder.
Then the header against the ctypes binding, the conventions pinned on the oracle's
LLRs (ORACLE_LDPC_LAYERED), two deliberately wrong decoders that these must catch,
and `python -m dsce.simulate --ldpc-schedule`.  No GPU call;
tests/test_gpu_ldpc_layered.py compares the engine with the twin and
tests/test_gpu_ldpc_layered_ref.py runs the tree and invariance cases of this
file through dsce_ldpc_layered."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from test_coding_host import oracle_llr  # noqa: F401  (the fixture)
from test_ldpc_host import (HDR, ORACLE_LDPC, bpsk_lam0, check_invariance, check_tree_ml, code_of, flip_of,
                            reference_encode)

# first-fit layers of make_ldpc(2560, rate), default seeds: the checks per layer
LAYER_SIZES = {"1/2": [298, 298, 268, 222, 140, 52, 2],
               "3/4": [85, 86, 85, 76, 73, 69, 57, 45, 36, 22, 4, 2],
               "5/6": [44, 42, 45, 39, 39, 38, 37, 34, 31, 26, 21, 15, 12, 4]}

# the setting of test_ldpc_host.ORACLE_LDPC with ldpc_decode_layered over make_layers(code): [snr][stage]
ORACLE_LDPC_LAYERED = {
    "1/2": dict(bit_err=[[1191, 1152, 1137, 1138, 1135], [30, 0, 0, 0, 0]],
                frame_err=[[3, 3, 3, 3, 3], [1, 0, 0, 0, 0]],
                iter_sum=[[90, 90, 90, 90, 90], [65, 16, 14, 13, 13]]),
    "3/4": dict(bit_err=[[1813, 1752, 1758, 1748, 1772], [662, 202, 184, 174, 171]],
                frame_err=[[3, 3, 3, 3, 3], [3, 2, 2, 2, 2]],
                iter_sum=[[90, 90, 90, 90, 90], [90, 63, 62, 62, 62]]),
}

# sigma at which the layered twin fails on between a quarter and three quarters of 40 frames of (2560, 1/2): at
# test_ldpc_host's 0.80 it fails on 6 only
SIGMA_2560_HALF = 0.82

_layers = {}


def layers_of(code):
    """make_layers, once per code table"""
    from dsce.coding import make_layers
    key = (code.n_vars, code.n_checks, code.col.tobytes(), code.row_ptr.tobytes())
    if key not in _layers:
        _layers[key] = make_layers(code)
    return _layers[key]


def layered(lam, code, _mutate=None):
    from dsce.coding import ldpc_decode_layered
    return ldpc_decode_layered(lam, code, layers_of(code), _mutate=_mutate)


def assert_partition(code, layers):
    """every check in exactly one layer, no two checks of a layer sharing a variable: by a dense product, not by
    check_layers"""
    lp, lc = layers
    assert lp.dtype == lc.dtype == np.int32 and lp[0] == 0 and lp[-1] == code.n_checks and (np.diff(lp) > 0).all()
    assert np.array_equal(np.sort(lc), np.arange(code.n_checks))
    H = np.zeros((code.n_checks, code.n_vars), dtype=np.int64)
    H[np.repeat(np.arange(code.n_checks), np.diff(code.row_ptr)), code.col] = 1
    for l in range(lp.size - 1):
        assert H[lc[lp[l]:lp[l + 1]]].sum(axis=0).max() <= 1, l


def check_invariance_2560_half(decode):
    """check_invariance of test_ldpc_host for (2560, 1/2) at SIGMA_2560_HALF: the same assertions and the same
    quarter window"""
    from dsce.coding import ldpc_encode, ldpc_syndrome
    N, rate, n = 2560, "1/2", 40
    code = code_of(N, rate)
    u = np.random.default_rng(N + 31).integers(0, 2, (n, code.n_info)).astype(np.uint8)
    cw = reference_encode(u, code)
    assert np.array_equal(cw, ldpc_encode(u, code)) and not ldpc_syndrome(cw, code).any()
    assert cw.any(axis=1).all()
    lam0, raw = bpsk_lam0(code, SIGMA_2560_HALF, n, 1000 + N)
    x0, it0 = decode(lam0, code)
    x1, it1 = decode(lam0 * flip_of(cw, code), code)
    fails = int(x0[:, :code.n_info].any(axis=1).sum())
    print("N %d rate %s sigma %.2f: %d of %d frames fail, mean iterations %.1f, raw BER %.3f"
          % (N, rate, SIGMA_2560_HALF, fails, n, float(np.mean(it0)), raw))
    assert np.array_equal(x1 ^ cw, x0), np.argwhere((x1 ^ cw) != x0)[:4]
    assert np.array_equal(it1, it0)
    assert fails >= n // 4 and n - fails >= n // 4, fails


def oracle_lam(oracle):
    llr, bits = oracle
    n, nk, ns, nd, m = llr.shape
    flat = llr.reshape(n, nk, ns, nd * m)
    return np.where(bits[:, None, None].astype(bool), -flat, flat).reshape(-1, nd * m), (n, nk, ns)


# ---- the tests ---------------------------------------------------------------------------------------------

def test_header_declares_the_layered_calls_and_binding_matches(tmp_path):
    from dsce import engine
    txt = open(HDR).read()
    for fn in ("dsce_run_ldpc_layered", "dsce_ldpc_layered"):
        assert re.search(r"^int\s+%s\s*\(" % fn, txt, re.M) and fn in engine.EXPORTED, fn
    assert re.search(r"^#define DSCE_HAS_LDPC_LAYERED\s+1\b", txt, re.M)
    assert re.search(r"#define DSCE_ABI_VERSION\s+10\b", txt) and engine.ABI_VERSION == 10
    # the arguments of the two declarations, in order
    proto = {fn: re.sub(r"\s+", " ", re.search(r"^int\s+%s\s*\(([^;]*)\);" % fn, txt, re.M | re.S).group(1))
             for fn in ("dsce_run_ldpc_layered", "dsce_ldpc_layered")}
    assert [a.strip().rsplit(" ", 1)[0] for a in proto["dsce_run_ldpc_layered"].split(",")] == [
        "dsce_ctx*", "int32_t", "uint64_t", "uint64_t", "uint64_t", "uint32_t", "const dsce_ldpc_desc*",
        "const dsce_ldpc_layers*", "const dsce_ldpc_out*"]
    assert [a.strip().rsplit(" ", 1)[0] for a in proto["dsce_ldpc_layered"].split(",")] == [
        "dsce_ctx*", "const dsce_ldpc_desc*", "const dsce_ldpc_layers*", "int64_t", "const double*", "int64_t",
        "uint8_t*", "int32_t*"]
    fields = ["n_layers", "layer_ptr", "layer_check"]
    body = re.search(r"typedef struct \{([^}]*)\} dsce_ldpc_layers;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == fields == [f for f, _ in engine.LdpcLayers._fields_]
    prog = 'printf(" %zu", sizeof(dsce_ldpc_layers));\n'
    prog += "".join('printf(" %%zu", offsetof(dsce_ldpc_layers, %s));\n' % f for f in fields)
    prog += 'printf(" %zu", sizeof(dsce_ldpc_desc));\n'          # the flooding descriptor has not grown
    py = [ctypes.sizeof(engine.LdpcLayers)] + [getattr(engine.LdpcLayers, f).offset for f in fields]
    py += [ctypes.sizeof(engine.LdpcDesc)]
    src = tmp_path / "c.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsce.h"\n'
                   '#if !DSCE_HAS_LDPC_LAYERED || !DSCE_HAS_LDPC_RUN\n#error "ldpc layered macro"\n#endif\n'
                   "int (*run)(dsce_ctx*, int32_t, uint64_t, uint64_t, uint64_t, uint32_t, const dsce_ldpc_desc*,\n"
                   "           const dsce_ldpc_layers*, const dsce_ldpc_out*) = dsce_run_ldpc_layered;\n"
                   "int (*probe)(dsce_ctx*, const dsce_ldpc_desc*, const dsce_ldpc_layers*, int64_t, const double*,\n"
                   "             int64_t, uint8_t*, int32_t*) = dsce_ldpc_layered;\n"
                   "int main(){\n" + prog + "return 0;}\n")
    exe = tmp_path / "c"
    # -c: the two pointers above need no library, only declarations of exactly these types
    subprocess.run(["gcc", "-Werror", "-I", os.path.dirname(HDR), "-c", str(src), "-o", str(tmp_path / "c.o")], check=True)
    src2 = tmp_path / "d.c"
    src2.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsce.h"\nint main(){\n' + prog + "return 0;}\n")
    subprocess.run(["gcc", "-I", os.path.dirname(HDR), str(src2), "-o", str(exe)], check=True)
    c = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert c == py and py[0] == 24


@pytest.mark.parametrize("rate", ["1/2", "3/4", "5/6"])
def test_make_layers_of_the_2560_codes(rate):
    from dsce.coding import make_layers, serial_layers
    code = code_of(2560, rate)
    lp, lc = make_layers(code)
    assert_partition(code, (lp, lc))
    assert np.diff(lp).tolist() == LAYER_SIZES[rate]
    for l in range(lp.size - 1):
        assert (np.diff(lc[lp[l]:lp[l + 1]]) > 0).all()             # check order inside a layer
    again = make_layers(code)
    assert np.array_equal(again[0], lp) and np.array_equal(again[1], lc)
    assert_partition(code, serial_layers(code))


def test_make_layers_first_fit_and_a_wide_variable():
    """First fit by hand on a small graph; a variable of degree 40, as in the limit codes of the GPU tests, forces
    at least 40 layers."""
    from dsce.coding import ldpc_from_rows, make_layers
    #        c0      c1      c2      c3      c4      c5
    rows = [[0, 1], [2, 3], [1, 2], [4, 5], [0, 4], [3, 5]]
    lp, lc = make_layers(ldpc_from_rows(rows, 6, 3))
    # c0 -> L0; c1 -> L0; c2 shares 1 with c0 -> L1; c3 -> L0; c4 shares 0 (L0), 4 (L0) -> L1, and L1 = {c2} is
    # free of 0 and 4; c5 shares 3 (c1, L0) and 5 (c3, L0) -> L1, free of 3 and 5
    assert lp.tolist() == [0, 3, 6] and lc.tolist() == [0, 1, 3, 2, 4, 5]
    rng = np.random.default_rng(5)
    for N in (63, 600):
        M = max(4, 2 * N // 3)
        rows = [[0] * (c < 40) + [int(v) for v in rng.choice(np.arange(1, N), 3, replace=False)] for c in range(M)]
        code = ldpc_from_rows(rows, N, N // 2)
        vdeg = np.bincount(code.col, minlength=N)
        layers = make_layers(code)
        assert_partition(code, layers)
        assert vdeg[0] == 40 and layers[0].size - 1 >= 40
        # the 40 checks of variable 0 sit in 40 different layers
        where = np.repeat(np.arange(layers[0].size - 1), np.diff(layers[0]))[np.argsort(layers[1])]
        assert len(set(where[:40].tolist())) == 40


def test_check_layers_refusals():
    """The Python mirror of the host's refusals, in the host's words."""
    from dsce.coding import check_layers, ldpc_from_rows, make_layers
    code = ldpc_from_rows([[0, 1], [2, 3], [1, 2], [4, 5]], 6, 3)
    lp, lc = make_layers(code)
    assert lp.tolist() == [0, 3, 4] and lc.tolist() == [0, 1, 3, 2]
    check_layers(code, (lp, lc))
    i32 = lambda *a: np.array(a, dtype=np.int32)                   # noqa: E731
    bad = [(None, "null"), ((None, lc), "null"), ((lp, None), "null"),
           ((i32(0), lc), "n_layers"), ((i32(0, 1, 2, 3, 4, 4), lc), "n_layers"),
           ((i32(1, 3, 4), lc), "layer_ptr[0]"), ((i32(0, 3, 3, 4), lc), "layer 1 no check"),
           ((i32(0, 3, 2, 4), lc), "layer 1 no check"), ((i32(0, 2, 3), lc), "layer_ptr[n_layers]"),
           ((lp, i32(0, 1, 3, 4)), "layer_check entry"), ((lp, i32(0, 1, 3, -1)), "layer_check entry"),
           ((lp, i32(0, 1, 3, 1)), "check 1 appears twice"),
           ((i32(0, 2, 4), i32(0, 1, 3, 2)), None),                    # valid: another partition
           ((i32(0, 2, 4), i32(0, 2, 1, 3)), "layer 0: checks 0 and 2 share variable 1"),
           ((i32(0, 4), i32(3, 1, 2, 0)), "layer 0: checks 1 and 2 share variable 2")]
    for layers, word in bad:
        if word is None:
            check_layers(code, layers)
            continue
        with pytest.raises(ValueError) as e:
            check_layers(code, layers)
        assert word in str(e.value), (word, e.value)


def test_layered_noiseless_zero_and_single():
    from dsce.coding import ldpc_decode_layered, ldpc_encode, ldpc_lam, serial_layers
    code = code_of(300, "3/4")
    cw = ldpc_encode(np.random.default_rng(11).integers(0, 2, (5, code.n_info)).astype(np.uint8), code)
    lam = ldpc_lam(cw, code, 3.0)
    for layers in (layers_of(code), serial_layers(code)):
        x, it = ldpc_decode_layered(lam, code, layers)
        assert x.dtype == np.uint8 and x.shape == cw.shape and it.dtype == np.int32
        assert np.array_equal(x, cw) and (it == 1).all()
        x1, it1 = ldpc_decode_layered(lam[0], code, layers)
        assert np.array_equal(x1, cw[0]) and it1 == 1
        x2, it2 = ldpc_decode_layered(lam, code._replace(early_stop=False, max_iter=7), layers)
        assert np.array_equal(x2, cw) and (it2 == 7).all()
        x3, it3 = ldpc_decode_layered(np.zeros_like(lam), code, layers)
        assert not x3.any() and (it3 == 1).all()


def test_layered_tree_codes_decode_to_the_ml_codeword():
    """test_ldpc_host's 1000 cycle-free cases: alpha = 1, 4 M + 4 iterations, integer lam.  On a tree every schedule
    of min-sum that serves each edge once per iteration ends in the exact max-marginals within the diameter."""
    from dsce.coding import ldpc_decode_layered, serial_layers
    assert check_tree_ml(layered) >= 1000
    assert check_tree_ml(lambda lam, code: ldpc_decode_layered(lam, code, serial_layers(code)), range(1000, 1020)) >= 200


@pytest.mark.parametrize("N,rate", [(96, "1/2"), (96, "3/4"), (96, "5/6"), (2560, "3/4"), (2560, "5/6")])
def test_layered_codeword_invariance(N, rate):
    check_invariance(layered, N, rate)


def test_layered_codeword_invariance_2560_half():
    check_invariance_2560_half(layered)


def test_layered_needs_fewer_iterations():
    """BPSK / AWGN, sigma 0.8, (2560, 1/2), 40 frames, the same noise: at a cap of 15 the layered schedule fails on
    no more frames than flooding at 30, and on fewer than flooding at 15."""
    from dsce.coding import ldpc_decode
    code = code_of(2560, "1/2")
    lam, raw = bpsk_lam0(code, 0.8, 40, 9)
    fail = lambda x: int(x[:, :code.n_info].any(axis=1).sum())     # noqa: E731
    f30 = fail(ldpc_decode(lam, code)[0])
    f15 = fail(ldpc_decode(lam, code._replace(max_iter=15))[0])
    l15 = fail(layered(lam, code._replace(max_iter=15))[0])
    print("flooding 30: %d, flooding 15: %d, layered 15: %d of 40" % (f30, f15, l15))
    assert l15 <= f30 < f15


@pytest.mark.parametrize("rate", ["1/2", "3/4"])
def test_layered_conventions_pinned_on_the_oracle(oracle_llr, rate):  # noqa: F811
    """ldpc_counts(layers=...) of the oracle's max-log LLRs gives the recorded table; random real codewords through
    the same LLRs give the same counts; at 35 dB the layered schedule needs fewer iterations than flooding."""
    from dsce.coding import ldpc_counts, ldpc_encode
    llr, bits = oracle_llr
    n, nk, ns, nd, m = llr.shape
    code = code_of(nd * m, rate)
    sym = (bits.reshape(n, nd, m).astype(np.int64) << np.arange(m)).sum(axis=-1)
    cc = ldpc_counts(llr, sym, code, layers=layers_of(code))
    print("rate %s %s" % (rate, {f: a.tolist() for f, a in cc.items()}))
    for f in ("bit_err", "frame_err", "iter_sum"):
        assert cc[f].dtype == np.int64 and cc[f].tolist() == ORACLE_LDPC_LAYERED[rate][f], (f, cc[f].tolist())
    # 35 dB: nowhere more iterations than flooding, and fewer in all (a frame that fails takes max_iter either way)
    lay, flood = (np.array(t[rate]["iter_sum"])[1] for t in (ORACLE_LDPC_LAYERED, ORACLE_LDPC))
    assert (lay <= flood).all() and lay.sum() < flood.sum()
    lam, shape = oracle_lam(oracle_llr)
    cw = ldpc_encode(np.random.default_rng(17).integers(0, 2, (lam.shape[0], code.n_info)).astype(np.uint8), code)
    x, it = layered(lam * flip_of(cw, code), code)
    bit = (x ^ cw)[:, :code.n_info].astype(np.int64).sum(axis=1).reshape(shape)
    assert bit.sum(axis=0).tolist() == ORACLE_LDPC_LAYERED[rate]["bit_err"]
    assert (bit > 0).sum(axis=0).tolist() == ORACLE_LDPC_LAYERED[rate]["frame_err"]
    assert it.astype(np.int64).reshape(shape).sum(axis=0).tolist() == ORACLE_LDPC_LAYERED[rate]["iter_sum"]
    # without layers the flooding definition, untouched
    assert ldpc_counts(llr, sym, code)["iter_sum"].tolist() == ORACLE_LDPC[rate]["iter_sum"]


@pytest.mark.parametrize("mutation", ["stale", "no_store"])
def test_wrong_layered_decoders_are_caught(oracle_llr, mutation):  # noqa: F811
    """Two mutations of the twin: every check reads the P of the iteration's start (the flooding schedule, which is a
    correct decoder: the two references hold for it, only the recorded table tells it apart), and R' is never stored
    (the own message is never taken out again: the tree check fails).  Each is caught by a reference or by the
    table, and each changes the table."""
    def wrong(lam, code):
        return layered(lam, code, _mutate=mutation)

    caught = []
    for name, check in (("tree", lambda: check_tree_ml(wrong, range(1000, 1020))),
                        ("invariance 96 1/2", lambda: check_invariance(wrong, 96, "1/2"))):
        try:
            check()
        except AssertionError:
            caught.append(name)
    lam, shape = oracle_lam(oracle_llr)
    code = code_of(lam.shape[1], "1/2")
    x, it = wrong(lam, code)
    table = dict(bit_err=x[:, :code.n_info].astype(np.int64).sum(axis=1).reshape(shape).sum(axis=0).tolist(),
                 iter_sum=it.astype(np.int64).reshape(shape).sum(axis=0).tolist())
    if any(table[f] != ORACLE_LDPC_LAYERED["1/2"][f] for f in table):
        caught.append("table")
    print("mutation %s: caught by %s" % (mutation, caught))
    assert "table" in caught
    assert ("tree" in caught) == (mutation == "no_store")


def test_simulate_ldpc_schedule_refusals():
    """--ldpc-schedule without --ldpc, and a schedule that is none, exit with a message before anything touches a
    GPU."""
    from dsce import simulate
    with pytest.raises(SystemExit) as e:
        simulate.main(["--ldpc-schedule", "layered", "--reps", "64"])
    assert "--ldpc-schedule" in str(e.value) and "--ldpc" in str(e.value), e.value
    with pytest.raises(SystemExit):
        simulate.main(["--ldpc", "3/4", "--ldpc-schedule", "serial"])
