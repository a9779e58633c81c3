"""CPU: the host side of the LDPC track (dsce_run_ldpc / dsce_ldpc,
DSCE_HAS_LDPC_RUN) — dsce.coding: make_ldpc's repeat-accumulate codes, their
encoder, and ldpc_decode, the NumPy twin of k_ldpc, against references that are
not the twin: the brute-force maximum-likelihood codeword on cycle-free codes
(normalised min-sum with alpha = 1 is exact there), and the codeword invariance
that makes the engine's all-zero simulation exact, with a separate encoder.
Then error correction over BPSK / AWGN, the header against the ctypes binding,
the conventions pinned on the oracle's LLRs (ORACLE_LDPC), three deliberately
wrong decoders that these references must catch, and the refusals of
`python -m dsce.simulate --ldpc`.  No GPU call; tests/test_gpu_ldpc.py compares
the engine with the twin and tests/test_gpu_ldpc_ref.py runs the tree and
invariance cases of this file through dsce_ldpc."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import harness
from test_coding_host import oracle_llr  # noqa: F401  (the fixture)

HDR = os.path.join(harness.ROOT, "include", "dsce.h")
RATES = ("1/2", "2/3", "3/4", "5/6")

# default setup, ofdm, 256-QAM, SNR (10, 35) dB, n_iter 4, SEED, realisations 5..7, max-log LLRs,
# make_ldpc(2560, rate) (seed 7, interleaver 7, 30 iterations, alpha 0.75, early stop): [snr][stage]
ORACLE_LDPC = {
    "1/2": dict(bit_err=[[1190, 1147, 1136, 1140, 1141], [33, 0, 0, 0, 0]],
                frame_err=[[3, 3, 3, 3, 3], [2, 0, 0, 0, 0]],
                iter_sum=[[90, 90, 90, 90, 90], [73, 27, 25, 23, 23]]),
    "3/4": dict(bit_err=[[1820, 1752, 1755, 1759, 1759], [664, 206, 183, 171, 169]],
                frame_err=[[3, 3, 3, 3, 3], [3, 2, 2, 2, 2]],
                iter_sum=[[90, 90, 90, 90, 90], [90, 65, 62, 62, 62]]),
}

# (N, rate) -> sigma of the BPSK / AWGN channel at which the twin fails on between a quarter and three quarters
# of 40 frames (measured on the twin; the invariance test asserts both)
INVARIANCE_SIGMA = {(96, "1/2"): 0.9, (96, "3/4"): 0.65, (96, "5/6"): 0.55,
                    (2560, "1/2"): 0.8, (2560, "3/4"): 0.62, (2560, "5/6"): 0.55}

_codes = {}


def code_of(n, rate, **kw):
    """make_ldpc, once per argument set (the 2560-variable codes take a second each)"""
    from dsce.coding import make_ldpc
    key = (n, rate, tuple(sorted(kw.items())))
    if key not in _codes:
        _codes[key] = make_ldpc(n, rate, **kw)
    return _codes[key]


def dense_h(code):
    H = np.zeros((code.n_checks, code.n_vars), dtype=np.uint8)
    H[np.repeat(np.arange(code.n_checks), np.diff(code.row_ptr)), code.col] = 1
    return H


def reference_encode(u, code):
    """An encoder written from the description of make_ldpc, not from ldpc_encode: H =
    [H1 | H2] dense, H2 the dual diagonal, so check i gives p_i = p_{i-1} ^ (H1 u)_i, one
    parity bit after the other."""
    H = dense_h(code)
    K, M = code.n_info, code.n_checks
    u = np.asarray(u, dtype=np.uint8)
    cw = np.zeros(u.shape[:-1] + (K + M,), dtype=np.uint8)
    cw[..., :K] = u
    s = (u.astype(np.int64) @ H[:, :K].T.astype(np.int64)) & 1
    prev = np.zeros(u.shape[:-1], dtype=np.int64)
    for i in range(M):
        prev = prev ^ s[..., i]
        cw[..., K + i] = prev
    return cw


def bpsk_lam0(code, sigma, n, seed):
    """lam of the all-zero codeword over BPSK (bit 0 -> +1) with noise sigma: lam = -2 y / sigma^2 in the slot of
    each variable; and the raw sign-error rate"""
    rng = np.random.default_rng(seed)
    y = 1.0 + sigma * rng.standard_normal((n, code.n_vars))
    lam = np.zeros((n, code.n_slots))
    lam[:, code.slot] = -2.0 * y / sigma ** 2
    return lam, float((y < 0).mean())


def flip_of(cw, code):
    """the factor (1 - 2 c) of each slot for the codewords cw [n][N]"""
    f = np.ones(cw.shape[:-1] + (code.n_slots,))
    f[..., code.slot] = 1.0 - 2.0 * cw.astype(np.float64)
    return f


# ---- cycle-free codes and their brute-force ML codeword (nothing of dsce.coding) ----------------------------

def tree_case(seed):
    """A random cycle-free code and decoder inputs: 1-6 checks, each joining one
    existing variable to 1-3 new ones; lam int in +-10^6, 10 words.  Returns (rows, N,
    lam [10][N], ml [10][N]): ml is the codeword of largest sum_v x_v lam_v (lam positive
    = the bit is 1), int64, by enumeration of all 2^(N - M) codewords, asserted unique."""
    rng = np.random.default_rng(seed)
    M = int(rng.integers(1, 7))
    rows, N, dep = [], 1, []
    for _ in range(M):
        new = int(rng.integers(1, 4))
        rows.append([int(rng.integers(0, N))] + list(range(N, N + new)))
        N += new
        dep.append(N - 1)                                        # the check's last new variable: XOR of its others
    free = [v for v in range(N) if v not in dep]
    words = np.zeros((1 << len(free), N), dtype=np.int64)
    words[:, free] = (np.arange(1 << len(free))[:, None] >> np.arange(len(free))) & 1
    for r in rows:                                               # in creation order: the others are already set
        words[:, r[-1]] = words[:, r[:-1]].sum(axis=1) & 1
    for r in rows:
        assert not (words[:, r].sum(axis=1) & 1).any()
    lam = rng.integers(-10 ** 6, 10 ** 6 + 1, (10, N)).astype(np.int64)
    metric = lam @ words.T                                       # [10][codewords]
    best = metric.max(axis=1)
    assert ((metric == best[:, None]).sum(axis=1) == 1).all(), "the ML codeword is not unique"
    return rows, N, lam.astype(np.float64), words[metric.argmax(axis=1)].astype(np.uint8)


TREE_SEEDS = range(1000, 1100)                                   # 100 codes x 10 words = 1000 cases


def tree_code(rows, N):
    from dsce.coding import ldpc_from_rows
    return ldpc_from_rows(rows, N, N, max_iter=4 * len(rows) + 4, alpha=1.0, early_stop=False)


def check_tree_ml(decode, seeds=TREE_SEEDS):
    """decode(lam, code) -> (x, it); every decoded word is the unique ML codeword.  Returns the number of cases."""
    cases, degs = 0, set()
    for seed in seeds:
        rows, N, lam, ml = tree_case(seed)
        code = tree_code(rows, N)
        x, it = decode(lam, code)
        assert np.array_equal(x, ml), (seed, np.argwhere(x != ml)[:4])
        assert (np.asarray(it) == code.max_iter).all()
        cases += lam.shape[0]
        degs.update(len(r) for r in rows)
    assert degs == {2, 3, 4}
    return cases


def check_invariance(decode, N, rate):
    """decode(lam0 * flip) ^ c == decode(lam0) with equal iteration counts for 40 random
    codewords c (reference_encode), at a sigma where the decoder both fails and succeeds
    on at least a quarter of the frames."""
    from dsce.coding import ldpc_encode, ldpc_syndrome
    code = code_of(N, rate)
    n = 40
    u = np.random.default_rng(N + 31).integers(0, 2, (n, code.n_info)).astype(np.uint8)
    cw = reference_encode(u, code)
    assert np.array_equal(cw, ldpc_encode(u, code)) and not ldpc_syndrome(cw, code).any()
    assert cw.any(axis=1).all()
    lam0, raw = bpsk_lam0(code, INVARIANCE_SIGMA[N, rate], n, 1000 + N)
    x0, it0 = decode(lam0, code)
    x1, it1 = decode(lam0 * flip_of(cw, code), code)
    fails = int(x0[:, :code.n_info].any(axis=1).sum())
    print("N %d rate %s sigma %.2f: %d of %d frames fail, mean iterations %.1f, raw BER %.3f"
          % (N, rate, INVARIANCE_SIGMA[N, rate], fails, n, float(np.mean(it0)), raw))
    assert np.array_equal(x1 ^ cw, x0), np.argwhere((x1 ^ cw) != x0)[:4]
    assert np.array_equal(it1, it0)
    assert fails >= n // 4 and n - fails >= n // 4, fails


# ---- the tests ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("N", [96, 2560])
def test_make_ldpc_structure(N, rate):
    from dsce.coding import LDPC_RATES, ldpc_encode, ldpc_four_cycles, ldpc_syndrome, make_ldpc
    num, den = LDPC_RATES[rate]
    c = code_of(N, rate)
    K, M = N * num // den, N - N * num // den
    assert (c.n_vars, c.n_info, c.n_checks, c.n_slots, c.rate) == (N, K, M, N, rate)
    assert (c.max_iter, c.alpha, c.early_stop) == (30, 0.75, True)
    assert c.row_ptr.dtype == c.col.dtype == c.slot.dtype == np.int32
    assert c.row_ptr.shape == (M + 1,) and c.row_ptr[0] == 0 and c.col.shape == (c.row_ptr[-1],)
    deg = np.diff(c.row_ptr)
    assert deg.min() >= 2 and deg.max() <= 32
    H = dense_h(c)
    assert H.sum() == c.col.size                                  # no repeated entry
    for i in range(M):
        r = c.col[c.row_ptr[i]:c.row_ptr[i + 1]]
        assert (np.diff(r) > 0).all() and r.min() >= 0 and r.max() < N
    assert (H[:, :K].sum(axis=0) == 3).all()                      # H1: column weight 3
    w1 = H[:, :K].sum(axis=1)
    assert w1.max() - w1.min() <= 1 and w1.sum() == 3 * K
    dual = np.eye(M, dtype=np.uint8) + np.eye(M, k=-1, dtype=np.uint8)
    assert np.array_equal(H[:, K:], dual)
    assert np.array_equal(np.sort(c.slot), np.arange(N))
    assert np.array_equal(c.slot, np.random.RandomState(7).permutation(N))
    assert c.four_cycles == ldpc_four_cycles(c)
    g = H.astype(np.int64) @ H.T.astype(np.int64)
    np.fill_diagonal(g, 0)
    assert c.four_cycles == int((g * (g - 1) // 2).sum()) // 2
    if rate == "1/2":
        assert c.four_cycles == 0
    u = np.random.default_rng(2).integers(0, 2, (6, K)).astype(np.uint8)
    cw = ldpc_encode(u, c)
    assert cw.dtype == np.uint8 and cw.shape == (6, N) and np.array_equal(cw[:, :K], u)
    assert not ((cw.astype(np.int64) @ H.T.astype(np.int64)) & 1).any() and not ldpc_syndrome(cw, c).any()
    assert np.array_equal(cw, reference_encode(u, c))
    if N == 96:
        again = make_ldpc(N, rate)
        for f in ("row_ptr", "col", "slot"):
            assert np.array_equal(getattr(again, f), getattr(c, f)), f
        other = make_ldpc(N, rate, seed=8, interleaver=None)
        assert not np.array_equal(other.col, c.col) and np.array_equal(other.slot, np.arange(N))
        for bad in (dict(rate="1/3"), dict(interleaver=[0, 0, 1]), dict(n_slots=4)):
            with pytest.raises(ValueError):
                make_ldpc(**dict(dict(n_slots=N, rate="1/2"), **bad))


def test_header_declares_the_ldpc_calls_and_binding_matches(tmp_path):
    from dsce import coding, engine
    txt = open(HDR).read()
    for fn in ("dsce_run_ldpc", "dsce_ldpc"):
        assert re.search(r"^int\s+%s\s*\(" % fn, txt, re.M) and fn in engine.EXPORTED, fn
    assert re.search(r"^#define DSCE_HAS_LDPC_RUN\s+1\b", txt, re.M)
    assert re.search(r"#define DSCE_ABI_VERSION\s+10\b", txt) and engine.ABI_VERSION == 10
    names = {"dsce_ldpc_desc": (engine.LdpcDesc, ["n_vars", "n_checks", "row_ptr", "col", "slot", "n_info", "max_iter",
                                                  "alpha", "early_stop"]),
             "dsce_ldpc_out": (engine.LdpcOut, ["bit_err", "frame_err", "iter_sum"])}
    prog, py = "", []
    for cname, (cls, fields) in names.items():
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % cname, txt, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"(\w+)\s*;", body) == fields == [f for f, _ in cls._fields_], cname
        prog += 'printf(" %%zu", sizeof(%s));\n' % cname
        prog += "".join('printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f in fields)
        py += [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
    prog += 'printf(" %d %d", DSCE_LDPC_MAX_CHECK_DEGREE, DSCE_LDPC_MAX_ITER);\n'
    py += [coding.LDPC_MAX_CHECK_DEGREE, coding.LDPC_MAX_ITER]
    assert py[-2:] == [32, 100]
    src = tmp_path / "c.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsce.h"\n'
                   '#if !DSCE_HAS_LDPC_RUN || !DSCE_HAS_CODED_RUN\n#error "ldpc run macro"\n#endif\n'
                   "int main(){\n" + prog + "return 0;}\n")
    exe = tmp_path / "c"
    subprocess.run(["gcc", "-I", os.path.dirname(HDR), str(src), "-o", str(exe)], check=True)
    c = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert c == py


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("interleaver", [None, 7])
def test_noiseless_round_trip(rate, interleaver):
    from dsce.coding import ldpc_decode, ldpc_encode, ldpc_lam
    code = code_of(300, rate, interleaver=interleaver)
    u = np.random.default_rng(11).integers(0, 2, (5, code.n_info)).astype(np.uint8)
    cw = ldpc_encode(u, code)
    lam = ldpc_lam(cw, code, 3.0)
    x, it = ldpc_decode(lam, code)
    assert x.dtype == np.uint8 and x.shape == cw.shape and it.dtype == np.int32
    assert np.array_equal(x, cw) and (it == 1).all()
    x1, it1 = ldpc_decode(lam[0], code)
    assert np.array_equal(x1, cw[0]) and it1 == 1
    # without early stop every iteration is performed, to the same word
    x2, it2 = ldpc_decode(lam, code._replace(early_stop=False, max_iter=7))
    assert np.array_equal(x2, cw) and (it2 == 7).all()
    # all-zero lam: every P stays 0 and is decided as 0
    x3, it3 = ldpc_decode(np.zeros_like(lam), code)
    assert not x3.any() and (it3 == 1).all()


def test_tree_codes_decode_to_the_ml_codeword():
    """alpha = 1, no early stop, 4 M + 4 iterations, integer lam: on a cycle-free code
    min-sum is the max-product algorithm and P_v ends as the exact max-marginal
    difference (integers below 2^53), so x is the unique ML codeword: 1000 cases."""
    from dsce.coding import ldpc_decode
    assert check_tree_ml(ldpc_decode) >= 1000


@pytest.mark.parametrize("rate", ["1/2", "3/4", "5/6"])
@pytest.mark.parametrize("N", [96, 2560])
def test_codeword_invariance(N, rate):
    from dsce.coding import ldpc_decode
    check_invariance(ldpc_decode, N, rate)


@pytest.mark.parametrize("rate", ["1/2", "3/4"])
def test_error_correction_over_awgn(rate):
    """sigma = 0.5: more than 2 % of the hard decisions are wrong, and 40 frames of 2560
    bits decode without an error."""
    from dsce.coding import ldpc_decode
    code = code_of(2560, rate)
    lam, raw = bpsk_lam0(code, 0.5, 40, 77)
    x, it = ldpc_decode(lam, code)
    print("rate %s: raw BER %.4f, decoded errors %d, mean iterations %.2f" % (rate, raw, int(x.sum()), it.mean()))
    assert raw > 0.02 and not x.any() and it.max() < code.max_iter


@pytest.mark.parametrize("rate", ["1/2", "3/4"])
def test_conventions_pinned_on_the_oracle(oracle_llr, rate):  # noqa: F811
    """ldpc_counts of the oracle's max-log LLRs gives the recorded table ORACLE_LDPC, with
    cells of zero, partial and total failure; random real codewords through the same
    LLRs give the same counts."""
    from dsce.coding import ldpc_counts, ldpc_decode, ldpc_encode
    llr, bits = oracle_llr
    n, nk, ns, nd, m = llr.shape
    code = code_of(nd * m, rate)
    sym = (bits.reshape(n, nd, m).astype(np.int64) << np.arange(m)).sum(axis=-1)
    cc = ldpc_counts(llr, sym, code)
    print("rate %s %s" % (rate, {f: a.tolist() for f, a in cc.items()}))
    for f in ("bit_err", "frame_err", "iter_sum"):
        assert cc[f].dtype == np.int64 and cc[f].tolist() == ORACLE_LDPC[rate][f], (f, cc[f].tolist())
    flat = llr.reshape(n, nk, ns, nd * m)
    lam = np.where(bits[:, None, None].astype(bool), -flat, flat).reshape(-1, nd * m)
    u = np.random.default_rng(17).integers(0, 2, (lam.shape[0], code.n_info)).astype(np.uint8)
    cw = ldpc_encode(u, code)
    x, it = ldpc_decode(lam * flip_of(cw, code), code)
    bit = (x ^ cw)[:, :code.n_info].astype(np.int64).sum(axis=1).reshape(n, nk, ns)
    assert bit.sum(axis=0).tolist() == ORACLE_LDPC[rate]["bit_err"]
    assert (bit > 0).sum(axis=0).tolist() == ORACLE_LDPC[rate]["frame_err"]
    assert it.astype(np.int64).reshape(n, nk, ns).sum(axis=0).tolist() == ORACLE_LDPC[rate]["iter_sum"]


def test_oracle_table_has_zero_partial_and_total_failure():
    fe = np.array([ORACLE_LDPC[r]["frame_err"] for r in ("1/2", "3/4")])
    assert (fe == 0).any() and (fe == 3).any() and ((fe > 0) & (fe < 3)).any()
    be = np.array([ORACLE_LDPC[r]["bit_err"] for r in ("1/2", "3/4")])
    assert ((be > 0) == (fe > 0)).all()


@pytest.mark.parametrize("mutation", ["sign", "no_exclude", "alpha_late"])
def test_wrong_decoders_are_caught(oracle_llr, mutation):  # noqa: F811
    """Three mutations of the twin: the check rule's sign as for the other LLR convention
    (wrong on checks of odd degree), the own message not excluded (m1 on every edge),
    alpha applied after the variable sum (P' = alpha (ell + sum R'), R' unscaled).  The
    tree-ML check or the invariance check fails for each.  The first two break both at
    once.  The third is sign-symmetric and is the decoder itself at alpha = 1, so the
    equalities of both references hold for it by construction; of the invariance check
    it fails only the window on the failing frames (N = 2560, rate 1/2: 8 of 40 where a
    quarter is asked).  What pins alpha's place firmly is the recorded table: the
    mutation's counts on the oracle's LLRs are not ORACLE_LDPC."""
    from dsce.coding import ldpc_decode

    def wrong(lam, code):
        return ldpc_decode(lam, code, _mutate=mutation)

    caught = []
    checks = [("tree", lambda: check_tree_ml(wrong, range(1000, 1020)))]
    checks += [("invariance %d %s" % (N, r), lambda N=N, r=r: check_invariance(wrong, N, r))
               for N in (96, 2560) for r in ("1/2", "3/4", "5/6")]
    for name, check in checks:
        if caught and name.startswith("invariance 2560"):
            break                                                # the small cases have already caught it
        try:
            check()
        except AssertionError:
            caught.append(name)
    print("mutation %s: caught by %s" % (mutation, caught))
    assert caught
    llr, bits = oracle_llr
    n, nk, ns, nd, m = llr.shape
    code = code_of(nd * m, "1/2")
    flat = llr.reshape(n, nk, ns, nd * m)
    lam = np.where(bits[:, None, None].astype(bool), -flat, flat).reshape(-1, nd * m)
    x, it = wrong(lam, code)
    bit = x[:, :code.n_info].astype(np.int64).sum(axis=1).reshape(n, nk, ns).sum(axis=0)
    assert bit.tolist() != ORACLE_LDPC["1/2"]["bit_err"]


@pytest.mark.parametrize("extra,word", [(["--checkpoint", "ck.json"], "--checkpoint"),
                                        (["--shard", "snr"], "--shard snr")])
def test_ldpc_refusals(extra, word):
    """--ldpc with a mode it does not cover exits with a message before anything
    touches a GPU."""
    from dsce import simulate
    with pytest.raises(SystemExit) as e:
        simulate.main(["--ldpc", "3/4", "--reps", "64"] + extra)
    assert "--ldpc" in str(e.value) and word in str(e.value), e.value
    with pytest.raises(SystemExit):
        simulate.main(["--ldpc", "7/8"])                         # not a rate
    for bad in (["--ldpc-iters", "0"], ["--ldpc-iters", "101"], ["--ldpc-alpha", "0"], ["--ldpc-alpha", "1.5"]):
        with pytest.raises(SystemExit) as e:
            simulate.main(["--ldpc", "3/4"] + bad)
        assert bad[0] in str(e.value)
