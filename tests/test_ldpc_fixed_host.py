"""CPU: the host side of the fixed-point LDPC decoder (dsce_run_ldpc_fixed /
dsce_ldpc_fixed, DSCE_HAS_LDPC_FIXED) — the header against the ctypes binding
and a compiled C program; dsce.coding.ldpc_decode_fixed, the vectorised NumPy
twin of k_ldpc_fixed, against a second implementation written in this file from
the header's text with plain Python loops, one edge at a time (small codes, every
word length, rule and input class of the header), and against a reference that is
not integer code at all: on integer inputs that nothing clips it is ldpc_decode
at alpha = 1.0, the decoder that tests/test_ldpc_host.py ties to the ML codeword.
Then the codeword of the run (flipped inputs through the decoder give the counts
of ldpc_counts_fixed), the bias of the all-zero word at short words, the recorded
table ORACLE_LDPC_FIXED, three deliberately wrong twins, and the Python mirrors of
the refusals.  No GPU call; tests/test_gpu_ldpc_fixed.py compares the engine with
the twin."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import harness
from test_coding_host import oracle_llr  # noqa: F401  (the fixture)
from test_ldpc_host import bpsk_lam0, code_of, flip_of

HDR = os.path.join(harness.ROOT, "include", "dsce.h")

# default setup, ofdm, 256-QAM, SNR (10, 35) dB, n_iter 4, SEED, realisations 5..7, max-log LLRs, make_ldpc(2560, rate)
# (seed 7, interleaver 7, 30 iterations, early stop), make_fixed() (6 / 6 / 8 bit, scale 2, alpha 1 / 1, beta 1), the
# codeword ldpc_encode(RandomState(11).randint(0, 2, n_info)): [snr][stage].  Computed by the twin after the scalar
# implementation of this file agreed with it.
ORACLE_LDPC_FIXED = {
    "1/2": dict(bit_err=[[1209, 1186, 1185, 1177, 1179], [322, 7, 7, 7, 7]],
                frame_err=[[3, 3, 3, 3, 3], [3, 1, 1, 1, 1]],
                iter_sum=[[90, 90, 90, 90, 90], [90, 39, 38, 39, 39]]),
    "3/4": dict(bit_err=[[1843, 1811, 1812, 1811, 1812], [789, 284, 241, 234, 227]],
                frame_err=[[3, 3, 3, 3, 3], [3, 2, 2, 2, 2]],
                iter_sum=[[90, 90, 90, 90, 90], [90, 68, 64, 64, 63]]),
}

WORDS = ((2, 2, 2), (4, 4, 6), (6, 6, 8), (8, 4, 8), (16, 16, 16))
ALPHAS = ((1, 0), (3, 2), (13, 4))                               # 1, 3/4, 13/16


# ---- the second implementation: the header's text, one edge at a time ---------------------------------------

def scalar_quantise(lam, scale, C):
    t = (-float(lam)) * float(scale)
    if t != t:
        return 0
    a = abs(t)
    mag = C if a >= C else int(math.floor(a + 0.5))
    return -mag if t < 0 else mag


def scalar_decode(lam, code, fx, ell=None):
    """(x, it, P) of every row of lam by the five steps of include/dsce.h, in Python ints"""
    C, X, A = [(1 << (q - 1)) - 1 for q in (fx.q_ch, fx.q_msg, fx.q_app)]
    rp, col, slot = [np.asarray(a).tolist() for a in (code.row_ptr, code.col, code.slot)]
    N, M = code.n_vars, code.n_checks
    xs, its, Ps = [], [], []
    for w in range(len(lam) if ell is None else len(ell)):
        if ell is None:
            L = [0 if slot[v] < 0 else scalar_quantise(lam[w][slot[v]], fx.scale, C) for v in range(N)]
        else:
            L = [int(e) for e in ell[w]]
        P, R, it = list(L), [0] * len(col), 0
        while True:
            Rn = [0] * len(col)
            for c in range(M):
                q = [max(-X, min(X, P[col[e]] - R[e])) for e in range(rp[c], rp[c + 1])]
                a = [abs(v) for v in q]
                s = [v < 0 for v in q]
                m1 = min(a)
                i1 = a.index(m1)
                m2 = min(a[:i1] + a[i1 + 1:])
                sg = sum(s) & 1
                for p in range(len(q)):
                    mu = m2 if p == i1 else m1
                    r = max(((mu * fx.alpha_num + ((1 << fx.alpha_shift) >> 1)) >> fx.alpha_shift) - fx.beta, 0)
                    Rn[rp[c] + p] = -r if sg ^ s[p] else r
            P = list(L)
            for e, v in enumerate(col):
                P[v] += Rn[e]
            P = [max(-A, min(A, v)) for v in P]
            R = Rn
            x = [int(v < 0) for v in P]
            it += 1
            if it >= code.max_iter:
                break
            if code.early_stop and not any(sum(x[col[e]] for e in range(rp[c], rp[c + 1])) & 1 for c in range(M)):
                break
        xs.append(x)
        its.append(it)
        Ps.append(P)
    return np.array(xs, dtype=np.uint8), np.array(its, dtype=np.int32), np.array(Ps, dtype=np.int16)


def small_code(N, rng, **kw):
    """A random code of N <= 40 variables on the limits of the description, in the style of
    test_gpu_ldpc.limit_code: check 0 of degree 2, check 1 of degree min(32, N - 3), variable 0
    in every check (at most 40), variable N - 1 in none; two punctured variables, two in one slot."""
    from dsce.coding import ldpc_from_rows
    M = max(4, 2 * N // 3)
    pool = np.arange(1, N - 2)
    rows = []
    for c in range(M):
        d = 2 if c == 0 else min(32, N - 3) if c == 1 else int(rng.integers(2, min(6, N - 3) + 1))
        special = [0] + ([N - 2] if c == 1 else [])
        rows.append(special + [int(v) for v in rng.choice(pool, d - len(special), replace=False)])
    slot = rng.permutation(N + 3)[:N].astype(np.int32)
    slot[3] = slot[5] = -1
    slot[2] = slot[1]
    code = ldpc_from_rows(rows, N, max(1, N // 2), slot=slot, n_slots=N + 3, **kw)
    deg = np.diff(code.row_ptr)
    assert deg[0] == 2 and deg.max() == min(32, N - 3)
    return code


def same(a, b, what):
    for name, u, v in zip(("x", "it", "P"), a, b):
        assert u.dtype == v.dtype and np.array_equal(u, v), (what, name, np.argwhere(np.asarray(u) != np.asarray(v))[:4])


def integer_case(code, n=50, iters=12):
    """Integer lam in +-40 and the parameters under which nothing of the fixed-point decoder clips"""
    from dsce.coding import make_fixed
    lam = np.random.default_rng(code.n_vars + 5).integers(-40, 41, (n, code.n_slots)).astype(np.float64)
    fx = make_fixed(16, 16, 16, scale=1.0, alpha_num=1, alpha_shift=0, beta=0)
    return lam, code._replace(alpha=1.0, max_iter=iters), fx


# ---- the tests ---------------------------------------------------------------------------------------------

def test_header_declares_the_fixed_calls_and_binding_matches(tmp_path):
    from dsce import coding, engine
    txt = open(HDR).read()
    for fn in ("dsce_run_ldpc_fixed", "dsce_ldpc_fixed"):
        assert re.search(r"^int\s+%s\s*\(" % fn, txt, re.M) and fn in engine.EXPORTED, fn
    assert re.search(r"^#define DSCE_HAS_LDPC_FIXED\s+1\b", txt, re.M)
    assert re.search(r"#define DSCE_ABI_VERSION\s+10\b", txt) and engine.ABI_VERSION == 10
    fields = ["scale", "q_ch", "q_msg", "q_app", "alpha_num", "alpha_shift", "beta"]
    body = re.search(r"typedef struct \{([^}]*)\} dsce_ldpc_fixed_desc;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == fields == [f for f, _ in engine.LdpcFixedDesc._fields_]
    assert list(coding.LdpcFixed._fields) == fields
    prog = 'printf(" %zu", sizeof(dsce_ldpc_fixed_desc));\n'
    prog += "".join('printf(" %%zu", offsetof(dsce_ldpc_fixed_desc, %s));\n' % f for f in fields)
    py = [ctypes.sizeof(engine.LdpcFixedDesc)] + [getattr(engine.LdpcFixedDesc, f).offset for f in fields]
    shapes = [(1, 1), (8, 4), (2560, 1280), (2560, 640), (16500, 200)]
    for N, M in shapes:
        prog += 'printf(" %%lld", (long long)DSCE_LDPC_FIXED_LDS_BYTES(%d, %d));\n' % (N, M)
        py.append(coding.ldpc_fixed_lds_bytes(N, M))
        assert py[-1] <= 4 * N + 12 * M + 8 and 2 * py[-1] <= 8 * N + 24 * M + 8 + 8
    assert coding.ldpc_fixed_lds_bytes(2560, 1280) == 23048
    src = tmp_path / "c.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsce.h"\n'
                   '#if !DSCE_HAS_LDPC_FIXED || !DSCE_HAS_LDPC_RUN || DSCE_ABI_VERSION != 10\n#error "ldpc fixed macro"\n#endif\n'
                   "int (*run)(dsce_ctx*, int32_t, uint64_t, uint64_t, uint64_t, uint32_t, const dsce_ldpc_desc*,\n"
                   "           const dsce_ldpc_fixed_desc*, const uint8_t*, const dsce_ldpc_out*) = dsce_run_ldpc_fixed;\n"
                   "int (*probe)(dsce_ctx*, const dsce_ldpc_desc*, const dsce_ldpc_fixed_desc*, int64_t, const double*,\n"
                   "             int64_t, uint8_t*, int32_t*, int16_t*) = dsce_ldpc_fixed;\n"
                   "int main(){\n" + prog + "return 0;}\n")
    obj = tmp_path / "c.o"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.dirname(HDR), "-c", str(src), "-o", str(obj)], check=True)
    # the prototypes are only referenced: link without them
    src2 = tmp_path / "d.c"
    src2.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsce.h"\nint main(){\n' + prog + "return 0;}\n")
    exe = tmp_path / "d"
    subprocess.run(["gcc", "-I", os.path.dirname(HDR), str(src2), "-o", str(exe)], check=True)
    c = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert c == py
    fx = coding.make_fixed()
    assert fx == coding.LdpcFixed(2.0, 6, 6, 8, 1, 0, 1) and coding.check_fixed(fx) == (31, 31, 127)


def test_quantiser():
    """Round half away from zero, saturate, odd, NaN to 0: against the scalar rule, value by value."""
    from dsce.coding import ldpc_quantise, make_fixed
    k = np.arange(-40, 41).astype(np.float64)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e300, -1e300, 1e-300, 0.49999999999999994, 0.5,
                        np.nextafter(0.5, 1), 30.5, 31.0, 31.49, 31.5, -31.5, 127.5, 32767.5, -32767.49])
    lam = np.concatenate([k, k + 0.5, k + 0.25, special, np.random.default_rng(1).standard_normal(200) * 20])
    for q_ch, scale in ((2, 1.0), (4, 1.0), (6, 2.0), (8, 0.37), (16, 1.0), (16, 1000.0), (6, 1e-9), (6, 1e9), (6, 1e300)):
        fx = make_fixed(q_ch, q_ch, 16 if q_ch == 16 else q_ch + 2, scale=scale)
        C = (1 << (q_ch - 1)) - 1
        got = ldpc_quantise(lam, fx)
        ref = np.array([scalar_quantise(v, scale, C) for v in lam])
        assert got.dtype == np.int32 and np.array_equal(got, ref), (q_ch, scale, lam[got != ref][:4])
        assert np.abs(got).max() <= C
        assert np.array_equal(ldpc_quantise(-lam, fx), -got)                     # odd
    fx = make_fixed(6, 6, 8, scale=1.0)
    assert ldpc_quantise(np.array([-0.5, -1.5, -2.5, 0.5, 1.5, 2.5, 0.49]), fx).tolist() == [1, 2, 3, -1, -2, -3, 0]
    assert ldpc_quantise(np.array([np.nan, np.inf, -np.inf, 1e9]), fx).tolist() == [0, -31, 31, -31]
    assert not ldpc_quantise(lam[np.abs(lam) < 1e6], make_fixed(6, 6, 8, scale=1e-9)).any()            # zeroes everything


@pytest.mark.parametrize("N", [8, 23, 40])
def test_twin_against_the_scalar_implementation(N):
    """ldpc_decode_fixed == the loops of this file in x, it and P: every word length, alpha = 1, 3/4 and 13/16,
    beta = 0, 1 and >= X (every message 0), scales that zero and that saturate everything, inputs k + 0.5, +-inf
    and NaN, both early_stop values, 1, 2 and 25 iterations."""
    from dsce.coding import LdpcFixed, ldpc_decode_fixed, make_fixed
    rng = np.random.default_rng(700 + N)
    code0 = small_code(N, rng)
    n = 6 if N < 20 else 3
    base = 2.0 * rng.standard_normal((n, code0.n_slots)) - 1.0
    halves = rng.integers(-6, 6, base.shape).astype(np.float64) + 0.5
    odd = base.copy()
    odd[0, :3] = [np.inf, -np.inf, np.nan]
    odd[1, ::2] = np.nan
    odd[2, 1::3] = np.inf
    cases, stops, flips = 0, set(), 0
    for q_ch, q_msg, q_app in WORDS:
        X = (1 << (q_msg - 1)) - 1
        for an, sh in ALPHAS:
            for beta in (0, 1, X, 32767):
                for early, max_iter in ((1, 25), (0, 2), (1, 1)):
                    code = code0._replace(early_stop=bool(early), max_iter=max_iter)
                    for kind, lam, scale in (("normal", base, 2.0), ("halves", halves, 1.0), ("odd", odd, 3.0),
                                             ("zeroed", base, 1e-6), ("saturated", base, 1e6)):
                        if beta == 32767 and kind != "normal":
                            continue
                        fx = make_fixed(q_ch, q_msg, q_app, scale=scale, alpha_num=an, alpha_shift=sh, beta=beta)
                        got = ldpc_decode_fixed(lam, code, fx)
                        same(got, scalar_decode(lam, code, fx), (q_ch, q_msg, q_app, an, sh, beta, early, max_iter, kind))
                        assert np.abs(got[2]).max() <= (1 << (q_app - 1)) - 1
                        if kind == "zeroed":
                            assert not got[0].any() and not got[2].any()
                        if beta >= X:                                             # every message is 0: P stays ell
                            assert np.array_equal(got[0], ldpc_decode_fixed(lam, code._replace(max_iter=1), fx)[0])
                        cases += 1
                        stops.update(got[1].tolist())
                        flips += int(got[0].sum())
    x1, it1, P1 = ldpc_decode_fixed(base[0], code0, make_fixed())
    ref = ldpc_decode_fixed(base, code0, make_fixed())
    assert np.array_equal(x1, ref[0][0]) and it1 == ref[1][0] and np.array_equal(P1, ref[2][0]) and P1.dtype == np.int16
    assert cases > 400 and {1, 2, 25} <= stops and flips > 0
    assert isinstance(make_fixed(), LdpcFixed)


@pytest.mark.parametrize("N,rate", [(96, "1/2"), (96, "3/4"), (600, "1/2")])
def test_integer_inputs_equal_the_fp64_decoder(N, rate):
    """Integer-valued lam, scale 1, 16 / 16 / 16 bit, alpha 1 / 1, beta 0: nothing rounds and nothing clips, so the
    fixed-point decoder is ldpc_decode at alpha = 1.0 in bits and iterations: the decoder test_ldpc_host ties to the
    ML codeword on trees.  max |P| stays far below 32767, which is the premise."""
    from dsce.coding import ldpc_decode, ldpc_decode_fixed
    lam, code, fx = integer_case(code_of(N, rate))
    x, it, P = ldpc_decode_fixed(lam, code, fx)
    rx, rit = ldpc_decode(lam, code)
    print("N %d rate %s: max |P| %d, iterations %s" % (N, rate, int(np.abs(P.astype(np.int64)).max()), sorted(set(it.tolist()))))
    assert int(np.abs(P.astype(np.int64)).max()) < 32767
    assert np.array_equal(x, rx) and np.array_equal(it, rit) and x.any()
    assert len(set(it.tolist())) > 1 or it[0] == code.max_iter


def awgn_case(rate, sigma, n=60):
    from dsce.coding import ldpc_encode
    code = code_of(2560, rate)
    lam0, raw = bpsk_lam0(code, sigma, n, 4000 + int(100 * sigma))
    cw = ldpc_encode(np.random.default_rng(23).integers(0, 2, (n, code.n_info)), code)
    return code, lam0, cw


def counts_by_flip(code, fx, lam0, cw):
    """Wrong information bits and iterations per frame when cw is really sent: inputs flipped, decoded, XOR cw"""
    from dsce.coding import ldpc_decode_fixed
    x, it, P = ldpc_decode_fixed(lam0 * flip_of(cw, code), code, fx)
    return (x ^ cw)[:, :code.n_info].astype(np.int64).sum(axis=1), it


@pytest.mark.parametrize("rate,sigma", [("1/2", 0.80), ("3/4", 0.62)])
def test_real_codewords_over_awgn(rate, sigma):
    """make_ldpc(2560, rate), BPSK / AWGN, 6 / 6 / 8 bit, scale 2, alpha 3/4, 60 frames with a random codeword each:
    at least a tenth of the frames fail and a tenth succeed."""
    from dsce.coding import make_fixed
    code, lam0, cw = awgn_case(rate, sigma)
    bit, it = counts_by_flip(code, make_fixed(6, 6, 8, scale=2.0, alpha_num=3, alpha_shift=2, beta=0), lam0, cw)
    fails = int((bit > 0).sum())
    print("rate %s sigma %.2f: %d of 60 frames fail, %d wrong bits, mean iterations %.1f" % (rate, sigma, fails, bit.sum(), it.mean()))
    assert 6 <= fails <= 54


def test_codeword_of_the_run_and_the_all_zero_bias():
    """ldpc_counts_fixed(codeword=c) on arrays in the export's layout equals flipping the inputs by (1 - 2 c),
    decoding and XORing c.  And at 3 / 3 / 5 bit the all-zero word, on the same noise, shows strictly fewer wrong
    information bits than real codewords: ties are decided in its favour (include/dsce.h)."""
    from dsce.coding import ldpc_counts_fixed, ldpc_decode_fixed, ldpc_encode, make_fixed
    code = code_of(2560, "1/2")
    n, nk, S, nd, m = 2, 2, 2, 320, 8
    rng = np.random.default_rng(41)
    sym = rng.integers(0, 256, (n, nd))
    t = ((sym[..., None] >> np.arange(m)) & 1).reshape(n, 1, 1, nd * m)
    y = 1.0 + 0.8 * rng.standard_normal((n, nk, S, nd * m))
    lam = -2.0 * y / 0.64                                                         # the all-zero word under t
    llr = np.where(t.astype(bool), -lam, lam).reshape(n, nk, S, nd, m)
    c = ldpc_encode(np.random.RandomState(11).randint(0, 2, code.n_info), code)
    for fx in (make_fixed(), make_fixed(4, 4, 6, scale=1.0, beta=0), make_fixed(6, 6, 8, alpha_num=3, alpha_shift=2, beta=0)):
        got = ldpc_counts_fixed(llr, sym, code, fx, codeword=c)
        x, it, P = ldpc_decode_fixed(lam.reshape(-1, nd * m) * flip_of(c, code), code, fx)
        bit = (x ^ c)[:, :code.n_info].astype(np.int64).sum(axis=1).reshape(n, nk, S)
        assert np.array_equal(got["bit_err"], bit.sum(axis=0)) and np.array_equal(got["frame_err"], (bit > 0).sum(axis=0))
        assert np.array_equal(got["iter_sum"], it.astype(np.int64).reshape(n, nk, S).sum(axis=0))
        zero = ldpc_counts_fixed(llr, sym, code, fx)
        x0, it0, P0 = ldpc_decode_fixed(lam.reshape(-1, nd * m), code, fx)
        assert zero["bit_err"].sum() == x0[:, :code.n_info].sum() and zero["iter_sum"].sum() == it0.sum()
    code, lam0, cw = awgn_case("1/2", 0.80)
    fx = make_fixed(3, 3, 5, scale=1.0, beta=0)
    real, it_real = counts_by_flip(code, fx, lam0, cw)
    zero, it_zero = counts_by_flip(code, fx, lam0, np.zeros_like(cw))
    print("3/3/5: all-zero word %d wrong information bits, real codewords %d; iterations %d and %d"
          % (zero.sum(), real.sum(), it_zero.sum(), it_real.sum()))
    assert zero.sum() < real.sum()


def oracle_counts(oracle, rate, fx, mutate=None):
    from dsce.coding import ldpc_counts_fixed, ldpc_decode_fixed, ldpc_encode, ldpc_quantise
    llr, bits = oracle
    n, nk, ns, nd, m = llr.shape
    code = code_of(nd * m, rate)
    c = ldpc_encode(np.random.RandomState(11).randint(0, 2, code.n_info), code)
    sym = (bits.reshape(n, nd, m).astype(np.int64) << np.arange(m)).sum(axis=-1)
    if mutate is None:
        return ldpc_counts_fixed(llr, sym, code, fx, codeword=c), code, c
    flat = llr.reshape(n, nk, ns, nd * m)
    lam = np.where(bits[:, None, None].astype(bool), -flat, flat).reshape(-1, nd * m)
    x, it, P = ldpc_decode_fixed(lam * flip_of(c, code), code, fx, _mutate=mutate)
    bit = (x ^ c)[:, :code.n_info].astype(np.int64).sum(axis=1).reshape(n, nk, ns)
    return dict(bit_err=bit.sum(axis=0), frame_err=(bit > 0).sum(axis=0),
                iter_sum=it.astype(np.int64).reshape(n, nk, ns).sum(axis=0)), code, c


@pytest.mark.parametrize("rate", ["1/2", "3/4"])
def test_conventions_pinned_on_the_oracle(oracle_llr, rate):  # noqa: F811
    """ldpc_counts_fixed of the oracle's max-log LLRs with make_fixed() and the RandomState(11) codeword gives the
    recorded table; the unmutated decode by flipping gives it too."""
    from dsce.coding import make_fixed
    cc, code, c = oracle_counts(oracle_llr, rate, make_fixed())
    print("rate %s %s" % (rate, {f: a.tolist() for f, a in cc.items()}))
    assert c.any() and not c.all()
    for f in ("bit_err", "frame_err", "iter_sum"):
        assert cc[f].dtype == np.int64 and cc[f].tolist() == ORACLE_LDPC_FIXED[rate][f], (f, cc[f].tolist())
    by_flip, _, _ = oracle_counts(oracle_llr, rate, make_fixed(), mutate="none")
    for f in cc:
        assert np.array_equal(by_flip[f], cc[f]), f
    # the cells the table pins include partial and total failure
    assert (cc["frame_err"] == 3).any() and ((cc["frame_err"] > 0) & (cc["frame_err"] < 3)).any()
    assert ((cc["bit_err"] > 0) == (cc["frame_err"] > 0)).all()
    assert (cc["iter_sum"][cc["frame_err"] == 3] == 90).all() and (cc["iter_sum"][cc["frame_err"] < 3] < 90).all()


@pytest.mark.parametrize("mutation", ["trunc", "late_clamp", "beta_first"])
def test_wrong_decoders_are_caught(mutation):
    """Three mutations of the twin: no rounding term in the normalisation, q_p not clamped to the message word, the
    offset subtracted before the normalisation.  The scalar implementation catches each, at the parameters where the
    mutation acts: alpha = 3/4 (trunc: mu = 1 gives 0 where the rule gives 1), a message word narrower than the
    a-posteriori word (late_clamp: 8 / 4 / 8), alpha = 3/4 with beta = 1 (beta_first: mu = 2 gives 1 where the rule
    gives 2 - 1 ... 1, mu = 3 gives 2 where the rule gives 1).  The recorded table is decoded at alpha = 1 / 1 with
    equal word lengths for q and P - R and so cannot see trunc; it is the scalar comparison that pins these."""
    from dsce.coding import ldpc_decode_fixed, make_fixed
    rng = np.random.default_rng(90)
    code = small_code(40, rng)
    lam = 2.0 * rng.standard_normal((12, code.n_slots)) - 1.0
    fx = {"trunc": make_fixed(6, 6, 8, alpha_num=3, alpha_shift=2, beta=0),
          "late_clamp": make_fixed(8, 4, 8, scale=4.0, beta=0),
          "beta_first": make_fixed(6, 6, 8, alpha_num=3, alpha_shift=2, beta=1)}[mutation]
    ref = scalar_decode(lam, code, fx)
    same(ldpc_decode_fixed(lam, code, fx), ref, "unmutated")
    wrong = ldpc_decode_fixed(lam, code, fx, _mutate=mutation)
    assert not (np.array_equal(wrong[2], ref[2]) and np.array_equal(wrong[1], ref[1])), mutation


def test_mutations_against_the_recorded_table(oracle_llr):  # noqa: F811
    """Which mutation the table catches: decoded with make_fixed() (alpha 1 / 1, beta 1, 6 / 6 / 8), trunc and
    beta_first are the decoder itself (no shift: nothing to round, nothing to reorder), and q_p needs no clamp
    beyond what |P| <= 127 and |R| <= 31 allow only if it is there: late_clamp changes the counts."""
    from dsce.coding import make_fixed
    table = ORACLE_LDPC_FIXED["1/2"]
    for mutation, caught in (("trunc", False), ("beta_first", False), ("late_clamp", True)):
        cc, _, _ = oracle_counts(oracle_llr, "1/2", make_fixed(), mutate=mutation)
        differs = any(cc[f].tolist() != table[f] for f in table)
        print("mutation %s: the table %s it" % (mutation, "catches" if differs else "does not see"))
        assert differs == caught, mutation


def test_python_mirrors_of_the_refusals():
    from dsce.coding import LdpcFixed, check_codeword, check_fixed, ldpc_decode_fixed, ldpc_encode, make_fixed
    ok = make_fixed()
    bad = [(dict(scale=0.0), "scale"), (dict(scale=-1.0), "scale"), (dict(scale=float("nan")), "scale"),
           (dict(scale=float("inf")), "scale"), (dict(q_ch=1), "q_ch"), (dict(q_ch=17, q_app=16), "q_ch"),
           (dict(q_msg=1), "q_msg"), (dict(q_msg=17), "q_msg"), (dict(q_app=5), "q_app"), (dict(q_app=17), "q_app"),
           (dict(q_ch=8, q_msg=4, q_app=7), "q_app"), (dict(alpha_shift=-1), "alpha_shift"), (dict(alpha_shift=9), "alpha_shift"),
           (dict(alpha_num=0), "alpha_num"), (dict(alpha_num=2), "alpha_num"), (dict(alpha_num=5, alpha_shift=2), "alpha_num"),
           (dict(beta=-1), "beta"), (dict(beta=32768), "beta")]
    for kw, word in bad:
        with pytest.raises(ValueError, match=word):
            check_fixed(ok._replace(**kw))
        with pytest.raises(ValueError, match=word):
            make_fixed(**dict(ok._asdict(), **kw))
    with pytest.raises(ValueError, match="null"):
        check_fixed(None)
    for good in (LdpcFixed(1e-300, 2, 2, 2, 1, 0, 0), LdpcFixed(1e300, 16, 16, 16, 256, 8, 32767), LdpcFixed(1.0, 8, 4, 8, 1, 8, 0)):
        check_fixed(good)
    code = code_of(96, "1/2")
    c = ldpc_encode(np.random.default_rng(3).integers(0, 2, code.n_info), code)
    assert np.array_equal(check_codeword(code, c), c)
    flipped = c.copy()
    flipped[code.n_info + 7] ^= 1                                                 # parity 7 is in checks 7 and 8
    with pytest.raises(ValueError, match="check 7$"):
        check_codeword(code, flipped)
    two = c.copy()
    two[5] = 2
    with pytest.raises(ValueError, match="entry 5 "):
        check_codeword(code, two)
    with pytest.raises(ValueError, match="n_vars"):
        check_codeword(code, c[:-1])
    with pytest.raises(ValueError, match="q_ch"):
        ldpc_decode_fixed(np.zeros((1, 96)), code, ok._replace(q_ch=1))


def test_engine_refuses_fixed_with_layers():
    """Engine.ldpc / run_ldpc raise before any library call: no context is needed to see it."""
    from dsce import engine
    from dsce.coding import make_fixed, make_layers
    code = code_of(96, "1/2")
    eng = engine.Engine.__new__(engine.Engine)
    with pytest.raises(ValueError, match="fixed and layers"):
        engine.Engine.ldpc(eng, np.zeros((1, 96)), code, layers=make_layers(code), fixed=make_fixed())
    with pytest.raises(ValueError, match="fixed and layers"):
        engine.Engine.run_ldpc(eng, 0, 1, 0, 1, code, layers=make_layers(code), fixed=make_fixed())
    with pytest.raises(ValueError, match="codeword needs fixed"):
        engine.Engine.run_ldpc(eng, 0, 1, 0, 1, code, codeword=np.zeros(96, dtype=np.uint8))


@pytest.mark.parametrize("extra,word", [(["--ldpc-schedule", "layered"], "layered"),
                                        (["--ldpc-fixed", "6,6"], "--ldpc-fixed"),
                                        (["--ldpc-fixed", "6,6,5"], "q_app"),
                                        (["--ldpc-scale", "0"], "scale"),
                                        (["--ldpc-offset", "-1"], "beta"),
                                        (["--ldpc-alpha-q", "5/2^2"], "alpha_num"),
                                        (["--ldpc-alpha-q", "3/4"], "--ldpc-alpha-q")])
def test_simulate_fixed_refusals(extra, word):
    """The fixed-point options exit with a message before anything touches a GPU."""
    from dsce import simulate
    base = ["--ldpc", "3/4", "--reps", "64", "--ldpc-fixed", "6,6,8", "--ldpc-scale", "2"]
    with pytest.raises(SystemExit) as e:
        simulate.main(base + extra)
    assert word in str(e.value), e.value
    with pytest.raises(SystemExit) as e:
        simulate.main(["--ldpc-fixed", "6,6,8"])                                # without --ldpc
    assert "--ldpc" in str(e.value)
