"""CPU: the host side of the coded-link track (dsce_run_coded / dsce_viterbi,
DSCE_HAS_CODED_RUN) — dsce.coding: the K = 7 code (133, 171), the code tables
(puncturing and interleaving), the NumPy twin of k_viterbi, its error correction
over BPSK / AWGN, the header's declarations against the ctypes binding, and the
conventions pinned on the oracle's LLRs: the decoded-error counts of the default
OFDM scheme recorded from a prototype of the definitions of include/dsce.h, and
the same counts from random codewords in place of the all-zero one.  No GPU
call; tests/test_gpu_coded.py compares the engine against this twin, and
tests/test_coding_ml_host.py compares the twin with references that are not a
decoder."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import harness
from oracle import philox
from test_llr_host import SEED, demapper_input

HDR = os.path.join(harness.ROOT, "include", "dsce.h")
RATES = ("1/2", "2/3", "3/4", "5/6")

# default setup, ofdm, 256-QAM, SNR (10, 35) dB, n_iter 4, SEED, realisations 5..7, max-log LLRs,
# make_code(2560, rate, interleaver=7) terminated: [snr][stage]
ORACLE_COUNTS = {
    "3/4": dict(bit_err=[[2861, 2831, 2859, 2861, 2873], [2236, 695, 666, 600, 603]],
                frame_err=[[3, 3, 3, 3, 3], [3, 2, 2, 2, 2]]),
    "1/2": dict(bit_err=[[1835, 1854, 1857, 1787, 1791], [7, 0, 0, 0, 0]],
                frame_err=[[3, 3, 3, 3, 3], [1, 0, 0, 0, 0]]),
}


def test_free_distance_is_ten():
    """The minimum encoded weight over the non-zero input sequences of length <= 7
    (followed by six zeros, so the path returns to state 0) is 10."""
    from dsce.coding import conv_encode
    u = np.array(list(itertools.product((0, 1), repeat=7)), dtype=np.uint8)[1:]
    w = conv_encode(np.concatenate([u, np.zeros((u.shape[0], 6), dtype=np.uint8)], axis=1)).sum(axis=(1, 2))
    assert w.min() == 10
    # the generators themselves: the impulse response is 133 / 171 octal, MSB = u_t
    imp = conv_encode([1, 0, 0, 0, 0, 0, 0])
    assert int("".join(map(str, imp[:, 0])), 2) == 0o133 and int("".join(map(str, imp[:, 1])), 2) == 0o171


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("interleaver", [None, 7])
@pytest.mark.parametrize("terminated", [True, False])
def test_noiseless_round_trip(rate, interleaver, terminated):
    from dsce.coding import code_lam, conv_encode, make_code, viterbi_decode
    code = make_code(300, rate, terminated=terminated, interleaver=interleaver)
    rng = np.random.default_rng(11)
    u = rng.integers(0, 2, (5, code.n_steps)).astype(np.uint8)
    if terminated:
        u[:, code.n_info:] = 0
    lam = code_lam(conv_encode(u), code.src, code.n_slots, 3.0)
    got = viterbi_decode(lam, code.src, terminated)
    assert got.dtype == np.uint8 and got.shape == u.shape
    # an unterminated, punctured tail can be ambiguous: the last bits are not protected
    k = code.n_steps if terminated else code.n_steps - 12
    assert np.array_equal(got[:, :k], u[:, :k])
    assert np.array_equal(viterbi_decode(lam[0], code.src, terminated), got[0])


@pytest.mark.parametrize("terminated", [True, False])
def test_all_zero_input_decodes_to_zero(terminated):
    """Every comparison is a tie (or -inf against -inf): the tie rule takes b = 0 and
    the traceback starts at the lowest index, so all-zero lam decodes to zeros."""
    from dsce.coding import make_code, viterbi_decode
    for rate in RATES:
        code = make_code(200, rate, terminated=terminated)
        assert not viterbi_decode(np.zeros((2, 200)), code.src, terminated).any()


@pytest.mark.parametrize("rate,ebn0_db", [("1/2", 4.0), ("2/3", 5.0), ("3/4", 6.0), ("5/6", 7.0)])
def test_error_correction_over_awgn(rate, ebn0_db):
    """BPSK over AWGN, B = 2560, 20 codewords: fewer decoded errors than a tenth of
    the raw sign errors."""
    from dsce.coding import code_lam, conv_encode, make_code, viterbi_decode
    B, n = 2560, 20
    code = make_code(B, rate)
    rng = np.random.default_rng(3)
    u = rng.integers(0, 2, (n, code.n_steps)).astype(np.uint8)
    u[:, code.n_info:] = 0
    tx = code_lam(conv_encode(u), code.src, B)                   # +1 = bit 1, 0 in unused slots
    r = code.n_info / code.n_kept
    sigma2 = 1.0 / (2.0 * r * 10.0 ** (ebn0_db / 10.0))
    y = -tx + np.sqrt(sigma2) * rng.standard_normal((n, B))      # BPSK: bit 0 -> +1, bit 1 -> -1
    lam = -2.0 * y / sigma2
    used = np.zeros(B, dtype=bool)
    used[code.src[code.src >= 0]] = True
    raw = int(((lam > 0) != (tx > 0))[:, used].sum())
    dec = viterbi_decode(lam, code.src, True)
    errs = int((dec != u).sum())
    print("rate %s at %.0f dB: %d raw sign errors of %d, %d decoded errors" % (rate, ebn0_db, raw, n * code.n_kept, errs))
    assert raw > 0 and errs < raw / 10.0


def test_make_code_tables():
    from dsce.coding import make_code
    want = {"1/2": (1280, 2560), "2/3": (1706, 2559), "3/4": (1920, 2560), "5/6": (2133, 2560)}
    pi = np.random.RandomState(7).permutation(2560)
    for rate, (T, kept) in want.items():
        c = make_code(2560, rate)
        assert (c.n_steps, c.n_kept, c.n_info, c.terminated) == (T, kept, T - 6, True), rate
        assert c.src.shape == (T, 2) and c.src.dtype == np.int32
        used = c.src[c.src >= 0]
        assert used.size == kept == np.unique(used).size and used.min() >= 0 and used.max() < 2560
        assert np.array_equal(used, pi[:kept])                   # the q-th kept output, in (t, k) order
        assert make_code(2560, rate, terminated=False).n_info == T
        ident = make_code(2560, rate, interleaver=None).src
        assert np.array_equal(ident[ident >= 0], np.arange(kept))
        assert np.array_equal(make_code(2560, rate, interleaver=pi).src, c.src)
    # the masks: (keep o0, keep o1) per step, repeating
    assert (make_code(40, "3/4", interleaver=None).src[:3] >= 0).tolist() == [[True, True], [True, False], [False, True]]
    assert (make_code(40, "5/6", interleaver=None).src[:5] >= 0).tolist() == [[True, True], [True, False], [False, True],
                                                                            [True, False], [False, True]]
    for bad in (dict(rate="1/3"), dict(interleaver=[0, 0, 1]), dict(n_slots=8)):
        with pytest.raises(ValueError):
            make_code(**dict(dict(n_slots=3, rate="1/2", terminated=True, interleaver=None), **bad))


def test_header_declares_the_coded_calls_and_binding_matches(tmp_path):
    from dsce import engine
    txt = open(HDR).read()
    for fn in ("dsce_run_coded", "dsce_viterbi"):
        assert re.search(r"^int\s+%s\s*\(" % fn, txt, re.M) and fn in engine.EXPORTED, fn
    assert re.search(r"^#define DSCE_HAS_CODED_RUN\s+1\b", txt, re.M)
    assert re.search(r"#define DSCE_ABI_VERSION\s+10\b", txt) and engine.ABI_VERSION == 10
    names = {"dsce_code_desc": (engine.CodeDesc, ["n_steps", "terminated", "src"]),
             "dsce_coded_out": (engine.CodedOut, ["bit_err", "frame_err"])}
    prog, py = "", []
    for cname, (cls, fields) in names.items():
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % cname, txt, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"(\w+)\s*;", body) == fields == [f for f, _ in cls._fields_], cname
        prog += 'printf(" %%zu", sizeof(%s));\n' % cname
        prog += "".join('printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f in fields)
        py += [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
    src = tmp_path / "c.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsce.h"\n'
                   '#if !DSCE_HAS_CODED_RUN\n#error "coded run macro"\n#endif\n'
                   "int main(){\n" + prog + "return 0;}\n")
    exe = tmp_path / "c"
    subprocess.run(["gcc", "-I", os.path.dirname(HDR), str(src), "-o", str(exe)], check=True)
    c = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert c == py


@pytest.fixture(scope="module")
def oracle_llr():
    """The recipe of test_llr_host.test_definitions_close_on_the_oracle for the
    default ofdm scheme: max-log LLRs [3][2][5][320][8] of the oracle's per-unit
    trace, and the transmitted bits [3][2560]."""
    from dsce.modulation import llr_awgn
    S = harness.setup("default", schemes=("ofdm",), snr_db=(10.0, 35.0), n_iter=4)
    sc = S.schemes["ofdm"]
    n, nk, ns, nd, m = 3, 2, S.n_iter + 1, sc["n_data"], sc["bits_per_symbol"]
    tr = {}
    harness.simulate(S, SEED, 5, n, ["ofdm"], trace=tr)
    LK = sc["G"].shape[1]
    y_ic = np.zeros((n, nk, ns, LK), dtype=complex)
    h_est = np.zeros_like(y_ic)
    for i in range(n):
        for k in range(nk):
            u = tr["units"][i * nk + k]
            y_ic[i, k], h_est[i, k] = np.asarray(u["yest"]), np.asarray(u["hest"])
    x, pe, _ = demapper_input(sc, S.pn_time, y_ic, h_est)
    llr = llr_awgn(sc["symbols"], sc["bitmap"], x, pe, "maxlog").reshape(n, nk, ns, nd, m)
    bits = np.stack([philox.bits(SEED, 5 + i, sc["bits_slot"], nd * m) for i in range(n)])
    assert (nd, m) == (320, 8)
    return llr, bits


@pytest.mark.parametrize("rate", ["3/4", "1/2"])
def test_conventions_pinned_on_the_oracle(oracle_llr, rate):
    """lam = (1 - 2 t) LLR of the oracle's LLRs decoded by the twin gives the counts
    a prototype of include/dsce.h's definitions recorded (ORACLE_COUNTS): cells with
    zero, partial and total failure.  A different polynomial, state order, tie rule
    or table order changes them."""
    from dsce.coding import coded_counts, count_errors, make_code, viterbi_decode
    llr, bits = oracle_llr
    n, nk, ns, nd, m = llr.shape
    code = make_code(nd * m, rate, interleaver=7)
    flat = llr.reshape(n, nk, ns, nd * m)
    lam = np.where(bits[:, None, None].astype(bool), -flat, flat)
    dec = viterbi_decode(lam.reshape(-1, nd * m), code.src, True)
    bit, frame = count_errors(dec, True)
    bit, frame = bit.reshape(n, nk, ns).sum(axis=0), frame.reshape(n, nk, ns).sum(axis=0)
    print("rate %s bit_err %s frame_err %s" % (rate, bit.tolist(), frame.tolist()))
    assert bit.tolist() == ORACLE_COUNTS[rate]["bit_err"]
    assert frame.tolist() == ORACLE_COUNTS[rate]["frame_err"]
    # coded_counts (what the GPU tests use) is the same computation from sym
    sym = (bits.reshape(n, nd, m).astype(np.int64) << np.arange(m)).sum(axis=-1)
    cc = coded_counts(llr, sym, code)
    assert np.array_equal(cc["bit_err"], bit) and np.array_equal(cc["frame_err"], frame)


@pytest.mark.parametrize("terminated", [True, False])
@pytest.mark.parametrize("rate", ["3/4", "1/2"])
def test_oracle_counts_with_real_codewords(oracle_llr, rate, terminated):
    """The counts without the all-zero shortcut: a random information word per
    (realisation, SNR point, stage) is encoded, lam = (1 - 2 t) LLR gets the sign
    of its coded bits, and the decoded word is compared with the one sent.  Per
    row the number of wrong information bits is that of the all-zero word, so the
    terminated tables give ORACLE_COUNTS again; the oracle's |lam| spans ten
    decades and is not rounded."""
    from dsce.coding import conv_encode, count_errors, make_code, viterbi_decode
    from test_coding_ml_host import flip_of
    llr, bits = oracle_llr
    n, nk, ns, nd, m = llr.shape
    code = make_code(nd * m, rate, terminated=terminated, interleaver=7)
    flat = llr.reshape(n, nk, ns, nd * m)
    lam = np.where(bits[:, None, None].astype(bool), -flat, flat).reshape(-1, nd * m)
    u = np.random.default_rng(17).integers(0, 2, (lam.shape[0], code.n_steps)).astype(np.uint8)
    u[:, code.n_info:] = 0
    zero, _ = count_errors(viterbi_decode(lam, code.src, terminated), terminated)
    sent, _ = count_errors(viterbi_decode(lam * flip_of(u, code, conv_encode), code.src, terminated) ^ u, terminated)
    assert zero.shape == (n * nk * ns,) and np.array_equal(sent, zero), np.flatnonzero(sent != zero)
    assert (zero > 0).sum() >= 15
    if terminated:
        assert sent.reshape(n, nk, ns).sum(axis=0).tolist() == ORACLE_COUNTS[rate]["bit_err"]
        assert (sent > 0).reshape(n, nk, ns).sum(axis=0).tolist() == ORACLE_COUNTS[rate]["frame_err"]


@pytest.mark.parametrize("extra,word", [(["--checkpoint", "ck.json"], "--checkpoint"),
                                        (["--shard", "snr"], "--shard snr")])
def test_coded_refusals(extra, word):
    """--coded with a mode it does not cover exits with a message before anything
    touches a GPU."""
    from dsce import simulate
    with pytest.raises(SystemExit) as e:
        simulate.main(["--coded", "3/4", "--reps", "64"] + extra)
    assert "--coded" in str(e.value) and word in str(e.value), e.value
    with pytest.raises(SystemExit):
        simulate.main(["--coded", "7/8"])                        # not a rate
