"""CPU: the host side of the soft outputs (dsce_llr_awgn / dsce_export_llr,
DSCE_HAS_LLR) — the header's declarations against the ctypes binding, the NumPy
reference SignalConstellation.LLR_AWGN against the literal formula of
SignalConstellation.m:118 and against the hard decisions, the definitions of
include/dsce.h closed against the oracle's own error counts, and the LLR arrays
through the shard writer / reader.  No GPU call.

demapper_input restates "Per-stage demapper input" of include/dsce.h in NumPy;
tests/test_gpu_llr.py applies it to the engine's own y_ic / h_est."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import harness
from oracle import philox

HDR = os.path.join(harness.ROOT, "include", "dsce.h")
SEED = 0x5EED0009


def demapper_input(sc, pn_time, y_ic, h_est):
    """(x_est, pn_eff, x_terms) of the MMSE branch by include/dsce.h from y_ic and
    h_est [..., n_snr, S, LK] of an oracle scheme dict sc: x_est complex and pn_eff
    real [..., n_snr, S, ND]; x_terms = the sum of the moduli of x_est's terms
    (the rounding scale of a despread sum; |x_est| for select schemes)."""
    Q, P, dd = sc["Q"], sc["P"], sc["data_div"]
    NP = len(sc["pilot_pos"])
    qn = (np.abs(Q) ** 2).sum(axis=0)                                  # ||Q[:, l]||^2
    Pn = np.asarray(pn_time, dtype=float)[:, None, None] * qn          # [n_snr][1][LK]
    h2 = np.abs(h_est) ** 2
    if sc["despread"]:
        Pd = P[:, NP:]                                                 # [LK][ND]
        z = y_ic / h_est
        x = (z @ Pd.conj()) / dd
        terms = (np.abs(z) @ np.abs(Pd)) / dd
        pe = ((Pn / h2) @ (np.abs(Pd) ** 2)) / dd ** 2
    else:
        l = np.asarray(sc["data_pos"])
        x = y_ic[..., l] / h_est[..., l] / dd
        terms = np.abs(x)
        pe = np.broadcast_to(Pn, h2.shape)[..., l] / (h2[..., l] * dd ** 2)
    if sc["real_detect"]:
        x = x.real + 0j
    return x, pe, terms


def test_header_declares_llr_and_binding_matches(tmp_path):
    from dsce import engine
    txt = open(HDR).read()
    for fn in ("dsce_llr_awgn", "dsce_export_llr", "dsce_llr_info"):
        assert re.search(r"^int\s+%s\s*\(" % fn, txt, re.M), fn
        assert fn in engine.EXPORTED
    assert re.search(r"^#define DSCE_HAS_LLR\s+1\b", txt, re.M)
    assert re.search(r"^#define DSCE_LLR_MAXLOG\s+\(1u << 2\)", txt, re.M) and engine.LLR_MAXLOG == 1 << 2
    assert re.search(r"#define DSCE_ABI_VERSION\s+10\b", txt) and engine.ABI_VERSION == 10
    body = re.search(r"typedef struct \{([^}]*)\} dsce_export_llr_out;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"void\s*\*\s*(\w+)\s*;", body)
    assert fields == [f for f, _ in engine.ExportLlrOut._fields_] == list(engine.LLR_FIELDS)
    assert fields == ["x_est", "pn_eff", "llr"]
    src = tmp_path / "l.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsce.h"\n'
                   '#if !DSCE_HAS_LLR || DSCE_LLR_MAXLOG != 4\n#error "LLR macros"\n#endif\n'
                   'int main(){printf("%zu", sizeof(dsce_export_llr_out));\n'
                   + "".join('printf(" %%zu", offsetof(dsce_export_llr_out, %s));\n' % f for f in fields)
                   + "return 0;}\n")
    exe = tmp_path / "l"
    subprocess.run(["gcc", "-I", os.path.dirname(HDR), str(src), "-o", str(exe)], check=True)
    c = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert c == [ctypes.sizeof(engine.ExportLlrOut)] + [getattr(engine.ExportLlrOut, f).offset for f in fields]


@pytest.mark.parametrize("method,order", [("QAM", 4), ("QAM", 16), ("QAM", 64), ("QAM", 256), ("PAM", 2), ("PAM", 4),
                                          ("PAM", 8), ("PAM", 16)])
def test_host_llr_awgn(method, order):
    """The stable form against the literal formula of SignalConstellation.m:118
    wherever both of that formula's sums exceed 1e-300, at 1e-12 (1 + |LLR|);
    finite everywhere; and the sign of the max-log LLR is the hard decision's bit
    on every point whose nearest-point margin is >= 1e-9."""
    from dsce.modulation import SignalConstellation
    c = SignalConstellation(order, method)
    rng = np.random.default_rng(order + (method == "PAM"))
    n = 4000
    x = 1.2 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    if method == "PAM":
        x[: n // 2] = x[: n // 2].real                     # real observations, and complex ones
    pn = 10.0 ** rng.uniform(-6, 2, n)
    for P in (pn, 0.37):
        ex = c.LLR_AWGN(x, P)
        ml = c.LLR_AWGN(x, P, method="maxlog")
        m = c.BitsPerSymbol
        assert ex.shape == ml.shape == (n, m) and np.isfinite(ex).all() and np.isfinite(ml).all()
        w = np.exp(-np.abs(x[:, None] - c.SymbolMapping[None, :]) ** 2 / np.broadcast_to(P, x.shape)[:, None])
        compared = 0
        for b in range(m):
            s1, s0 = w[:, c.BitMapping[:, b]].sum(axis=1), w[:, ~c.BitMapping[:, b]].sum(axis=1)
            ok = (s1 > 1e-300) & (s0 > 1e-300)
            lit = np.log(s1[ok] / s0[ok])
            assert (np.abs(ex[ok, b] - lit) <= 1e-12 * (1 + np.abs(lit))).all(), (b, np.abs(ex[ok, b] - lit).max())
            compared += int(ok.sum())
        assert compared > n * m // 4
        if P is pn:
            assert compared < n * m                        # the literal formula does fail somewhere
        d = np.sort(np.abs(x[:, None] - c.SymbolMapping[None, :]), axis=1)
        safe = d[:, 1] - d[:, 0] >= 1e-9
        hard = c.BitMapping[c._nearest(x)]
        assert safe.sum() > n // 2 and np.array_equal((ml > 0)[safe], hard[safe])
    with pytest.raises(ValueError):
        c.LLR_AWGN(x, pn[:-1])
    with pytest.raises(ValueError):
        c.LLR_AWGN(x, 1.0, method="soft")
    assert np.isnan(c.LLR_AWGN([np.nan], 1.0)).all() and np.isnan(c.LLR_AWGN([0.1], np.nan, "maxlog")).all()


def test_definitions_close_on_the_oracle():
    """Default fbmc_cod, realisations 5..7, SNR (10, 35) dB, n_iter 4: x_est and
    pn_eff formed by include/dsce.h from refsim.simulate's per-unit trace (yest,
    hest), the host max-log LLR of them, and the sign errors against the BITS
    stream are the oracle's MMSE-branch error counts (all bits) at every SNR point
    and stage, exactly."""
    from dsce.modulation import llr_awgn
    S = harness.setup("default", schemes=("fbmc_cod",), snr_db=(10.0, 35.0), n_iter=4)
    sc = S.schemes["fbmc_cod"]
    n, nk, ns, nd, m = 3, 2, S.n_iter + 1, sc["n_data"], sc["bits_per_symbol"]
    tr = {}
    ref = harness.simulate(S, SEED, 5, n, ["fbmc_cod"], trace=tr)
    LK = sc["G"].shape[1]
    y_ic = np.zeros((n, nk, ns, LK), dtype=complex)
    h_est = np.zeros_like(y_ic)
    for i in range(n):
        for k in range(nk):
            u = tr["units"][i * nk + k]
            y_ic[i, k], h_est[i, k] = np.asarray(u["yest"]), np.asarray(u["hest"])
    x, pe, _ = demapper_input(sc, S.pn_time, y_ic, h_est)
    assert x.shape == pe.shape == (n, nk, ns, nd) and (pe > 0).all() and not x.imag.any()
    llr = llr_awgn(sc["symbols"], sc["bitmap"], x, pe, "maxlog").reshape(n, nk, ns, nd, m)
    bits = np.stack([philox.bits(SEED, 5 + i, sc["bits_slot"], nd * m).reshape(nd, m) for i in range(n)])
    err = ((llr > 0) != bits[:, None, None].astype(bool)).sum(axis=(0, 3, 4))
    assert ref["err"].shape == (1, 2, 2, nk, ns) and ref["err"][0, 0, 0].min() > 0
    assert np.array_equal(err, ref["err"][0, 0, 0]), (err, ref["err"][0, 0, 0])


def test_llr_arrays_round_trip_through_the_shards(tmp_path):
    from dsce import dataset
    rng = np.random.default_rng(2)
    n, nk, S, ND, m = 9, 2, 3, 7, 4
    full = dict(sym=rng.integers(0, 16, (n, ND)).astype(np.int32),
                x_est=(rng.standard_normal((n, nk, S, ND)) + 1j * rng.standard_normal((n, nk, S, ND))).astype(np.complex64),
                pn_eff=rng.random((n, nk, S, ND)).astype(np.float32),
                llr=rng.standard_normal((n, nk, S, ND, m)).astype(np.float32))
    assert dataset.LLR_ARRAYS == ("x_est", "pn_eff", "llr")
    prefix = str(tmp_path / "set")
    for i, (first, cnt) in enumerate(dataset.shard_ranges(40, n, 4)):
        part = {k: v[first - 40:first - 40 + cnt] for k, v in full.items()}
        dataset.write_shard(dataset.shard_path(prefix, i), part,
                            dict(seed=7, first_rep=first, n_rep=cnt, n_iter=S - 1, llr_method="maxlog"))
    arrays, meta = dataset.read_shard(dataset.shard_path(prefix, 0))
    assert sorted(arrays) == sorted(full) and meta["llr_method"] == "maxlog" and arrays["llr"].shape == (4, nk, S, ND, m)
    arrays, meta = dataset.load(prefix)
    assert sorted(arrays) == sorted(full)
    for k in full:
        assert arrays[k].dtype == full[k].dtype and np.array_equal(arrays[k], full[k]), k
    assert (meta["first_rep"], meta["n_rep"], meta["n_iter"], meta["llr_method"]) == (40, n, 2, "maxlog")
    with pytest.raises(ValueError):                 # an LLR array of another length than the shard
        dataset.write_shard(str(tmp_path / "bad-00000.npz"), {"llr": full["llr"][:3]}, dict(seed=7, first_rep=0, n_rep=4))
    # the command line: --llr implies the stage settings, and needs the estimator
    ap = dataset.parser()
    a = ap.parse_args(["--reps", "8", "--out", "x", "--llr", "maxlog", "--n-iter", "2"])
    assert a.llr == "maxlog" and a.n_iter == 2 and not a.stages
    assert ap.parse_args(["--reps", "8", "--out", "x"]).llr is None
    with pytest.raises(SystemExit):
        dataset.main(["--reps", "8", "--out", "x", "--llr", "exact", "--no-mmse"])
